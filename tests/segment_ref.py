"""The definition of the segmenter (include/zs_amd_segment.h, zs_seg_viterbi), numpy only and sharing no code with the product:

* viterbi32: the fp32 recurrence of the header, every operation an explicit np.float32 operation, which the device reproduces bit
  for bit (idx, n_seg, cost);
* viterbi64: a plain fp64 dynamic programme over (frame, codeword) -- the optimum of the objective;
* brute: the optimum by enumeration of all K^T paths;
* objective, runs, expand: the objective of a path, run-length coding and its inverse."""
import itertools

import numpy as np


def viterbi32(s, lam):
    """(idx int32 [T], n_seg, cost) of fp32 scores s [T, K] under fp32 lam, as the header writes it."""
    s = np.asarray(s, dtype=np.float32)
    T, K = s.shape
    lam = np.float32(lam)
    if T == 0:
        return np.zeros(0, dtype=np.int32), 0, 0.0
    ks = np.arange(K)
    c = s[0].copy()
    a = np.zeros(T, dtype=np.int64)
    sw = np.zeros((T, K), dtype=bool)
    cost = 0.0
    for t in range(T):
        if t >= 1:
            d = (c - m).astype(np.float32)                          # fl32(c_(t-1)[k] - m_(t-1))
            stay = (d < lam) | ((d == lam) & (ks <= a[t - 1]))      # (d, k) against (lam, a_(t-1)), lexicographic
            sw[t] = ~stay
            p = np.where(stay, d, lam).astype(np.float32)
            c = (s[t] + p).astype(np.float32)                       # fl32(s[t][k] + p)
        m = np.float32(c.min())
        a[t] = int(np.flatnonzero(c == m)[0])                       # the lowest k that attains it
        cost += float(np.float64(m))
    idx = np.zeros(T, dtype=np.int32)
    k = int(a[T - 1])
    for t in range(T - 1, 0, -1):
        idx[t] = k
        if sw[t, k]:
            k = int(a[t - 1])
    idx[0] = k
    return idx, 1 + int((np.diff(idx) != 0).sum()), cost


def objective(s, lam, idx):
    """sum_t s[t][k_t] + lam #{switches}, in the arithmetic of its operands (Python integers for integer inputs)."""
    s = np.asarray(s)
    tot = sum(s[t][int(k)].item() for t, k in enumerate(idx))
    return tot + lam * int((np.diff(np.asarray(idx)) != 0).sum())


def viterbi64(s, lam):
    """(the optimum of the objective, one optimal path) by a plain fp64 dynamic programme."""
    s = np.asarray(s, dtype=np.float64)
    T, K = s.shape
    if T == 0:
        return 0.0, np.zeros(0, dtype=np.int32)
    c = s[0].copy()
    back = np.zeros((T, K), dtype=np.int64)
    for t in range(1, T):
        j = int(c.argmin())
        jump = c[j] + lam
        stay = c <= jump
        back[t] = np.where(stay, np.arange(K), j)
        c = s[t] + np.where(stay, c, jump)
    k = int(c.argmin())
    best = float(c[k])
    idx = np.zeros(T, dtype=np.int32)
    for t in range(T - 1, -1, -1):
        idx[t] = k
        k = int(back[t][k])
    return best, idx


def brute(s, lam):
    """The optimum of the objective over all K^T paths (small K and T)."""
    s = np.asarray(s)
    T, K = s.shape
    if T == 0:
        return 0
    return min(objective(s, lam, p) for p in itertools.product(range(K), repeat=T))


def runs(idx):
    """[(codeword, duration)] of a sequence of indices."""
    out = []
    for k in np.asarray(idx).tolist():
        if out and out[-1][0] == k:
            out[-1][1] += 1
        else:
            out.append([k, 1])
    return [tuple(r) for r in out]


def expand(rs):
    return [k for k, d in rs for _ in range(d)]
