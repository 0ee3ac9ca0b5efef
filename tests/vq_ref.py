"""The definition of the vector codebook, numpy only: what zs_vq_assign / zs_vq_accum / zs_vq_update / zs_vq_gather and
zs_amd.vq.fit_vectors are tested against.  Scores are fp64; the sums of an iteration are int64 fixed point and the means are taken in
double, exactly as include/zs_amd.h writes them, so nothing here shares code with the kernels."""
import numpy as np

U = 2.0 ** -24


def planted(n, E, K0, sigma, seed):
    """K0 centres (standard normal through a leaky ReLU of slope 0.01) and n float32 rows around them."""
    rs = np.random.RandomState(seed)
    cen = rs.standard_normal((K0, E))
    cen = np.where(cen > 0, cen, 0.01 * cen)
    return (cen[rs.randint(K0, size=n)] + sigma * rs.standard_normal((n, E))).astype(np.float32)


def cnorm(code):
    """fp32 rounding of sum_j code^2 accumulated in double."""
    c = np.asarray(code, dtype=np.float64)
    return (c * c).sum(1).astype(np.float32)


def scores(x, code, cn=None):
    """fp64 s(i, k) = cnorm[k] - 2 x_i . c_k [n, K]; cn defaults to the exact squared norms."""
    x, c = np.asarray(x, dtype=np.float64), np.asarray(code, dtype=np.float64)
    cn = (c * c).sum(1) if cn is None else np.asarray(cn, dtype=np.float64)
    return cn[None, :] - 2.0 * (x @ c.T)


def assign(x, code, cn=None):
    """(idx int32 [n], dist fp64 [n]): the codeword of least fp64 score, the lowest index on ties; dist = max(0, |x|^2 + s)."""
    x = np.asarray(x, dtype=np.float64)
    s = scores(x, code, cn)
    idx = s.argmin(1).astype(np.int32)                           # argmin: the first least entry
    return idx, np.maximum(0.0, (x * x).sum(1) + s[np.arange(len(x)), idx])


def bound(x, code, cn=None):
    """B_i [n]: what any fp32 evaluation of the score of row i may err by, whatever the order and the fusing."""
    x, c = np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(code, dtype=np.float64))
    E = x.shape[1]
    gamma = E * U / (1.0 - E * U)
    cn = (c * c).sum(1) if cn is None else np.abs(np.asarray(cn, dtype=np.float64))
    return ((2.0 * gamma + 2.0 ** -22) * (x @ c.T) + 2.0 ** -23 * cn[None, :]).max(1)


def near_rows(x, code, cn=None):
    """Rows whose fp64 gap between best and second best is within 2 B_i (every row when K == 1 has an infinite gap)."""
    s = np.sort(scores(x, code, cn), axis=1)
    gap = s[:, 1] - s[:, 0] if s.shape[1] > 1 else np.full(len(s), np.inf)
    return gap <= 2.0 * bound(x, code, cn)


def quantise(x, shift):
    """q(v) = (int64) rint(v 2^shift) in double, half to even."""
    return np.rint(np.asarray(x, dtype=np.float64) * 2.0 ** shift).astype(np.int64)


def accum(x, idx, K, shift):
    """(cnt int32 [K], sum int64 [K, E], bad): rows with idx outside [0, K) are skipped and counted."""
    idx = np.asarray(idx)
    ok = (idx >= 0) & (idx < K)
    cnt = np.bincount(idx[ok], minlength=K).astype(np.int32)
    s = np.zeros((K, np.asarray(x).shape[1]), dtype=np.int64)
    np.add.at(s, idx[ok], quantise(np.asarray(x)[ok], shift))
    return cnt, s, int((~ok).sum())


def update(code, cnt, s, shift):
    """(new code fp32, cnorm fp32, changed): the mean of a cluster; cnt <= 0 keeps the row."""
    old = np.asarray(code, dtype=np.float32)
    new = old.copy()
    for k in range(len(old)):
        if cnt[k] > 0:
            new[k] = (s[k].astype(np.float64) / np.float64(cnt[k]) * 2.0 ** -shift).astype(np.float32)
    return new, cnorm(new), int((new.view(np.uint32) != old.view(np.uint32)).any(1).sum())


def vq_shift(n, maxabs):
    """The largest shift <= 30 with n maxabs 2^shift < 2^61."""
    from fractions import Fraction
    s = 30
    while Fraction(float(maxabs)) * int(n) * Fraction(2) ** s >= Fraction(2) ** 61:
        s -= 1
    return s


def init_rows(x, K, seed):
    """The first K pairwise different rows along RandomState(seed).permutation(n): their indices."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    seen, out = set(), []
    for i in np.random.RandomState(seed).permutation(len(x)):
        key = x[i].tobytes()
        if key not in seen:
            seen.add(key)
            out.append(int(i))
            if len(out) == K:
                return np.asarray(out, dtype=np.int64)
    raise ValueError('%d distinct rows, fewer than K = %d' % (len(seen), K))


def reseed(cnt, dist):
    """(empty k in increasing order, the rows they take): the rows of largest dist, ties to the lowest row, each row once."""
    empties = np.flatnonzero(np.asarray(cnt) == 0)
    order = np.argsort(-np.asarray(dist, dtype=np.float64), kind='stable')[:len(empties)]
    return empties, order


def fit(x, K, iters=40, seed=0):
    """k-means.  Returns (code, history [(sum dist, moved, empties)], per iteration dict(start, idx, code, near)).  Per iteration:
    assign against the fp64 scores, accumulate, update, reseed the empty clusters; stop at moved == 0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    shift = vq_shift(len(x), np.abs(x).max())
    code = x[init_rows(x, K, seed)].copy()
    prev = np.full(len(x), -1, dtype=np.int32)
    history, steps = [], []
    for _ in range(iters):
        start = code.copy()
        idx, dist = assign(x, code)
        near = int(near_rows(x, code).sum())
        moved = int((idx != prev).sum())
        prev = idx
        cnt, s, _ = accum(x, idx, K, shift)
        code, _, _ = update(code, cnt, s, shift)
        empties, rows = reseed(cnt, dist)
        for k, i in zip(empties, rows):
            code[k] = x[i]
        history.append((float(dist.sum()), moved, int(len(empties))))
        steps.append(dict(start=start, idx=idx, code=code.copy(), near=near))
        if moved == 0:
            break
    return code, history, steps


def gather(idx, code, start, length, T, ld, n_idx=None):
    """zs_vq_gather in fp32 [n_frag, T, ld] and the count of bad indices."""
    idx, code = np.asarray(idx), np.asarray(code, dtype=np.float32)
    n_idx = len(idx) if n_idx is None else n_idx
    K, E = code.shape
    out = np.zeros((len(start), T, ld), dtype=np.float32)
    bad = 0
    for f, (s, l) in enumerate(zip(start, length)):
        if not (0 <= l <= T and s >= 0 and s + l <= n_idx):
            continue
        for t in range(l):
            k = idx[s + t]
            if 0 <= k < K:
                out[f, t, :E] = code[k]
            else:
                bad += 1
    return out, bad
