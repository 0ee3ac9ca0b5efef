"""The definition of the residual vector codebook, numpy only: what zs_rvq_residual / zs_rvq_gather and zs_amd.rvq are tested against.
Every stage's search is tests/vq_ref.py's; what is added here is the one fp32 subtraction between the stages, the reconstruction as
fp32 adds in increasing stage with one cast behind them, and the greedy fit on top of vq_ref's k-means.  Nothing here shares code with
the product."""
import numpy as np

import vq_ref as R


def to_bf16(x):
    """fp32 -> the fp32 value of its bf16 rounding, to nearest even (finite values)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def residual(x, idx, code):
    """(r fp32 [n, E], bad): r = fl32(x - code[idx]), one IEEE subtraction per element; a row whose idx is outside [0, K) is copied and
    counted.  x holds fp32 values (a bf16 operand: its widened values)."""
    x, code, idx = np.asarray(x, dtype=np.float32), np.asarray(code, dtype=np.float32), np.asarray(idx).astype(np.int64)
    ok = (idx >= 0) & (idx < len(code))
    r = x.copy()
    r[ok] = x[ok] - code[idx[ok]]                                 # float32 - float32: one rounding
    assert r.dtype == np.float32
    return r, int((~ok).sum())


def snap_given(x, codes, idxs):
    """The residuals [r_0 = x, r_1, ..] of the rows x under given per-stage indices (one more than the stages given)."""
    rs = [np.asarray(x, dtype=np.float32)]
    for code, idx in zip(codes, idxs):
        rs.append(residual(rs[-1], idx, code)[0])
    return rs


def snap(x, codes):
    """(idx [S, n], dist fp64 [S, n], residuals): every stage assigned against the fp64 scores (vq_ref.assign) of its input."""
    r, idxs, dists, rs = np.asarray(x, dtype=np.float32), [], [], []
    for code in codes:
        rs.append(r)
        idx, dist = R.assign(r, code, R.cnorm(code))
        idxs.append(idx)
        dists.append(dist)
        r = residual(r, idx, code)[0]
    return np.stack(idxs), np.stack(dists), rs + [r]


def reconstruct(idxs, codes, s_use=None, bf16=False):
    """(q fp32 [n, E], bad): ((code_0[k_0] + code_1[k_1]) + ..) + code_{s'-1}[k_{s'-1}], fp32 adds in increasing stage, one cast behind
    them (bf16: to nearest even, returned at its fp32 value).  A frame with any used index outside [0, K) is a zero row, counted
    once; no index of it is used."""
    idxs = np.asarray(idxs).astype(np.int64)
    s_use = len(idxs) if s_use is None else s_use
    K = codes[0].shape[0]
    ok = np.ones(idxs.shape[1], dtype=bool)
    for s in range(s_use):
        ok &= (idxs[s] >= 0) & (idxs[s] < K)
    q = np.zeros((idxs.shape[1], codes[0].shape[1]), dtype=np.float32)
    if ok.any():
        acc = np.asarray(codes[0], dtype=np.float32)[idxs[0][ok]]
        for s in range(1, s_use):
            acc = acc + np.asarray(codes[s], dtype=np.float32)[idxs[s][ok]]
            assert acc.dtype == np.float32
        q[ok] = acc
    return (to_bf16(q) if bf16 else q), int((~ok).sum())


def gather(idxs, codes, s_use, start, length, T, ld, bf16=False, n_idx=None):
    """zs_rvq_gather [n_frag, T, ld] (at fp32 values) and the count of bad frames: idxs [S, n_idx] planes."""
    idxs = np.asarray(idxs)
    n_idx = idxs.shape[1] if n_idx is None else n_idx
    E = codes[0].shape[1]
    out = np.zeros((len(start), T, ld), dtype=np.float32)
    bad = 0
    for f, (s, l) in enumerate(zip(start, length)):
        if not (0 <= l <= T and s >= 0 and s + l <= n_idx):
            continue
        q, b = reconstruct(idxs[:, s:s + l], codes, s_use, bf16)
        out[f, :l, :E] = q
        bad += b
    return out, bad


def fit(x, K, S, iters=40, seed=0):
    """The greedy fit on vq_ref's k-means: stage s is vq_ref.fit(r_s, K, iters, seed + s); the rows are assigned again under the
    fitted codebook and the residual goes on.  Returns (codes, per stage dict(rows, code, idx, dist, history, near))."""
    r, codes, stages = np.ascontiguousarray(x, dtype=np.float32), [], []
    for s in range(S):
        code, history, steps = R.fit(r, K, iters=iters, seed=seed + s)
        idx, dist = R.assign(r, code, R.cnorm(code))
        near = max([st['near'] for st in steps] + [int(R.near_rows(r, code, R.cnorm(code)).sum())])      # in any assignment of the stage
        stages.append(dict(rows=r, code=code, idx=idx, dist=dist, history=history, near=near))
        codes.append(code)
        r = residual(r, idx, code)[0]
    return codes, stages


def planted2(n, E, K0, sigma, seed):
    """A planted mixture of two scales: coarse centres with fine offsets around them (vq_ref.planted twice): rows = coarse + 0.1 fine."""
    return (R.planted(n, E, K0, 0.0, seed) + np.float32(0.1) * R.planted(n, E, K0, sigma, seed + 1)).astype(np.float32)
