"""The definition of one training iteration through the vector codebook, numpy only: what zs_vq_commit, zs_vq_st_bwd,
zs_vq_ema and zs_amd.vq_train.VqBottleneck are tested against.  Every fp32 result is one IEEE operation and one rounding, as
include/zs_amd.h writes them, so the kernels are compared bit for bit; nothing here shares code with them.  The assignment, the
fixed-point sums and the planted inputs are tests/vq_ref.py's."""
import numpy as np

import vq_ref as R

MAX_ABS = 65536.0
MIN_COUNT = 1e-3
F32, F64 = np.float32, np.float64


def bf16_round(x):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32; finite inputs."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(F32)


def cast(x, bf16):
    return bf16_round(x) if bf16 else np.asarray(x, dtype=F32)


def quantise(code, idx, ld, bf16=False):
    """(q fp32 [n, ld] holding the cast codewords, zero behind E and in rows whose idx is outside [0, K); bad)."""
    code, idx = np.asarray(code, dtype=F32), np.asarray(idx)
    K, E = code.shape
    ok = (idx >= 0) & (idx < K)
    q = np.zeros((len(idx), ld), dtype=F32)
    q[ok, :E] = cast(code[idx[ok]], bf16)
    return q, int((~ok).sum())


def loss_vq(z, code, idx, beta):
    """beta / (rows E) * sum (z - code[idx])^2 in double over the rows whose idx is inside [0, K); rows counts every row."""
    z, code, idx = np.asarray(z, dtype=F64), np.asarray(code, dtype=F64), np.asarray(idx)
    ok = (idx >= 0) & (idx < len(code))
    d = z[ok] - code[idx[ok]]
    return beta / (float(z.shape[0]) * z.shape[1]) * float((d * d).sum())


def grad_scale(beta, rows, E):
    return F32(2.0 * beta / (float(rows) * E))


def st_bwd(dq, z, code, idx, g, bf16=False):
    """dz = cast(dq + g * (z - code[idx])): three fp32 operations, a rounding each; a row whose idx is outside [0, K) passes dq."""
    dq, z, code, idx = np.asarray(dq, dtype=F32), np.asarray(z, dtype=F32), np.asarray(code, dtype=F32), np.asarray(idx)
    ok = (idx >= 0) & (idx < len(code))
    out = dq.copy()
    d = (z[ok] - code[idx[ok]]).astype(F32)
    t = (F32(g) * d).astype(F32)
    out[ok] = (dq[ok] + t).astype(F32)
    return cast(out, bf16), int((~ok).sum())


def acc_index(z, idx):
    """(the idx zs_vq_accum is given, rows over): a row with an element that is not of magnitude < MAX_ABS, or whose idx is
    outside [0, K) as far as the caller knows K, becomes -1 and is not accumulated."""
    z = np.asarray(z, dtype=F32)
    big = ~(np.abs(z) < F32(MAX_ABS)).all(axis=1)
    return np.where(big, -1, np.asarray(idx)).astype(np.int32), int(big.sum())


def norm_as_update(code):
    """cnorm as zs_vq_update and zs_vq_ema write it: lane t of 256 adds code[k][j]^2 for j = t, t + 256, .. in double, a wave's 64
    lanes are added pairwise at distances 32, 16, .., 1, and the four waves left to right; one rounding to fp32."""
    c = np.asarray(code, dtype=F64)
    K, E = c.shape
    rounds = (E + 255) // 256
    sq = np.zeros((K, rounds * 256), dtype=F64)
    sq[:, :E] = c * c                                            # exact: 24-bit factors
    lane = np.zeros((K, 256), dtype=F64)
    for r in range(rounds):
        lane = lane + sq[:, 256 * r:256 * (r + 1)]
    w = lane.reshape(K, 4, 64)
    ids = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, ids ^ o]
    s = w[:, :, 0]
    return (((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]).astype(F32)


def ema(N, m, code, cnt, s, shift, decay):
    """Expression 4: (N', m', code', cnorm', used).  Doubles, one fp32 rounding per stored value, nothing summed across k."""
    N, m, code = np.asarray(N, dtype=F32), np.asarray(m, dtype=F32), np.asarray(code, dtype=F32)
    cnt, s = np.asarray(cnt), np.asarray(s, dtype=np.int64)
    decay = F64(decay)
    keep = F64(1.0) - decay
    n_new = (decay * N.astype(F64) + keep * cnt.astype(F64)).astype(F32)
    m_new = (decay * m.astype(F64) + (keep * s.astype(F64)) * F64(2.0) ** -shift).astype(F32)
    new = code.copy()
    live = n_new.astype(F64) >= MIN_COUNT
    with np.errstate(divide='ignore', invalid='ignore'):
        new[live] = (m_new[live].astype(F64) / n_new[live].astype(F64)[:, None]).astype(F32)
    return n_new, m_new, new, norm_as_update(new), int((cnt > 0).sum())


class State(object):
    """The bottleneck's state from a starting codebook: code = vectors, N = 1, m = code."""

    def __init__(self, vectors):
        self.code = np.array(vectors, dtype=F32)
        self.cnorm = R.cnorm(self.code)
        self.N = np.ones(len(self.code), dtype=F32)
        self.m = self.code.copy()

    def step(self, z, idx, shift, decay):
        """The codebook's average for the rows z (fp32 values) under the assignment idx; returns (cnt, used)."""
        ia, _ = acc_index(z, idx)
        cnt, s, _ = R.accum(z, ia, len(self.code), shift)
        self.N, self.m, self.code, self.cnorm, used = ema(self.N, self.m, self.code, cnt, s, shift, decay)
        return cnt, used


def iteration(state, z, dq, beta, decay, shift, ld, bf16=False, idx=None):
    """One training iteration on rows z (values exact in the activation type): dict(idx, q, loss_vq, dz); `state` moves to the next
    codebook.  idx: the assignment to use (the fp64 argmin of vq_ref.assign when None)."""
    z = np.asarray(z, dtype=F32)
    code = state.code.copy()                                     # the codebook the step before left: every term below reads it
    if idx is None:
        idx, _ = R.assign(z, code, state.cnorm)
    q, _ = quantise(code, idx, ld, bf16)
    lv = loss_vq(z, code, idx, beta)
    dz, _ = st_bwd(dq, z, code, idx, grad_scale(beta, *z.shape), bf16)
    state.step(z, idx, shift, decay)
    return dict(idx=idx, q=q, loss_vq=lv, dz=dz)
