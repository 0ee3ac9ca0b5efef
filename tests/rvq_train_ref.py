"""The definition of one training iteration through the residual codebook, numpy and Python integers only: what
zs_rvq_commit, zs_rvq_loss, zs_rvq_st_bwd and zs_amd.rvq_train.RvqBottleneck are tested against.  Every fp32 result is one IEEE
operation and one rounding, as include/zs_amd.h writes them, so the kernels are compared bit for bit; nothing here shares code with
the product.  The assignment and the fixed-point sums are tests/vq_ref.py's, the codebook's average tests/vq_train_ref.py's, the
restart tests/vq_restart_ref.py's and the Decoder's operand tests/rvq_ref.py's reconstruct."""
import numpy as np

import rvq_ref as Q
import vq_ref as R
import vq_restart_ref as X
import vq_train_ref as T

F32, F64 = np.float32, np.float64
MAX_ABS = T.MAX_ABS
GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def commit(x, idx, code, a=None):
    """One stage: x fp32 [n, E] is the stage's input r_s (a bf16 operand: its widened values), a the running sum of the residuals
    behind it (None at the first stage).  Returns dict(r, a, idx_acc, sq, bad, over): r = fl32(x - code[idx]), a' = r at the first
    stage and fl32(a + r) behind it, sq the double sum of the stored r squared.  A row whose idx is outside [0, K) is never used as
    an index: it passes unsubtracted, adds nothing to sq or to a (zero at the first stage), and its idx_acc is -1; so is that of a row
    of x with an element that is not of magnitude < MAX_ABS."""
    x, code, idx = np.asarray(x, dtype=F32), np.asarray(code, dtype=F32), np.asarray(idx).astype(np.int64)
    ok = (idx >= 0) & (idx < len(code))
    r = x.copy()
    r[ok] = x[ok] - code[idx[ok]]                                 # float32 - float32: one rounding
    assert r.dtype == F32
    new = np.zeros_like(x) if a is None else np.array(a, dtype=F32)
    new[ok] = r[ok] if a is None else (new[ok] + r[ok])
    assert new.dtype == F32
    with np.errstate(invalid='ignore'):
        big = ~(np.abs(x) < F32(MAX_ABS)).all(axis=1)
    d = r[ok].astype(F64)
    with np.errstate(over='ignore', invalid='ignore'):
        sq = float((d * d).sum())
    return dict(r=r, a=new, idx_acc=np.where(ok & ~big, idx, -1).astype(np.int32), sq=sq, bad=int((~ok).sum()), over=int(big.sum()))


def cascade(z, codes, idxs=None):
    """Every stage of the rows z (fp32 values).  idxs: the assignment to use per stage (the fp64 argmin of vq_ref.assign of the
    stage's own input when None).  Returns dict(idx [S, n], r: [r_0 = z, .., r_S], a = a_S, idx_acc [S, n], sq [S], bad, over)."""
    r, a, out = np.asarray(z, dtype=F32), None, dict(idx=[], r=[], idx_acc=[], sq=[], bad=0, over=0)
    for s, code in enumerate(codes):
        idx = R.assign(r, code, R.cnorm(code))[0] if idxs is None else np.asarray(idxs[s])
        c = commit(r, idx, code, a)
        out['idx'].append(np.asarray(idx).astype(np.int32))
        out['r'].append(r)
        out['idx_acc'].append(c['idx_acc'])
        out['sq'].append(c['sq'])
        out['bad'] += c['bad']
        out['over'] += c['over']
        r, a = c['r'], c['a']
    out['r'].append(r)
    out['a'] = a
    out['idx'], out['idx_acc'] = np.stack(out['idx']), np.stack(out['idx_acc'])
    return out


def losses(sq, beta, rows, E):
    """(loss_vq, [per stage]) in double: beta / (rows E) times the stages' sums, added in increasing stage."""
    scale = beta / (float(rows) * E)
    total = 0.0
    for v in sq:
        total = total + v
    return scale * total, [scale * v for v in sq]


def grad_scale(beta, rows, E):
    return F32(2.0 * beta / (float(rows) * E))


def st_bwd(dq, a, g, bf16=False):
    """dz = cast(dq + g * a): the product and the sum are fp32 operations with a rounding each, then the cast."""
    dq, a = np.asarray(dq, dtype=F32), np.asarray(a, dtype=F32)
    t = F32(g) * a
    out = dq + t
    assert t.dtype == F32 and out.dtype == F32
    return T.cast(out, bf16)


def operand(codes, idxs, ld, bf16=False):
    """(q fp32 [n, ld], bad frames): what the Decoder reads -- rvq_ref.reconstruct of every stage, zero behind E."""
    q, bad = Q.reconstruct(np.asarray(idxs), [np.asarray(c, dtype=F32) for c in codes], None, bf16)
    out = np.zeros((q.shape[0], ld), dtype=F32)
    out[:, :q.shape[1]] = q
    return out, bad


def stage_seed(seed, s):
    return (int(seed) + s * GOLDEN) & M64


class State(object):
    """The bottleneck's state from a starting residual codebook: per stage a vq_train_ref.State (code = vectors[s], N = 1, m = code)."""

    def __init__(self, vectors):
        self.stages = [T.State(v) for v in np.asarray(vectors, dtype=F32)]

    def codes(self):
        return [st.code.copy() for st in self.stages]


def iteration(state, z, dq, beta, decay, shift, ld, bf16=False, idxs=None, restart=None, seed=0, seed_dev=0, stride=None):
    """One training iteration on rows z (values exact in the activation type): dict(idx, q, loss_vq, loss_stage, dz, r, a, idx_acc,
    used, restarted); `state` moves to the next codebooks.  Every stage reads the codebook the step before left."""
    z = np.asarray(z, dtype=F32)
    codes = state.codes()
    c = cascade(z, codes, idxs)
    q, _ = operand(codes, c['idx'], ld, bf16)
    n, E = z.shape
    lv, per = losses(c['sq'], beta, n, E)
    dz = st_bwd(dq, c['a'], grad_scale(beta, n, E), bf16)
    used, restarted = [], 0
    for s, st in enumerate(state.stages):
        cnt, sums, _ = R.accum(c['r'][s], c['idx_acc'][s], len(st.code), shift)
        st.N, st.m, st.code, st.cnorm, u = T.ema(st.N, st.m, st.code, cnt, sums, shift, decay)
        used.append(u)
        if restart is not None:
            (st.N, st.m, st.code, st.cnorm), got, _, _ = X.restart(restart, c['r'][s], c['idx_acc'][s], cnt, st.N, st.m, st.code, st.cnorm,
                                                                   stage_seed(seed, s), seed_dev, stride)
            restarted += got
    return dict(idx=c['idx'], q=q, loss_vq=lv, loss_stage=per, dz=dz, r=c['r'], a=c['a'], idx_acc=c['idx_acc'], used=used, restarted=restarted)
