"""The definition of quantiser dropout in training through the residual codebook, numpy and Python integers only: what
zs_rvq_drop_draw, zs_rvq_commit_drop, zs_rvq_gather_frag and RvqBottleneck(dropout=P) are tested against.  The notation is
tests/rvq_train_ref.py's: rows are i = b T' + t, and act_s(i) = s < s_use[b(i)].  An active row is rvq_train_ref.commit's row, bit for
bit; an inactive one passes its fp32 value on, leaves a alone, has idx_acc -1 and counts nowhere.  Nothing here shares code with the
product."""
import numpy as np

import rvq_ref as Q
import rvq_train_ref as RT
import vq_ref as R
import vq_restart_ref as X
import vq_train_ref as T

F32, F64 = np.float32, np.float64
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
SALT = 0x5256515F44524F50           # "RVQ_DROP": ZS_RVQ_DROP_SALT
THR_ONE = 1 << 24


def mix64(z):
    """include/zs_amd.h's, under zs_vq_restart: wrapping unsigned 64-bit."""
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def threshold(P):
    """thr = floor(P 2^24), an integer; P = 1 gives 2^24."""
    return int(np.floor(float(P) * THR_ONE))


def u_of(seed, seed_dev, b):
    return mix64((int(seed) + int(seed_dev) + SALT + b * GOLDEN) & M64)


def count_of(u, thr, S):
    """s_use of one sample from its 64 random bits: the top 24 decide whether it drops, the low 32 how far."""
    return 1 + (u & 0xFFFFFFFF) % S if (u >> 40) < thr else S


def draw(seed, seed_dev, B, S, thr):
    """s_use int32 [B]; seed_dev is the word at seed_ptr (0 without one)."""
    return np.array([count_of(u_of(seed, seed_dev, b), thr, S) for b in range(B)], dtype=np.int32)


def active(s_use, S, Tq):
    """active[s] = T' * #{b : s_use[b] > s}."""
    s_use = np.asarray(s_use)
    return np.array([Tq * int((s_use > s).sum()) for s in range(S)], dtype=np.int32)


def row_mask(s_use, Tq, n, stage):
    """act_stage(i) for the n rows i = b T' + t."""
    return np.asarray(s_use)[np.arange(n) // Tq] > stage


def commit(x, idx, code, a, act):
    """One stage with the rows act [n] taking part: rvq_train_ref.commit on those rows alone (their values are row-wise, so the
    other rows do not matter to them); the others copy x to r, keep a (None at the first stage: they stay unwritten, NaN here), have
    idx_acc -1, and add nothing to sq, bad or over.  The sum of squares is over the active rows in the reference's double."""
    x, act = np.asarray(x, dtype=F32), np.asarray(act, dtype=bool)
    n = len(x)
    r = x.copy()
    new = np.full_like(x, np.nan) if a is None else np.array(a, dtype=F32)
    ia = np.full(n, -1, dtype=np.int32)
    sq, bad, over = 0.0, 0, 0
    if act.any():
        c = RT.commit(x[act], np.asarray(idx)[act], code, None if a is None else new[act])
        r[act], new[act], ia[act] = c['r'], c['a'], c['idx_acc']
        sq, bad, over = c['sq'], c['bad'], c['over']
    return dict(r=r, a=new, idx_acc=ia, sq=sq, bad=bad, over=over)


def cascade(z, codes, s_use, Tq, idxs=None):
    """Every stage of the rows z under the counts s_use [B] (n = B T').  zs_vq_assign runs on all rows at every stage: idx [S, n] is
    complete, whatever took part.  Returns rvq_train_ref.cascade's dict."""
    r, a, out = np.asarray(z, dtype=F32), None, dict(idx=[], r=[], idx_acc=[], sq=[], bad=0, over=0)
    n = len(r)
    for s, code in enumerate(codes):
        idx = R.assign(r, code, R.cnorm(code))[0] if idxs is None else np.asarray(idxs[s])
        c = commit(r, idx, code, a, row_mask(s_use, Tq, n, s))
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


def operand(codes, idxs, s_use, Tq, ld, bf16=False):
    """(q fp32 [n, ld], bad frames): fragment b is rvq_ref.reconstruct of its own rows with its own count; a count outside [1, S] gives
    zero rows and a bad frame each, and none of that fragment's indices is looked at."""
    idxs = np.asarray(idxs)
    S, n = idxs.shape
    E = codes[0].shape[1]
    out = np.zeros((n, ld), dtype=F32)
    bad = 0
    for b, su in enumerate(np.asarray(s_use).tolist()):
        lo, hi = b * Tq, (b + 1) * Tq
        if not 1 <= su <= S:
            bad += Tq
            continue
        q, k = Q.reconstruct(idxs[:, lo:hi], [np.asarray(c, dtype=F32) for c in codes], su, bf16)
        out[lo:hi, :E] = q
        bad += k
    return out, bad


def iteration(state, z, dq, beta, decay, shift, ld, Tq, s_use, bf16=False, idxs=None, restart=None, seed=0, seed_dev=0, stride=None):
    """rvq_train_ref.iteration under the counts s_use: the loss and the gradient are scaled over all n rows (a masked mean), and the
    accumulation, the average and the restart are the unchanged ones, which leave idx_acc < 0 rows out."""
    z = np.asarray(z, dtype=F32)
    codes = state.codes()
    c = cascade(z, codes, s_use, Tq, idxs)
    q, _ = operand(codes, c['idx'], s_use, Tq, ld, bf16)
    n, E = z.shape
    lv, per = RT.losses(c['sq'], beta, n, E)
    dz = RT.st_bwd(dq, c['a'], RT.grad_scale(beta, n, E), bf16)
    used, restarted, skipped = [], 0, 0
    for s, st in enumerate(state.stages):
        cnt, sums, _ = R.accum(c['r'][s], c['idx_acc'][s], len(st.code), shift)
        st.N, st.m, st.code, st.cnorm, u = T.ema(st.N, st.m, st.code, cnt, sums, shift, decay)
        used.append(u)
        if restart is not None:
            (st.N, st.m, st.code, st.cnorm), got, skip, _ = X.restart(restart, c['r'][s], c['idx_acc'][s], cnt, st.N, st.m, st.code, st.cnorm,
                                                                      RT.stage_seed(seed, s), seed_dev, stride)
            restarted += got
            skipped += skip
    return dict(idx=c['idx'], q=q, loss_vq=lv, loss_stage=per, dz=dz, r=c['r'], a=c['a'], idx_acc=c['idx_acc'], used=used, restarted=restarted,
                skipped=skipped, active=active(s_use, len(codes), Tq))
