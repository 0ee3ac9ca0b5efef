"""Training through the vector codebook on the device:

* zs_vq_commit, zs_vq_st_bwd and zs_vq_ema against the numpy definition of tests/vq_train_ref.py, bit for bit (the loss within 1e-6
  of fp64), on the smallest shapes that cross ZS_VQ_TILE_K = 128, the 128-row workgroup, an E that is no multiple of 8, ld > E and
  ZS_CODE_MAX_E, in fp32 and bf16; bad indices, rows above ZS_VQ_MAX_ABS and every ZS_EINVAL case with guards around every output;
* one AEStep iteration with the bottleneck against the oracle's torch modules under autograd (the quantiser as z + (q - z).detach()
  plus the commitment term, fed the device's idx), eager against captured over 5 iterations, the codebook's fixed point with
  frozen weights, the step without a bottleneck launching no zs_vq_* entry point, and main.py --vq_train end to end."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import vq_ref as R  # noqa: E402
import vq_train_ref as T  # noqa: E402

GUARD = 64
FILL_I = -0x55555556
SEED = 1                                                          # (n, E, K) below have no near row at seeds 0, 1, 2 in fp32
SHAPES = [(48, 8, 1), (37, 6, 5), (256, 20, 37), (300, 64, 300), (130, 1024, 129)]
LD = {8: 16, 6: 8, 20: 24, 64: 72, 1024: 1024}                    # the operand's pitch: a whole padding piece, a partial one, none


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pitched(rows, ld, fill):
    n, E = rows.shape
    buf = np.full(n * ld + GUARD, fill, dtype=np.float32)
    buf[:n * ld].reshape(n, ld)[:, :E] = rows
    return buf


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _case(n, E, K, bf16, seed=SEED):
    x, code = R.planted(n, E, 8, 0.3, seed), R.planted(K, E, 8, 0.3, seed + 100)
    return (T.bf16_round(x) if bf16 else x), code


def _device_idx(dev, x, code, bf16):
    """zs_vq_assign's idx for the rows x, checked against the fp64 argmin on every row that is not near."""
    from zs_amd import vq as V
    cn = R.cnorm(code)
    x_d = torch.from_numpy(x).to(dev).to(torch.bfloat16 if bf16 else torch.float32)
    idx = torch.full((len(x),), -1, dtype=torch.int32, device=dev)
    V.assign(x_d, torch.from_numpy(code).to(dev), torch.from_numpy(cn).to(dev), idx=idx, work=V.workspace(dev))
    idx = idx.cpu().numpy()
    near = R.near_rows(x, code, cn)
    assert near.sum() <= 0.01 * len(x), 'bad input: %d of %d rows are near' % (near.sum(), len(x))
    want, _ = R.assign(x, code, cn)
    assert np.array_equal(idx[~near], want[~near]) and idx.min() >= 0 and idx.max() < len(code)
    return idx


def _commit(dev, x, idx, code, ld_z, ld_q, ld_code, bf16, beta=0.25, skip=()):
    """zs_vq_commit with guards behind every output; returns numpy results and asserts the guards and the read-only operands."""
    from zs_amd import _lib as L
    n, E = x.shape
    K = code.shape[0]
    dt = torch.bfloat16 if bf16 else torch.float32
    zb, cb = _pitched(x, ld_z, np.nan), _pitched(code, ld_code, np.nan)
    z_d, c_d = torch.from_numpy(zb).to(dev).to(dt), torch.from_numpy(cb).to(dev)
    ib = np.concatenate([np.asarray(idx, np.int32), np.full(GUARD, FILL_I, np.int32)])
    i_d = torch.from_numpy(ib).to(dev)
    q_d = torch.full((n * ld_q + GUARD,), 9.0, dtype=dt, device=dev)
    f_d = torch.full((n * E + GUARD,), 9.0, device=dev)
    ia = torch.full((n + GUARD,), FILL_I, dtype=torch.int32, device=dev)
    part = torch.full((L.ZS_VQ_COMMIT_PARTS + GUARD,), -1.0, dtype=torch.float64, device=dev)
    loss = torch.full((2,), -7.0, device=dev)
    stat = torch.full((4,), 7, dtype=torch.int32, device=dev)
    kw = dict(dtype=(L.ZS_BF16 if bf16 else L.ZS_F32), z=L.ptr(z_d), n=n, ld_z=ld_z, idx=L.ptr(i_d), code=L.ptr(c_d), ld_code=ld_code, K=K, E=E,
              q=L.ptr(q_d), ld_q=ld_q, z_f32=L.ptr(f_d), ld_zf=E, idx_acc=L.ptr(ia), scale=beta / (float(n) * E), partial=L.ptr(part),
              loss=L.ptr(loss), bad=L.ptr(stat), over=L.ptr(stat, 1))
    for k in skip:
        kw[k] = None
    L.call('zs_vq_commit', 'ZsVqCommit', _stream(), **kw)
    torch.cuda.synchronize()
    assert (q_d[n * ld_q:] == 9.0).all() and (f_d[n * E:] == 9.0).all() and (ia[n:] == FILL_I).all()
    assert (part[L.ZS_VQ_COMMIT_PARTS:] == -1.0).all() and float(loss[1]) == -7.0 and (stat[2:] == 7).all()
    assert np.array_equal(c_d.cpu().numpy(), cb, equal_nan=True) and np.array_equal(i_d.cpu().numpy(), ib)
    assert np.array_equal(z_d.float().cpu().numpy(), zb, equal_nan=True)
    return dict(q=q_d[:n * ld_q].float().cpu().numpy().reshape(n, ld_q), z_f32=f_d[:n * E].cpu().numpy().reshape(n, E),
                idx_acc=ia[:n].cpu().numpy(), loss=float(loss[0]), bad=int(stat[0]) - 7, over=int(stat[1]) - 7)


# ---- zs_vq_commit --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('n,E,K', SHAPES)
def test_commit_equals_the_definition(dev, n, E, K, bf16):
    x, code = _case(n, E, K, bf16)
    idx = _device_idx(dev, x, code, bf16)
    want_q, _ = T.quantise(code, idx, LD[E], bf16)
    want_loss = T.loss_vq(x, code, idx, 0.25)
    ld_alt = E + (9 if bf16 else 5)                               # rows at no 16-byte pitch: the element-wise loads
    for ld_z, ld_code in ((LD[E], E), (ld_alt, E + 1)):
        got = _commit(dev, x, idx, code, ld_z, LD[E], ld_code, bf16)
        assert np.array_equal(_bits(got['q']), _bits(want_q)) and (got['q'][:, E:] == 0).all()
        assert np.array_equal(_bits(got['z_f32']), _bits(x))
        assert np.array_equal(got['idx_acc'], idx) and got['bad'] == 0 and got['over'] == 0
        rel = abs(got['loss'] - want_loss) / want_loss
        print('n %d E %d K %d bf16 %d ld_z %d: loss_vq %.9g, fp64 %.9g, relative error %.3g' % (n, E, K, bf16, ld_z, got['loss'], want_loss, rel))
        assert rel <= 1e-6
    none = _commit(dev, x, idx, code, LD[E], LD[E], E, bf16, skip=('z_f32', 'idx_acc', 'over', 'loss', 'partial'))
    assert np.array_equal(_bits(none['q']), _bits(want_q)) and (none['z_f32'] == 9.0).all() and (none['idx_acc'] == FILL_I).all()
    assert none['loss'] == -7.0


@pytest.mark.parametrize('bf16', [False, True])
def test_commit_bad_indices_and_rows_above_the_bound(dev, bf16):
    """An idx outside [0, K) is never an index (2^30 would be far outside the codebook): a zero row, left out of the loss, counted.  A
    row with an element of magnitude >= 65536, infinite or NaN is quantised like any other, counted, and handed to zs_vq_accum as -1."""
    n, E, K = 300, 64, 300
    x, code = _case(n, E, K, bf16)
    idx = _device_idx(dev, x, code, bf16).copy()
    idx[3], idx[5], idx[130], idx[299] = K, -1, 2 ** 30, -2 ** 31
    x = x.copy()
    x[9, 2], x[11, 63], x[200, 0], x[5, 1] = 65536.0, -np.inf, -70000.0 if not bf16 else -70144.0, np.nan      # (row 5: bad as well)
    x[12, 7] = 65280.0                                            # below the bound (exact in bf16): kept
    got = _commit(dev, x, idx, code, LD[E], LD[E], E, bf16)
    want_q, bad = T.quantise(code, idx, LD[E], bf16)
    ia, over = T.acc_index(x, idx)
    ia[[3, 5, 130, 299]] = -1
    assert bad == 4 and over == 4 and got['bad'] == 4 and got['over'] == 4
    assert np.array_equal(_bits(got['q']), _bits(want_q)) and (got['q'][[3, 5, 130, 299]] == 0).all()
    assert np.array_equal(got['idx_acc'], ia) and (ia == -1).sum() == 7
    assert np.array_equal(_bits(got['z_f32']), _bits(x))
    ok = np.ones(n, bool)
    ok[11] = False                                               # (the infinite row makes the loss infinite: take it out of the comparison)
    assert got['loss'] == np.inf
    x[11, 63] = 0.0
    got = _commit(dev, x, idx, code, LD[E], LD[E], E, bf16)
    want = T.loss_vq(x, code, idx, 0.25)
    assert abs(got['loss'] - want) <= 1e-6 * want and got['over'] == 3


# ---- zs_vq_st_bwd --------------------------------------------------------------------------------------------------------------------
def _st_bwd(dev, dq, x, idx, code, g, ld_dq, ld_dz, ld_z, ld_code, bf16, in_place):
    from zs_amd import _lib as L
    n, E = x.shape
    K = code.shape[0]
    dt = torch.bfloat16 if bf16 else torch.float32
    zb, cb = _pitched(x, ld_z, np.nan), _pitched(code, ld_code, np.nan)
    z_d, c_d = torch.from_numpy(zb).to(dev).to(dt), torch.from_numpy(cb).to(dev)
    i_d = torch.from_numpy(np.asarray(idx, np.int32)).to(dev)
    dq_d = torch.from_numpy(_pitched(dq, ld_dq, 5.0)).to(dev).to(dt)
    dz_d = dq_d if in_place else torch.full((n * ld_dz + GUARD,), 9.0, dtype=dt, device=dev)
    stat = torch.full((2,), 7, dtype=torch.int32, device=dev)
    L.call('zs_vq_st_bwd', 'ZsVqStBwd', _stream(), dtype=(L.ZS_BF16 if bf16 else L.ZS_F32), dq=L.ptr(dq_d), n=n, ld_dq=ld_dq, z=L.ptr(z_d),
           ld_z=ld_z, idx=L.ptr(i_d), code=L.ptr(c_d), ld_code=ld_code, K=K, E=E, g=float(g), dz=L.ptr(dz_d), ld_dz=ld_dz, bad=L.ptr(stat))
    torch.cuda.synchronize()
    assert (dz_d[n * ld_dz:] == (5.0 if in_place else 9.0)).all() and int(stat[1]) == 7
    assert np.array_equal(c_d.cpu().numpy(), cb, equal_nan=True) and np.array_equal(z_d.float().cpu().numpy(), zb, equal_nan=True)
    if not in_place:
        assert np.array_equal(dq_d.float().cpu().numpy(), T.cast(_pitched(dq, ld_dq, 5.0), bf16))
    return dz_d[:n * ld_dz].float().cpu().numpy().reshape(n, ld_dz), int(stat[0]) - 7


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('n,E,K', SHAPES)
def test_st_bwd_equals_the_definition_in_and_out_of_place(dev, n, E, K, bf16):
    """g of the step (2 beta / (n E), small against dq) and a large one, so that every one of the three roundings shows."""
    x, code = _case(n, E, K, bf16)
    idx = _device_idx(dev, x, code, bf16).copy()
    dq = T.cast(np.random.RandomState(n + E).standard_normal((n, E)).astype(np.float32), bf16)
    if n > 7:
        idx[7] = K                                                # a bad row passes dq
    for g in (T.grad_scale(0.25, n, E), np.float32(0.37)):
        want, bad = T.st_bwd(dq, x, code, idx, g, bf16)
        for in_place, ld_dq, ld_dz, ld_z, ld_code in ((False, LD[E], LD[E] + 8, LD[E], E), (True, LD[E], LD[E], E + (9 if bf16 else 5), E + 1)):
            got, n_bad = _st_bwd(dev, dq, x, idx, code, g, ld_dq, ld_dz, ld_z, ld_code, bf16, in_place)
            assert n_bad == bad == 1
            assert np.array_equal(_bits(got[:, :E]), _bits(want)), 'g %g in_place %d' % (g, in_place)
            assert (got[:, E:] == 0).all() and np.array_equal(_bits(got[7, :E]), _bits(dq[7]))
    moved = (want != dq).mean()
    print('n %d E %d K %d bf16 %d: %.3g of the elements differ from dq' % (n, E, K, bf16, moved))
    assert moved > 0.5


# ---- zs_vq_ema -----------------------------------------------------------------------------------------------------------------------
def _ema(dev, N, m, code, cnt, s, shift, decay, ld_code=None, used0=5):
    from zs_amd import _lib as L
    K, E = code.shape
    ld_code = ld_code or E
    g = np.full(GUARD, -3.0, np.float32)
    N_d = torch.from_numpy(np.concatenate([N, g])).to(dev)
    m_d = torch.from_numpy(np.concatenate([m.ravel(), g])).to(dev)
    c_d = torch.from_numpy(_pitched(code, ld_code, 0.125)).to(dev)
    cn = torch.full((K + GUARD,), -3.0, device=dev)
    used = torch.full((2,), used0, dtype=torch.int32, device=dev)
    cnt_d, s_d = torch.from_numpy(np.asarray(cnt, np.int32)).to(dev), torch.from_numpy(np.ascontiguousarray(s, np.int64)).to(dev)
    L.call('zs_vq_ema', 'ZsVqEma', _stream(), cnt=L.ptr(cnt_d), sum=L.ptr(s_d), K=K, E=E, shift=shift, decay=float(decay), N=L.ptr(N_d),
           m=L.ptr(m_d), code=L.ptr(c_d), ld_code=ld_code, cnorm=L.ptr(cn), used=L.ptr(used))
    torch.cuda.synchronize()
    out = c_d.cpu().numpy()
    new = out[:K * ld_code].reshape(K, ld_code)[:, :E].copy()
    assert np.array_equal(out, _pitched(new, ld_code, 0.125))              # the slack of a pitch and the guard are not touched
    assert (N_d[K:] == -3.0).all() and (m_d[K * E:] == -3.0).all() and (cn[K:] == -3.0).all() and int(used[1]) == used0
    assert np.array_equal(cnt_d.cpu().numpy(), cnt) and np.array_equal(s_d.cpu().numpy(), s)
    return N_d[:K].cpu().numpy(), m_d[:K * E].cpu().numpy().reshape(K, E), new, cn[:K].cpu().numpy(), int(used[0]) - used0


def _three_updates(dev, x, code, decay, ld_code=None, N0=None):
    """Three consecutive updates on one batch (the assignment follows the moving codebook); every array after every update bit for bit."""
    n, E = x.shape
    K = code.shape[0]
    shift = R.vq_shift(n, T.MAX_ABS)
    st = T.State(code)
    if N0 is not None:
        st.N = N0.copy()
    N, m, c = st.N.copy(), st.m.copy(), st.code.copy()
    cnts = []
    for t in range(3):
        idx, _ = R.assign(x, st.code, st.cnorm)
        cnt, s, _ = R.accum(x, idx, K, shift)
        N, m, c, cn, used = _ema(dev, N, m, c, cnt, s, shift, decay, ld_code)
        st.N, st.m, st.code, st.cnorm, w_used = T.ema(st.N, st.m, st.code, cnt, s, shift, decay)
        assert used == w_used == int((cnt > 0).sum())
        for name, a, b in (('N', N, st.N), ('m', m, st.m), ('code', c, st.code), ('cnorm', cn, st.cnorm)):
            assert np.array_equal(_bits(a), _bits(b)), 'update %d: %s differs in %d places' % (t, name, (_bits(a) != _bits(b)).sum())
        cnts.append(cnt)
    return cnts, st


@pytest.mark.parametrize('n,E,K', SHAPES)
def test_ema_equals_the_definition_over_three_updates(dev, n, E, K):
    x, code = _case(n, E, K, False)
    cnts, st = _three_updates(dev, x, code, 0.99, ld_code=E + 1)
    assert K == 1 or any((c == 0).any() for c in cnts)                     # an unused codeword decays
    _three_updates(dev, x, code, 0.5)


def test_ema_every_codeword_used_starved_codewords_and_decay_zero(dev):
    from zs_amd import _lib as L
    n, E, K = 300, 64, 300
    x = R.planted(n, E, 8, 0.3, SEED)
    code = x[R.init_rows(x, K, 0)]
    cnts, _ = _three_updates(dev, x, code, 0.99)
    assert (cnts[0] == 1).all()                                            # every codeword is used
    # N' < 1e-3 leaves the row as it is: codewords that start with a tiny count and take no row
    x2, code2 = _case(256, 20, 37, False)
    N0 = np.ones(37, np.float32)
    idx, _ = R.assign(x2, code2)
    unused = np.flatnonzero(np.bincount(idx, minlength=37) == 0)
    assert len(unused) >= 3
    N0[unused[:3]] = [1e-4, 9e-4, 1.02e-3]                                 # times 0.99: two below 1e-3, one above
    _, st = _three_updates(dev, x2, code2, 0.99, N0=N0)
    assert np.array_equal(st.code[unused[:2]], code2[unused[:2]]) and not np.array_equal(st.code[unused[2]], code2[unused[2]])
    # decay 0: N' = cnt, m' = the sum, code = the mean through m's extra rounding -- zs_vq_update's means within 2 fp32 spacings
    # (|fl(s) - s| <= ulp / 2 moves the quotient by at most one spacing, the two final roundings by half a spacing each), and
    # bit for bit where that rounding is exact; a codeword that took no row stays, as in zs_vq_update
    for (nn, EE, KK) in SHAPES[1:]:
        x3, code3 = _case(nn, EE, KK, False)
        shift = R.vq_shift(nn, T.MAX_ABS)
        idx, _ = R.assign(x3, code3)
        cnt, s, _ = R.accum(x3, idx, KK, shift)
        N, m, c, cn, used = _ema(dev, np.ones(KK, np.float32), code3, code3, cnt, s, shift, 0.0)
        wN, wm, wc, wcn, _ = T.ema(np.ones(KK, np.float32), code3, code3, cnt, s, shift, 0.0)
        assert np.array_equal(_bits(N), _bits(wN)) and np.array_equal(_bits(m), _bits(wm)) and np.array_equal(_bits(c), _bits(wc))
        assert np.array_equal(_bits(cn), _bits(wcn)) and np.array_equal(N, cnt.astype(np.float32))
        c_d = torch.from_numpy(code3.copy()).to(dev)
        cn_d, ch = torch.zeros(KK, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        cnt_d, s_d = torch.from_numpy(cnt).to(dev), torch.from_numpy(s).to(dev)
        L.call('zs_vq_update', 'ZsVqUpdate', _stream(), code=L.ptr(c_d), ld_code=EE, cnorm=L.ptr(cn_d), K=KK, E=EE, shift=shift,
               cnt=L.ptr(cnt_d), sum=L.ptr(s_d), changed=L.ptr(ch))
        mean = c_d.cpu().numpy()
        gap = np.abs(c.astype(np.float64) - mean) / np.spacing(np.abs(mean))
        print('n %d E %d K %d decay 0: %.3g of the means equal bit for bit, worst %.3g spacings' % (nn, EE, KK, (gap == 0).mean(), gap.max()))
        assert gap.max() <= 2.0 and np.array_equal(c[cnt == 0], code3[cnt == 0]) and np.array_equal(mean[cnt == 0], code3[cnt == 0])
        exact = (m.astype(np.float64) == s.astype(np.float64) * 2.0 ** -shift)
        assert np.array_equal(_bits(c[exact]), _bits(mean[exact]))


# ---- argument errors -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(dev):
    from zs_amd import _lib as L
    E, n, K, ld = 20, 50, 7, 24
    z = torch.full((n, ld), 0.5, device=dev)
    code = torch.full((K, E), 0.25, device=dev)
    idx = torch.zeros(n, dtype=torch.int32, device=dev)
    q = torch.full((n, ld), 9.0, device=dev)
    zf = torch.full((n, E), 9.0, device=dev)
    ia = torch.full((n,), -7, dtype=torch.int32, device=dev)
    part = torch.full((L.ZS_VQ_COMMIT_PARTS,), -1.0, dtype=torch.float64, device=dev)
    loss = torch.full((2,), -7.0, device=dev)
    stat = torch.full((4,), 5, dtype=torch.int32, device=dev)
    ok = dict(dtype=L.ZS_F32, z=L.ptr(z), n=n, ld_z=ld, idx=L.ptr(idx), code=L.ptr(code), ld_code=E, K=K, E=E, q=L.ptr(q), ld_q=ld,
              z_f32=L.ptr(zf), ld_zf=E, idx_acc=L.ptr(ia), scale=1.0, partial=L.ptr(part), loss=L.ptr(loss), bad=L.ptr(stat), over=L.ptr(stat, 1))
    for change in (dict(K=0), dict(K=-1), dict(K=65537), dict(E=0), dict(E=1025), dict(n=-1), dict(n=2 ** 31), dict(z=None), dict(idx=None),
                   dict(code=None), dict(q=None), dict(bad=None), dict(ld_z=E - 1), dict(ld_q=16), dict(ld_q=20), dict(ld_code=E - 1),
                   dict(ld_zf=E - 1), dict(dtype=5), dict(q=L.ptr(q) + 8), dict(idx=L.ptr(idx) + 2), dict(z=L.ptr(z) + 2),
                   dict(code=L.ptr(code) + 1), dict(z_f32=L.ptr(zf) + 2), dict(partial=L.ptr(part) + 4), dict(loss=None), dict(partial=None),
                   dict(idx_acc=L.ptr(idx)), dict(idx_acc=L.ptr(ia) + 1)):
        with pytest.raises(L.ZsError, match='zs_vq_commit'):
            L.call('zs_vq_commit', 'ZsVqCommit', _stream(), **dict(ok, **change))
    L.call('zs_vq_commit', 'ZsVqCommit', _stream(), **dict(ok, n=0, z=None, idx=None, code=None, q=None, bad=None))      # n == 0 succeeds
    dq = torch.full((n, ld), 3.0, device=dev)
    dz = torch.full((n, 32), 9.0, device=dev)
    ok = dict(dtype=L.ZS_F32, dq=L.ptr(dq), n=n, ld_dq=ld, z=L.ptr(z), ld_z=ld, idx=L.ptr(idx), code=L.ptr(code), ld_code=E, K=K, E=E, g=0.5,
              dz=L.ptr(dz), ld_dz=32, bad=L.ptr(stat, 2))
    for change in (dict(K=0), dict(K=65537), dict(E=0), dict(E=1025), dict(n=-1), dict(dq=None), dict(z=None), dict(idx=None), dict(code=None),
                   dict(dz=None), dict(bad=None), dict(ld_dq=20), dict(ld_dz=20), dict(ld_dq=16), dict(ld_dz=16), dict(ld_z=E - 1),
                   dict(ld_code=E - 1), dict(dtype=7), dict(dq=L.ptr(dq) + 8), dict(dz=L.ptr(dz) + 8), dict(z=L.ptr(z) + 2),
                   dict(idx=L.ptr(idx) + 2), dict(dz=L.ptr(dq))):                           # (the last: in place at another pitch)
        with pytest.raises(L.ZsError, match='zs_vq_st_bwd'):
            L.call('zs_vq_st_bwd', 'ZsVqStBwd', _stream(), **dict(ok, **change))
    L.call('zs_vq_st_bwd', 'ZsVqStBwd', _stream(), **dict(ok, n=0, dq=None, z=None, idx=None, code=None, dz=None, bad=None))
    cnt = torch.full((K,), 3, dtype=torch.int32, device=dev)
    sums = torch.full((K, E), 2, dtype=torch.int64, device=dev)
    N, m, cn = torch.full((K,), 1.5, device=dev), torch.full((K, E), 0.75, device=dev), torch.full((K,), 1.25, device=dev)
    ok = dict(cnt=L.ptr(cnt), sum=L.ptr(sums), K=K, E=E, shift=3, decay=0.9, N=L.ptr(N), m=L.ptr(m), code=L.ptr(code), ld_code=E,
              cnorm=L.ptr(cn), used=L.ptr(stat, 3))
    for change in (dict(K=0), dict(K=65537), dict(E=0), dict(E=1025), dict(cnt=None), dict(sum=None), dict(N=None), dict(m=None), dict(code=None),
                   dict(cnorm=None), dict(ld_code=E - 1), dict(shift=63), dict(shift=-65), dict(decay=1.0), dict(decay=-0.1),
                   dict(decay=float('nan')), dict(sum=L.ptr(sums) + 4), dict(cnt=L.ptr(cnt) + 2), dict(used=L.ptr(stat) + 2)):
        with pytest.raises(L.ZsError, match='zs_vq_ema'):
            L.call('zs_vq_ema', 'ZsVqEma', _stream(), **dict(ok, **change))
    for fn in ('zs_vq_commit', 'zs_vq_st_bwd', 'zs_vq_ema'):
        assert getattr(L.lib(), fn)(None, None) == L.ZS_EINVAL             # a null struct
    torch.cuda.synchronize()
    assert (q == 9.0).all() and (zf == 9.0).all() and (ia == -7).all() and (part == -1.0).all() and (loss == -7.0).all() and (stat == 5).all()
    assert (dz == 9.0).all() and (dq == 3.0).all() and (z == 0.5).all() and (code == 0.25).all() and (idx == 0).all()
    assert (cnt == 3).all() and (sums == 2).all() and (N == 1.5).all() and (m == 0.75).all() and (cn == 1.25).all()


# ---- the step ------------------------------------------------------------------------------------------------------------------------
NS = 0.01
SIZES = dict(c_in=80, c_h1=16, c_h2=32, c_h3=16, E=8, c_h=32, n_spk=4, seg_len=128)          # tests/test_gpu_encmodes.py's small model


def _nets(dev, dtype='fp32', seed=0, dp=0.0):
    from zs_amd.model import Decoder, Encoder
    s = SIZES
    torch.manual_seed(seed)
    enc = Encoder(c_in=s['c_in'], c_h1=s['c_h1'], c_h2=s['c_h2'], c_h3=s['c_h3'], ns=NS, dp=dp, enc_size=s['E'], seg_len=s['seg_len'],
                  enc_mode='continues', dtype=dtype).to(dev)
    dec = Decoder(c_in=s['E'], c_out=s['c_in'], c_h=s['c_h'], c_a=s['n_spk'], ns=NS, seg_len=s['seg_len'], dtype=dtype).to(dev)
    return enc, dec


def _bottleneck(dev, vectors, rows, beta=0.25, decay=0.99, dtype='fp32'):
    from zs_amd import layers
    from zs_amd.vq import VectorCodebook
    from zs_amd.vq_train import VqBottleneck
    return VqBottleneck(VectorCodebook(np.ascontiguousarray(vectors, np.float32), {'enc_mode': 'continues'}), beta, decay, rows,
                        layers.Ctx(dev, dtype))


def _oracle_z(esd, x_bft):
    """The oracle's 'continues' encoding [B, E, T'] (leaky_relu of the encoder's pre-activation, model/model.py:457-472): the
    multilabel head encoder_forward also computes is ignored (enc_size = E / 2 only gives it a shape it accepts)."""
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import zs_oracle as O
    _, pre = O.encoder_forward(esd, x_bft, NS, 0.0, SIZES['E'] // 2, SIZES['seg_len'])
    return torch.nn.functional.leaky_relu(pre, NS)


def _oracle_step(esd, dsd, x_bft, c, code, idx, beta, dt):
    """loss_rec, loss_vq and the gradients of one step in precision dt, the quantiser as z + (q - z).detach() with the given idx."""
    import zs_oracle as O
    ep = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in esd.items()}
    dp = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in dsd.items()}
    z = _oracle_z(ep, x_bft.to(dt))                                                     # [B, E, T']
    B, E, T4 = z.shape
    q = torch.from_numpy(code[idx]).to(dt).view(B, T4, E).permute(0, 2, 1)
    x_dec = O.decoder_forward(dp, z + (q - z).detach(), c, NS, SIZES['seg_len'])
    l_rec = O.l1_loss(x_dec, x_bft.to(dt))
    l_vq = beta * ((z - q) ** 2).mean()
    (l_rec + l_vq).backward()
    return l_rec.item(), l_vq.item(), {k: v.grad for k, v in ep.items()}, {k: v.grad for k, v in dp.items()}, z.detach()


def test_one_iteration_against_the_oracle(dev):
    """Bounds of tests/test_gpu_encmodes.py test_train_step_vs_reference for the same tensors: |loss - reference| < 1e-5 (its line
    271) and gradients within 2e-3 of the tensor's largest |reference| (its line 284).  Before the device is compared, the fp32
    oracle must lie within a tenth of those bounds of the same oracle in fp64 (else the seed is ill-conditioned: pick another)."""
    from zs_amd.trainer import AEStep
    enc, dec = _nets(dev, seed=0)
    esd = {k: v.detach().cpu() for k, v in enc.state_dict().items()}
    dsd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    B, T, beta = 3, 32, 0.25
    x = torch.rand(B, T, SIZES['c_in'], generator=g) * 0.98 + 1e-3
    c = torch.randint(0, SIZES['n_spk'], (B,), generator=g)
    with torch.no_grad():
        z64 = _oracle_z({k: v.double() for k, v in esd.items()}, x.permute(0, 2, 1).double())
    rows = z64.permute(0, 2, 1).reshape(-1, SIZES['E']).numpy()                         # [B T', E]: 12 rows
    rs = np.random.RandomState(3)
    code = (rows[[0, 3, 6, 9, 11]] * (1.0 + 0.2 * rs.standard_normal((5, SIZES['E'])))).astype(np.float32)
    bn = _bottleneck(dev, code, len(rows), beta=beta)
    ae = AEStep(enc, dec, lr=1e-4, max_grad_norm=5.0, use_graph=False, vq=bn)
    loss = ae.step(x.to(dev), c.to(dev), update=False)
    torch.cuda.synchronize()
    idx = bn.idx.cpu().numpy()
    near = R.near_rows(rows.astype(np.float32), code)
    want_idx, _ = R.assign(rows, code)
    assert np.array_equal(idx[~near], want_idx[~near]) and len(set(idx.tolist())) >= 2
    assert np.array_equal(bn.code_live.cpu().numpy(), code) and not np.array_equal(bn.code.cpu().numpy(), code)     # the step read the old codebook
    xb = x.permute(0, 2, 1)
    r32, v32, ge32, gd32, _ = _oracle_step(esd, dsd, xb, c, code, idx, beta, torch.float32)
    r64, v64, ge64, gd64, _ = _oracle_step(esd, dsd, xb, c, code, idx, beta, torch.float64)
    assert abs(r32 - r64) < 1e-6 and abs(v32 - v64) < 1e-6
    picks = (('enc', enc, ge32, ge64, 'linear.weight'), ('enc', enc, ge32, ge64, 'conv2.weight'), ('dec', dec, gd32, gd64, 'conv1.weight'))
    for name, net, g32, g64, k in picks:
        scale = g64[k].abs().max().item()
        assert scale > 1e-6 and (g32[k].double() - g64[k]).abs().max().item() <= 2e-4 * scale, 'the fp32 oracle is ill-conditioned here'
    print('loss_rec %.7f (oracle %.7f, |d| %.3g)  loss_vq %.7f (oracle %.7f, |d| %.3g)' %
          (loss.item(), r32, abs(loss.item() - r32), bn.loss.item(), v32, abs(bn.loss.item() - v32)))
    assert abs(loss.item() - r32) < 1e-5 and abs(bn.loss.item() - v32) < 1e-5
    for name, net, g32, g64, k in picks:
        ref = g32[k].double()
        scale = ref.abs().max().item()
        e = (net.grad_view(k).detach().cpu().double() - ref).abs().max().item() / scale
        print('grad %s.%s: relative error %.3g of scale %.3g' % (name, k, e, scale))
        assert e < 2e-3
    # the commitment term is in that gradient: without it linear.weight's gradient is another one
    _, _, ge0, _, _ = _oracle_step(esd, dsd, xb, c, code, idx, 0.0, torch.float64)
    k = 'linear.weight'
    assert (ge0[k] - ge64[k]).abs().max().item() > 10 * 2e-3 * ge64[k].abs().max().item()
    st = bn.stats()
    assert st['K'] == 5 and st['used'] == len(set(idx.tolist())) and abs(st['loss_vq'] - v64) < 1e-5 and 1.0 <= st['perplexity'] <= 5.0


def _run_five(dev, graph_warmup, dtype):
    from zs_amd.trainer import AEStep
    enc, dec = _nets(dev, dtype=dtype, seed=0, dp=0.5)
    B, T = 4, 32
    code = R.planted(7, SIZES['E'], 4, 0.3, 2) * 0.1
    bn = _bottleneck(dev, code, B * 4, dtype=dtype)
    ae = AEStep(enc, dec, lr=1e-3, max_grad_norm=5.0, use_graph=True, vq=bn)
    ae.graph_warmup = graph_warmup
    g = torch.Generator().manual_seed(1)
    losses = []
    for _ in range(5):
        x = torch.rand(B, T, SIZES['c_in'], generator=g).to(dev)
        c = torch.randint(0, SIZES['n_spk'], (B,), generator=g).to(dev)
        losses.append((ae.step(x, c).item(), bn.loss.item()))
    torch.cuda.synchronize()
    state = [enc.flat_params()[0], dec.flat_params()[0]] + [getattr(ae.opt[k], a) for k in ('enc', 'dec') for a in ('m', 'v')] + \
        [bn.code, bn.cnorm, bn.N, bn.m, bn.idx]
    assert bn.stats()['used'] >= 1 and bn.steps == (5 if graph_warmup > 5 else 3)       # (a replay does not pass through forward())
    return losses, [t.clone() for t in state], len(ae._graphs)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_captured_equals_eager_and_a_rerun(dev, dtype):
    la, sa, na = _run_five(dev, 2, dtype)
    lb, sb, nb = _run_five(dev, 10 ** 9, dtype)
    lc, sc, nc = _run_five(dev, 2, dtype)
    assert na == nc == 1 and nb == 0
    assert la == lb == lc, (la, lb, lc)
    for a, b, c in zip(sa, sb, sc):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert len({l[0] for l in la}) == 5 and all(np.isfinite(v) and v > 0 for l in la for v in l)


def test_the_codebook_follows_the_encoder(dev):
    """Frozen weights, one batch, 40 iterations at decay 0.5.  Once the assignment has stopped changing, N and m approach cnt and the
    rows' sum geometrically, so code = m / N is the mean of the rows up to decay^s of a unit-sized start after s stable iterations
    (s >= 25: 3e-8) plus fp32 rounding: 1e-5 of the mean's largest element is derived, not measured."""
    from zs_amd.trainer import AEStep
    enc, dec = _nets(dev, seed=0)
    B, T = 8, 32
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(B, T, SIZES['c_in'], generator=g) * 0.98 + 1e-3).to(dev)
    c = torch.randint(0, SIZES['n_spk'], (B,), generator=g).to(dev)
    ee = enc._engine()
    enc.train()
    _, z, _ = ee.forward(x, True, seed=0)
    rows = z.reshape(-1, SIZES['E']).cpu().numpy().copy()                               # [32, E]
    bn = _bottleneck(dev, rows[[1, 9, 17, 25, 30]] * 1.5, len(rows), decay=0.5)
    ae = AEStep(enc, dec, lr=1e-4, max_grad_norm=5.0, use_graph=False, vq=bn)
    p0 = enc.flat_params()[0].clone()
    seen = []
    for _ in range(40):
        ae.step(x, c, update=False)
        seen.append(bn.idx.cpu().numpy().copy())
    assert torch.equal(enc.flat_params()[0], p0)
    stable = 0
    while stable < 39 and np.array_equal(seen[-1 - stable - 1], seen[-1]):
        stable += 1
    assert stable >= 25, 'the assignment was still moving %d iterations before the end' % stable
    idx, code = seen[-1], bn.code.cpu().numpy()
    used = np.unique(idx)
    assert len(used) >= 2
    for k in used:
        mean = rows[idx == k].astype(np.float64).mean(0)
        err = np.abs(code[k] - mean).max() / np.abs(mean).max()
        print('codeword %d: %d rows, |code - mean| / |mean| = %.3g' % (k, (idx == k).sum(), err))
        assert err <= 1e-5
    bn.stats()


def test_a_step_without_the_bottleneck_calls_no_vq_entry_point(dev, monkeypatch):
    from zs_amd import _lib as L
    from zs_amd.trainer import AEStep
    names, direct = [], []                                                          # through L.call; looked up on L.lib()
    real_call, real_lib = L.call, L.lib

    class Spy(object):
        def __getattr__(self, name):
            direct.append(name)
            return getattr(real_lib(), name)
    monkeypatch.setattr(L, 'call', lambda fname, *a, **k: (names.append(fname), real_call(fname, *a, **k))[1])
    monkeypatch.setattr(L, 'lib', lambda: Spy())
    enc, dec = _nets(dev, seed=0)
    ae = AEStep(enc, dec, lr=1e-4, max_grad_norm=5.0, use_graph=False)
    assert ae.vq is None
    g = torch.Generator().manual_seed(1)
    x = torch.rand(3, 32, SIZES['c_in'], generator=g).to(dev)
    c = torch.randint(0, SIZES['n_spk'], (3,), generator=g).to(dev)
    ae.step(x, c)
    ae._execute(ae.plan(x, c, False, True), counted=True)                              # the counted plan too
    torch.cuda.synchronize()
    assert len(names) > 50 and 'zs_step_counters' in direct and not [n for n in names + direct if n.startswith('zs_vq')]
    ae.vq = _bottleneck(dev, R.planted(5, SIZES['E'], 4, 0.3, 2) * 0.1, 12)
    del names[:]
    ae.step(x, c)
    torch.cuda.synchronize()
    assert [n for n in names if n.startswith('zs_vq')] == ['zs_vq_assign', 'zs_vq_commit', 'zs_vq_accum', 'zs_vq_ema', 'zs_vq_st_bwd']


def test_main_vq_train_then_convert_with_the_trained_codebook(dev, tmp_path, monkeypatch, capsys):
    from scipy.io import wavfile
    sys.path.insert(0, ROOT)
    import main as M
    from zs_amd import convert as cv, layers, vq as V
    from zs_amd.hps import hp
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('ZS_CKPT_EVERY', '4')
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    h = json.load(open(os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')))
    h.update(n_speakers=4, n_target_speakers=2, batch_size=4, enc_pretrain_iters=4, max_to_keep=3, enc_size=8, emb_size=32, seg_len=32)
    hps_path = str(tmp_path / 'hps.json')
    json.dump(h, open(hps_path, 'w'))
    K = 6
    start = str(tmp_path / 'K6.vq.npz')
    V.VectorCodebook(R.planted(K, 8, 4, 0.3, 4) * 0.1, {'enc_mode': 'continues', 'seed': 0}).save(start)
    ck = tmp_path / 'ck'
    M.main(['--train_ae', '--synthetic', '--enc_mode', 'continues', '--hps_path', hps_path, '--ckpt_dir', str(ck), '--dtype', 'fp32',
            '--vq_train', start, '--vq_decay', '0.9'])
    out = capsys.readouterr().out
    assert 'pre_AE:[000004/000004]' in out and 'loss_vq=' in out and 'perplexity=' in out
    cb_path = str(ck / 'model.pth-ae-4.vq.npz')
    cb = V.load_codebook(cb_path, 'continues', E=8)
    assert (cb.K, cb.E) == (K, 8) and not np.array_equal(cb.vectors, V.load_codebook(start, 'continues', 8).vectors)
    assert cb.meta['trained_iterations'] == 4 and cb.meta['beta'] == 0.25 and cb.meta['decay'] == 0.9 and 1 <= cb.meta['used'] <= K
    assert cb.meta['enc_mode'] == 'continues' and os.path.exists(str(ck / 'model.pth-ae-4'))
    d = tmp_path / 'in'
    d.mkdir()
    rng = np.random.RandomState(5)
    for i, n in enumerate((9000, 12000)):
        t = np.arange(n) / 16000.0
        y = 0.3 * np.sin(2 * np.pi * (200.0 + 150.0 * i + 400.0 * t) * t) + 0.05 * rng.randn(n)
        wavfile.write(str(d / ('w%d.wav' % i)), 16000, (y * 32767).astype(np.int16))
    s2id = str(tmp_path / 'speaker2id.json')
    json.dump({'S015': 0, 'S020': 1, 'V001': 2, 'V002': 3}, open(s2id, 'w'))
    monkeypatch.setattr(hp, 'n_iter', 4)
    res = tmp_path / 'result'
    M.main(['--convert_dir', str(d), '--t_speaker', 'V001', '--result_dir', str(res), '--codebook', cb_path, '--enc_only', '--hps_path', hps_path,
            '--speaker2id_path', s2id, '--ckpt_pth', str(ck / 'model.pth-ae-4'), '--enc_mode', 'continues', '--g_mode', 'targeted_residual'])
    conv = os.path.join(os.path.join(str(res), './english/'), 'convert')
    for s in ('w0', 'w1'):
        idx = cv.read_indices(os.path.join(conv, 'V001', s + '.idx.txt'), K)           # raises for an index outside [0, K)
        assert len(idx) >= 2 and idx.min() >= 0 and idx.max() < K
        assert os.path.getsize(os.path.join(conv, 'V001', s + '.wav')) > 44
    layers.check_status(dev)
