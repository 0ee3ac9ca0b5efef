"""Training through the residual codebook on the device:

* zs_rvq_commit, zs_rvq_loss and zs_rvq_st_bwd against the numpy definition of tests/rvq_train_ref.py, bit for bit (the loss within
  1e-6 of fp64), on the smallest shapes that cross one row, a team of one lane, an E that is no multiple of 4, ld > E, more than one
  workgroup and ZS_CODE_MAX_E, in fp32 and bf16, over chains of 1, 2, 3 and 8 stages; bad indices, rows at ZS_VQ_MAX_ABS and every
  ZS_EINVAL case with NaN guards around every output; one stage against the single-stage kernels of DESIGN 30;
* RvqBottleneck.forward against ResidualCodebook.snap and Decoder.forward_index_planes (training shows the Decoder what conversion
  shows it), one AEStep iteration against the oracle's torch modules under autograd, eager against captured over 5 iterations with
  restarts on, the codebooks' fixed point on a planted three-level mixture, the steps without it launching none of the new entry
  points, and main.py --rvq_train end to end."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import rvq_train_ref as RT  # noqa: E402
import vq_ref as R  # noqa: E402
import vq_train_ref as T  # noqa: E402

F32 = np.float32
GUARD = 64
FILL_I = -0x55555556
SEED = 1
SHAPES = [(1, 1, 1), (37, 6, 5), (65, 20, 37), (300, 64, 300), (130, 1024, 129)]
LD = {1: 8, 6: 8, 20: 24, 64: 72, 1024: 1024}                     # the Decoder-side operands' pitch (a multiple of 8)


def _pitches(E, bf16):
    """(ld_x, ld_code, ld_r, ld_a, ld_xf): dense; E + odd everywhere (the element-wise accesses); a multiple of 4 above E."""
    up4 = (E + 4) // 4 * 4
    return ((E, E, E, E, E), (E + (9 if bf16 else 5), E + 1, E + 3, E + 7, E + 1), (up4 + 4, up4, up4, up4 + 8, up4))


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pitched(rows, ld, fill=np.nan):
    n, E = rows.shape
    buf = np.full(n * ld + GUARD, fill, dtype=F32)
    buf[:n * ld].reshape(n, ld)[:, :E] = rows
    return buf


def _unpitch(t, n, ld, E):
    """(the valid [n, E] part, whether the slack of the pitch and the guard still hold NaN) of a pitched fp32 device buffer."""
    a = t.cpu().numpy()
    body = a[:n * ld].reshape(n, ld)
    return body[:, :E].copy(), bool(np.isnan(body[:, E:]).all() and np.isnan(a[n * ld:]).all())


def _same(a, b):
    """Bit for bit, NaN matching NaN whatever its payload."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def _case(n, E, K, S, bf16, seed=SEED):
    x = R.planted(n, E, 8, 0.3, seed)
    codes = [(R.planted(K, E, 8, 0.3, seed + 100 + s) * F32(0.5 ** s)).astype(F32) for s in range(S)]
    return (T.bf16_round(x) if bf16 else x), codes


def _assign(dev, x, code, wide_bf16):
    """zs_vq_assign's idx for the rows x (fp32 values; uploaded as bf16 when wide_bf16)."""
    from zs_amd import vq as V
    x_d = torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(torch.bfloat16 if wide_bf16 else torch.float32)
    idx = torch.full((len(x),), -1, dtype=torch.int32, device=dev)
    V.assign(x_d, torch.from_numpy(code).to(dev), torch.from_numpy(R.cnorm(code)).to(dev), idx=idx)
    return idx.cpu().numpy()


def _commit(dev, x, src_bf16, idx, code, a_in, ld, want_xf=True, partial=None, change=None, run_bf16=None):
    """zs_rvq_commit on rows x (fp32 values; a bf16 operand when src_bf16) with NaN behind every output; a_in None: the first stage.
    run_bf16: the run's compute dtype is bf16 (fp32 rows then go in with src_f32 set); default: the operand's own.
    Returns numpy results and asserts the guards and the read-only operands."""
    from zs_amd import _lib as L
    n, E = x.shape
    K = code.shape[0]
    ld_x, ld_code, ld_r, ld_a, ld_xf = ld
    xb, cb = _pitched(x, ld_x), _pitched(code, ld_code)
    x_d = torch.from_numpy(xb).to(dev).to(torch.bfloat16 if src_bf16 else torch.float32)
    c_d = torch.from_numpy(cb).to(dev)
    ib = np.concatenate([np.asarray(idx, np.int32), np.full(GUARD, FILL_I, np.int32)])
    i_d = torch.from_numpy(ib).to(dev)
    r_d = torch.full((n * ld_r + GUARD,), np.nan, device=dev)
    f_d = torch.full((n * ld_xf + GUARD,), np.nan, device=dev)
    a_d = torch.from_numpy(_pitched(a_in if a_in is not None else np.full((n, E), np.nan, F32), ld_a)).to(dev)
    ia = torch.full((n + GUARD,), FILL_I, dtype=torch.int32, device=dev)
    part = partial if partial is not None else torch.full((L.ZS_VQ_COMMIT_PARTS + GUARD,), np.nan, dtype=torch.float64, device=dev)
    stat = torch.full((4,), 7, dtype=torch.int32, device=dev)
    run_bf16 = src_bf16 if run_bf16 is None else run_bf16
    kw = dict(dtype=(L.ZS_BF16 if run_bf16 else L.ZS_F32), src_f32=int(run_bf16 and not src_bf16), first=int(a_in is None), x=L.ptr(x_d), n=n, ld_x=ld_x, idx=L.ptr(i_d),
              code=L.ptr(c_d), ld_code=ld_code, K=K, E=E, r=L.ptr(r_d), ld_r=ld_r, x_f32=(L.ptr(f_d) if want_xf else None),
              ld_xf=(ld_xf if want_xf else 0), idx_acc=L.ptr(ia), a=L.ptr(a_d), ld_a=ld_a, partial=L.ptr(part), bad=L.ptr(stat), over=L.ptr(stat, 1))
    kw.update(change or {})
    L.call('zs_rvq_commit', 'ZsRvqCommit', _stream(), **kw)
    torch.cuda.synchronize()
    r, ok_r = _unpitch(r_d, n, ld_r, E)
    a, ok_a = _unpitch(a_d, n, ld_a, E)
    f, ok_f = _unpitch(f_d, n, ld_xf, E)
    assert ok_r and ok_a and ok_f and (ia[n:] == FILL_I).all() and (stat[2:] == 7).all()
    if partial is None:
        assert torch.isnan(part[L.ZS_VQ_COMMIT_PARTS:]).all() and not torch.isnan(part[:L.ZS_VQ_COMMIT_PARTS]).any()
    assert np.array_equal(c_d.cpu().numpy(), cb, equal_nan=True) and np.array_equal(i_d.cpu().numpy(), ib)
    assert np.array_equal(x_d.float().cpu().numpy(), xb, equal_nan=True)
    if not want_xf:
        assert np.isnan(f).all()
    return dict(r=r, a=a, x_f32=f, idx_acc=ia[:n].cpu().numpy(), sq=float(part[:L.ZS_VQ_COMMIT_PARTS].sum().item()),
                bad=int(stat[0]) - 7, over=int(stat[1]) - 7)


# ---- zs_rvq_commit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [1, 2, 3, 8])
@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('n,E,K', SHAPES)
def test_commit_equals_the_definition_over_a_chain_of_stages(dev, n, E, K, bf16, S):
    """Stage 0 reads the rows in the compute dtype, every later stage the fp32 residual the stage before wrote; each stage's index is
    zs_vq_assign's of its own input.  r, a, idx_acc and the fp32 copy bit for bit at three pitches; the sum of squares within 1e-12."""
    x, codes = _case(n, E, K, S, bf16)
    for ld in _pitches(E, bf16):
        r, a = x, None
        for s in range(S):
            src_bf16 = bf16 and s == 0
            idx = _assign(dev, r, codes[s], src_bf16)
            want = RT.commit(r, idx, codes[s], a)
            got = _commit(dev, r, src_bf16, idx, codes[s], a, ld, want_xf=(s == 0), run_bf16=bf16)
            assert _same(got['r'], want['r']) and _same(got['a'], want['a']), 'stage %d ld %s' % (s, ld)
            assert np.array_equal(got['idx_acc'], idx) and np.array_equal(want['idx_acc'], idx) and got['bad'] == 0 and got['over'] == 0
            assert abs(got['sq'] - want['sq']) <= 1e-12 * want['sq']
            if s == 0:
                assert _same(got['x_f32'], x)
            r, a = want['r'], want['a']
    if S > 1 and n > 1:
        assert not np.array_equal(a, r)                                # a is a sum of S residuals, not the last one


@pytest.mark.parametrize('bf16', [False, True])
def test_commit_bad_indices_and_rows_at_the_bound(dev, bf16):
    """An idx outside [0, K) is never an index (2^30 would be far outside the codebook): the row passes unsubtracted, adds nothing to
    the sum or to a, idx_acc -1, counted.  A row with an element of magnitude >= 65536, infinite or NaN is quantised like any other,
    counted, and handed to zs_vq_accum as -1: at the first stage and behind it."""
    n, E, K = 300, 64, 300
    x, codes = _case(n, E, K, 2, bf16)
    ld = _pitches(E, bf16)[0]
    for first in (True, False):
        src_bf16 = bf16 and first
        rows = x.copy()
        idx = _assign(dev, rows, codes[0], src_bf16).copy()
        idx[3], idx[5], idx[130], idx[299] = K, -1, 2 ** 30, -2 ** 31
        rows[9, 2], rows[11, 63], rows[200, 0], rows[5, 1] = 65536.0, -np.inf, -70000.0 if not src_bf16 else -70144.0, np.nan
        rows[12, 7] = 65280.0                                           # below the bound (exact in bf16): kept
        a_in = None if first else R.planted(n, E, 8, 0.3, 77)
        want = RT.commit(rows, idx, codes[0], a_in)
        got = _commit(dev, rows, src_bf16, idx, codes[0], a_in, ld, want_xf=first, run_bf16=bf16)
        assert want['bad'] == 4 and want['over'] == 4 and got['bad'] == 4 and got['over'] == 4
        assert _same(got['r'], want['r']) and _same(got['a'], want['a']) and np.array_equal(got['idx_acc'], want['idx_acc'])
        assert (want['idx_acc'] == -1).sum() == 7 and _same(got['r'][[3, 5, 130, 299]], rows[[3, 5, 130, 299]])
        if first:
            assert (got['a'][[3, 130, 299]] == 0).all() and _same(got['x_f32'], rows)
        else:
            assert _same(got['a'][[3, 5, 130, 299]], a_in[[3, 5, 130, 299]])
        assert got['sq'] == np.inf                                      # (the infinite row)
        rows[11, 63] = 0.0
        want = RT.commit(rows, idx, codes[0], a_in)
        got = _commit(dev, rows, src_bf16, idx, codes[0], a_in, ld, want_xf=first)
        assert abs(got['sq'] - want['sq']) <= 1e-12 * want['sq'] and got['over'] == 3


# ---- zs_rvq_loss ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('n,E,K', SHAPES)
def test_loss_is_within_1e_6_of_fp64(dev, n, E, K, bf16):
    """DESIGN 30's bound for loss_vq: relative 1e-6 against the fp64 sum of the stored residuals squared, total and per stage."""
    from zs_amd import _lib as L
    S, beta = 3, 0.25
    x, codes = _case(n, E, K, S, bf16)
    P = L.ZS_VQ_COMMIT_PARTS
    part = torch.full((S * P + GUARD,), np.nan, dtype=torch.float64, device=dev)
    r, a, sq = x, None, []
    for s in range(S):
        idx = _assign(dev, r, codes[s], bf16 and s == 0)
        want = RT.commit(r, idx, codes[s], a)
        _commit(dev, r, bf16 and s == 0, idx, codes[s], a, _pitches(E, bf16)[0], partial=part[s * P:], run_bf16=bf16)
        sq.append(want['sq'])
        r, a = want['r'], want['a']
    loss = torch.full((1 + S + 2,), np.nan, device=dev)
    L.call('zs_rvq_loss', 'ZsRvqLoss', _stream(), partial=L.ptr(part), S=S, scale=beta / (float(n) * E), loss=L.ptr(loss))
    torch.cuda.synchronize()
    assert torch.isnan(loss[1 + S:]).all() and torch.isnan(part[S * P:]).all()
    got = loss[:1 + S].cpu().numpy().astype(np.float64)
    total, per = RT.losses(sq, beta, n, E)
    worst = max(abs(g - w) / w for g, w in zip(got, [total] + per))
    print('n %d E %d K %d bf16 %d: loss_vq %.9g (fp64 %.9g), stages %s, worst relative error %.3g' % (n, E, K, bf16, got[0], total, got[1:], worst))
    assert total > 0 and all(w > 0 for w in per) and worst <= 1e-6


# ---- zs_rvq_st_bwd -------------------------------------------------------------------------------------------------------------------
def _st_bwd(dev, dq, a, g, ld_dq, ld_dz, ld_a, bf16, in_place, change=None):
    from zs_amd import _lib as L
    n, E = a.shape
    dt = torch.bfloat16 if bf16 else torch.float32
    ab = _pitched(a, ld_a)
    a_d = torch.from_numpy(ab).to(dev)
    dq_d = torch.from_numpy(_pitched(dq, ld_dq, 5.0)).to(dev).to(dt)
    dz_d = dq_d if in_place else torch.full((n * ld_dz + GUARD,), 9.0, dtype=dt, device=dev)
    kw = dict(dtype=(L.ZS_BF16 if bf16 else L.ZS_F32), dq=L.ptr(dq_d), n=n, ld_dq=ld_dq, a=L.ptr(a_d), ld_a=ld_a, E=E, g=float(g), dz=L.ptr(dz_d),
              ld_dz=ld_dz)
    kw.update(change or {})
    L.call('zs_rvq_st_bwd', 'ZsRvqStBwd', _stream(), **kw)
    torch.cuda.synchronize()
    assert (dz_d[n * ld_dz:] == (5.0 if in_place else 9.0)).all() and np.array_equal(a_d.cpu().numpy(), ab, equal_nan=True)
    if not in_place:
        assert np.array_equal(dq_d.float().cpu().numpy(), T.cast(_pitched(dq, ld_dq, 5.0), bf16))
    return dz_d[:n * ld_dz].float().cpu().numpy().reshape(n, ld_dz)


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('n,E,K', SHAPES)
def test_st_bwd_equals_the_definition_in_and_out_of_place(dev, n, E, K, bf16):
    """g of the step (2 beta / (n E), small against dq) and a large one, so that each of the roundings shows; a at a 16-byte pitch
    and at an odd one."""
    a = (R.planted(n, E, 8, 0.3, SEED) - R.planted(n, E, 8, 0.3, SEED + 1)).astype(F32)
    dq = T.cast(np.random.RandomState(n + E).standard_normal((n, E)).astype(F32), bf16)
    for g in (RT.grad_scale(0.25, n, E), F32(0.37)):
        want = RT.st_bwd(dq, a, g, bf16)
        for in_place, ld_dq, ld_dz, ld_a in ((False, LD[E], LD[E] + 8, E), (True, LD[E], LD[E], E + 3), (False, LD[E] + 8, LD[E], (E + 4) // 4 * 4)):
            got = _st_bwd(dev, dq, a, g, ld_dq, ld_dz, ld_a, bf16, in_place)
            assert _same(got[:, :E], want), 'g %g in_place %d' % (g, in_place)
            assert (got[:, E:] == 0).all()
    moved = (want != dq).mean()
    print('n %d E %d bf16 %d: %.3g of the elements differ from dq' % (n, E, bf16, moved))
    assert moved > 0.5


# ---- argument errors -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(dev):
    from zs_amd import _lib as L
    E, n, K, ld = 20, 50, 7, 24
    x = torch.full((n, ld), 0.5, device=dev)
    code = torch.full((K, E), 0.25, device=dev)
    idx = torch.zeros(n, dtype=torch.int32, device=dev)
    r, zf, a = (torch.full((n, ld), v, device=dev) for v in (9.0, 8.0, 6.0))
    ia = torch.full((n,), -7, dtype=torch.int32, device=dev)
    part = torch.full((L.ZS_VQ_COMMIT_PARTS,), -1.0, dtype=torch.float64, device=dev)
    loss = torch.full((4,), -7.0, device=dev)
    stat = torch.full((4,), 5, dtype=torch.int32, device=dev)
    ok = dict(dtype=L.ZS_F32, src_f32=0, first=1, x=L.ptr(x), n=n, ld_x=ld, idx=L.ptr(idx), code=L.ptr(code), ld_code=E, K=K, E=E, r=L.ptr(r), ld_r=ld,
              x_f32=L.ptr(zf), ld_xf=ld, idx_acc=L.ptr(ia), a=L.ptr(a), ld_a=ld, partial=L.ptr(part), bad=L.ptr(stat), over=L.ptr(stat, 1))
    for change in (dict(K=0), dict(K=-1), dict(K=65537), dict(E=0), dict(E=1025), dict(n=-1), dict(n=2 ** 31), dict(x=None), dict(idx=None),
                   dict(code=None), dict(r=None), dict(idx_acc=None), dict(a=None), dict(partial=None), dict(bad=None), dict(over=None),
                   dict(ld_x=E - 1), dict(ld_code=E - 1), dict(ld_r=E - 1), dict(ld_xf=E - 1), dict(ld_a=E - 1), dict(dtype=5),
                   dict(x=L.ptr(x) + 2), dict(dtype=L.ZS_BF16, x=L.ptr(x) + 1), dict(idx=L.ptr(idx) + 2), dict(code=L.ptr(code) + 1),
                   dict(r=L.ptr(r) + 2), dict(x_f32=L.ptr(zf) + 2), dict(a=L.ptr(a) + 1), dict(partial=L.ptr(part) + 4), dict(idx_acc=L.ptr(ia) + 1),
                   dict(r=L.ptr(x)), dict(a=L.ptr(x)), dict(x_f32=L.ptr(x)), dict(a=L.ptr(r)), dict(x_f32=L.ptr(r)), dict(x_f32=L.ptr(a)),
                   dict(idx_acc=L.ptr(idx))):
        with pytest.raises(L.ZsError, match='zs_rvq_commit'):
            L.call('zs_rvq_commit', 'ZsRvqCommit', _stream(), **dict(ok, **change))
    L.call('zs_rvq_commit', 'ZsRvqCommit', _stream(), **dict(ok, n=0, x=None, idx=None, code=None, r=None, a=None, idx_acc=None, partial=None,
                                                            bad=None, over=None))                      # n == 0 succeeds
    okl = dict(partial=L.ptr(part), S=1, scale=1.0, loss=L.ptr(loss))
    for change in (dict(S=0), dict(S=9), dict(S=-1), dict(partial=None), dict(loss=None), dict(partial=L.ptr(part) + 4), dict(loss=L.ptr(loss) + 2)):
        with pytest.raises(L.ZsError, match='zs_rvq_loss'):
            L.call('zs_rvq_loss', 'ZsRvqLoss', _stream(), **dict(okl, **change))
    dq = torch.full((n, ld), 3.0, device=dev)
    dz = torch.full((n, 32), 9.0, device=dev)
    okb = dict(dtype=L.ZS_F32, dq=L.ptr(dq), n=n, ld_dq=ld, a=L.ptr(a), ld_a=ld, E=E, g=0.5, dz=L.ptr(dz), ld_dz=32)
    for change in (dict(E=0), dict(E=1025), dict(n=-1), dict(n=2 ** 31), dict(dq=None), dict(a=None), dict(dz=None), dict(ld_dq=20), dict(ld_dz=20),
                   dict(ld_dq=16), dict(ld_dz=16), dict(ld_a=E - 1), dict(dtype=7), dict(dq=L.ptr(dq) + 8), dict(dz=L.ptr(dz) + 8),
                   dict(a=L.ptr(a) + 2), dict(dz=L.ptr(dq)), dict(a=L.ptr(dq)), dict(a=L.ptr(dz))):     # (dz = dq: in place at another pitch)
        with pytest.raises(L.ZsError, match='zs_rvq_st_bwd'):
            L.call('zs_rvq_st_bwd', 'ZsRvqStBwd', _stream(), **dict(okb, **change))
    L.call('zs_rvq_st_bwd', 'ZsRvqStBwd', _stream(), **dict(okb, n=0, dq=None, a=None, dz=None))
    for fn in ('zs_rvq_commit', 'zs_rvq_loss', 'zs_rvq_st_bwd'):
        assert getattr(L.lib(), fn)(None, None) == L.ZS_EINVAL             # a null struct
    torch.cuda.synchronize()
    assert (r == 9.0).all() and (zf == 8.0).all() and (a == 6.0).all() and (ia == -7).all() and (part == -1.0).all() and (loss == -7.0).all()
    assert (stat == 5).all() and (dz == 9.0).all() and (dq == 3.0).all() and (x == 0.5).all() and (code == 0.25).all() and (idx == 0).all()


# ---- one stage is DESIGN 30's quantiser ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('n,E,K', SHAPES)
def test_one_stage_against_the_single_stage_kernels(dev, n, E, K, bf16):
    from zs_amd import _lib as L, rvq as V
    x, codes = _case(n, E, K, 1, bf16)
    code = codes[0]
    idx = _assign(dev, x, code, bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    ld = LD[E]
    z_d = torch.from_numpy(_pitched(x, ld, 0.0)).to(dev).to(dt)
    c_d, i_d = torch.from_numpy(code).to(dev), torch.from_numpy(idx).to(dev)
    q_d = torch.full((n * ld,), 9.0, dtype=dt, device=dev)
    zf, ia = torch.zeros(n, E, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    stat = torch.zeros(4, dtype=torch.int32, device=dev)
    L.call('zs_vq_commit', 'ZsVqCommit', _stream(), dtype=(L.ZS_BF16 if bf16 else L.ZS_F32), z=L.ptr(z_d), n=n, ld_z=ld, idx=L.ptr(i_d),
           code=L.ptr(c_d), ld_code=E, K=K, E=E, q=L.ptr(q_d), ld_q=ld, z_f32=L.ptr(zf), ld_zf=E, idx_acc=L.ptr(ia), bad=L.ptr(stat), over=L.ptr(stat, 1))
    got = _commit(dev, x, bf16, idx, code, None, (ld, E, E, E, E))
    assert _same(got['x_f32'], zf.cpu().numpy()) and np.array_equal(got['idx_acc'], ia.cpu().numpy())
    B = 1                                                                # the operand: one fragment of n frames
    op = torch.full((B, n, ld), 9.0, dtype=dt, device=dev)
    V.gather(i_d.view(1, n), 1, c_d.view(1, K, E), torch.zeros(B, dtype=torch.int64, device=dev), torch.full((B,), n, dtype=torch.int32, device=dev),
             n, op, stat[2:])
    assert torch.equal(op.view(-1), q_d) and int(stat[2]) == 0
    dq = T.cast(np.random.RandomState(n + E).standard_normal((n, E)).astype(F32), bf16)
    g = RT.grad_scale(0.25, n, E)
    dq_d = torch.from_numpy(_pitched(dq, ld, 0.0)).to(dev).to(dt)
    dz1 = torch.full((n * ld,), 9.0, dtype=dt, device=dev)
    L.call('zs_vq_st_bwd', 'ZsVqStBwd', _stream(), dtype=(L.ZS_BF16 if bf16 else L.ZS_F32), dq=L.ptr(dq_d), n=n, ld_dq=ld, z=L.ptr(z_d), ld_z=ld,
           idx=L.ptr(i_d), code=L.ptr(c_d), ld_code=E, K=K, E=E, g=float(g), dz=L.ptr(dz1), ld_dz=ld, bad=L.ptr(stat, 3))
    dz2 = _st_bwd(dev, dq, got['a'], g, ld, ld, E, bf16, False)
    torch.cuda.synchronize()
    assert _same(dz2, dz1.float().cpu().numpy().reshape(n, ld)) and int(stat[3]) == 0


# ---- the bottleneck ------------------------------------------------------------------------------------------------------------------
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


def _bottleneck(dev, vectors, rows, beta=0.25, decay=0.99, dtype='fp32', restart=None):
    from zs_amd import layers
    from zs_amd.rvq import ResidualCodebook
    from zs_amd.rvq_train import RvqBottleneck
    return RvqBottleneck(ResidualCodebook(np.ascontiguousarray(vectors, F32), {'enc_mode': 'continues'}), beta, decay, rows,
                         layers.Ctx(dev, dtype), restart=restart)


def _rows_act(bn, rows, B, T):
    """The rows as the Act an encoder would hand over (compute dtype, the engine's pitch)."""
    bits = bn.ctx.act('test_z_%d_%d' % (B, T), B, T, rows.shape[1])
    bits.view2d().zero_()
    bits.view2d()[:, :rows.shape[1]] = torch.from_numpy(rows).to(bn.device).to(bits.t.dtype)
    return bits


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('K,S', [(16, 3), (1, 2)])
def test_training_equals_conversion(dev, K, S, dtype):
    """After one forward: the index planes are ResidualCodebook(code_live).snap(z)'s, and q is the operand Decoder.forward_index_planes
    builds from them -- what training shows the Decoder is what conversion shows it, bit for bit."""
    from zs_amd.rvq import ResidualCodebook
    B, T4, E = 3, 4, SIZES['E']
    bf16 = dtype == 'bf16'
    rows = T.cast(R.planted(B * T4, E, 4, 0.3, 3), bf16)
    vec = np.stack([(R.planted(K, E, 4, 0.3, 10 + s) * F32(0.4 ** s)).astype(F32) for s in range(S)])
    bn = _bottleneck(dev, vec, B * T4, dtype=dtype)
    bits = _rows_act(bn, rows, B, T4)
    q = bn.forward(bits)
    torch.cuda.synchronize()
    live = bn.code_live.cpu().numpy()
    assert np.array_equal(live, vec) and (K == 1 or not np.array_equal(bn.code.cpu().numpy(), vec))
    idx, _ = ResidualCodebook(live, {'enc_mode': 'continues'}).snap(bits.view2d())
    assert torch.equal(idx, bn.idx)
    want = RT.cascade(rows, list(vec), idxs=idx.cpu().numpy())
    assert _same(bn.a.cpu().numpy(), want['a']) and np.array_equal(bn.idx_acc.cpu().numpy(), want['idx_acc'])
    _, dec = _nets(dev, dtype=dtype)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    c = torch.zeros(B, dtype=torch.int64, device=dev)
    q_rows = q.view2d().clone()
    start, length = bn._table(B, T4)
    op, _ = dec.forward_index_planes(idx, S, bn.code_live, start, length, B, T4, c, bad)
    torch.cuda.synchronize()
    assert op.ld == q.ld and torch.equal(op.view2d(), q_rows) and int(bad) == 0
    assert _same(q_rows.float().cpu().numpy(), RT.operand(list(vec), idx.cpu().numpy(), q.ld, bf16)[0])
    s = bn.stats()
    total, per = RT.losses(want['sq'], 0.25, B * T4, E)
    assert s['S'] == S and s['K'] == K and len(s['stages']) == S and abs(s['loss_vq'] - total) <= 1e-6 * total
    for st, w, plane in zip(s['stages'], per, idx.cpu().numpy()):
        assert abs(st['loss_vq'] - w) <= 1e-6 * w and st['used'] == len(set(plane.tolist())) and 1.0 <= st['perplexity'] <= K + 1e-9


def _oracle_z(esd, x_bft):
    """The oracle's 'continues' encoding [B, E, T'] (tests/test_gpu_vq_train.py's)."""
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import zs_oracle as O
    _, pre = O.encoder_forward(esd, x_bft, NS, 0.0, SIZES['E'] // 2, SIZES['seg_len'])
    return torch.nn.functional.leaky_relu(pre, NS)


def _oracle_step(esd, dsd, x_bft, c, codes, idx, beta, dt):
    """loss_rec, loss_vq and the gradients of one step in precision dt: the quantiser is z + (sum_s code_s[idx_s] - z).detach() with the
    given idx, and every stage commits its input z - sum_{t<s} code_t[idx_t] (detached codewords) to its codeword."""
    import zs_oracle as O
    ep = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in esd.items()}
    dp = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in dsd.items()}
    z = _oracle_z(ep, x_bft.to(dt))                                                     # [B, E, T']
    B, E, T4 = z.shape
    qs = [torch.from_numpy(code[i]).to(dt).view(B, T4, E).permute(0, 2, 1) for code, i in zip(codes, idx)]
    q = qs[0]
    for t in qs[1:]:
        q = q + t
    x_dec = O.decoder_forward(dp, z + (q - z).detach(), c, NS, SIZES['seg_len'])
    l_rec = O.l1_loss(x_dec, x_bft.to(dt))
    l_vq, r = 0.0, z
    for t in qs:
        r = r - t.detach()
        l_vq = l_vq + beta * (r ** 2).mean()
    (l_rec + l_vq).backward()
    return l_rec.item(), l_vq.item(), {k: v.grad for k, v in ep.items()}, {k: v.grad for k, v in dp.items()}


def test_one_iteration_against_the_oracle(dev):
    """tests/test_gpu_vq_train.py test_one_iteration_against_the_oracle's sizes and bounds: |loss - reference| < 1e-5 on both losses and
    gradients within 2e-3 of the tensor's largest |reference|; before the device is compared, the fp32 oracle must lie within a tenth
    of those bounds of the same oracle in fp64.  Without the commitment term Encoder.linear.weight's gradient is outside the bound."""
    from zs_amd.trainer import AEStep
    enc, dec = _nets(dev, seed=0)
    esd = {k: v.detach().cpu() for k, v in enc.state_dict().items()}
    dsd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    B, T_, beta = 3, 32, 0.25
    x = torch.rand(B, T_, SIZES['c_in'], generator=g) * 0.98 + 1e-3
    c = torch.randint(0, SIZES['n_spk'], (B,), generator=g)
    with torch.no_grad():
        z64 = _oracle_z({k: v.double() for k, v in esd.items()}, x.permute(0, 2, 1).double())
    rows = z64.permute(0, 2, 1).reshape(-1, SIZES['E']).numpy()                         # [B T', E]: 12 rows
    rs = np.random.RandomState(3)
    code0 = (rows[[0, 3, 6, 9, 11]] * (1.0 + 0.2 * rs.standard_normal((5, SIZES['E'])))).astype(F32)
    left = rows - code0[R.assign(rows, code0)[0]]
    code1 = (left[[1, 4, 7, 10, 2]] * (1.0 + 0.2 * rs.standard_normal((5, SIZES['E'])))).astype(F32)
    codes = [code0, code1]
    bn = _bottleneck(dev, np.stack(codes), len(rows), beta=beta)
    ae = AEStep(enc, dec, lr=1e-4, max_grad_norm=5.0, use_graph=False, vq=bn)
    loss = ae.step(x.to(dev), c.to(dev), update=False)
    torch.cuda.synchronize()
    idx = bn.idx.cpu().numpy()
    near = R.near_rows(rows.astype(F32), code0)
    assert np.array_equal(idx[0][~near], R.assign(rows, code0)[0][~near]) and all(len(set(p.tolist())) >= 2 for p in idx)
    assert np.array_equal(bn.code_live.cpu().numpy(), np.stack(codes)) and not np.array_equal(bn.code.cpu().numpy(), np.stack(codes))
    xb = x.permute(0, 2, 1)
    r32, v32, ge32, gd32 = _oracle_step(esd, dsd, xb, c, codes, idx, beta, torch.float32)
    r64, v64, ge64, gd64 = _oracle_step(esd, dsd, xb, c, codes, idx, beta, torch.float64)
    assert abs(r32 - r64) < 1e-6 and abs(v32 - v64) < 1e-6
    picks = (('enc', enc, ge32, ge64, 'linear.weight'), ('enc', enc, ge32, ge64, 'conv2.weight'), ('dec', dec, gd32, gd64, 'conv1.weight'))
    for name, net, g32, g64, k in picks:
        scale = g64[k].abs().max().item()
        assert scale > 1e-6 and (g32[k].double() - g64[k]).abs().max().item() <= 2e-4 * scale, 'the fp32 oracle is ill-conditioned here'
    lv = float(bn.loss[0].item())
    print('loss_rec %.7f (oracle %.7f, |d| %.3g)  loss_vq %.7f (oracle %.7f, |d| %.3g)' % (loss.item(), r32, abs(loss.item() - r32), lv, v32, abs(lv - v32)))
    assert abs(loss.item() - r32) < 1e-5 and abs(lv - v32) < 1e-5
    for name, net, g32, g64, k in picks:
        ref = g32[k].double()
        scale = ref.abs().max().item()
        e = (net.grad_view(k).detach().cpu().double() - ref).abs().max().item() / scale
        print('grad %s.%s: relative error %.3g of scale %.3g' % (name, k, e, scale))
        assert e < 2e-3
    # the commitment term is in that gradient: without it linear.weight's gradient is outside the bound
    _, _, ge0, _ = _oracle_step(esd, dsd, xb, c, codes, idx, 0.0, torch.float64)
    k = 'linear.weight'
    assert (ge0[k] - ge64[k]).abs().max().item() > 2e-3 * ge64[k].abs().max().item()
    assert (enc.grad_view(k).detach().cpu().double() - ge0[k]).abs().max().item() > 2e-3 * ge0[k].abs().max().item()
    st = bn.stats()
    assert st['K'] == 5 and st['used'] == [len(set(p.tolist())) for p in idx] and abs(st['loss_vq'] - v64) < 1e-5


def _run_five(dev, graph_warmup, dtype):
    from zs_amd.trainer import AEStep
    enc, dec = _nets(dev, dtype=dtype, seed=0, dp=0.5)
    B, T_ = 4, 32
    vec = np.stack([R.planted(7, SIZES['E'], 4, 0.3, 2) * F32(0.1), R.planted(7, SIZES['E'], 4, 0.3, 3) * F32(0.02)])
    bn = _bottleneck(dev, vec, B * 4, decay=0.5, dtype=dtype, restart=0.9)       # (an unused codeword is dead after one step)
    ae = AEStep(enc, dec, lr=1e-3, max_grad_norm=5.0, use_graph=True, vq=bn)
    ae.graph_warmup = graph_warmup
    g = torch.Generator().manual_seed(1)
    losses = []
    for _ in range(5):
        x = torch.rand(B, T_, SIZES['c_in'], generator=g).to(dev)
        c = torch.randint(0, SIZES['n_spk'], (B,), generator=g).to(dev)
        losses.append((ae.step(x, c).item(),) + tuple(bn.loss.cpu().tolist()))
    torch.cuda.synchronize()
    state = [enc.flat_params()[0], dec.flat_params()[0]] + [getattr(ae.opt[k], a) for k in ('enc', 'dec') for a in ('m', 'v')] + \
        [bn.code, bn.cnorm, bn.N, bn.m, bn.idx, bn.stat]
    s = bn.stats()
    assert min(s['used']) >= 1 and bn.steps == (5 if graph_warmup > 5 else 3)          # (a replay does not pass through forward())
    return losses, [t.clone() for t in state], len(ae._graphs), s['restarts']


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_captured_equals_eager_and_a_rerun(dev, dtype):
    la, sa, na, ra = _run_five(dev, 2, dtype)
    lb, sb, nb, rb = _run_five(dev, 10 ** 9, dtype)
    lc, sc, nc, rc = _run_five(dev, 2, dtype)
    assert na == nc == 1 and nb == 0
    assert la == lb == lc, (la, lb, lc)
    for a, b, c in zip(sa, sb, sc):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert ra == rb == rc and ra >= 1                                                   # the restarts ran, inside the captured step too
    assert len({l[0] for l in la}) == 5 and all(np.isfinite(v) and v > 0 for l in la for v in l)


def _mixture(seed, n=600, E=8, K=4):
    """A planted three-level mixture: centres randn (8, 1, 1/8), noise 0.004; the starting codebooks are the centres perturbed by 2 % of
    each level's scale."""
    rs = np.random.RandomState(seed)
    scales = (8.0, 1.0, 0.125)
    centres = [rs.standard_normal((K, E)) * sc for sc in scales]
    rows = sum(c[rs.randint(0, K, n)] for c in centres) + 0.004 * rs.standard_normal((n, E))
    start = np.stack([c + 0.02 * sc * rs.standard_normal((K, E)) for c, sc in zip(centres, scales)])
    return rows.astype(F32), start.astype(F32)


def test_the_codebooks_follow_their_stages(dev):
    """RvqBottleneck.forward alone on fixed rows, 60 iterations at decay 0.5.  Once every stage's assignment has stopped changing, N and
    m approach cnt and the sum of the stage's input rows geometrically, so code = m / N is their mean up to decay^s of a unit-sized
    start after s stable iterations (s >= 25: 3e-8) plus fp32 rounding and what the stage before still moved its input by: within
    1e-5 of the fp64 mean of the residual rows the codeword took (the rows as the last step's cascade formed them)."""
    n, E, K, S = 600, 8, 4, 3
    rows, start = _mixture(0, n, E, K)
    bn = _bottleneck(dev, start, n, decay=0.5)
    bits = _rows_act(bn, rows, 6, 100)
    seen = []
    for _ in range(60):
        bn.forward(bits)
        seen.append(bn.idx.cpu().numpy().copy())
    stable = 0
    while stable < 59 and np.array_equal(seen[-1 - stable - 1], seen[-1]):
        stable += 1
    assert stable >= 25, 'an assignment was still moving %d iterations before the end' % stable
    live, code = bn.code_live.cpu().numpy(), bn.code.cpu().numpy()
    c = RT.cascade(rows, list(live), idxs=seen[-1])
    worst = 0.0
    for s in range(S):
        used = np.unique(seen[-1][s])
        assert len(used) >= 2
        for k in used:
            mean = c['r'][s][seen[-1][s] == k].astype(np.float64).mean(0)
            err = np.abs(code[s, k] - mean).max()
            worst = max(worst, err)
            print('stage %d codeword %d: %d rows, |code - mean| = %.3g (|mean| %.3g)' % (s, k, (seen[-1][s] == k).sum(), err, np.abs(mean).max()))
            assert err <= 1e-5
    print('stable for %d iterations, worst %.3g' % (stable, worst))
    bn.stats()


# ---- the steps without it --------------------------------------------------------------------------------------------------------------
def test_steps_without_the_residual_bottleneck_call_none_of_its_entry_points(dev, monkeypatch):
    from zs_amd import _lib as L, layers
    from zs_amd.trainer import AEStep
    from zs_amd.vq import VectorCodebook
    from zs_amd.vq_train import VqBottleneck
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
    assert len(names) > 50 and not [n for n in names + direct if n.startswith('zs_rvq') or n.startswith('zs_vq')]
    new = ('zs_rvq_commit', 'zs_rvq_loss', 'zs_rvq_st_bwd')
    ae.vq = VqBottleneck(VectorCodebook(R.planted(5, SIZES['E'], 4, 0.3, 2) * F32(0.1), {'enc_mode': 'continues'}), 0.25, 0.99, 12,
                         layers.Ctx(dev, 'fp32'))
    del names[:], direct[:]
    ae.step(x, c)                                                                       # the --vq_train step: none of the three new ones
    torch.cuda.synchronize()
    assert [n for n in names if n.startswith('zs_vq')] == ['zs_vq_assign', 'zs_vq_commit', 'zs_vq_accum', 'zs_vq_ema', 'zs_vq_st_bwd']
    assert not [n for n in names + direct if n in new or n.startswith('zs_rvq')]
    ae.vq = _bottleneck(dev, np.stack([R.planted(5, SIZES['E'], 4, 0.3, 2) * F32(0.1), R.planted(5, SIZES['E'], 4, 0.3, 3) * F32(0.01)]), 12)
    del names[:]
    ae.step(x, c)
    torch.cuda.synchronize()
    stage = ['zs_vq_assign', 'zs_rvq_commit', 'zs_vq_accum', 'zs_vq_ema']
    assert [n for n in names if n.startswith('zs_vq') or n.startswith('zs_rvq')] == stage * 2 + ['zs_rvq_loss', 'zs_rvq_gather', 'zs_rvq_st_bwd']


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_main_rvq_train_then_convert_with_the_trained_codebook(dev, tmp_path, monkeypatch, capsys):
    from scipy.io import wavfile
    sys.path.insert(0, ROOT)
    import main as M
    from zs_amd import convert as cv, layers, rvq as V, vq as V1
    from zs_amd.hps import hp
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('ZS_CKPT_EVERY', '4')
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    h = json.load(open(os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')))
    h.update(n_speakers=4, n_target_speakers=2, batch_size=4, enc_pretrain_iters=4, max_to_keep=3, enc_size=8, emb_size=32, seg_len=32)
    hps_path = str(tmp_path / 'hps.json')
    json.dump(h, open(hps_path, 'w'))
    K, S = 6, 3
    start = str(tmp_path / 'K6x3.rvq.npz')
    vec = np.stack([R.planted(K, 8, 4, 0.3, 4 + s) * F32(0.1 * 0.3 ** s) for s in range(S)]).astype(F32)
    V.ResidualCodebook(vec, {'enc_mode': 'continues', 'seed': 0}).save(start)
    ck = tmp_path / 'ck'
    M.main(['--train_ae', '--synthetic', '--enc_mode', 'continues', '--hps_path', hps_path, '--ckpt_dir', str(ck), '--dtype', 'fp32',
            '--rvq_train', start, '--vq_decay', '0.9', '--vq_restart', '0.5'])
    out = capsys.readouterr().out
    assert 'pre_AE:[000004/000004]' in out and 'loss_vq=' in out and 'used2=' in out and 'perplexity2=' in out and 'restarts=' in out
    cb_path = str(ck / 'model.pth-ae-4.rvq.npz')
    cb = V1.load_codebook(cb_path, 'continues', E=8)
    assert isinstance(cb, V.ResidualCodebook) and (cb.S, cb.K, cb.E) == (S, K, 8) and not np.array_equal(cb.vectors, vec)
    assert cb.meta['trained_iterations'] == 4 and cb.meta['beta'] == 0.25 and cb.meta['decay'] == 0.9 and cb.meta['restart'] == 0.5
    assert len(cb.meta['used']) == S and all(1 <= u <= K for u in cb.meta['used'])
    assert cb.meta['enc_mode'] == 'continues' and os.path.exists(str(ck / 'model.pth-ae-4')) and not os.path.exists(str(ck / 'model.pth-ae-4.vq.npz'))
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
    for stages in (1, S):
        res = tmp_path / ('result%d' % stages)
        M.main(['--convert_dir', str(d), '--t_speaker', 'V001', '--result_dir', str(res), '--codebook', cb_path, '--rvq_stages', str(stages), '--enc_only',
                '--hps_path', hps_path, '--speaker2id_path', s2id, '--ckpt_pth', str(ck / 'model.pth-ae-4'), '--enc_mode', 'continues',
                '--g_mode', 'targeted_residual'])
        conv = os.path.join(os.path.join(str(res), './english/'), 'convert')
        for s in ('w0', 'w1'):
            idx = cv.read_index_rows(os.path.join(conv, 'V001', s + '.idx.txt'), K, S)      # raises for an index outside [0, K)
            assert idx.shape[1] == stages and len(idx) >= 2 and idx.min() >= 0 and idx.max() < K
            assert os.path.getsize(os.path.join(conv, 'V001', s + '.wav')) > 44
    layers.check_status(dev)
