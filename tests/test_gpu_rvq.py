"""The residual vector codebook on the device:

* zs_rvq_residual and zs_rvq_gather against the numpy definition of tests/rvq_ref.py with array_equal, guards behind every row and
  every buffer, every ZS_EINVAL case, and zs_rvq_gather at S = 1 against zs_vq_gather bit for bit;
* ResidualCodebook.snap stage by stage: every stage's indices under tests/vq_ref.py's bound on that stage's input, every residual
  bit-equal to the definition given the device's indices, on both zs_vq_assign decompositions;
* fit_residual stage by stage through on_stage, its reproducibility, the falling distortion and the planted mixture of two scales;
* encode_batch / resynth_batch / synth_index_batch / the unit files with a residual codebook on the tiny 'continues' trainer: the
  Decoder reads cast(reconstruct(idx)); main.py --fit_codebook --rvq, --convert_dir and --synth_dir --rvq_stages on a temporary folder;
* with a plain vector codebook or none, conversion launches no zs_rvq_* entry point."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import rvq_ref as Q  # noqa: E402
import vq_ref as R  # noqa: E402

GUARD = 64
SENT = -7.25                                  # what every output buffer holds before a launch
U = 2.0 ** -24
BAD_IDX = (-1, None, 2 ** 30, -2 ** 31)       # None: K


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pitched(rows, ld, fill):
    """[n, E] -> flat fp32 of n rows at pitch ld + GUARD, the slack and the guard filled."""
    n, E = rows.shape
    buf = np.full(n * ld + GUARD, fill, dtype=np.float32)
    buf[:n * ld].reshape(n, ld)[:, :E] = rows
    return buf


def _bf16_round(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).float().numpy()


def _r4(E):
    return (E + 3) // 4 * 4


def _criterion(x, code, cn, idx, dist=None):
    """tests/test_gpu_vq.py's assignment criterion (the derived bound of vq_ref) without its cap on near rows: x as the kernel saw it."""
    n, E = x.shape
    s, B = R.scores(x, code, cn), R.bound(x, code, cn)
    near = R.near_rows(x, code, cn)
    assert idx.min() >= 0 and idx.max() < code.shape[0]
    at = s[np.arange(n), idx]
    assert (at <= s.min(1) + 2 * B).all()
    assert np.array_equal(idx[~near], s.argmin(1)[~near])
    if dist is not None:
        xx = (x.astype(np.float64) ** 2).sum(1)
        gamma = E * U / (1 - E * U)
        assert (np.abs(dist - np.maximum(0.0, xx + at)) <= 2 * B + (gamma + 2.0 ** -22) * xx).all() and (dist >= 0).all()
    return int(near.sum())


# ---- zs_rvq_residual -----------------------------------------------------------------------------------------------------------------
def _run_residual(dev, x, idx, code, bf16=False, ld_x=None, ld_code=None, ld_r=None, in_place=False):
    """zs_rvq_residual with NaN behind every row of x and of code, the sentinel in every word of r, and guards behind all three.
    Returns (r [n, E], bad); asserts the guards, the columns past E of r and that the operands are read only."""
    from zs_amd import _lib as L
    n, E = x.shape
    K = code.shape[0]
    ld_x, ld_code, ld_r = ld_x or E, ld_code or E, ld_r or E
    xb, cb = _pitched(x, ld_x, np.nan), _pitched(code, ld_code, np.nan)
    x_d = torch.from_numpy(xb).to(dev)
    if bf16:
        x_d = x_d.to(torch.bfloat16)
    c_d = torch.from_numpy(cb).to(dev)
    i_d = torch.from_numpy(np.concatenate([np.asarray(idx, np.int32), np.full(GUARD, 0x55555555, np.int32)])).to(dev)
    if in_place:
        assert not bf16 and ld_r == ld_x
        r_d = x_d
    else:
        r_d = torch.full((n * ld_r + GUARD,), SENT, dtype=torch.float32, device=dev)
    bad = torch.full((2,), 4, dtype=torch.int32, device=dev)
    L.call('zs_rvq_residual', 'ZsRvqResidual', _stream(), dtype=(L.ZS_BF16 if bf16 else L.ZS_F32), src_f32=0, x=L.ptr(x_d), n=n, ld_x=ld_x,
           idx=L.ptr(i_d), code=L.ptr(c_d), ld_code=ld_code, K=K, E=E, r=L.ptr(r_d), ld_r=ld_r, bad=L.ptr(bad))
    torch.cuda.synchronize()
    out = r_d.cpu().numpy()
    rows = out[:n * ld_r].reshape(n, ld_r)
    want_rest = xb if in_place else np.full(n * ld_r + GUARD, SENT, np.float32)
    probe = out.copy()
    probe[:n * ld_r].reshape(n, ld_r)[:, :E] = want_rest[:n * ld_r].reshape(n, ld_r)[:, :E]
    assert np.array_equal(probe, want_rest, equal_nan=True)              # past E, behind every row and behind the buffer: untouched
    assert np.array_equal(c_d.cpu().numpy(), cb, equal_nan=True) and int(bad[1]) == 4
    if not in_place:
        assert np.array_equal(x_d.float().cpu().numpy(), xb, equal_nan=True)
    return rows[:, :E].copy(), int(bad[0]) - 4


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('n,E,K', [(1, 1, 1), (37, 6, 5), (65, 20, 37), (300, 64, 300), (130, 1024, 129)])
def test_residual_equals_the_definition(dev, n, E, K, bf16):
    """Pitches equal to E (16-byte pieces where E is a multiple of 4), E + odd (element by element) and a multiple of 4 above E (16-byte
    pieces with a ragged last one); indices -1, K, 2^30 and -2^31 are counted and their rows copied."""
    pool = R.planted(n + K, E, 8, 1.0, 8)
    x, code = pool[:n], pool[n:]
    if bf16:
        x = _bf16_round(x)
    rs = np.random.RandomState(n + E)
    idx = rs.randint(0, K, size=n).astype(np.int64)
    n_bad = 0
    if n >= 8:
        for at, k in zip((0, 3, n // 2, n - 1), BAD_IDX):
            idx[at] = K if k is None else k
        n_bad = 4
    want, w_bad = Q.residual(x, idx, code)
    assert w_bad == n_bad and (n_bad == 0 or np.array_equal(want[3], x[3]))
    for ld_x, ld_code, ld_r in ((E, E, E), (E + 1, E + 3, E + 1), (_r4(E) + 4, _r4(E) + 8, _r4(E) + 4)):
        got, bad = _run_residual(dev, x, idx.astype(np.int32), code, bf16=bf16, ld_x=ld_x, ld_code=ld_code, ld_r=ld_r)
        assert bad == n_bad and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        if not bf16:
            got, bad = _run_residual(dev, x, idx.astype(np.int32), code, ld_x=ld_x, ld_code=ld_code, ld_r=ld_x, in_place=True)
            assert bad == n_bad and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if n == 1:                                                             # the single row with an index that is none
        for k in (-1, K, 2 ** 30, -2 ** 31):
            got, bad = _run_residual(dev, x, np.array([k], np.int32), code, bf16=bf16)
            assert bad == 1 and np.array_equal(got, x)


def test_residual_rounds_once_and_keeps_signed_zero(dev):
    """x - c in fp32: one rounding (neither 1 - 2^-25 nor 2^25 - 1 is an fp32 value), -0 - 0 = -0, c - c = +0."""
    x = np.array([[1.0, -0.0, 3.5, 2.0 ** 25, 1e-40, 5.0]], dtype=np.float32)
    code = np.array([[2.0 ** -25, 0.0, 3.5, 1.0, 1e-40, -5.0]], dtype=np.float32)
    want, _ = Q.residual(x, [0], code)
    assert want[0, 0] == 1.0 and np.signbit(want[0, 1]) and not np.signbit(want[0, 2]) and want[0, 3] == np.float32(2.0 ** 25)
    got, _ = _run_residual(dev, x, np.array([0], np.int32), code)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_rvq_argument_errors_launch_nothing(dev):
    from zs_amd import _lib as L
    E, n, K = 20, 50, 7
    x = torch.full((n, E), 0.5, device=dev)
    xh = torch.full((n, E), 0.5, device=dev, dtype=torch.bfloat16)
    code = torch.full((3, K, E), 0.25, device=dev)
    idx = torch.zeros(3, n, dtype=torch.int32, device=dev)
    r = torch.full((n, E), SENT, device=dev)
    bad = torch.full((2,), 5, dtype=torch.int32, device=dev)
    ok = dict(dtype=L.ZS_F32, src_f32=0, x=L.ptr(x), n=n, ld_x=E, idx=L.ptr(idx), code=L.ptr(code), ld_code=E, K=K, E=E, r=L.ptr(r), ld_r=E,
              bad=L.ptr(bad))
    for change in (dict(K=0), dict(K=-1), dict(K=65537), dict(E=0), dict(E=1025), dict(E=-3), dict(n=-1), dict(n=2 ** 31), dict(ld_x=E - 1),
                   dict(ld_code=E - 1), dict(ld_r=E - 1), dict(x=None), dict(idx=None), dict(code=None), dict(r=None), dict(bad=None),
                   dict(dtype=5), dict(x=L.ptr(x) + 2), dict(dtype=L.ZS_BF16, x=L.ptr(xh) + 1), dict(idx=L.ptr(idx) + 2),
                   dict(code=L.ptr(code) + 1), dict(r=L.ptr(r) + 2), dict(bad=L.ptr(bad) + 1),
                   dict(r=L.ptr(x), ld_r=E + 4), dict(dtype=L.ZS_BF16, x=L.ptr(xh), r=L.ptr(xh))):       # in place: fp32 and equal pitches alone
        with pytest.raises(L.ZsError, match='zs_rvq_residual'):
            L.call('zs_rvq_residual', 'ZsRvqResidual', _stream(), **dict(ok, **change))
    L.call('zs_rvq_residual', 'ZsRvqResidual', _stream(), **dict(ok, n=0, x=None, idx=None, code=None, r=None, bad=None))    # n == 0 succeeds
    dst = torch.full((2, 4, 24), 9.0, device=dev)
    start = torch.zeros(2, dtype=torch.int64, device=dev)
    ln = torch.full((2,), 4, dtype=torch.int32, device=dev)
    ok = dict(dtype=L.ZS_F32, idx=L.ptr(idx), n_idx=n, ld_idx=n, S=3, s_use=2, code=L.ptr(code), ld_code=E, plane_code=K * E, K=K, E=E,
              start=L.ptr(start), len=L.ptr(ln), n_frag=2, T=4, dst=L.ptr(dst), ld_dst=24, bad=L.ptr(bad))
    for change in (dict(K=0), dict(K=65537), dict(E=0), dict(E=1025), dict(S=0), dict(S=9), dict(s_use=0), dict(s_use=4), dict(S=-1),
                   dict(ld_idx=n - 1), dict(plane_code=(K - 1) * E + E - 1), dict(idx=None), dict(code=None), dict(start=None), dict(len=None),
                   dict(dst=None), dict(bad=None), dict(ld_dst=16), dict(ld_dst=20), dict(ld_code=E - 1), dict(n_idx=-1), dict(n_frag=-1),
                   dict(n_frag=1048577), dict(T=0), dict(dtype=7), dict(dst=L.ptr(dst) + 8), dict(idx=L.ptr(idx) + 2),
                   dict(start=L.ptr(start) + 4), dict(code=L.ptr(code) + 2)):
        with pytest.raises(L.ZsError, match='zs_rvq_gather'):
            L.call('zs_rvq_gather', 'ZsRvqGather', _stream(), **dict(ok, **change))
    L.call('zs_rvq_gather', 'ZsRvqGather', _stream(), **dict(ok, n_frag=0, dst=None, start=None, len=None))
    for fn in ('zs_rvq_residual', 'zs_rvq_gather'):
        assert getattr(L.lib(), fn)(None, None) == L.ZS_EINVAL              # a null struct
    torch.cuda.synchronize()
    assert (x == 0.5).all() and (code == 0.25).all() and (r == SENT).all() and (bad == 5).all() and (dst == 9.0).all() and (idx == 0).all()


# ---- zs_rvq_gather -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('E,ld', [(6, 8), (20, 24), (20, 32), (64, 64), (1024, 1024)])
def test_gather_equals_the_definition(dev, E, ld, bf16):
    """S in {1, 2, 3, 8} and every s_use <= S; fragments of unequal length with T padding; the codebooks dense (16-byte loads) and at
    an odd pitch (element by element).  A bad index in a used stage: a zero row counted once; in an unused stage: ignored."""
    from zs_amd import rvq as V
    K, T, n_idx = 5, 9, 60
    start = np.array([0, 9, 14, 14, 55, 58, -1, 36, 0, 5], dtype=np.int64)
    length = np.array([9, 5, 0, 9, 5, 3, 2, 7, 10, -1], dtype=np.int32)    # ragged; 55 + 5 = 60 fits, 58 + 3 does not, len > T, len < 0
    dt = torch.bfloat16 if bf16 else torch.float32
    rs = np.random.RandomState(E + ld)
    for S in (1, 2, 3, 8):
        codes = np.stack([R.planted(K, E, 8, 1.0, 2 + s) * np.float32(3.0 ** -s) for s in range(S)])
        idx = rs.randint(0, K, size=(S, n_idx + 4)).astype(np.int32)       # planes 4 entries further apart than they are long
        idx[:, n_idx:] = 0x55555555
        idx[0, 3], idx[S - 1, 17], idx[S // 2, 40], idx[0, 41] = K, -1, 2 ** 30, -2 ** 31
        idx[S - 1, 41] = K + 1                                             # two bad indices in one frame: counted once
        for dense in (True, False):
            ld_code = E if dense else E + 1
            plane = K * ld_code + (0 if dense else 3)
            cbuf = np.full(S * plane + GUARD, np.nan, np.float32)
            for s in range(S):
                cbuf[s * plane:s * plane + K * ld_code].reshape(K, ld_code)[:, :E] = codes[s]
            c_d = torch.from_numpy(cbuf).to(dev)
            code_t = torch.as_strided(c_d, (S, K, E), (plane, ld_code, 1))
            i_d = torch.from_numpy(idx).to(dev)
            for s_use in range(1, S + 1):
                dst = torch.full((len(start) * T * ld + GUARD,), 9.0, dtype=dt, device=dev)
                bad = torch.full((2,), 4, dtype=torch.int32, device=dev)
                V.gather(i_d[:, :n_idx], s_use, code_t, torch.from_numpy(start).to(dev), torch.from_numpy(length).to(dev), T,
                         dst[:len(start) * T * ld].view(len(start), T, ld), bad)
                torch.cuda.synchronize()
                want, n_bad = Q.gather(idx[:, :n_idx], list(codes), s_use, start, length, T, ld)
                assert int(bad[0]) == 4 + n_bad and int(bad[1]) == 4 and (dst[len(start) * T * ld:] == 9.0).all()
                got = dst[:len(start) * T * ld].view(len(start), T, ld).cpu()
                exp = torch.from_numpy(want).to(dt)                        # torch's cast: round to nearest even, once
                view = torch.int16 if bf16 else torch.int32
                assert torch.equal(got.view(view), exp.view(view)), (S, s_use, dense)
                assert (got[..., E:] == 0).all() and all((got[f] == 0).all() for f in (2, 5, 6, 8, 9))
            assert np.array_equal(c_d.cpu().numpy(), cbuf, equal_nan=True)
        # used stages hold the bad frames 3, 41 (stage 0), 40 (stage S // 2), 17 and 41 again (stage S - 1)
        used_all = Q.gather(idx[:, :n_idx], list(codes), S, start, length, T, ld)[1]
        used_one = Q.gather(idx[:, :n_idx], list(codes), 1, start, length, T, ld)[1]
        assert used_one >= 2 and (S == 1 or used_all > used_one)


@pytest.mark.parametrize('bf16', [False, True])
def test_gather_with_one_stage_is_zs_vq_gather(dev, bf16):
    from zs_amd import rvq as V, vq as V1
    E, ld, K, T = 20, 24, 37, 9
    code = R.planted(K, E, 8, 1.0, 2)
    code[3, 4] = -0.0
    idx = np.random.RandomState(1).randint(0, K, size=60).astype(np.int32)
    idx[3], idx[17], idx[40] = K, -1, 2 ** 30
    start = torch.tensor([0, 9, 14, 14, 55, 58, -1, 36, 0, 5], dtype=torch.int64, device=dev)
    length = torch.tensor([9, 5, 0, 9, 5, 3, 2, 7, 10, -1], dtype=torch.int32, device=dev)
    dt = torch.bfloat16 if bf16 else torch.float32
    outs = []
    for which in (0, 1):
        dst = torch.full((10, T, ld), 9.0, dtype=dt, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        c_d, i_d = torch.from_numpy(code).to(dev), torch.from_numpy(idx).to(dev)
        if which:
            V.gather(i_d[None], 1, c_d[None], start, length, T, dst, bad)
        else:
            V1.gather(i_d, c_d, start, length, T, dst, bad)
        torch.cuda.synchronize()
        outs.append((dst.cpu(), int(bad)))
    view = torch.int16 if bf16 else torch.int32
    assert torch.equal(outs[0][0].view(view), outs[1][0].view(view)) and outs[0][1] == outs[1][1] == 3


# ---- ResidualCodebook.snap -----------------------------------------------------------------------------------------------------------
def _stage_codes(K, E, S, seed):
    return np.stack([R.planted(K, E, 8, 1.0, seed + s) * np.float32(0.5 ** s) for s in range(S)])


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('n,E,K,S', [(1000, 20, 300, 3), (65, 64, 37, 2), (130, 1024, 165, 2), (63, 6, 1, 3)])
def test_snap_stage_by_stage(dev, n, E, K, S, bf16):
    """Stage 0 sees test_gpu_vq.py's inputs (rows and K further rows of vq_ref.planted(.., 8, 1.0, 8)) under its cap on near rows; every
    later stage's input is the device's residual, bit-equal to the definition given the device's indices, and its indices meet the
    same bound on that input.  Two runs and both zs_vq_assign decompositions give the same planes."""
    from zs_amd import rvq as V, vq as V1
    pool = R.planted(n + K, E, 8, 1.0, 8)
    x = _bf16_round(pool[:n]) if bf16 else pool[:n]
    codes = _stage_codes(K, E, S, 40)
    codes[0] = pool[n:]
    cb = V.ResidualCodebook(codes)
    assert R.near_rows(x, codes[0], cb.cnorm[0]).sum() <= 0.02 * n          # the cap, on the definition alone, before the device is looked at
    x_d = torch.from_numpy(x).to(dev)
    x_d = x_d.to(torch.bfloat16) if bf16 else x_d
    res = []
    idx, dist = cb.snap(x_d, work=V1.workspace(dev), residuals=res)
    idx_h, dist_h = idx.cpu().numpy(), dist.cpu().numpy()
    assert idx_h.shape == (S, n) and idx_h.dtype == np.int32 and dist_h.shape == (S, n) and len(res) == S - 1
    want = Q.snap_given(x, list(codes), list(idx_h))
    for s in range(S):
        if s:
            assert np.array_equal(res[s - 1].cpu().numpy().view(np.uint32), want[s].view(np.uint32))
        near = _criterion(want[s], codes[s], cb.cnorm[s], idx_h[s], dist_h[s])
        print('n %d E %d K %d stage %d: %d near rows' % (n, E, K, s, near))
    again, dist2 = cb.snap(x_d, work=V1.workspace(dev))
    rows, dist3 = cb.snap(x_d, work=None)                                  # the row decomposition
    assert torch.equal(again, idx) and torch.equal(rows, idx) and torch.equal(dist2, dist) and torch.equal(dist3, dist)
    for s_use in range(1, S + 1):                                          # the embedded code: the first s' planes are the s'-stage snap
        part, dpart = cb.snap(x_d, stages=s_use)
        assert torch.equal(part, idx[:s_use]) and torch.equal(dpart, dist[:s_use])
    got = cb.reconstruct(idx_h)
    assert np.array_equal(got.view(np.uint32), Q.reconstruct(idx_h, list(codes))[0].view(np.uint32))
    with pytest.raises(ValueError, match=r'stages must be in \[1, S = %d\]' % S):
        cb.snap(x_d, stages=S + 1)


# ---- fit_residual --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,E,K,S', [(600, 8, 4, 3), (1000, 20, 37, 2)])
def test_fit_residual_stage_by_stage(dev, n, E, K, S):
    from zs_amd import rvq as V, vq as V1
    x = R.planted(n, E, 8, 1.0, 21)
    x_d = torch.from_numpy(x).to(dev)
    stages = []
    cb = V.fit_residual(x_d, K, S, iters=40, seed=5, on_stage=lambda s, d: stages.append(d))
    assert np.array_equal(x_d.cpu().numpy(), x) and (cb.S, cb.K, cb.E) == (S, K, E) and len(stages) == S == len(cb.meta['stages'])
    rows = x
    for s, d in enumerate(stages):
        assert np.array_equal(d['rows'].view(np.uint32), rows.view(np.uint32))          # the definition's residual of the device's indices
        one = V1.fit_vectors(torch.from_numpy(rows).to(dev), K, iters=40, seed=5 + s)     # the stage is fit_vectors of those rows, seed + s
        assert np.array_equal(d['code'].view(np.uint32), one.vectors.view(np.uint32)) and np.array_equal(cb.vectors[s], d['code'])
        assert d['history'] == one.meta['history']
        _criterion(rows, d['code'], R.cnorm(d['code']), d['idx'], d['dist'])             # assigned again, under the fitted codebook
        m = cb.meta['stages'][s]
        assert abs(m['summed_distance'] - d['dist'].astype(np.float64).sum()) <= 1e-9 * m['summed_distance']
        assert m['symbols_used'] == len(set(d['idx'].tolist())) and m['history'] == d['history'] and 0.0 <= m['bits_per_unit'] <= np.log2(K) + 1e-12
        rows = Q.residual(rows, d['idx'], d['code'])[0]
    totals = [m['summed_distance'] for m in cb.meta['stages']]
    print('n %d E %d K %d: summed distance by stage %s' % (n, E, K, totals))
    # a stage's means leave at most what it was given; the slack is the one tests/test_gpu_vq.py allows on a summed distance
    assert all(b <= a * (1 + 1e-9) for a, b in zip(totals, totals[1:]))
    assert abs(cb.meta['bits_per_unit'] - sum(m['bits_per_unit'] for m in cb.meta['stages'])) < 1e-12
    ref_codes, ref = Q.fit(x, K, S, iters=40, seed=5)
    if all(st['near'] == 0 for st in ref):                                 # no near row anywhere in the definition: the whole fit is equal
        print('  whole-fit equality applies')
        for s in range(S):
            assert np.array_equal(ref[s]['idx'], stages[s]['idx']) and np.array_equal(ref_codes[s].view(np.uint32), cb.vectors[s].view(np.uint32))
    again = V.fit_residual(x_d, K, S, iters=40, seed=5)
    assert np.array_equal(again.vectors.view(np.uint32), cb.vectors.view(np.uint32)) and again.meta == cb.meta
    for bad_s in (1, 9):
        with pytest.raises(ValueError, match=r'fit_residual: S must be in \[2, 8\]'):
            V.fit_residual(x_d, K, bad_s)


def test_two_stages_beat_one_on_a_planted_mixture(dev):
    """Coarse centres with fine offsets (tests/test_rvq_host.py checks the property on the definition first)."""
    from zs_amd import rvq as V
    x = Q.planted2(1200, 8, 8, 0.05, 31)
    cb = V.fit_residual(torch.from_numpy(x).to(dev), 8, 2, iters=40, seed=0)
    one, two = (m['summed_distance'] for m in cb.meta['stages'])
    print('planted mixture: one stage %.6g, two stages %.6g' % (one, two))
    assert two < one


# ---- through the conversion paths ----------------------------------------------------------------------------------------------------
SEG = 32
FRAMES = [200, 75, 45, 33, 90, 5]           # tests/test_gpu_vq.py's batch: five on the unit-fragment rule and one below MIN_LEN
SPK = [2, 3, 2, 3, 2, 3]


def _trainer(path, dtype='fp32', g_mode='targeted_residual', enc_mode='continues', seed=3):
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    torch.manual_seed(seed)
    hps = make_hps(enc_size=8, emb_size=32, n_speakers=4, n_target_speakers=2, seg_len=SEG)
    return Trainer(hps, None, g_mode, enc_mode, log_dir=os.path.join(str(path), 'log'), dtype=dtype, device=torch.device('cuda:0')), hps


def _specs(frames, seed=7):
    rng = np.random.RandomState(seed)
    return [(rng.rand(n, 513) * 0.98 + 1e-3).astype(np.float32) for n in frames]


@pytest.fixture(scope='module')
def cont(dev, tmp_path_factory):
    """cont(dtype): the tiny 'continues' trainer of that dtype, the batch, its encodings without a codebook and the residual codebooks
    (K = 16, S = 3) and (K = 1, S = 2) fitted to them (built once per dtype)."""
    from zs_amd import convert as cv, rvq as V
    made = {}

    def get(dtype):
        if dtype not in made:
            tr, _ = _trainer(tmp_path_factory.mktemp('rvq_' + dtype), dtype=dtype)
            specs = _specs(FRAMES)
            e, _ = cv.encode_batch(specs, tr, SEG)
            rows = torch.from_numpy(np.concatenate(e)).to(dev)
            made[dtype] = dict(tr=tr, specs=specs, e=e, dtype=dtype, cb16=V.fit_residual(rows, 16, 3, iters=10, seed=1),
                               cb1=V.fit_residual(rows, 1, 2, iters=3, seed=1))
        return made[dtype]
    return get


def _decode_from_indices(cv, tr, cb, idx, spk):
    """Decoder.forward of cast(reconstruct(idx)), fragment by fragment as unit_fragments cuts the utterance: [8 U, 513] fp32."""
    out, at = [], 0
    q = cb.reconstruct(idx.T)
    for n in cv.unit_fragments(len(idx), SEG):
        x = torch.from_numpy(q[at:at + n].T.copy()).unsqueeze(0).to(tr.device)                           # [1, E, n]
        out.append(tr.Decoder(x, torch.tensor([spk])).permute(0, 2, 1)[0].float().cpu().numpy())
        at += n
    return np.concatenate(out, axis=0)


@pytest.mark.parametrize('K,S', [(16, 3), (1, 2)])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_conversion_decodes_the_sum_of_the_codewords(dev, cont, tmp_path, dtype, K, S):
    from zs_amd import convert as cv, layers
    cont = cont(dtype)
    tr, specs, e, full = cont['tr'], cont['specs'], cont['e'], cont['cb%d' % K]
    assert (full.S, full.K, full.E) == (S, K, 8)
    dt = torch.float32 if dtype == 'fp32' else torch.bfloat16
    for s_use in (1, S):
        cb = full.with_stages(s_use)
        es, dd, idxs = cv.encode_batch(specs, tr, SEG, decode_speakers=SPK, codebook=cb, want_idx=True)
        assert [i.shape for i in idxs] == [(len(a), s_use) for a in e] and all(i.dtype == np.int32 and i.min() >= 0 and i.max() < K for i in idxs)
        assert all(a.dtype == np.float32 and np.array_equal(a, full.reconstruct(i.T)) for a, i in zip(es, idxs))
        # the planes are the snap of the encoder's rows as the engine holds them (its compute dtype)
        for a, i in zip(e, idxs):
            got, _ = full.snap(torch.from_numpy(a).to(dev).to(dt), stages=s_use)
            assert np.array_equal(got.cpu().numpy().T, i)
        if s_use == S and S > 1:                                           # the first column is the one-stage run's: an embedded code
            one = cv.encode_batch(specs, tr, SEG, codebook=full.with_stages(1), want_idx=True)[2]
            assert all(np.array_equal(a[:, :1], b) for a, b in zip(idxs, one))
        # the decoded spectrogram is Decoder.forward of cast(reconstruct(idx)), bit for bit
        for u in range(5):
            want = _decode_from_indices(cv, tr, full, idxs[u], SPK[u])
            assert dd[u].shape == want.shape and np.array_equal(dd[u], want)
        # the input shorter than MIN_LEN: one row of indices is returned, both units of its zero-padded form are decoded
        padded = np.concatenate([specs[5], np.zeros((cv.MIN_LEN - len(specs[5]), 513), np.float32)])
        both = cv.encode_batch([padded], tr, SEG)[0][0]
        i2 = full.snap(torch.from_numpy(both).to(dev).to(dt), stages=s_use)[0].cpu().numpy().T
        assert len(both) == 2 and np.array_equal(i2[0], idxs[5][0]) and len(idxs[5]) == 1
        want = _decode_from_indices(cv, tr, full, i2, SPK[5])
        assert np.array_equal(dd[5], want) and len(want) == 16
        side = cb.units()
        for enc_only in (True, False):                                     # without and with the generator
            er, wr, ir, total = cv.resynth_batch(specs, tr, SEG, SPK, n_iter=4, enc_only=enc_only, codebook=cb, want_idx=True)
            assert all(np.array_equal(a, b) for a, b in zip(ir, idxs)) and all(np.array_equal(a, b) for a, b in zip(er, es))
            assert np.size(total) == s_use and (np.asarray(total) >= 0).all()      # the distance left behind every used stage
            _, dg = cv.encode_batch(specs, tr, SEG, decode_speakers=SPK, enc_only=enc_only, codebook=cb)
            s5, _ = cv.synth_index_batch(idxs[:5], tr, SEG, SPK[:5], full, enc_only=enc_only, n_iter=4, want_specs=True)
            assert all(np.array_equal(a, b) for a, b in zip(dg[:5], s5))
            if enc_only:
                assert all(np.array_equal(a, b) for a, b in zip(dg, dd))
            # the unit files conversion writes, read back and spoken: the same waveforms
            units = []
            for u in range(5):
                p = str(tmp_path / ('u%d_%d_%d.idx.txt' % (u, s_use, enc_only)))
                side.write_idx(p, idxs[u])
                units.append(side.read_unit_file(p, 8))
                assert np.array_equal(units[-1], idxs[u])
            _, w5 = side.speak(units, tr, SEG, SPK[:5], enc_only=enc_only, n_iter=4)
            assert all(len(a) > 0 and np.array_equal(a, b) for a, b in zip(wr[:5], w5))
        # --test_encode's writer: the .txt as without a codebook, s' indices per line beside it
        txt = str(tmp_path / ('enc_%d.txt' % s_use))
        side.write_encoded(txt, e[0], dev)
        assert np.array_equal(cv.read_index_rows(cv.idx_path(txt), K, S), full.snap(torch.from_numpy(e[0]).to(dev), stages=s_use)[0].cpu().numpy().T)
        assert len(open(txt).read().splitlines()) == len(e[0])
    if S == 3:                                                             # files of different widths in one folder group: each with its own columns
        mixed = [idxs[0][:, :1].copy(), idxs[1], idxs[2][:, :2].copy()]
        _, wm = full.units().speak(mixed, tr, SEG, SPK[:3], n_iter=4)
        for u, m in enumerate(mixed):
            _, w1 = cv.synth_index_batch([m], tr, SEG, SPK[u:u + 1], full, n_iter=4)
            assert np.array_equal(wm[u], w1[0])
    layers.check_status(dev)


def test_residual_refusals_come_before_any_launch(dev, cont, tmp_path, monkeypatch):
    from zs_amd import _lib as L, convert as cv, rvq as V
    cont = cont('fp32')
    tr, specs, cb = cont['tr'], cont['specs'], cont['cb16']
    bits_tr, _ = _trainer(tmp_path, enc_mode='multilabel_binary')
    wide = V.ResidualCodebook(np.stack([R.planted(4, 20, 2, 0.3, s) for s in range(2)]))
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda *a, **k: (calls.append(a[0]), real(*a, **k))[1])
    good = [np.array([[0, 1], [1, 2], [2, 3]], np.int32), np.array([[3, 3], [3, 0]], np.int32)]
    for fn in (lambda c, t: cv.encode_batch(specs[:2], t, SEG, codebook=c),
               lambda c, t: cv.resynth_batch(specs[:2], t, SEG, SPK[:2], n_iter=4, codebook=c),
               lambda c, t: cv.synth_index_batch(good, t, SEG, SPK[:2], c, n_iter=4)):
        with pytest.raises(ValueError, match='field E is 20'):
            fn(wide, tr)
        with pytest.raises(ValueError, match=r"residual codebook serves enc_mode 'continues'.*multilabel_binary"):
            fn(cb, bits_tr)
    for bad, match in (([np.array([[0, 16]] * 2, np.int32)] * 2, r'outside \[0, K = 16\)'), ([np.array([[0, -1]] * 2, np.int32)] * 2, 'outside'),
                       ([np.array([[1, 1]], np.int32)] * 2, 'fewer than 2'), ([np.array([0, 1], np.int32)] * 2, r'integers \[U, 1 \.\. S = 3\]'),
                       ([np.zeros((2, 4), np.int32)] * 2, r'integers \[U, 1 \.\. S = 3\]'), ([np.zeros((2, 2))] * 2, 'integers'),
                       ([good[0], good[1][:, :1]], '1 indices per frame where utterance 0 has 2'), (good[:1], '2 target speakers for 1')):
        with pytest.raises(ValueError, match=match):
            cv.synth_index_batch(bad, tr, SEG, SPK[:2], cb)
    assert calls == []


def test_without_a_residual_codebook_no_rvq_entry_point_is_launched(dev, cont, monkeypatch):
    from zs_amd import _lib as L, convert as cv, vq as V1
    cont = cont('fp32')
    tr, specs, cb = cont['tr'], cont['specs'], cont['cb16']
    plain = V1.VectorCodebook(cb.vectors[0])
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda *a, **k: (calls.append(a[0]), real(*a, **k))[1])
    for codebook in (None, plain):
        del calls[:]
        cv.resynth_batch(specs, tr, SEG, SPK, n_iter=4, codebook=codebook)
        cv.encode_batch(specs, tr, SEG, decode_speakers=SPK, codebook=codebook, enc_only=False)
        if codebook is not None:
            cv.synth_index_batch([np.array([0, 1, 2], np.int32)], tr, SEG, SPK[:1], codebook, n_iter=4)
        assert len(calls) > 10 and not [c for c in calls if c.startswith('zs_rvq')]
        assert (codebook is None) == (not [c for c in calls if c.startswith('zs_vq')])
    del calls[:]
    _, _, idxs = cv.encode_batch(specs, tr, SEG, decode_speakers=SPK, codebook=cb, want_idx=True)
    names = [c for c in calls if c.startswith(('zs_vq', 'zs_rvq'))]
    chunks = names.count('zs_rvq_gather')
    assert chunks >= 1 and names.count('zs_vq_assign') == 3 * chunks and names.count('zs_rvq_residual') == 2 * chunks
    assert 'zs_vq_gather' not in names
    del calls[:]
    cv.encode_batch(specs, tr, SEG, decode_speakers=SPK, codebook=cb.with_stages(1))                     # one stage: nothing left over to form
    names = [c for c in calls if c.startswith(('zs_vq', 'zs_rvq'))]
    assert 'zs_rvq_residual' not in names and names.count('zs_vq_assign') == names.count('zs_rvq_gather') == chunks


def test_main_fit_convert_and_synth_with_a_residual_codebook(dev, cont, tmp_path, monkeypatch):
    from scipy.io import wavfile
    sys.path.insert(0, ROOT)
    import main as M
    from zs_amd import convert as cv, layers, rvq as V, vq as V1
    from zs_amd.hps import hp, make_hps
    tr = cont('fp32')['tr']
    hps = make_hps(enc_size=8, emb_size=32, n_speakers=4, n_target_speakers=2, seg_len=SEG)
    rng = np.random.RandomState(5)
    d = tmp_path / 'in'
    d.mkdir()
    for i, n in enumerate((14000, 9000, 20000, 12000)):              # short synthetic wavs: a gliding tone and noise
        t = np.arange(n) / 16000.0
        y = 0.3 * np.sin(2 * np.pi * (200.0 + 150.0 * i + 400.0 * t) * t) + 0.05 * rng.randn(n)
        wavfile.write(str(d / ('w%d.wav' % i)), 16000, (y * 32767).astype(np.int16))
    s2id = str(tmp_path / 'speaker2id.json')
    json.dump({'S015': 0, 'S020': 1, 'V001': 2, 'V002': 3}, open(s2id, 'w'))
    hps_path = str(tmp_path / 'hps.json')
    json.dump(hps._asdict(), open(hps_path, 'w'))
    tr.save_model(str(tmp_path / 'model.pth'), 's2', 1)
    monkeypatch.setattr(hp, 'n_iter', 4)
    common = ['--hps_path', hps_path, '--speaker2id_path', s2id, '--ckpt_pth', str(tmp_path / 'model.pth-s2-1'), '--g_mode', 'targeted_residual',
              '--enc_mode', 'continues']
    ckpt = tmp_path / 'ckpt'
    M.main(['--fit_codebook', '8', '--rvq', '2', '--fit_dir', str(d), '--ckpt_dir', str(ckpt), '--codebook_iters', '10', '--codebook_seed', '2']
           + common)
    cb_path = str(ckpt / 'codebooks' / 'K8x2.rvq.npz')
    cb = V1.load_codebook(cb_path, 'continues', E=8)
    rep = json.load(open(str(ckpt / 'codebooks' / 'fit_codebook.json')))
    assert isinstance(cb, V.ResidualCodebook) and (cb.S, cb.K, cb.E, cb.meta['seed']) == (2, 8, 8, 2)
    assert rep['kind'] == 'residual' and rep['S'] == 2 and len(rep['stages']) == 2 and rep['stages'] == cb.meta['stages']
    assert rep['n_units'] == sum(f['units'] for f in rep['files']) == cb.meta['n_rows'] and rep['history'] == cb.meta['history']
    assert rep['stages'][1]['summed_distance'] <= rep['stages'][0]['summed_distance'] * (1 + 1e-9)
    assert abs(rep['entropy_bits_per_unit'] - sum(s['bits_per_unit'] for s in rep['stages'])) < 1e-12 and 0 <= rep['entropy_bits_per_unit'] <= 6.0
    res = tmp_path / 'result'
    M.main(['--convert_dir', str(d), '--t_speaker', 'V001,V002', '--result_dir', str(res), '--codebook', cb_path] + common)
    out = os.path.join(os.path.join(str(res), './english/'), 'convert')
    man = json.load(open(os.path.join(out, 'convert_dir.json')))['codebook']
    assert man['file'] == cb_path and man['K'] == 8 and man['S'] == 2 and len(man['stages']) == 2
    assert man['stages'][1]['mean_distance'] <= man['stages'][0]['mean_distance'] and man['mean_distance'] == man['stages'][1]['mean_distance']
    idx_dir = tmp_path / 'idx'
    idx_dir.mkdir()
    for s in ('w0', 'w1', 'w2', 'w3'):
        for t in ('V001', 'V002'):
            base = os.path.join(out, t, s)
            rows = cv.read_index_rows(base + '.idx.txt', 8, 2)
            assert os.path.getsize(base + '.wav') > 44 and rows.shape == (len(open(base + '.txt').read().splitlines()), 2)
    for s in ('w0', 'w1'):                                           # the index files it wrote, spoken from their first stage
        (idx_dir / (s + '.idx.txt')).write_text(open(os.path.join(out, 'V001', s + '.idx.txt')).read())
    (idx_dir / 'bad.idx.txt').write_text('1 2\n9 0\n')
    (idx_dir / 'thin.idx.txt').write_text('1\n2\n3\n')
    M.main(['--synth_dir', str(idx_dir), '--t_speaker', 'V001', '--result_dir', str(res), '--codebook', cb_path, '--rvq_stages', '1'] + common)
    syn = os.path.join(os.path.join(str(res), './english/'), 'synth')
    man = json.load(open(os.path.join(syn, 'synth_dir.json')))
    assert sorted(os.path.basename(it['input']) for it in man['items']) == ['thin.idx.txt', 'w0.idx.txt', 'w1.idx.txt']
    assert [os.path.basename(s['input']) for s in man['skipped']] == ['bad.idx.txt'] and len(man['codebook']['stages']) == 1
    for s in ('w0', 'w1'):
        spoken = cv.read_index_rows(os.path.join(syn, 'V001', s + '.idx.txt'), 8, 2)
        assert np.array_equal(spoken, cv.read_index_rows(os.path.join(out, 'V001', s + '.idx.txt'), 8, 2)[:, :1])
        assert os.path.getsize(os.path.join(syn, 'V001', s + '.wav')) > 44
    syn2 = tmp_path / 'result2'
    M.main(['--synth_dir', str(idx_dir), '--t_speaker', 'V001', '--result_dir', str(syn2), '--codebook', cb_path, '--rvq_stages', '2'] + common)
    man = json.load(open(os.path.join(str(syn2), './english/', 'synth', 'synth_dir.json')))
    thin = [s for s in man['skipped'] if os.path.basename(s['input']) == 'thin.idx.txt']
    assert len(thin) == 1 and 'c = 1' in thin[0]['reason'] and 's = 2' in thin[0]['reason'] and 'thin.idx.txt' in thin[0]['reason']
    # a file conversion wrote, read as --synth_dir reads it and spoken with every column: what synth_index_batch gives for its rows
    full = cv.read_index_rows(os.path.join(out, 'V001', 'w0.idx.txt'), 8, 2)
    _, wa = cv.synth_index_batch([full], tr, SEG, [2], cb, n_iter=4)
    _, wb = cb.units().speak([cb.units().read_unit_file(os.path.join(out, 'V001', 'w0.idx.txt'), 8)], tr, SEG, [2], n_iter=4)
    assert np.array_equal(wa[0], wb[0])
    layers.check_status(dev)
