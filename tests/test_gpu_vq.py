"""The vector codebook on the device:

* zs_vq_assign against the fp64 scores of tests/vq_ref.py under the derived bound, on both decompositions, and the tie rule exactly;
* zs_vq_accum / zs_vq_update / zs_vq_gather against the definition with array_equal;
* zs_amd.vq.fit_vectors step by step, and codebook by codebook where the definition has no near row;
* encode_batch / resynth_batch / synth_index_batch with a vector codebook on the tiny 'continues' trainer: the Decoder reads code[idx];
* main.py --fit_codebook, --convert_dir --codebook and --synth_dir --codebook for 'continues' on a temporary folder."""
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

GUARD = 64
FILL_I = -0x55555556
U = 2.0 ** -24


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pitched(rows, ld, fill):
    """[n, E] -> flat fp32 of n rows at pitch ld + GUARD, the slack and the guard filled (NaN: a read behind a row poisons a score)."""
    n, E = rows.shape
    buf = np.full(n * ld + GUARD, fill, dtype=np.float32)
    buf[:n * ld].reshape(n, ld)[:, :E] = rows
    return buf


def _bf16_round(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).float().numpy()


def _run_assign(dev, x, code, cn, bf16=False, ld_x=None, ld_code=None, skip=(), split=True, idx0=None, moved0=7):
    """zs_vq_assign with guards behind every row and every output.  x must hold values exact in its dtype.  Returns dict(idx, dist,
    moved) as numpy; asserts the guards and that the operands are read only."""
    from zs_amd import _lib as L, vq as V
    n, E = x.shape
    K = code.shape[0]
    ld_x, ld_code = ld_x or E, ld_code or E
    xb, cb = _pitched(x, ld_x, np.nan), _pitched(code, ld_code, np.nan)
    x_d = torch.from_numpy(xb).to(dev)
    if bf16:
        x_d = x_d.to(torch.bfloat16)
    c_d = torch.from_numpy(cb).to(dev)
    cn_d = torch.from_numpy(np.concatenate([cn, np.full(GUARD, np.nan, np.float32)])).to(dev)
    idx = torch.full((n + GUARD,), FILL_I, dtype=torch.int32, device=dev)
    if idx0 is not None:
        idx[:n] = torch.from_numpy(idx0).to(dev)
    dist = torch.full((n + GUARD,), -7.0, dtype=torch.float32, device=dev)
    moved = torch.full((2,), moved0, dtype=torch.int32, device=dev)
    work = V.workspace(dev) if split else None
    kw = dict(dtype=(L.ZS_BF16 if bf16 else L.ZS_F32), x=L.ptr(x_d), n=n, ld_x=ld_x, code=L.ptr(c_d), ld_code=ld_code, cnorm=L.ptr(cn_d), K=K, E=E,
              idx=L.ptr(idx), dist=L.ptr(dist), moved=L.ptr(moved), count_moved=1, work=L.ptr(work),
              work_bytes=(V.WORK_BYTES if split else 0))
    for k in skip:
        kw[k] = None
        if k in ('idx', 'moved'):
            kw['count_moved'] = 0
    L.call('zs_vq_assign', 'ZsVqAssign', _stream(), **kw)
    torch.cuda.synchronize()
    assert (idx[n:] == FILL_I).all() and (dist[n:] == -7.0).all() and int(moved[1]) == moved0
    assert np.array_equal(c_d.cpu().numpy(), cb, equal_nan=True)
    assert np.array_equal(x_d.float().cpu().numpy(), xb, equal_nan=True)
    return dict(idx=idx[:n].cpu().numpy(), dist=dist[:n].cpu().numpy(), moved=int(moved[0]) - moved0)


def _criterion(x, code, cn, idx, dist=None, cap=True):
    """The assignment criterion of the derived bound; x as the kernel saw it (exact values), cn the fp32 norms it was given."""
    n, E = x.shape
    s, B = R.scores(x, code, cn), R.bound(x, code, cn)
    near = R.near_rows(x, code, cn)
    print('n %d E %d K %d: %d near rows' % (n, E, code.shape[0], int(near.sum())))
    if cap:
        assert near.sum() <= 0.02 * n, 'bad input: %d of %d rows are near' % (near.sum(), n)      # before the device is looked at
    assert idx.min() >= 0 and idx.max() < code.shape[0]
    at = s[np.arange(n), idx]
    worst = float(((at - s.min(1)) / np.maximum(2 * B, 1e-300)).max())
    print('  worst (s(k^) - min s) / 2B = %.3g' % worst)
    assert (at <= s.min(1) + 2 * B).all()
    assert np.array_equal(idx[~near], s.argmin(1)[~near])
    if dist is not None:
        xx = (x.astype(np.float64) ** 2).sum(1)
        gamma = E * U / (1 - E * U)
        err = np.abs(dist - np.maximum(0.0, xx + at))
        tol = 2 * B + (gamma + 2.0 ** -22) * xx
        print('  worst dist error / tolerance = %.3g' % float((err / np.maximum(tol, 1e-300)).max()))
        assert (err <= tol).all() and (dist >= 0).all()


def _case(n, E, K, seed=8):
    """Rows and K further rows of the same generator as codewords.  The seeds used keep every case inside the cap on near rows, which
    _criterion asserts on the definition alone."""
    pool = R.planted(n + K, E, 8, 1.0, seed)
    return pool[:n], pool[n:]


# ---- zs_vq_assign --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('E', [6, 20, 64, 1024])
def test_assign_meets_the_bound_on_both_decompositions(dev, E, bf16):
    """K = 165 is one tile of codewords plus 37, K = 300 three tiles (three workgroups per row tile when split)."""
    for n in (1, 63, 64, 65, 1000):
        for K in ((1, 2, 37, 165, 300) if E == 1024 else (1, 2, 37, 300)):
            x, code = _case(n, E, K)
            if bf16:
                x = _bf16_round(x)
            cn = R.cnorm(code)
            got = _run_assign(dev, x, code, cn, bf16=bf16, idx0=np.full(n, -1, np.int32))
            _criterion(x, code, cn, got['idx'], got['dist'])
            assert got['moved'] == n
            rows = _run_assign(dev, x, code, cn, bf16=bf16, split=False)
            assert np.array_equal(rows['idx'], got['idx']) and np.array_equal(rows['dist'], got['dist'])       # bitwise, both paths


@pytest.mark.parametrize('K', [37, 300])
def test_assign_around_the_split_threshold(dev, K):
    from zs_amd import vq as V
    E = 20
    for n in (V.SPLIT_N - 1, V.SPLIT_N, V.SPLIT_N + 1):
        x, code = _case(n, E, K, seed=7)
        cn = R.cnorm(code)
        got = _run_assign(dev, x, code, cn)
        _criterion(x, code, cn, got['idx'], got['dist'])
        rows = _run_assign(dev, x, code, cn, split=False)
        assert np.array_equal(rows['idx'], got['idx']) and np.array_equal(rows['dist'], got['dist'])


def test_assign_pitches_null_outputs_moved_and_reruns(dev):
    E, n, K = 20, 130, 300
    x, code = _case(n, E, K, seed=7)
    cn = R.cnorm(code)
    full = _run_assign(dev, x, code, cn, idx0=np.full(n, -1, np.int32))
    _criterion(x, code, cn, full['idx'], full['dist'])
    for split in (True, False):
        for ld_x, ld_code in ((E, E), (E + 3, E + 1), (24, 32)):          # unaligned pitches, and 16-byte aligned ones behind E
            got = _run_assign(dev, x, code, cn, ld_x=ld_x, ld_code=ld_code, split=split)
            assert np.array_equal(got['idx'], full['idx']) and np.array_equal(got['dist'], full['dist'])
        for name in ('idx', 'dist', 'moved'):
            got = _run_assign(dev, x, code, cn, skip=(name,), split=split, idx0=np.full(n, -1, np.int32))
            if name != 'idx':
                assert np.array_equal(got['idx'], full['idx'])
            else:
                assert (got['idx'] == -1).all()
            if name != 'dist':
                assert np.array_equal(got['dist'], full['dist'])
            else:
                assert (got['dist'] == -7.0).all()
            assert got['moved'] == (n if name == 'dist' else 0)
        # moved over two calls: nothing moves against the same codebook; then exactly the rows whose codeword changes
        again = _run_assign(dev, x, code, cn, split=split, idx0=full['idx'])
        assert again['moved'] == 0 and np.array_equal(again['idx'], full['idx'])
        code2 = code.copy()
        code2[full['idx'][0]] += 50.0                                      # the winner of row 0 leaves
        other = _run_assign(dev, x, code2, R.cnorm(code2), split=split, idx0=full['idx'])
        assert other['moved'] == int((other['idx'] != full['idx']).sum()) >= 1
    xb = _bf16_round(x)
    a, b = _run_assign(dev, xb, code, cn, bf16=True, ld_x=E + 1), _run_assign(dev, xb, code, cn, bf16=True, ld_x=24)
    assert np.array_equal(a['idx'], b['idx']) and np.array_equal(a['dist'], b['dist'])


@pytest.mark.parametrize('split', [True, False])
def test_assign_ties_go_to_the_lowest_index(dev, split):
    """Duplicate codewords (identical rows, identical cnorm) score bitwise equal: the lower index wins inside an accumulator, across the
    accumulators of a tile, across the tile boundary at 128 and, split, across the workgroups that hold the two tiles."""
    E, K, n = 20, 300, 200
    rs = np.random.RandomState(3)
    code = rs.standard_normal((K, E)).astype(np.float32)
    pairs = [(5, 9), (5, 70), (20, 133), (100, 299), (130, 131), (140, 260)]
    for lo, hi in pairs[1:]:
        code[hi] = code[lo]
    code[9] = code[5]
    dup_hi = sorted({hi for _, hi in pairs})
    x = code[rs.randint(K, size=n)] + 0.01 * rs.standard_normal((n, E)).astype(np.float32)
    for j, (lo, hi) in enumerate(pairs):
        x[j] = code[hi]
    x = x.astype(np.float32)
    cn = R.cnorm(code)
    got = _run_assign(dev, x, code, cn, split=split)
    _criterion(x, code, cn, got['idx'], got['dist'], cap=False)
    assert not np.isin(got['idx'], dup_hi).any()
    assert got['idx'][:len(pairs)].tolist() == [5, 5, 20, 100, 130, 140]
    want, _ = R.assign(x, code, cn)
    assert np.array_equal(got['idx'], want)                               # well separated apart from the ties


def test_vq_argument_errors_launch_nothing(dev):
    from zs_amd import _lib as L, vq as V
    E, n, K = 20, 50, 7
    x = torch.full((n, E), 0.5, device=dev)
    code = torch.full((K, E), 0.25, device=dev)
    cn = torch.full((K,), 1.25, device=dev)
    idx = torch.full((n,), -7, dtype=torch.int32, device=dev)
    dist = torch.full((n,), -7.0, device=dev)
    moved = torch.full((2,), 5, dtype=torch.int32, device=dev)
    work = V.workspace(dev)
    work.fill_(3)
    ok = dict(dtype=L.ZS_F32, x=L.ptr(x), n=n, ld_x=E, code=L.ptr(code), ld_code=E, cnorm=L.ptr(cn), K=K, E=E, idx=L.ptr(idx), dist=L.ptr(dist),
              moved=L.ptr(moved), count_moved=1, work=L.ptr(work), work_bytes=V.WORK_BYTES)
    for change in (dict(K=0), dict(K=-1), dict(K=65537), dict(E=0), dict(E=1025), dict(E=-3), dict(x=None), dict(code=None), dict(cnorm=None),
                   dict(ld_x=E - 1), dict(ld_code=E - 1), dict(n=-1), dict(dtype=5), dict(idx=L.ptr(idx) + 2), dict(dist=L.ptr(dist) + 1),
                   dict(x=L.ptr(x) + 2), dict(code=L.ptr(code) + 1), dict(work=L.ptr(work) + 4), dict(idx=None), dict(moved=None),
                   dict(K=300, work_bytes=8 * n), dict(work_bytes=-1)):
        with pytest.raises(L.ZsError, match='zs_vq_assign'):
            L.call('zs_vq_assign', 'ZsVqAssign', _stream(), **dict(ok, **change))
    L.call('zs_vq_assign', 'ZsVqAssign', _stream(), **dict(ok, n=0, x=None, code=None, cnorm=None))          # n == 0 succeeds
    torch.cuda.synchronize()
    assert (idx == -7).all() and (dist == -7.0).all() and (moved == 5).all() and (work == 3).all()
    cnt = torch.full((K,), 3, dtype=torch.int32, device=dev)
    sums = torch.full((K, E), 2, dtype=torch.int64, device=dev)
    idx.zero_()
    ok = dict(x=L.ptr(x), idx=L.ptr(idx), n=n, ld_x=E, K=K, E=E, shift=3, cnt=L.ptr(cnt), sum=L.ptr(sums), bad=L.ptr(moved))
    for change in (dict(K=0), dict(K=65537), dict(E=0), dict(E=1025), dict(x=None), dict(idx=None), dict(cnt=None), dict(sum=None), dict(bad=None),
                   dict(ld_x=E - 1), dict(n=-1), dict(shift=63), dict(shift=-65), dict(cnt=L.ptr(cnt) + 2), dict(sum=L.ptr(sums) + 4)):
        with pytest.raises(L.ZsError, match='zs_vq_accum'):
            L.call('zs_vq_accum', 'ZsVqAccum', _stream(), **dict(ok, **change))
    L.call('zs_vq_accum', 'ZsVqAccum', _stream(), **dict(ok, n=0, x=None, idx=None))
    ok = dict(code=L.ptr(code), ld_code=E, cnorm=L.ptr(cn), K=K, E=E, shift=3, cnt=L.ptr(cnt), sum=L.ptr(sums), changed=L.ptr(moved, 1))
    for change in (dict(K=0), dict(K=65537), dict(E=0), dict(E=1025), dict(code=None), dict(cnorm=None), dict(cnt=None), dict(sum=None),
                   dict(changed=None), dict(ld_code=E - 1), dict(shift=63), dict(sum=L.ptr(sums) + 4)):
        with pytest.raises(L.ZsError, match='zs_vq_update'):
            L.call('zs_vq_update', 'ZsVqUpdate', _stream(), **dict(ok, **change))
    dst = torch.full((2, 4, 24), 9.0, device=dev)
    start = torch.zeros(2, dtype=torch.int64, device=dev)
    ln = torch.full((2,), 4, dtype=torch.int32, device=dev)
    ok = dict(dtype=L.ZS_F32, idx=L.ptr(idx), n_idx=n, code=L.ptr(code), ld_code=E, K=K, E=E, start=L.ptr(start), len=L.ptr(ln), n_frag=2, T=4,
              dst=L.ptr(dst), ld_dst=24, bad=L.ptr(moved))
    for change in (dict(K=0), dict(K=65537), dict(E=0), dict(E=1025), dict(idx=None), dict(code=None), dict(start=None), dict(len=None),
                   dict(dst=None), dict(bad=None), dict(ld_dst=16), dict(ld_dst=20), dict(ld_code=E - 1), dict(n_idx=-1), dict(n_frag=-1),
                   dict(n_frag=1048577), dict(T=0), dict(dtype=7), dict(dst=L.ptr(dst) + 8), dict(idx=L.ptr(idx) + 2)):
        with pytest.raises(L.ZsError, match='zs_vq_gather'):
            L.call('zs_vq_gather', 'ZsVqGather', _stream(), **dict(ok, **change))
    L.call('zs_vq_gather', 'ZsVqGather', _stream(), **dict(ok, n_frag=0, dst=None, start=None, len=None))
    for fn, sname in (('zs_vq_assign', 'ZsVqAssign'), ('zs_vq_accum', 'ZsVqAccum'), ('zs_vq_update', 'ZsVqUpdate'), ('zs_vq_gather', 'ZsVqGather')):
        assert getattr(L.lib(), fn)(None, None) == L.ZS_EINVAL             # a null struct
    torch.cuda.synchronize()
    assert (cnt == 3).all() and (sums == 2).all() and (moved == 5).all() and (code == 0.25).all() and (x == 0.5).all() and (cn == 1.25).all()
    assert (dst == 9.0).all() and (idx == 0).all()


# ---- zs_vq_accum / zs_vq_update -------------------------------------------------------------------------------------------------------
def _accum_update(dev, x, idx, code, shift, ld_x=None, ld_code=None):
    """One accum + update on the device, checked against the definition with array_equal (cnorm within 1 fp32 ulp)."""
    from zs_amd import _lib as L
    n, E = x.shape
    K = code.shape[0]
    ld_x, ld_code = ld_x or E, ld_code or E
    xb, cb = _pitched(x, ld_x, np.nan), _pitched(code, ld_code, 0.125)
    x_d, c_d = torch.from_numpy(xb).to(dev), torch.from_numpy(cb).to(dev)
    i_d = torch.from_numpy(np.asarray(idx, dtype=np.int32)).to(dev)
    cnt = torch.zeros(K + GUARD, dtype=torch.int32, device=dev)
    sums = torch.zeros(K * E + GUARD, dtype=torch.int64, device=dev)
    cn = torch.full((K + GUARD,), -3.0, device=dev)
    misc = torch.zeros(4, dtype=torch.int32, device=dev)                  # bad, changed, two guards
    L.call('zs_vq_accum', 'ZsVqAccum', _stream(), x=L.ptr(x_d), idx=L.ptr(i_d), n=n, ld_x=ld_x, K=K, E=E, shift=shift, cnt=L.ptr(cnt),
           sum=L.ptr(sums), bad=L.ptr(misc))
    L.call('zs_vq_update', 'ZsVqUpdate', _stream(), code=L.ptr(c_d), ld_code=ld_code, cnorm=L.ptr(cn), K=K, E=E, shift=shift, cnt=L.ptr(cnt),
           sum=L.ptr(sums), changed=L.ptr(misc, 1))
    torch.cuda.synchronize()
    assert (cnt[K:] == 0).all() and (sums[K * E:] == 0).all() and (misc[2:] == 0).all() and (cn[K:] == -3.0).all()
    w_cnt, w_sum, w_bad = R.accum(x, idx, K, shift)
    assert np.array_equal(cnt[:K].cpu().numpy(), w_cnt) and int(misc[0]) == w_bad
    assert np.array_equal(sums[:K * E].cpu().numpy().reshape(K, E), w_sum)
    w_code, w_cn, w_changed = R.update(code, w_cnt, w_sum, shift)
    out = c_d.cpu().numpy()
    assert np.array_equal(out[:K * ld_code].reshape(K, ld_code)[:, :E].view(np.uint32), w_code.view(np.uint32))
    assert np.array_equal(out, _pitched(w_code, ld_code, 0.125))          # the slack of a pitch and the guard are not touched
    assert int(misc[1]) == w_changed
    g_cn = cn[:K].cpu().numpy()
    assert (np.abs(g_cn.astype(np.float64) - w_cn.astype(np.float64)) <= np.spacing(w_cn)).all()
    return w_cnt, w_sum


@pytest.mark.parametrize('n,E,K', [(5000, 20, 37), (3000, 1024, 40), (9000, 6, 300), (700, 64, 3)])
def test_accum_update_equal_the_definition(dev, n, E, K):
    """E = 1024: 6 tiles of 7 codewords; n = 5000 and 9000: several row slices.  One cluster holds 90 % of the rows, the last cluster
    is empty (its codeword stays), and a few indices are bad."""
    from zs_amd import vq as V
    x = R.planted(n, E, 8, 1.0, 5)
    rs = np.random.RandomState(n)
    idx = np.where(rs.rand(n) < 0.9, K // 2, rs.randint(0, max(1, K - 1), size=n)).astype(np.int32)
    idx[idx == K - 1] = 0
    idx[::97] = K
    idx[5::211] = -1
    idx[7] = 2 ** 30
    code = R.planted(K, E, 8, 1.0, 6)
    for shift in (0, V.vq_shift(n, float(np.abs(x).max()))):
        cnt, _ = _accum_update(dev, x, idx, code, shift, ld_x=E + (3 if E < 1024 else 0), ld_code=E + 1)
        assert cnt[K // 2] >= 0.85 * n and (K < 3 or cnt[K - 1] == 0)


def test_update_rounds_a_sum_above_2_53_to_even(dev):
    """A few thousand equal rows at a large shift and one row of a few units of 2^-shift: the int64 sum has more than 53 significant
    bits (the units land below the double's last place: under, at and over its half), so int64 -> double rounds."""
    n, E, K, shift = 4001, 8, 2, 42
    x = np.tile(np.array([1.7, -1.3, 0.9, 3.1, -2.7, 1.1, 0.3, 1.9], dtype=np.float32), (n, 1))
    x[1234] = np.array([1, -2, 3, 5, -6, 7, 9, 10], dtype=np.float32) * np.float32(2.0 ** -shift)
    idx = np.zeros(n, dtype=np.int32)
    _, s = _accum_update(dev, x, idx, np.zeros((K, E), np.float32), shift)
    assert (np.abs(s[0]) > 2 ** 53).sum() >= 4 and (s[0].astype(np.float64).astype(np.int64) != s[0]).any()


# ---- zs_vq_gather -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('E,ld', [(20, 24), (20, 32), (64, 64), (6, 8)])
def test_gather_equals_the_definition(dev, E, ld, bf16):
    from zs_amd import vq as V
    K, T = 37, 9
    code = R.planted(K, E, 8, 1.0, 2)
    rs = np.random.RandomState(E + ld)
    idx = rs.randint(0, K, size=60).astype(np.int32)
    idx[3], idx[17], idx[40] = K, -1, 2 ** 30                               # bad: zero rows
    start = np.array([0, 9, 14, 14, 55, 58, -1, 36, 0, 5], dtype=np.int64)
    length = np.array([9, 5, 0, 9, 5, 3, 2, 7, 10, -1], dtype=np.int32)    # ragged; 55 + 5 = 60 fits, 58 + 3 does not, len > T, len < 0
    dt = torch.bfloat16 if bf16 else torch.float32
    dst = torch.full((len(start) * T * ld + GUARD,), 9.0, dtype=dt, device=dev)
    bad = torch.full((2,), 4, dtype=torch.int32, device=dev)
    ld_code = E + 1
    c_d = torch.from_numpy(_pitched(code, ld_code, np.nan)).to(dev)
    V.gather(torch.from_numpy(idx).to(dev), c_d[:K * ld_code].view(K, ld_code), torch.from_numpy(start).to(dev), torch.from_numpy(length).to(dev),
             T, dst[:len(start) * T * ld].view(len(start), T, ld), bad, E=E)
    torch.cuda.synchronize()
    want, n_bad = R.gather(idx, code, start, length, T, ld)
    assert n_bad == 3 and int(bad[0]) == 4 + n_bad and int(bad[1]) == 4
    assert (dst[len(start) * T * ld:] == 9.0).all()
    got = dst[:len(start) * T * ld].view(len(start), T, ld).cpu()
    exp = torch.from_numpy(want).to(dt)                                    # torch's cast: round to nearest even
    assert torch.equal(got.view(torch.int16 if bf16 else torch.int32), exp.view(torch.int16 if bf16 else torch.int32))
    assert (got[..., E:] == 0).all() and all((got[f] == 0).all() for f in (2, 5, 6, 8, 9)) and (got[7, :7, :E] != 0).any()


# ---- fit_vectors ---------------------------------------------------------------------------------------------------------------------
# (n, E, K, s, seed of the generator, whole): whole-fit equality where the definition has no near row in any iteration
FITS = [(2000, 64, 8, 0, 10, True), (2000, 64, 8, 1, 11, True), (2000, 64, 8, 2, 12, True), (2000, 64, 37, 0, 10, True),
        (2000, 64, 37, 1, 11, True), (2000, 20, 37, 0, 10, True), (2000, 20, 37, 2, 12, True), (2000, 6, 3, 1, 11, True),
        (2000, 6, 3, 2, 12, True), (600, 1024, 8, 1, 11, True), (2000, 1024, 37, 0, 10, False), (2000, 1024, 3, 1, 11, False),
        (2000, 20, 8, 0, 10, False)]


@pytest.mark.parametrize('n,E,K,s,gen,whole', FITS)
def test_fit_vectors_step_by_step(dev, n, E, K, s, gen, whole):
    from zs_amd import vq as V
    x = R.planted(n, E, 8, 1.0, gen)
    steps = []
    cb = V.fit_vectors(torch.from_numpy(x).to(dev), K, iters=40, seed=s, on_iter=lambda i, d: steps.append(d))
    assert len(steps) == len(cb.meta['history']) <= 40 and cb.meta['history'][-1][1] == 0
    assert cb.meta['shift'] == R.vq_shift(n, np.abs(x).max())
    assert np.array_equal(steps[0]['start'], x[R.init_rows(x, K, s)])
    prev = np.full(n, -1, np.int32)
    for i, d in enumerate(steps):
        cn = R.cnorm(d['start'])
        _criterion(x, d['start'], cn, d['idx'], d['dist'])                 # against the codebook the iteration started from
        cnt, sm, _ = R.accum(x, d['idx'], K, d['shift'])
        new, new_cn, _ = R.update(d['start'], cnt, sm, d['shift'])
        assert (cnt > 0).all() and np.array_equal(d['cnt'], cnt)           # no empties in these fits
        assert np.array_equal(d['code'].view(np.uint32), new.view(np.uint32))
        assert (np.abs(d['cnorm'].astype(np.float64) - new_cn) <= np.spacing(new_cn)).all()
        h = cb.meta['history'][i]
        assert h[1] == int((d['idx'] != prev).sum()) and h[2] == 0
        assert abs(h[0] - d['dist'].astype(np.float64).sum()) <= 1e-9 * h[0]
        prev = d['idx']
        if i + 1 < len(steps):
            assert np.array_equal(steps[i + 1]['start'], d['code'])
    assert np.array_equal(cb.vectors, steps[-1]['code']) and np.array_equal(cb.cnorm, R.cnorm(cb.vectors))
    if whole:
        code, history, ref = R.fit(x, K, iters=40, seed=s)
        assert all(st['near'] == 0 for st in ref), 'precondition: the definition has a near row'
        assert len(ref) == len(steps)
        for a, b in zip(ref, steps):
            assert np.array_equal(a['idx'], b['idx']) and np.array_equal(a['code'].view(np.uint32), b['code'].view(np.uint32))
        assert np.array_equal(code, cb.vectors) and [h[1:] for h in history] == [tuple(h[1:]) for h in cb.meta['history']]


def test_fit_vectors_is_reproducible_and_snaps(dev):
    """Two fits are bitwise equal (iters cuts the fit short: the history says so), and VectorCodebook.snap is the assignment."""
    from zs_amd import vq as V
    x = R.planted(1500, 20, 8, 1.0, 4)
    a = V.fit_vectors(torch.from_numpy(x).to(dev), 37, iters=3, seed=9)
    b = V.fit_vectors(torch.from_numpy(x).to(dev), 37, iters=3, seed=9)
    assert np.array_equal(a.vectors.view(np.uint32), b.vectors.view(np.uint32)) and a.meta == b.meta
    assert len(a.meta['history']) == 3 and a.meta['history'][-1][1] > 0
    idx, dist = a.snap(torch.from_numpy(x).to(dev))
    _criterion(x, a.vectors, a.cnorm, idx.cpu().numpy(), dist.cpu().numpy())


# ---- through the conversion paths ------------------------------------------------------------------------------------------------------
SEG = 32
FRAMES = [200, 75, 45, 33, 90, 5]           # five on the unit-fragment rule (none = 0 or 1 mod 32 above 64) and one below MIN_LEN
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
    """cont(dtype): the tiny 'continues' trainer of that dtype, the batch, its encodings without a codebook and the K = 16 and K = 1
    codebooks fitted to them (built once per dtype)."""
    from zs_amd import convert as cv, vq as V
    made = {}

    def get(dtype):
        if dtype not in made:
            tr, _ = _trainer(tmp_path_factory.mktemp('cont_' + dtype), dtype=dtype)
            specs = _specs(FRAMES)
            e, _ = cv.encode_batch(specs, tr, SEG)
            rows = torch.from_numpy(np.concatenate(e)).to(dev)
            assert len(e) == 6 and len(e[5]) == 1 and sum(len(a) for a in e) >= 32 and all(a.dtype == np.float32 and a.shape[1] == 8 for a in e)
            made[dtype] = dict(tr=tr, specs=specs, e=e, dtype=dtype, cb16=V.fit_vectors(rows, 16, iters=10, seed=1),
                               cb1=V.fit_vectors(rows, 1, iters=3, seed=1))
        return made[dtype]
    return get


def _decode_from_indices(cv, tr, cb, idx, spk):
    """Decoder.forward of code[idx], fragment by fragment as unit_fragments cuts the utterance: [8 U, 513] fp32."""
    out, at = [], 0
    for n in cv.unit_fragments(len(idx), SEG):
        x = torch.from_numpy(cb.vectors[idx[at:at + n]].T.copy()).unsqueeze(0).to(tr.device)           # [1, E, n]
        out.append(tr.Decoder(x, torch.tensor([spk])).permute(0, 2, 1)[0].float().cpu().numpy())
        at += n
    return np.concatenate(out, axis=0)


@pytest.mark.parametrize('K', [16, 1])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_conversion_decodes_the_codewords_of_the_indices(dev, cont, dtype, K):
    from zs_amd import convert as cv, layers
    cont = cont(dtype)
    tr, specs, e, cb = cont['tr'], cont['specs'], cont['e'], cont['cb%d' % K]
    assert (cb.K, cb.E) == (K, 8)
    es, dd, idxs = cv.encode_batch(specs, tr, SEG, decode_speakers=SPK, codebook=cb, want_idx=True)
    assert [len(i) for i in idxs] == [len(a) for a in e] and all(i.dtype == np.int32 and i.min() >= 0 and i.max() < K for i in idxs)
    assert all(a.dtype == np.float32 and np.array_equal(a, cb.vectors[i]) for a, i in zip(es, idxs))         # the snapped vectors
    # the indices are the assignment of the encoder's rows as the engine holds them (its compute dtype)
    dt = torch.float32 if cont['dtype'] == 'fp32' else torch.bfloat16
    for a, i in zip(e, idxs):
        got, _ = cb.snap(torch.from_numpy(a).to(dev).to(dt))
        assert np.array_equal(got.cpu().numpy(), i)
        _criterion(torch.from_numpy(a).to(dt).float().numpy(), cb.vectors, cb.cnorm, i, cap=False)
    if K == 16:
        assert len({int(k) for i in idxs for k in i}) > 4                      # the codebook is used, not one symbol
    # the decoded spectrogram is Decoder.forward of code[idx], bit for bit
    for u in range(5):
        want = _decode_from_indices(cv, tr, cb, idxs[u], SPK[u])
        assert dd[u].shape == want.shape and np.array_equal(dd[u], want)
    # the input shorter than MIN_LEN: one index is returned, both units of its zero-padded form are decoded
    padded = np.concatenate([specs[5], np.zeros((cv.MIN_LEN - len(specs[5]), 513), np.float32)])
    both = cv.encode_batch([padded], tr, SEG)[0][0]
    i2 = cb.snap(torch.from_numpy(both).to(dev).to(dt))[0].cpu().numpy()
    assert len(both) == 2 and i2[0] == idxs[5][0]
    want = _decode_from_indices(cv, tr, cb, i2, SPK[5])
    assert np.array_equal(dd[5], want) and len(want) == 16
    # resynth_batch: the same encodings and indices; synth_index_batch of those indices: the same rows, the same waveforms
    for enc_only in (True, False):                                             # without and with the generator
        er, wr, ir, total = cv.resynth_batch(specs, tr, SEG, SPK, n_iter=4, enc_only=enc_only, codebook=cb, want_idx=True)
        assert all(np.array_equal(a, b) for a, b in zip(ir, idxs)) and all(np.array_equal(a, b) for a, b in zip(er, es))
        assert isinstance(total, float) and total >= 0.0
        _, dg = cv.encode_batch(specs, tr, SEG, decode_speakers=SPK, enc_only=enc_only, codebook=cb)
        s5, _ = cv.synth_index_batch(idxs[:5], tr, SEG, SPK[:5], cb, enc_only=enc_only, n_iter=4, want_specs=True)
        assert all(np.array_equal(a, b) for a, b in zip(dg[:5], s5))
        if enc_only:
            assert all(np.array_equal(a, b) for a, b in zip(dg, dd))
        _, w5 = cv.synth_index_batch(idxs[:5], tr, SEG, SPK[:5], cb, enc_only=enc_only, n_iter=4)
        assert all(len(a) > 0 and np.array_equal(a, b) for a, b in zip(wr[:5], w5))
    layers.check_status(dev)


def test_vector_codebook_refusals_come_before_any_launch(dev, cont, tmp_path, monkeypatch):
    from zs_amd import _lib as L, codebook as C, convert as cv, vq as V
    cont = cont('fp32')
    tr, specs, cb = cont['tr'], cont['specs'], cont['cb16']
    bits_tr, _ = _trainer(tmp_path, enc_mode='multilabel_binary')
    wide = V.VectorCodebook(R.planted(4, 20, 2, 0.3, 0))
    bit_cb = C.Codebook(np.arange(4, dtype=np.uint8).reshape(4, 1), 8)
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda *a, **k: (calls.append(a[0]), real(*a, **k))[1])
    good = [np.array([0, 1, 2], np.int32), np.array([3, 3], np.int32)]
    for fn in (lambda c, t: cv.encode_batch(specs[:2], t, SEG, codebook=c),
               lambda c, t: cv.resynth_batch(specs[:2], t, SEG, SPK[:2], n_iter=4, codebook=c),
               lambda c, t: cv.synth_index_batch(good, t, SEG, SPK[:2], c, n_iter=4)):
        with pytest.raises(ValueError, match='field E is 20'):
            fn(wide, tr)
        with pytest.raises(ValueError, match=r"vector codebook serves enc_mode 'continues'.*multilabel_binary"):
            fn(cb, bits_tr)
    # the existing refusals keep their wording
    with pytest.raises(ValueError, match=r"enc_mode 'continues' has no units to pack \(its encodings are not 0 / 1\)"):
        cv.encode_batch(specs[:2], tr, SEG, codebook=bit_cb)
    with pytest.raises(ValueError, match=r"enc_mode 'continues' has no units to pack \(its encodings are not 0 / 1\)"):
        cv.encode_batch(specs[:2], tr, SEG, packed=True)
    with pytest.raises(ValueError, match=r"enc_mode 'continues' has no units to pack \(its encodings are not 0 / 1\)"):
        cv.encode_batch(specs[:2], tr, SEG, packed=True, codebook=cb)
    for c in (None, bit_cb):
        with pytest.raises(ValueError, match="enc_mode 'continues' has no units: its encodings are real-valued"):
            cv.synth_index_batch(good, tr, SEG, SPK[:2], c)
    with pytest.raises(ValueError, match="enc_mode 'continues' has no units: its encodings are real-valued"):
        cv.synth_units_batch([np.zeros((3, 8), np.float32)], tr, SEG, SPK[:1])
    with pytest.raises(ValueError, match='must be a vector codebook'):
        cv.synth_index_batch(good, bits_tr, SEG, SPK[:2], bit_cb)
    for bad, match in (([np.array([0, 16], np.int32)] * 2, r'outside \[0, K = 16\)'), ([np.array([0, -1], np.int32)] * 2, 'outside'),
                       ([np.array([1], np.int32)] * 2, 'fewer than 2'), ([np.array([0.5, 1.0])] * 2, '1-D integer'),
                       ([np.zeros((2, 2), np.int32)] * 2, '1-D integer'), (good[:1], '2 target speakers for 1')):
        with pytest.raises(ValueError, match=match):
            cv.synth_index_batch(bad, tr, SEG, SPK[:2], cb)
    assert calls == []
    p = tmp_path / 'a.idx.txt'
    for text, match in (('3\n1 2\n', 'line 2: 2 values'), ('3\nx\n', r"line 2: 'x' is not an integer"), ('3\n16\n', 'line 2: index 16 is outside'),
                        ('-1\n', 'line 1: index -1'), ('', 'no indices')):
        p.write_text(text)
        with pytest.raises(ValueError, match='a.idx.txt.*' + match if text else match):
            cv.read_indices(str(p), 16)
    p.write_text('3\n0\n15\n')
    assert cv.read_indices(str(p), 16).tolist() == [3, 0, 15]


def test_main_fit_convert_and_synth_with_a_vector_codebook(dev, cont, tmp_path, monkeypatch):
    from scipy.io import wavfile
    sys.path.insert(0, ROOT)
    import main as M
    from zs_amd import convert as cv, layers, vq as V
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
    wavfile.write(str(d / 'one.wav'), 16000, np.array([1000], dtype=np.int16))
    (d / 'more.txt').write_text('0 0 0 0 0 0 0 0\n')                 # ignored: a 'continues' .txt carries no encoding
    s2id = str(tmp_path / 'speaker2id.json')
    json.dump({'S015': 0, 'S020': 1, 'V001': 2, 'V002': 3}, open(s2id, 'w'))
    hps_path = str(tmp_path / 'hps.json')
    json.dump(hps._asdict(), open(hps_path, 'w'))
    tr.save_model(str(tmp_path / 'model.pth'), 's2', 1)
    monkeypatch.setattr(hp, 'n_iter', 4)
    common = ['--hps_path', hps_path, '--speaker2id_path', s2id, '--ckpt_pth', str(tmp_path / 'model.pth-s2-1'), '--g_mode', 'targeted_residual',
              '--enc_mode', 'continues']
    ckpt = tmp_path / 'ckpt'
    M.main(['--fit_codebook', '8', '--fit_dir', str(d), '--ckpt_dir', str(ckpt), '--codebook_iters', '10', '--codebook_seed', '2'] + common)
    cb_path = str(ckpt / 'codebooks' / 'K8.vq.npz')
    cb = V.load_codebook(cb_path, 'continues', E=8)
    rep = json.load(open(str(ckpt / 'codebooks' / 'fit_codebook.json')))
    assert isinstance(cb, V.VectorCodebook) and (cb.K, cb.E, cb.meta['seed']) == (8, 8, 2) and 1 <= len(cb.meta['history']) <= 10
    assert {'codebook', 'K', 'E', 'files', 'skipped', 'n_units', 'history', 'symbols_used', 'entropy_bits_per_unit'} <= set(rep)
    assert sorted(os.path.basename(f['input']) for f in rep['files']) == ['w0.wav', 'w1.wav', 'w2.wav', 'w3.wav']
    assert [os.path.basename(s['input']) for s in rep['skipped']] == ['one.wav']
    assert rep['n_units'] == sum(f['units'] for f in rep['files']) == cb.meta['n_rows'] and rep['history'] == cb.meta['history']
    assert 1 <= rep['symbols_used'] <= 8 and 0.0 <= rep['entropy_bits_per_unit'] <= 3.0
    res = tmp_path / 'result'
    M.main(['--convert_dir', str(d), '--t_speaker', 'V001,V002', '--result_dir', str(res), '--codebook', cb_path] + common)

    def check(out, name, stems, with_txt):
        man = json.load(open(os.path.join(out, name)))
        assert set(man['codebook']) == {'file', 'K', 'symbols_used', 'entropy_bits_per_unit', 'mean_distance'}
        assert man['codebook']['file'] == cb_path and man['codebook']['K'] == 8 and 1 <= man['codebook']['symbols_used'] <= 8
        assert man['codebook']['mean_distance'] >= 0.0 and 0.0 <= man['codebook']['entropy_bits_per_unit'] <= 3.0
        used = set()
        for t in ('V001', 'V002'):
            for s in stems:
                base = os.path.join(out, t, s)
                assert os.path.getsize(base + '.wav') > 44
                text = open(base + '.idx.txt').read()
                assert text.endswith('\n') and all(ln.strip() == ln and ln.isdigit() for ln in text.splitlines())       # well-formed
                idx = cv.read_indices(base + '.idx.txt', 8)                   # every index in [0, K)
                if with_txt:
                    assert len(idx) == len(open(base + '.txt').read().splitlines())                                        # one line per unit
                used |= set(idx.tolist())
        assert len(used) == man['codebook']['symbols_used']
        return man

    out = os.path.join(os.path.join(str(res), './english/'), 'convert')
    man = check(out, 'convert_dir.json', ['w0', 'w1', 'w2', 'w3'], True)
    frames = {os.path.basename(it['input']): it['frames'] for it in man['items']}
    for s in ('w0', 'w1', 'w2', 'w3'):
        n = len(cv.read_indices(os.path.join(out, 'V001', s + '.idx.txt'), 8))
        assert n == sum(((((b - a) + 1) // 2 + 1) // 2 + 1) // 2 for a, b in
                        (cv.fragments(frames[s + '.wav'], SEG) if frames[s + '.wav'] > SEG else [(0, max(frames[s + '.wav'], cv.MIN_LEN))]))
    idx_dir = tmp_path / 'idx'
    idx_dir.mkdir()
    for s in ('w0', 'w1'):                                           # the index files it wrote, spoken
        (idx_dir / (s + '.idx.txt')).write_text(open(os.path.join(out, 'V001', s + '.idx.txt')).read())
    (idx_dir / 'bad.idx.txt').write_text('1\n9\n')
    M.main(['--synth_dir', str(idx_dir), '--t_speaker', 'V001,V002', '--result_dir', str(res), '--codebook', cb_path] + common)
    man = check(os.path.join(os.path.join(str(res), './english/'), 'synth'), 'synth_dir.json', ['w0', 'w1'], False)
    assert len(man['items']) == 4 and [os.path.basename(s['input']) for s in man['skipped']] == ['bad.idx.txt']
    with pytest.raises(ValueError, match="enc_mode 'continues' has no units"):                        # without a codebook: today's message
        M.main(['--synth_dir', str(idx_dir), '--t_speaker', 'V001', '--result_dir', str(res)] + common)
    layers.check_status(dev)
