"""The unit codebook on the device, every comparison exact (everything is integer):

* zs_code_assign, zs_code_accum and zs_code_update against tests/codebook_ref.py, the numpy definition, on every path of the kernels;
* zs_amd.codebook.fit against the definition's fit, codebook by codebook, through the empty-cluster reseed;
* resynth_batch / encode_batch / synth_units_batch with a codebook: the Decoder and the generator read the snapped units;
* main.py --fit_codebook, --convert_dir --codebook and --synth_dir --codebook on a temporary folder."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import codebook_ref as R  # noqa: E402

GUARD = 64
SEG = 32
FRAMES = [200, 75, 45, 33, 90, 5]           # five on the unit-fragment rule (none = 0 or 1 mod 32 above 64) and one below MIN_LEN
SPK = [2, 3, 2, 3, 2, 3]
WITH_EMPTIES = [(64, 37, 0), (64, 37, 1), (64, 37, 2), (1024, 37, 0), (1024, 37, 1), (1024, 37, 2), (64, 8, 1), (64, 8, 2)]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pitched(rows, pitch, fill=0xAA):
    """[n, nb] -> flat uint8 of n rows at `pitch` + GUARD bytes, the slack and the guard filled."""
    n, nb = rows.shape
    buf = np.full(n * pitch + GUARD, fill, dtype=np.uint8)
    buf[:n * pitch].reshape(n, pitch)[:, :nb] = rows
    return buf


def _random_code(K, E, seed, units=None):
    r = np.random.RandomState(seed)
    code = R.pack(r.randint(0, 2, (K, E)))
    if units is not None and len(units):                             # some codewords near the data, so that distances differ widely
        take = r.randint(0, len(units), K)
        near = r.rand(K) < 0.5
        code[near] = units[take[near], :code.shape[1]]
    return code


def _assign(dev, units, code, E, pitch=None, cpitch=None, alias=False, skip=(), total0=7):
    """zs_code_assign with every output pre-filled with 0xAA and a guard behind it.  Returns dict(idx, dist, snapped [n, pitch],
    total) as numpy; asserts the guards."""
    from zs_amd import _lib as L
    n, nb = units.shape[0], (E + 7) // 8
    pitch, cpitch = pitch or units.shape[1], cpitch or code.shape[1]
    u_d = torch.from_numpy(_pitched(units[:, :nb], pitch, 0x55)).to(dev)
    c_d = torch.from_numpy(_pitched(code[:, :nb], cpitch, 0x33)).to(dev)
    idx = torch.full((n + GUARD,), -0x55555556, dtype=torch.int32, device=dev)
    dist = torch.full((n + GUARD,), -0x55555556, dtype=torch.int32, device=dev)
    snapped = u_d if alias else torch.full((n * pitch + GUARD,), 0xAA, dtype=torch.uint8, device=dev)
    total = torch.full((2,), total0, dtype=torch.int64, device=dev)
    kw = dict(units=L.ptr(u_d), n=n, row_bytes=pitch, code=L.ptr(c_d), K=code.shape[0], code_bytes=cpitch, E=E, idx=L.ptr(idx),
              dist=L.ptr(dist), snapped=L.ptr(snapped), total=L.ptr(total))
    for k in skip:
        kw[k] = None
    L.call('zs_code_assign', 'ZsCodeAssign', _stream(), **kw)
    torch.cuda.synchronize()
    assert (idx[n:] == -0x55555556).all() and (dist[n:] == -0x55555556).all() and int(total[1]) == total0
    assert (snapped[n * pitch:] == (0x55 if alias else 0xAA)).all()
    assert np.array_equal(c_d.cpu().numpy(), _pitched(code[:, :nb], cpitch, 0x33))          # the codebook is read only
    if not alias:
        assert np.array_equal(u_d.cpu().numpy(), _pitched(units[:, :nb], pitch, 0x55))
    return dict(idx=idx[:n].cpu().numpy(), dist=dist[:n].cpu().numpy(), snapped=snapped[:n * pitch].cpu().numpy().reshape(n, pitch),
                total=int(total[0]) - total0)


def _check_assign(got, units, code, E, pitch_fill=0xAA):
    nb = (E + 7) // 8
    idx, want, dist = R.snap(units, code, E)
    assert np.array_equal(got['idx'], idx)
    assert np.array_equal(got['dist'], dist)
    assert np.array_equal(got['snapped'][:, :nb], want)              # the bits above E zero: pack() of the codeword's columns
    assert (got['snapped'][:, nb:] == pitch_fill).all()              # the bytes of a pitch behind the columns are not touched
    assert got['total'] == int(dist.astype(np.int64).sum())


# ---- zs_code_assign ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E', [6, 20, 64, 1024])
def test_assign_equals_reference(dev, E):
    """Row bytes 1, 3, 8 and 128: a partial last byte, a pitch that is no multiple of 4, one 64-bit word, the full width."""
    from zs_amd import codebook as C
    units_all = R.planted(1000, E, 8, 0.05, 3)
    Ks = [1, 2, 37, 300] + ([C.assign_tile(E) + 37] if E == 1024 else [])
    for K in Ks:
        code = _random_code(K, E, 100 + K, units_all)
        for n in (1, 63, 64, 65, 1000):
            _check_assign(_assign(dev, units_all[:n], code, E), units_all[:n], code, E)
    again = _assign(dev, units_all, code, E)
    assert all(np.array_equal(again[k], v) for k, v in _assign(dev, units_all, code, E).items() if k != 'total')


@pytest.mark.parametrize('E,n_extra', [(20, 65), (1024, 130)])
def test_assign_on_the_paths_for_many_rows(dev, E, n_extra):
    """n at and above ZS_CODE_SPLIT_N (one row per lane, four waves of their own rows) and ZS_CODE_BIG_N (two rows per lane), with a
    last workgroup that is partly empty."""
    from zs_amd import _lib as L
    K = 5
    for n in (L.ENUMS['ZS_CODE_SPLIT_N'] - 1, L.ENUMS['ZS_CODE_SPLIT_N'] + n_extra, L.ENUMS['ZS_CODE_BIG_N'] + n_extra):
        units = R.planted(n, E, 8, 0.05, 4)
        code = _random_code(K, E, 5, units)
        _check_assign(_assign(dev, units, code, E), units, code, E)


def test_assign_ties_go_to_the_lowest_index_across_tiles(dev):
    from zs_amd import codebook as C
    E = 1024
    tile = C.assign_tile(E)
    K = tile + 9
    r = np.random.RandomState(8)
    code = R.pack(r.randint(0, 2, (K, E)))
    code[tile + 3] = code[5]                                         # a duplicate behind the tile boundary
    code[tile + 4] = code[tile - 1]                                  # and one of the tile's last codeword
    base = R.bits(code[7:8], E).copy()
    a, b = base.copy(), base.copy()
    a[0, 11] ^= 1
    b[0, 900] ^= 1
    code[9], code[tile + 5] = R.pack(a)[0], R.pack(b)[0]             # code[7] removed below: both at distance 1 of `base`
    code[7] = R.pack(1 - base)[0]
    units = np.concatenate([code[5:6], code[tile - 1:tile], R.pack(base), code[tile + 8:tile + 9]])
    got = _assign(dev, units, code, E)
    assert got['idx'].tolist() == [5, tile - 1, 9, tile + 8] and got['dist'].tolist() == [0, 0, 1, 0]
    _check_assign(got, units, code, E)
    for E2 in (6, 64):                                               # few columns: most units are equidistant from several codewords
        units = R.planted(300, E2, 8, 0.2, 1)
        code = np.concatenate([_random_code(20, E2, 2), _random_code(20, E2, 2)])        # every codeword twice
        got = _assign(dev, units, code, E2)
        assert got['idx'].max() < 20
        _check_assign(got, units, code, E2)


@pytest.mark.parametrize('E', [6, 20, 1021])
def test_assign_ignores_the_bits_above_e(dev, E):
    units = R.planted(200, E, 8, 0.05, 6)
    code = _random_code(37, E, 7, units)
    clean = _assign(dev, units, code, E)
    hi = (0xff << (E % 8)) & 0xff
    du, dc = units.copy(), code.copy()
    du[:, -1] |= hi
    dc[:, -1] |= hi
    dirty = _assign(dev, du, dc, E)
    assert all(np.array_equal(dirty[k], clean[k]) for k in ('idx', 'dist', 'snapped')) and dirty['total'] == clean['total']
    assert not (dirty['snapped'][:, (E + 7) // 8 - 1] & hi).any()
    _check_assign(dirty, units, code, E)
    alias = _assign(dev, du, dc, E, alias=True)                      # in place too: the dirty bits are gone
    assert np.array_equal(alias['snapped'], clean['snapped'])


@pytest.mark.parametrize('E,pitch,cpitch', [(20, 6, 5), (20, 8, 4), (64, 12, 8), (64, 16, 24), (1024, 144, 128), (1024, 132, 160), (1024, 131, 129)])
def test_assign_pitches_and_in_place(dev, E, pitch, cpitch):
    """Pitches above (E + 7) / 8, with 16-byte, 4-byte and no alignment of the rows; `snapped` the very buffer `units`."""
    units = R.planted(300, E, 8, 0.05, 9)
    code = _random_code(37, E, 10, units)
    _check_assign(_assign(dev, units, code, E, pitch=pitch, cpitch=cpitch), units, code, E)
    _check_assign(_assign(dev, units, code, E, pitch=pitch, cpitch=cpitch, alias=True), units, code, E, pitch_fill=0x55)


def test_assign_optional_outputs_and_total(dev):
    from zs_amd import _lib as L
    E = 64
    units = R.planted(130, E, 8, 0.05, 11)
    code = _random_code(37, E, 12, units)
    full = _assign(dev, units, code, E)
    _check_assign(full, units, code, E)
    for name in ('idx', 'dist', 'snapped', 'total'):
        got = _assign(dev, units, code, E, skip=(name,))
        for k in ('idx', 'dist', 'snapped'):
            if k == name:
                assert (got[k] == (0xAA if k == 'snapped' else -0x55555556)).all()
            else:
                assert np.array_equal(got[k], full[k])
        assert got['total'] == (0 if name == 'total' else full['total'])
    # total accumulates across two calls
    u_d, c_d = torch.from_numpy(units).to(dev), torch.from_numpy(code).to(dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    for _ in range(2):
        L.call('zs_code_assign', 'ZsCodeAssign', _stream(), units=L.ptr(u_d), n=130, row_bytes=8, code=L.ptr(c_d), K=37, code_bytes=8, E=E,
               total=L.ptr(total))
    assert int(total[0]) == 2 * full['total']


def test_code_argument_errors_launch_nothing(dev):
    from zs_amd import _lib as L
    E, n, K = 20, 50, 7
    u_d = torch.full((n, 3), 0x55, dtype=torch.uint8, device=dev)
    c_d = torch.full((K, 3), 0x33, dtype=torch.uint8, device=dev)
    idx = torch.full((n,), -7, dtype=torch.int32, device=dev)
    dist = torch.full((n,), -7, dtype=torch.int32, device=dev)
    snapped = torch.full((n, 3), 0xAA, dtype=torch.uint8, device=dev)
    total = torch.full((1,), 5, dtype=torch.int64, device=dev)
    ok = dict(units=L.ptr(u_d), n=n, row_bytes=3, code=L.ptr(c_d), K=K, code_bytes=3, E=E, idx=L.ptr(idx), dist=L.ptr(dist),
              snapped=L.ptr(snapped), total=L.ptr(total))
    for change in (dict(K=0), dict(K=-1), dict(K=65537), dict(E=0), dict(E=1025), dict(E=-3), dict(units=None), dict(code=None),
                   dict(row_bytes=2), dict(code_bytes=2), dict(n=-1), dict(idx=L.ptr(idx) + 2), dict(total=L.ptr(total) + 4)):
        with pytest.raises(L.ZsError, match='zs_code_assign'):
            L.call('zs_code_assign', 'ZsCodeAssign', _stream(), **dict(ok, **change))
    L.call('zs_code_assign', 'ZsCodeAssign', _stream(), **dict(ok, n=0, units=None, code=None))          # n == 0 succeeds
    torch.cuda.synchronize()
    assert (idx == -7).all() and (dist == -7).all() and (snapped == 0xAA).all() and int(total[0]) == 5
    cnt = torch.full((K,), 3, dtype=torch.int32, device=dev)
    ones = torch.full((K, E), 2, dtype=torch.int32, device=dev)
    bad = torch.full((2,), 1, dtype=torch.int32, device=dev)
    ok = dict(units=L.ptr(u_d), idx=L.ptr(idx), n=n, row_bytes=3, K=K, E=E, cnt=L.ptr(cnt), ones=L.ptr(ones), bad=L.ptr(bad))
    for change in (dict(K=0), dict(K=65537), dict(E=0), dict(E=1025), dict(units=None), dict(idx=None), dict(cnt=None), dict(ones=None),
                   dict(bad=None), dict(row_bytes=2), dict(n=-1), dict(cnt=L.ptr(cnt) + 2)):
        with pytest.raises(L.ZsError, match='zs_code_accum'):
            L.call('zs_code_accum', 'ZsCodeAccum', _stream(), **dict(ok, **change))
    L.call('zs_code_accum', 'ZsCodeAccum', _stream(), **dict(ok, n=0, units=None, idx=None))
    ok = dict(code=L.ptr(c_d), K=K, code_bytes=3, E=E, cnt=L.ptr(cnt), ones=L.ptr(ones), changed=L.ptr(bad, 1))
    for change in (dict(K=0), dict(K=65537), dict(E=0), dict(E=1025), dict(code=None), dict(cnt=None), dict(ones=None), dict(changed=None),
                   dict(code_bytes=2)):
        with pytest.raises(L.ZsError, match='zs_code_update'):
            L.call('zs_code_update', 'ZsCodeUpdate', _stream(), **dict(ok, **change))
    torch.cuda.synchronize()
    assert (cnt == 3).all() and (ones == 2).all() and (bad == 1).all() and (c_d == 0x33).all() and (u_d == 0x55).all()


# ---- zs_code_accum / zs_code_update ---------------------------------------------------------------------------------------------------
def _accum_update(dev, units, idx, code, K, E, pitch, cpitch):
    from zs_amd import _lib as L
    nb = (E + 7) // 8
    n = len(units)
    u_d = torch.from_numpy(_pitched(units[:, :nb], pitch, 0xFF)).to(dev)          # ones in the slack: they are not columns
    i_d = torch.from_numpy(np.asarray(idx, dtype=np.int32)).to(dev)
    c_d = torch.from_numpy(_pitched(code[:, :nb], cpitch)).to(dev)
    cnt = torch.zeros(K + GUARD, dtype=torch.int32, device=dev)
    ones = torch.zeros(K * E + GUARD, dtype=torch.int32, device=dev)
    misc = torch.zeros(4, dtype=torch.int32, device=dev)                          # bad, changed, two guards
    L.call('zs_code_accum', 'ZsCodeAccum', _stream(), units=L.ptr(u_d), idx=L.ptr(i_d), n=n, row_bytes=pitch, K=K, E=E, cnt=L.ptr(cnt),
           ones=L.ptr(ones), bad=L.ptr(misc))
    L.call('zs_code_update', 'ZsCodeUpdate', _stream(), code=L.ptr(c_d), K=K, code_bytes=cpitch, E=E, cnt=L.ptr(cnt), ones=L.ptr(ones),
           changed=L.ptr(misc, 1))
    torch.cuda.synchronize()
    assert (cnt[K:] == 0).all() and (ones[K * E:] == 0).all() and (misc[2:] == 0).all()
    assert (c_d[K * cpitch:] == 0xAA).all()
    return (cnt[:K].cpu().numpy(), ones[:K * E].cpu().numpy().reshape(K, E), int(misc[0]), int(misc[1]),
            c_d[:K * cpitch].cpu().numpy().reshape(K, cpitch))


@pytest.mark.parametrize('E,pitch,cpitch', [(6, 1, 1), (20, 3, 5), (64, 8, 8), (1024, 128, 128), (1024, 131, 144)])
def test_accum_and_update_equal_reference(dev, E, pitch, cpitch):
    n, K, nb = 1000, 9, (E + 7) // 8
    r = np.random.RandomState(E)
    units = R.planted(n, E, 8, 0.3, 13)
    idx = r.randint(1, K, n)
    idx[r.rand(n) < 0.9] = 0                                        # skewed: one cluster holds 90 %
    idx[idx == 3] = 4                                               # cluster 3 is empty
    idx[idx == 2] = 5
    pair = np.array([17, 600])                                      # cluster 2 holds exactly two units: every column they differ in ties
    idx[pair] = 2
    units[600] = R.pack(1 - R.bits(units[17:18], E))[0] if E == 6 else units[600]
    idx[40], idx[41], idx[999] = K, -1, 2 ** 30                     # never an index
    code = _random_code(K, E, 14)
    code[2] = R.pack((np.arange(E) % 2)[None])[0]                   # old bits 0 and 1 alternate under the ties
    code[3, -1] |= (0xff << (E % 8)) & 0xff if E % 8 else 0         # the empty cluster's codeword keeps even its dirty bits
    cnt, ones, bad, changed, new = _accum_update(dev, units, idx, code, K, E, pitch, cpitch)
    w_cnt, w_ones, w_bad = R.accum(units, idx, K, E)
    assert np.array_equal(cnt, w_cnt) and np.array_equal(ones, w_ones) and bad == w_bad == 3
    assert cnt[3] == 0 and cnt[2] == 2 and cnt[0] > 800
    ties = 2 * w_ones[2] == w_cnt[2]
    old2 = R.bits(code[2:3], E)[0]
    assert (ties & (old2 == 0)).any() and (ties & (old2 == 1)).any()         # exact ties with the old bit 0 and with the old bit 1
    w_new, w_changed = R.update(code, w_cnt, w_ones, E)
    live = w_cnt > 0
    assert np.array_equal(new[live][:, :nb], w_new[live]) and changed == w_changed
    assert np.array_equal(new[3, :nb], code[3]) and np.array_equal(R.bits(new[3:4], E), R.bits(w_new[3:4], E))
    assert (new[:, nb:] == 0xAA).all()
    again = _accum_update(dev, units, idx, code, K, E, pitch, cpitch)        # integer atomics: two runs are bitwise equal
    assert np.array_equal(again[0], cnt) and np.array_equal(again[1], ones) and again[2:4] == (bad, changed) and np.array_equal(again[4], new)


@pytest.mark.parametrize('E,K,n', [(1024, 37, 3000), (20, 2100, 5000)])
def test_accum_over_several_codeword_tiles_and_row_slices(dev, E, K, n):
    """More codewords than one workgroup keeps counters for in LDS (16 at E = 1024; 1024 at most) and more rows than one round of
    the scan (1024): several workgroups along both axes of the grid, the last of each partly empty."""
    r = np.random.RandomState(K)
    units = R.planted(n, E, 8, 0.3, 21)
    idx = r.randint(0, K, n)
    idx[r.rand(n) < 0.5] = K - 1                                    # half of the rows in the last codeword of the last tile
    idx[[0, 1023, 1024, n - 1]] = [-5, K, K + 7, -1]
    code = _random_code(K, E, 22)
    nb = (E + 7) // 8
    cnt, ones, bad, changed, new = _accum_update(dev, units, idx, code, K, E, nb, nb)
    w_cnt, w_ones, w_bad = R.accum(units, idx, K, E)
    assert np.array_equal(cnt, w_cnt) and np.array_equal(ones, w_ones) and bad == w_bad == 4
    w_new, w_changed = R.update(code, w_cnt, w_ones, E)
    assert np.array_equal(new, w_new) and changed == w_changed


# ---- fit ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E,K,s', WITH_EMPTIES + [(20, 8, 0)])
def test_fit_equals_reference(dev, E, K, s):
    from zs_amd import codebook as C
    n = 600 if E == 1024 else 2000
    units = R.planted(n, E, 8, 0.05, 10 + s)
    w_code, w_hist, w_codes, w_idx = R.fit(units, K, E, iters=30, seed=s)
    if (E, K, s) in WITH_EMPTIES:
        assert any(h[2] > 0 for h in w_hist)
    codes = []
    u_d = torch.from_numpy(units).to(dev)
    cb = C.fit(u_d, K, iters=30, seed=s, E=E, on_iter=lambda i, c: codes.append(c.copy()))
    assert [tuple(h) for h in cb.meta['history']] == w_hist
    assert len(codes) == len(w_codes) and all(np.array_equal(a, b) for a, b in zip(codes, w_codes))
    assert np.array_equal(cb.packed, w_code) and (cb.K, cb.E) == (K, E) and cb.meta['n_units'] == n and cb.meta['seed'] == s
    idx, snapped = cb.snap(u_d)
    assert np.array_equal(idx.cpu().numpy(), w_idx) and np.array_equal(snapped.cpu().numpy(), w_code[w_idx])
    assert np.array_equal(u_d.cpu().numpy(), units)                  # the units are left as they were
    assert C.usage(idx, K) == C.usage(w_idx, K)
    with pytest.raises(ValueError, match='distinct rows'):
        C.fit(torch.from_numpy(units[:3].repeat(5, axis=0)).to(dev), 4, E=E)


# ---- through the conversion paths ------------------------------------------------------------------------------------------------------
def _trainer(path, dtype='fp32', g_mode='targeted_residual', enc_mode='multilabel_binary', seed=3):
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    torch.manual_seed(seed)
    hps = make_hps(enc_size=8, emb_size=32, n_speakers=4, n_target_speakers=2, seg_len=SEG)
    return Trainer(hps, None, g_mode, enc_mode, log_dir=os.path.join(str(path), 'log'), dtype=dtype, device=torch.device('cuda:0')), hps


def _field_noise(E, seed=1234, T=64):
    """noise_fn whose every batch position reads the same field: a fragment's noise does not depend on where it is batched."""
    U = torch.rand(T, E, 2, generator=torch.Generator().manual_seed(seed))
    base = (-torch.log(-torch.log(U + 1e-20) + 1e-20)).cuda()

    def noise_fn(n, t, e):
        assert e == E and t <= base.shape[0]
        return base[:t].unsqueeze(0).expand(n, t, E, 2).contiguous()
    return noise_fn


def _specs(frames, seed=7):
    rng = np.random.RandomState(seed)
    return [(rng.rand(n, 513) * 0.98 + 1e-3).astype(np.float32) for n in frames]


def _all_units(cv, tr, specs, noise_fn):
    """Every unit the Decoder decodes for `specs` without a codebook, packed: the returned units, and for an input shorter than MIN_LEN
    both units of its zero-padded form (only the first is returned for it)."""
    e, _ = cv.encode_batch(specs, tr, SEG, noise_fn=noise_fn)
    short = [np.concatenate([s, np.zeros((cv.MIN_LEN - len(s), 513), np.float32)]) for s in specs if len(s) < cv.MIN_LEN]
    hidden = cv.encode_batch(short, tr, SEG, noise_fn=noise_fn)[0] if short else []
    assert all(len(h) == 2 for h in hidden)
    return e, np.concatenate([cv.pack_units(a) for a in list(e) + list(hidden)])


@pytest.fixture(scope='module')
def plain(dev, tmp_path_factory):
    """The small fp32 trainers (a g_mode that reads the encoding, and 'spectrogram'), the batch, its units without a codebook and the
    K = 16 codebook fitted to them."""
    from zs_amd import codebook as C, convert as cv
    out = {'specs': _specs(FRAMES), 'noise_fn': _field_noise(8)}
    for g_mode in ('targeted_residual', 'spectrogram'):
        out[g_mode] = _trainer(tmp_path_factory.mktemp(g_mode), g_mode=g_mode)[0]
    tr = out['targeted_residual']
    out['e'], own = _all_units(cv, tr, out['specs'], out['noise_fn'])
    returned = np.concatenate([cv.pack_units(a) for a in out['e']])
    print('the batch: %d units returned, %d distinct; %d decoded, %d distinct' %
          (len(returned), len(np.unique(returned, axis=0)), len(own), len(np.unique(own, axis=0))))
    out['cb16'] = C.fit(torch.from_numpy(returned).to(dev), 16, E=8)
    out['cb_all'] = C.Codebook(np.unique(own, axis=0), 8)
    out['cb1'] = C.fit(torch.from_numpy(returned).to(dev), 1, E=8)
    return out


def _snapped(cv, cb, e):
    return [cv.unpack_units(R.snap(cv.pack_units(a), cb.packed, cb.E)[1], cb.E) for a in e]


@pytest.mark.parametrize('g_mode,enc_only', [('targeted_residual', True), ('targeted_residual', False), ('spectrogram', False)])
def test_conversion_reads_the_snapped_units(dev, plain, g_mode, enc_only):
    from zs_amd import convert as cv, layers
    tr, specs, noise_fn = plain[g_mode], plain['specs'], plain['noise_fn']
    e, own = _all_units(cv, tr, specs, noise_fn)
    if g_mode == 'targeted_residual':
        assert all(np.array_equal(a, b) for a, b in zip(e, plain['e']))
    cb16 = plain['cb16']
    # (a) K = 16: the units returned are the host-snapped units of the plain run; the waveforms those of the snapped units
    want = _snapped(cv, cb16, e)
    assert any(not np.array_equal(a, b) for a, b in zip(want, e))                 # the codebook does change this batch
    es, ws, idxs, total = cv.resynth_batch(specs, tr, SEG, SPK, n_iter=4, noise_fn=noise_fn, enc_only=enc_only, codebook=cb16, want_idx=True)
    assert [a.shape for a in es] == [a.shape for a in e] and len(es[5]) == 1
    assert all(a.dtype == np.float32 and np.array_equal(a, b) for a, b in zip(es, want))
    ref = [R.snap(cv.pack_units(a), cb16.packed, 8) for a in e]
    assert all(i.dtype == np.int32 and np.array_equal(i, r[0]) for i, r in zip(idxs, ref)) and total == sum(int(r[2].sum()) for r in ref)
    _, w5 = cv.synth_units_batch(want[:5], tr, SEG, SPK[:5], enc_only=enc_only, n_iter=4)
    assert all(len(a) > 0 and np.array_equal(a, b) for a, b in zip(ws[:5], w5))
    # synth_units_batch snaps its one buffer itself: from the unsnapped units, the same waveforms and the same indices
    _, w5b, i5, t5 = cv.synth_units_batch(e[:5], tr, SEG, SPK[:5], enc_only=enc_only, n_iter=4, codebook=cb16, want_idx=True)
    assert all(np.array_equal(a, b) for a, b in zip(w5, w5b)) and all(np.array_equal(a, b) for a, b in zip(i5, idxs[:5]))
    # encode_batch: the decoded spectrograms are those of the snapped units; packed or not, the same units; the indices
    ep, dp, ip = cv.encode_batch(specs, tr, SEG, decode_speakers=SPK, noise_fn=noise_fn, enc_only=enc_only, packed=True, codebook=cb16,
                                 want_idx=True)
    assert all(p.dtype == np.uint8 and np.array_equal(p, cv.pack_units(a)) for p, a in zip(ep, want))
    assert all(np.array_equal(a, b) for a, b in zip(ip, idxs))
    if enc_only:
        s5, _ = cv.synth_units_batch(want[:5], tr, SEG, SPK[:5], n_iter=4, want_specs=True)
        assert all(np.array_equal(a, b) for a, b in zip(dp[:5], s5))
    # (b) a codebook of every distinct unit of the batch changes nothing, the short utterance included
    cb_all = plain['cb_all'] if g_mode == 'targeted_residual' else type(cb16)(np.unique(own, axis=0), 8)
    e0, w0 = cv.resynth_batch(specs, tr, SEG, SPK, n_iter=4, noise_fn=noise_fn, enc_only=enc_only)
    e1, w1 = cv.resynth_batch(specs, tr, SEG, SPK, n_iter=4, noise_fn=noise_fn, enc_only=enc_only, codebook=cb_all)
    assert all(np.array_equal(a, b) for a, b in zip(e0, e1)) and all(np.array_equal(a, b) for a, b in zip(e0, e))
    assert all(np.array_equal(a, b) for a, b in zip(w0, w1))
    _, d0 = cv.encode_batch(specs, tr, SEG, decode_speakers=SPK, noise_fn=noise_fn, enc_only=enc_only)
    _, d1 = cv.encode_batch(specs, tr, SEG, decode_speakers=SPK, noise_fn=noise_fn, enc_only=enc_only, codebook=cb_all)
    assert all(np.array_equal(a, b) for a, b in zip(d0, d1))
    # (c) K = 1: every unit written is the one codeword
    cb1 = plain['cb1']
    ek, wk = cv.resynth_batch(specs, tr, SEG, SPK, n_iter=4, noise_fn=noise_fn, enc_only=enc_only, codebook=cb1)
    word = cv.unpack_units(cb1.packed, 8)[0]
    assert all(len(a) == len(b) and (a == word[None]).all() for a, b in zip(ek, e)) and all(np.isfinite(w).all() for w in wk)
    layers.check_status(dev)


def test_codebook_refusals_come_before_any_launch(dev, plain, tmp_path, monkeypatch):
    from zs_amd import _lib as L, codebook as C, convert as cv
    tr, specs = plain['targeted_residual'], plain['specs']
    cont, _ = _trainer(tmp_path, enc_mode='continues')
    wide = C.Codebook(R.planted(4, 20, 2, 0.2, 0), 20)
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda *a, **k: (calls.append(a[0]), real(*a, **k))[1])
    for fn in (lambda cb, t: cv.encode_batch(specs[:2], t, SEG, codebook=cb),
               lambda cb, t: cv.resynth_batch(specs[:2], t, SEG, SPK[:2], n_iter=4, codebook=cb),
               lambda cb, t: cv.synth_units_batch(plain['e'][:2], t, SEG, SPK[:2], n_iter=4, codebook=cb)):
        with pytest.raises(ValueError, match='field E is 20'):
            fn(wide, tr)
        with pytest.raises(ValueError, match='continues'):
            fn(plain['cb16'], cont)
    with pytest.raises(ValueError, match='want_idx needs a codebook'):
        cv.encode_batch(specs[:2], tr, SEG, want_idx=True)
    assert calls == []


def test_codebook_bf16(dev, plain, tmp_path):
    """In bf16 the snapped units equal the fp32 run's wherever the unsnapped units already agreed, and the decoded spectrograms of
    the snapped units stay within the bound tests/test_gpu_ragged.py allows between two batchings of the same fragments (relative
    difference below 2e-2 of the maximum)."""
    from zs_amd import convert as cv, layers
    tr, _ = _trainer(tmp_path, dtype='bf16')
    specs, noise_fn, cb = plain['specs'], plain['noise_fn'], plain['cb16']
    e32 = plain['e']
    s32 = _snapped(cv, cb, e32)
    e16, _ = cv.encode_batch(specs, tr, SEG, noise_fn=noise_fn)
    es, ds = cv.encode_batch(specs, tr, SEG, decode_speakers=SPK, noise_fn=noise_fn, codebook=cb)
    agreed = 0
    for a32, a16, b32, b16 in zip(e32, e16, s32, es):
        same = (a32 == a16).all(axis=1)
        agreed += int(same.sum())
        assert np.array_equal(b16[same], b32[same])
    assert agreed > 0
    s, w = cv.synth_units_batch(es[:5], tr, SEG, SPK[:5], n_iter=4, want_specs=True)
    worst = 0.0
    for a, b in zip(ds[:5], s):
        assert a.shape == b.shape
        worst = max(worst, float(np.abs(a - b).max() / max(1e-6, np.abs(a).max())))
    print('bf16, codebook: %d units agreed with fp32; decoded spectrograms worst rel diff %.3g' % (agreed, worst))
    assert worst < 2e-2
    assert all(np.isfinite(x).all() and len(x) > 0 for x in w)
    layers.check_status(dev)


# ---- main.py ---------------------------------------------------------------------------------------------------------------------------
def test_main_fit_convert_and_synth_with_a_codebook(dev, plain, tmp_path, monkeypatch):
    from scipy.io import wavfile
    sys.path.insert(0, ROOT)
    import main as M
    from zs_amd import codebook as C, convert as cv, layers
    from zs_amd.hps import hp, make_hps
    tr = plain['targeted_residual']
    hps = make_hps(enc_size=8, emb_size=32, n_speakers=4, n_target_speakers=2, seg_len=SEG)
    rng = np.random.RandomState(5)
    d = tmp_path / 'in'
    d.mkdir()
    for i, n in enumerate((14000, 9000, 20000, 12000)):              # short synthetic wavs: a gliding tone and noise
        t = np.arange(n) / 16000.0
        y = 0.3 * np.sin(2 * np.pi * (200.0 + 150.0 * i + 400.0 * t) * t) + 0.05 * rng.randn(n)
        wavfile.write(str(d / ('w%d.wav' % i)), 16000, (y * 32767).astype(np.int16))
    wavfile.write(str(d / 'one.wav'), 16000, np.array([1000], dtype=np.int16))
    cv.write_encodings(str(d / 'more.txt'), plain['e'][0])           # a unit file in the folder is added
    s2id = str(tmp_path / 'speaker2id.json')
    json.dump({'S015': 0, 'S020': 1, 'V001': 2, 'V002': 3}, open(s2id, 'w'))
    hps_path = str(tmp_path / 'hps.json')
    json.dump(hps._asdict(), open(hps_path, 'w'))
    tr.save_model(str(tmp_path / 'model.pth'), 's2', 1)
    monkeypatch.setattr(hp, 'n_iter', 4)
    common = ['--hps_path', hps_path, '--speaker2id_path', s2id, '--ckpt_pth', str(tmp_path / 'model.pth-s2-1'), '--g_mode', 'targeted_residual']
    ckpt = tmp_path / 'ckpt'
    M.main(['--fit_codebook', '8', '--fit_dir', str(d), '--ckpt_dir', str(ckpt), '--codebook_iters', '10', '--codebook_seed', '2'] + common)
    cb_path = str(ckpt / 'codebooks' / 'K8.codebook.npz')
    cb = C.Codebook.load(cb_path, E=8)
    rep = json.load(open(str(ckpt / 'codebooks' / 'fit_codebook.json')))
    assert (cb.K, cb.E, cb.meta['seed']) == (8, 8, 2) and 1 <= len(cb.meta['history']) <= 10
    assert {'codebook', 'K', 'E', 'files', 'skipped', 'n_units', 'history', 'symbols_used', 'entropy_bits_per_unit'} <= set(rep)
    assert sorted(os.path.basename(f['input']) for f in rep['files']) == ['more.txt', 'w0.wav', 'w1.wav', 'w2.wav', 'w3.wav']
    assert [os.path.basename(s['input']) for s in rep['skipped']] == ['one.wav']
    assert rep['n_units'] == sum(f['units'] for f in rep['files']) == cb.meta['n_units'] and rep['history'] == cb.meta['history']
    assert 1 <= rep['symbols_used'] <= 8 and 0.0 <= rep['entropy_bits_per_unit'] <= 3.0
    res = tmp_path / 'result'
    M.main(['--convert_dir', str(d), '--t_speaker', 'V001,V002', '--result_dir', str(res), '--codebook', cb_path] + common)
    out = os.path.join(os.path.join(str(res), './english/'), 'convert')

    def check(out, name, stems, with_wav_txt):
        man = json.load(open(os.path.join(out, name)))
        assert set(man['codebook']) == {'file', 'K', 'symbols_used', 'entropy_bits_per_unit', 'mean_distance'}
        assert man['codebook']['file'] == cb_path and man['codebook']['K'] == 8 and 1 <= man['codebook']['symbols_used'] <= 8
        assert man['codebook']['mean_distance'] >= 0.0 and 0.0 <= man['codebook']['entropy_bits_per_unit'] <= 3.0
        lines, used = set(), set()
        for t in ('V001', 'V002'):
            for s in stems:
                base = os.path.join(out, t, s)
                assert os.path.getsize(base + '.wav') > 44
                units = cv.read_units(base + '.txt', 8)
                idx = [int(x) for x in open(base + '.idx.txt').read().split()]
                assert len(idx) == len(units) and all(0 <= i < 8 for i in idx)
                assert np.array_equal(cv.pack_units(units), cb.packed[idx])       # the .idx.txt agree with the .txt
                lines |= {ln for ln in open(base + '.txt').read().splitlines()}
                used |= set(idx)
        assert len(lines) <= 8 and len(used) == man['codebook']['symbols_used']
        return man

    check(out, 'convert_dir.json', ['w0', 'w1', 'w2', 'w3'], True)
    units_dir = tmp_path / 'units'
    units_dir.mkdir()
    for s in ('w0', 'w1'):                                           # unit files written without a codebook, spoken through it
        cv.write_encodings(str(units_dir / (s + '.txt')), plain['e'][1 if s == 'w0' else 2])
    M.main(['--synth_dir', str(units_dir), '--t_speaker', 'V001,V002', '--result_dir', str(res), '--codebook', cb_path] + common)
    man = check(os.path.join(os.path.join(str(res), './english/'), 'synth'), 'synth_dir.json', ['w0', 'w1'], True)
    assert len(man['items']) == 4
    with pytest.raises(ValueError, match='field E is 8'):            # another width: refused when the file is loaded, before any launch
        C.Codebook.load(cb_path, E=16)
    layers.check_status(dev)
