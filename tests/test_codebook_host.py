"""The unit codebook on the host: the properties of the numpy definition (tests/codebook_ref.py) that zs_amd.codebook.fit relies on,
the codebook file, the parser errors, the refusals and usage().  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import codebook_ref as R  # noqa: E402

SHAPES = [(2000, 6), (2000, 20), (2000, 64), (600, 1024)]
# runs that go through the empty-cluster reseed (the generator and the rule of the definition decide; the test asserts that they do)
WITH_EMPTIES = [(64, 37, 0), (64, 37, 1), (64, 37, 2), (1024, 37, 0), (1024, 37, 1), (1024, 37, 2), (64, 8, 1), (64, 8, 2)]


def _units(E, s):
    n = dict((e, n) for n, e in SHAPES)[E]
    return R.planted(n, E, 8, 0.05, 10 + s)


@pytest.mark.parametrize('s', [0, 1, 2])
@pytest.mark.parametrize('K', [1, 3, 8, 37])
@pytest.mark.parametrize('n,E', SHAPES)
def test_reference_fit_is_monotone_and_converges(n, E, K, s):
    units = R.planted(n, E, 8, 0.05, 10 + s)
    assert units.shape == (n, (E + 7) // 8) and units.dtype == np.uint8
    code, history, codes, idx = R.fit(units, K, E, iters=30, seed=s)
    totals = [h[0] for h in history]
    assert all(b <= a for a, b in zip(totals, totals[1:])), totals        # never rises
    assert history[-1][1] == 0 and len(history) <= 30                     # changed == 0 within 30 iterations
    assert len(codes) == len(history) and np.array_equal(codes[-1], code)
    i2, snapped, dist = R.snap(code, code, E)                             # the codewords snap to themselves
    assert np.array_equal(snapped, code) and (dist == 0).all()
    assert idx.shape == (n,) and idx.min() >= 0 and idx.max() < K
    if (E, K, s) in WITH_EMPTIES:
        assert any(h[2] > 0 for h in history), history


def test_reference_figures_of_one_run():
    """E = 64, K = 37, s = 0: the figures quoted with the feature are what the definition gives."""
    _, history, _, _ = R.fit(_units(64, 0), 37, 64, iters=30, seed=0)
    print(history)
    assert [h[0] for h in history] == [8664, 6316, 6287] and sum(h[2] for h in history) == 3 and history[-1][1] == 0


def test_init_rows_needs_k_distinct_rows():
    units = _units(6, 0)
    distinct = len({r.tobytes() for r in units})
    assert 37 <= distinct <= 64
    first = R.init_rows(units, distinct, 0)
    assert len({units[i].tobytes() for i in first}) == distinct
    perm = np.random.RandomState(0).permutation(len(units))
    assert first[0] == perm[0] and list(first) == sorted(first, key=lambda i: int(np.flatnonzero(perm == i)[0]))
    with pytest.raises(ValueError, match=str(distinct)):
        R.init_rows(units, distinct + 1, 0)
    from zs_amd import codebook as C
    assert np.array_equal(C.init_rows(units, 37, 5), R.init_rows(units, 37, 5))
    with pytest.raises(ValueError, match='%d distinct rows' % distinct):
        C.init_rows(units, distinct + 1, 0)
    # the bits above E do not make rows different
    dirty = units.copy()
    dirty[::2] |= 0xC0
    assert np.array_equal(C.init_rows(dirty, 37, 5, E=6), R.init_rows(units, 37, 5))


def test_reference_assign_ties_and_update_rule():
    E = 6
    code = R.pack(np.array([[1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0]]))
    units = R.pack(np.array([[1, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1]]))
    idx, dist = R.assign(units, code, E)
    assert idx.tolist() == [0, 0, 0] and dist.tolist() == [1, 0, 4]       # equidistant / duplicate: the lowest index
    cnt, ones, bad = R.accum(units, [0, 0, 7], 3, E)
    assert cnt.tolist() == [2, 0, 0] and bad == 1 and ones[0].tolist() == [2, 1, 0, 0, 0, 0]
    new, changed = R.update(code, cnt, ones, E)                           # column 1: a tie keeps the old 1; cluster 1, 2 empty: kept
    assert R.bits(new, E).tolist() == [[1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0]] and changed == 0
    new, changed = R.update(R.pack(np.array([[0, 0, 1, 0, 0, 0]] * 3)), cnt, ones, E)
    assert R.bits(new, E)[0].tolist() == [1, 0, 0, 0, 0, 0] and changed == 1      # column 1: the tie keeps the old 0


def test_codebook_file_round_trip_and_refusals(tmp_path):
    from zs_amd.codebook import Codebook, FORMAT_VERSION
    E, K = 20, 5
    packed = R.planted(K, E, 2, 0.3, 1)
    meta = {'enc_mode': 'multilabel_binary', 'n_units': 77, 'seed': 3, 'history': [[10, 2, 1], [8, 0, 0]]}
    cb = Codebook(packed, E, meta)
    path = str(tmp_path / 'K5.codebook.npz')
    cb.save(path)
    back = Codebook.load(path, E=E)
    assert (back.K, back.E) == (K, E) and np.array_equal(back.packed, packed) and back.meta == meta
    with pytest.raises(ValueError, match=r'field E is 20.*c_in\) is 8'):  # the width mismatch, naming the field
        Codebook.load(path, E=8)
    good = dict(format_version=np.int64(FORMAT_VERSION), K=np.int64(K), E=np.int64(E), packed=packed, meta=np.array('{}'))

    def refused(match, **change):
        d = dict(good, **change)
        d = {k: v for k, v in d.items() if v is not None}
        p = str(tmp_path / 'bad.npz')
        with open(p, 'wb') as f:
            np.savez(f, **d)
        with pytest.raises(ValueError, match=match):
            Codebook.load(p)

    refused("'packed' is missing", packed=None)
    refused("'E' is missing", E=None)
    refused('format_version is 99', format_version=np.int64(99))
    refused('K is 6', K=np.int64(6))
    refused('packed', packed=packed.astype(np.int32))
    refused('packed', packed=packed[:, :2])
    refused('packed', E=np.int64(2000))
    refused("'E' must be one integer", E=np.array([20, 20]))
    refused('meta', meta=np.array('[1, 2'))
    dirty = packed.copy()
    dirty[0, -1] |= 0x80
    refused('bit set above column 20', packed=dirty)
    (tmp_path / 'text.npz').write_text('not a zip')
    with pytest.raises(ValueError, match='not a codebook file'):
        Codebook.load(str(tmp_path / 'text.npz'))
    for args in ((packed, 0), (packed, 1025), (packed[:0], E), (packed.astype(np.float32), E)):
        with pytest.raises(ValueError, match='codebook'):
            Codebook(*args)


def test_continues_is_refused_with_the_pack_wording():
    from zs_amd import codebook as C
    with pytest.raises(ValueError, match=r"enc_mode 'continues' has no units to pack \(its encodings are not 0 / 1\)"):
        C.fit(None, 8, enc_mode='continues')                              # before the units are looked at
    with pytest.raises(ValueError, match='continues'):
        C.refuse_continues('continues')
    C.refuse_continues('multilabel_binary')
    for K in (0, 65537):
        with pytest.raises(ValueError, match='K must be in'):
            C.fit(None, K)


def test_parser_errors():
    sys.path.insert(0, ROOT)
    import main as M

    def parse(argv):
        p = M.build_parser()
        a = p.parse_args(argv)
        M.check_codebook(p, a)
        return a

    for argv in (['--fit_codebook', '0', '--fit_dir', 'd'], ['--fit_codebook', '65537', '--fit_dir', 'd'], ['--fit_codebook', 'many', '--fit_dir', 'd'],
                 ['--fit_codebook', '8'], ['--fit_dir', 'd'], ['--codebook_iters', '3'], ['--fit_codebook', '8', '--fit_dir', 'd', '--codebook_iters', '0'],
                 ['--codebook', 'f.npz'], ['--codebook', 'f.npz', '--test'], ['--codebook', 'f.npz', '--cross_test'],
                 ['--codebook', 'f.npz', '--train_ae'], ['--fit_codebook', '8', '--fit_dir', 'd', '--train_ae'],
                 ['--fit_codebook', '8', '--fit_dir', 'd', '--codebook', 'f.npz', '--test_encode']):
        with pytest.raises(SystemExit) as e:
            parse(argv)
        assert e.value.code == 2, argv
    a = parse(['--fit_codebook', '65536', '--fit_dir', 'd', '--codebook_out', 'o.npz', '--codebook_iters', '5', '--codebook_seed', '4', '--use_ema'])
    assert (a.fit_codebook, a.fit_dir, a.codebook_out, a.codebook_iters, a.codebook_seed) == (65536, 'd', 'o.npz', 5, 4)
    M.check_ema(a)                                                         # --use_ema goes with --fit_codebook
    for mode in (['--convert_dir', 'd'], ['--synth_dir', 'd'], ['--test_encode']):
        assert parse(['--codebook', 'f.npz'] + mode).codebook == 'f.npz'
    assert parse(['--test_encode']).codebook is None


def test_usage_on_hand_made_histograms():
    from zs_amd.codebook import usage, usage_counts
    assert usage([3, 3, 3, 3], 8) == (1, 0.0)
    assert usage([0, 1, 2, 3]) == (4, 2.0)
    assert usage(np.array([0, 0, 1, 1], dtype=np.int32), 2) == (2, 1.0)
    used, h = usage([0, 0, 0, 5], 6)
    assert used == 2 and abs(h - (0.75 * np.log2(4 / 3) + 0.25 * 2)) < 1e-12
    assert usage([], 4) == (0, 0.0)
    assert usage_counts([2, 0, 2, 0]) == (2, 1.0) and usage_counts([0, 0]) == (0, 0.0)
    for bad in ([0, 4], [-1, 0]):
        with pytest.raises(ValueError, match='outside'):
            usage(bad, 4)


def test_assign_tile_is_the_header_constant():
    from zs_amd import _lib as L, codebook as C
    W = L.ENUMS['ZS_CODE_TILE_WORDS']
    assert [C.assign_tile(E) for E in (1, 32, 33, 64, 65, 1000, 1024)] == [W, W, W // 2, W // 2, W // 4, W // 32, W // 32]
    assert L.ENUMS['ZS_ABI_VERSION'] == 1 and {'zs_code_assign', 'zs_code_accum', 'zs_code_update'} <= set(L.FUNCTIONS)
    assert {'ZsCodeAssign', 'ZsCodeAccum', 'ZsCodeUpdate'} <= set(L.STRUCTS)
