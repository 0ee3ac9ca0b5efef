"""The vector codebook on the host: the properties of the numpy definition (tests/vq_ref.py) that zs_amd.vq.fit_vectors relies on,
vq_shift, the codebook file, load_codebook's dispatch and the refusals.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import codebook_ref as BR  # noqa: E402
import vq_ref as R  # noqa: E402


@pytest.mark.parametrize('n,E,K,s', [(2000, 6, 3, 1), (2000, 20, 37, 0), (2000, 64, 8, 0), (2000, 64, 37, 1), (600, 1024, 8, 1),
                                     (600, 1024, 37, 2)])
def test_reference_fit_converges_and_never_rises(n, E, K, s):
    x = R.planted(n, E, 8, 1.0, 10 + s)
    assert x.shape == (n, E) and x.dtype == np.float32
    code, history, steps = R.fit(x, K, iters=40, seed=s)
    totals = [h[0] for h in history]
    print(E, K, s, len(history), [st['near'] for st in steps])
    assert history[-1][1] == 0 and len(history) <= 40                      # moved == 0 within 40 iterations
    # assignment minimises per row and the mean per cluster: in fp64 the sum falls, up to the fp32 rounding of the means
    assert all(b <= a * (1 + 1e-6) for a, b in zip(totals, totals[1:])), totals
    assert max(st['near'] for st in steps) <= 0.02 * n                     # the cap on near rows holds for this generator
    idx, dist = R.assign(code, code)                                       # the codewords snap to themselves
    assert np.array_equal(idx, np.arange(K)) and (dist <= 1e-9 * (code.astype(np.float64) ** 2).sum(1)).all()
    assert code.dtype == np.float32 and np.array_equal(steps[-1]['code'], code)


def test_reference_rules_on_hand_made_input():
    code = np.array([[1, 0], [0, 1], [1, 0]], dtype=np.float32)
    x = np.array([[2, 0], [0.5, 0.5], [0, 3], [-1, -1]], dtype=np.float32)
    idx, dist = R.assign(x, code)
    assert idx.tolist() == [0, 0, 1, 0]                                    # duplicate / equidistant: the lowest index
    assert np.allclose(dist, [1, 0.5, 4, 5])
    assert R.near_rows(x, code).tolist() == [True, True, False, True]      # a duplicate codeword makes the rows it wins near
    assert R.quantise(np.array([0.5, 1.5, 2.5, -0.5, -1.5], dtype=np.float32), 0).tolist() == [0, 2, 2, 0, -2]   # half to even
    assert R.quantise(np.float32(0.75), 2).tolist() == 3
    cnt, s, bad = R.accum(x, [0, 0, 5, -1], 3, 1)
    assert cnt.tolist() == [2, 0, 0] and bad == 2 and s.tolist() == [[5, 1], [0, 0], [0, 0]]
    new, cn, changed = R.update(code, cnt, s, 1)
    assert new.tolist() == [[1.25, 0.25], [0, 1], [1, 0]] and changed == 1 and cn.tolist() == [1.625, 1, 1]
    # the int64 -> double rounding is to nearest even: 2^53 + 1 -> 2^53
    new, _, _ = R.update(np.zeros((1, 1), np.float32), [1], np.array([[2 ** 53 + 1]], dtype=np.int64), 30)
    assert new[0, 0] == np.float32(2.0 ** 23)
    empties, rows = R.reseed([3, 0, 2, 0], [1.0, 7.0, 7.0, 0.5, 9.0])
    assert empties.tolist() == [1, 3] and rows.tolist() == [4, 1]          # the largest first, then the lower of the tied rows
    out, bad = R.gather([0, 2, 9, 1], code, [0, 2, 3], [2, 2, 5], 3, 4)
    assert bad == 1 and out[0, :, :2].tolist() == [[1, 0], [1, 0], [0, 0]] and (out[2] == 0).all() and (out[..., 2:] == 0).all()
    assert out[1, :, :2].tolist() == [[0, 0], [0, 1], [0, 0]]


def test_vq_shift_edges():
    from zs_amd.vq import vq_shift
    assert vq_shift(1, 0.0) == 30 and vq_shift(1000, 1.0) == 30 and vq_shift(2 ** 20, 100.0) == 30
    assert vq_shift(2 ** 31 - 1, 1.0) == 30                                 # (2^31 - 1) 2^30 < 2^61
    assert vq_shift(2 ** 31, 1.0) == 29                                     # 2^31 2^30 = 2^61 is not below it
    assert vq_shift(2 ** 20, 2.0 ** 11) == 29 and vq_shift(2 ** 20, np.nextafter(np.float32(2.0 ** 11), np.float32(0))) == 30
    assert vq_shift(1, 2.0 ** 70) == -10
    for n, m in ((2000, 5.5), (2 ** 20, 1e6), (7, 3e20)):
        s = vq_shift(n, m)
        assert s == R.vq_shift(n, m) and n * m * 2.0 ** s < 2.0 ** 61 and (s == 30 or n * m * 2.0 ** (s + 1) >= 2.0 ** 61)
    for n, m in ((0, 1.0), (-1, 1.0), (10, float('inf')), (10, float('nan')), (10, -1.0), (4, 3.0e38)):
        with pytest.raises(ValueError, match='vq_shift'):
            vq_shift(n, m)


def test_vector_codebook_file_round_trip_and_refusals(tmp_path):
    from zs_amd.vq import FORMAT_VERSION, VectorCodebook
    K, E = 5, 20
    vec = R.planted(K, E, 2, 0.3, 1)
    meta = {'enc_mode': 'continues', 'n_rows': 77, 'seed': 3, 'shift': 30, 'history': [[10.5, 77, 0], [8.25, 0, 0]]}
    cb = VectorCodebook(vec, meta)
    assert cb.kind == 'vector' and np.array_equal(cb.cnorm, R.cnorm(vec)) and cb.cnorm.dtype == np.float32
    path = str(tmp_path / 'K5.vq.npz')
    cb.save(path)
    back = VectorCodebook.load(path, E=E)
    assert (back.K, back.E) == (K, E) and np.array_equal(back.vectors, vec) and back.meta == meta and np.array_equal(back.cnorm, cb.cnorm)
    with pytest.raises(ValueError, match=r'field E is 20.*c_in\) is 8'):
        VectorCodebook.load(path, E=8)
    back.check_width(20)
    good = dict(kind=np.array('vector'), format_version=np.int64(FORMAT_VERSION), K=np.int64(K), E=np.int64(E), vectors=vec,
                meta=np.array('{}'))

    def refused(match, **change):
        d = {k: v for k, v in dict(good, **change).items() if v is not None}
        p = str(tmp_path / 'bad.npz')
        with open(p, 'wb') as f:
            np.savez(f, **d)
        with pytest.raises(ValueError, match=match):
            VectorCodebook.load(p)

    refused("'vectors' is missing", vectors=None)
    refused("'kind' is missing", kind=None)
    refused("kind must be 'vector'", kind=np.array('bits'))
    refused("'E' is missing", E=None)
    refused('format_version is 99', format_version=np.int64(99))
    refused('K is 6', K=np.int64(6))
    refused('E is 21', E=np.int64(21))
    refused('vectors', vectors=vec.astype(np.float64))
    refused('vectors', vectors=vec[0])
    refused("'K' must be one integer", K=np.array([5, 5]))
    refused('meta', meta=np.array('[1, 2'))
    nan = vec.copy()
    nan[1, 2] = np.nan
    refused('vectors.*not finite', vectors=nan)
    (tmp_path / 'text.npz').write_text('not a zip')
    with pytest.raises(ValueError, match='not a codebook file'):
        VectorCodebook.load(str(tmp_path / 'text.npz'))
    for v in (vec[:0], np.zeros((2, 1025), np.float32), np.zeros((2, 0), np.float32), vec.astype(np.float64)):
        with pytest.raises(ValueError, match='vector codebook'):
            VectorCodebook(v)


def test_load_codebook_dispatches_on_the_file(tmp_path):
    from zs_amd.codebook import Codebook
    from zs_amd.vq import VectorCodebook, load_codebook
    vpath, bpath = str(tmp_path / 'K4.vq.npz'), str(tmp_path / 'K4.codebook.npz')
    VectorCodebook(R.planted(4, 8, 2, 0.3, 1)).save(vpath)
    Codebook(BR.planted(4, 8, 2, 0.3, 1), 8).save(bpath)
    v = load_codebook(vpath, 'continues', 8)
    assert isinstance(v, VectorCodebook) and (v.K, v.E) == (4, 8)
    b = load_codebook(bpath, 'multilabel_binary', 8)
    assert isinstance(b, Codebook) and (b.K, b.E) == (4, 8)
    for mode in ('multilabel_binary', 'one_hot', 'binary', 'gumbel_t'):
        with pytest.raises(ValueError, match=r"vector codebook.*'continues'.*%s" % mode):
            load_codebook(vpath, mode, 8)
    with pytest.raises(ValueError, match=r"enc_mode 'continues' has no units to pack \(its encodings are not 0 / 1\)"):
        load_codebook(bpath, 'continues', 8)                                # a bit codebook for continues: today's wording
    with pytest.raises(ValueError, match=r'field E is 8.*c_in\) is 16'):
        load_codebook(vpath, 'continues', 16)
    with pytest.raises(ValueError, match=r'field E is 8.*c_in\) is 16'):
        load_codebook(bpath, 'binary', 16)
    (tmp_path / 'text.npz').write_text('not a zip')
    with pytest.raises(ValueError, match='not a codebook file'):
        load_codebook(str(tmp_path / 'text.npz'), 'continues', 8)


def test_host_rules_match_the_definition():
    from zs_amd import vq as V
    x = R.planted(300, 6, 8, 1.0, 3)
    x[10] = x[4]
    x[200:] = x[7]                                                          # duplicates are passed over
    assert np.array_equal(V.init_rows(x, 37, 5), R.init_rows(x, 37, 5))
    distinct = len({r.tobytes() for r in x})
    with pytest.raises(ValueError, match='%d distinct vectors' % distinct):
        V.init_rows(x, distinct + 1, 0)
    cnt, dist = [3, 0, 2, 0, 0], [1.0, 7.0, 7.0, 0.5, 9.0, 9.0]
    for got, want in zip(V.reseed_rows(cnt, dist), R.reseed(cnt, dist)):
        assert np.array_equal(got, want)
    assert V.reseed_rows(cnt, dist)[1].tolist() == [4, 5, 1]
    assert np.array_equal(V.host_cnorm(x), R.cnorm(x))
    for K, kw in ((0, {}), (65537, {}), (4, dict(iters=0))):
        with pytest.raises(ValueError, match='fit_vectors'):
            V.fit_vectors(None, K, **kw)
    with pytest.raises(ValueError, match='contiguous fp32 device tensor'):
        V.fit_vectors(np.zeros((4, 4), np.float32), 2)


def test_existing_refusals_still_raise():
    from zs_amd import codebook as C
    with pytest.raises(ValueError, match=r"enc_mode 'continues' has no units to pack \(its encodings are not 0 / 1\)"):
        C.fit(None, 8, enc_mode='continues')
    with pytest.raises(ValueError, match='there is nothing a codebook could snap'):
        C.refuse_continues('continues')


def test_header_declares_the_four_entry_points():
    from zs_amd import _lib as L, vq as V
    assert L.ENUMS['ZS_ABI_VERSION'] == 1
    assert {'zs_vq_assign', 'zs_vq_accum', 'zs_vq_update', 'zs_vq_gather'} <= set(L.FUNCTIONS)
    assert {'ZsVqAssign', 'ZsVqAccum', 'ZsVqUpdate', 'ZsVqGather'} <= set(L.STRUCTS)
    assert V.WORK_BYTES == 12 * V.SPLIT_N and V.TILE_K == 128               # 8 bytes of (score, k) and 4 of |x|^2 per row
