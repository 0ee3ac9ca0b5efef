"""The residual vector codebook on the host: the numpy definition (tests/rvq_ref.py) on hand-computed cases, the host
reconstruction against it, the codebook file, load_codebook's dispatch over the three kinds, the index-row unit files and every refusal
of the command line.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import codebook_ref as BR  # noqa: E402
import rvq_ref as Q  # noqa: E402
import vq_ref as R  # noqa: E402

HPS = os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')          # enc_mode multilabel_binary, enc_size 1024


# ---- the definition on hand-computed cases -------------------------------------------------------------------------------------------
def test_residual_and_reconstruction_by_hand():
    c0 = np.array([[1, 0], [0, 2]], dtype=np.float32)
    c1 = np.array([[0.5, 0.5], [-0.25, 0]], dtype=np.float32)
    c2 = np.array([[0.125, -0.125], [0, 0]], dtype=np.float32)
    x = np.array([[1.5, 0.25], [0, 2], [-0.25, 2.5]], dtype=np.float32)
    idx, dist, rs = Q.snap(x, [c0, c1])                                    # S = 2
    assert idx.tolist() == [[0, 1, 1], [0, 1, 1]]
    assert rs[1].tolist() == [[0.5, 0.25], [0, 0], [-0.25, 0.5]]
    assert rs[2].tolist() == [[0, -0.25], [0.25, 0], [0, 0.5]]
    assert np.allclose(dist[0], [0.3125, 0, 0.3125]) and np.allclose(dist[1], [0.0625, 0.0625, 0.25])
    q, bad = Q.reconstruct(idx, [c0, c1])
    assert bad == 0 and q.tolist() == [[1.5, 0.5], [-0.25, 2], [-0.25, 2]]
    assert Q.reconstruct(idx, [c0, c1], s_use=1)[0].tolist() == [[1, 0], [0, 2], [0, 2]]          # the embedded coarser code
    idx3, _, rs3 = Q.snap(x, [c0, c1, c2])                                 # S = 3
    assert idx3[:2].tolist() == idx.tolist() and idx3[2].tolist() == [0, 0, 1]
    assert rs3[3].tolist() == [[-0.125, -0.125], [0.125, 0.125], [0, 0.5]]
    assert Q.reconstruct(idx3, [c0, c1, c2])[0].tolist() == [[1.625, 0.375], [-0.125, 1.875], [-0.25, 2]]
    # the residuals of given indices, and a bad index at stage 1: the row is copied, counted, and its frame reconstructs to zero
    given = np.array([[0, 1, 1], [0, 7, -1]])
    r1, b1 = Q.residual(x, given[0], c0)
    r2, b2 = Q.residual(r1, given[1], c1)
    assert (b1, b2) == (0, 2) and r2.tolist() == [[0, -0.25], [0, 0], [-0.25, 0.5]]
    q, bad = Q.reconstruct(given, [c0, c1])
    assert bad == 2 and q.tolist() == [[1.5, 0.5], [0, 0], [0, 0]]
    q, bad = Q.reconstruct(given, [c0, c1], s_use=1)                       # the bad indices lie in an unused stage
    assert bad == 0 and q.tolist() == [[1, 0], [0, 2], [0, 2]]
    out, bad = Q.gather(given, [c0, c1], 2, [0, 1, 2], [2, 2, 2], 3, 4)
    # fragment 0 holds frames 0, 1 (one bad), fragment 1 frames 1, 2 (both bad), fragment 2 runs past the 3 indices and reads nothing
    assert bad == 3 and out[0, :, :2].tolist() == [[1.5, 0.5], [0, 0], [0, 0]] and (out[1] == 0).all() and (out[2] == 0).all()


def test_K_1_and_the_order_of_the_adds():
    one = [np.array([[0.5, -1]], dtype=np.float32), np.array([[0.25, 0.25]], dtype=np.float32)]
    x = np.array([[3, 3], [0, 0]], dtype=np.float32)
    idx, _, rs = Q.snap(x, one)                                            # K = 1: every index is 0
    assert idx.tolist() == [[0, 0], [0, 0]] and rs[2].tolist() == [[2.25, 3.75], [-0.75, 0.75]]
    assert Q.reconstruct(idx, one)[0].tolist() == [[0.75, -0.75]] * 2
    # (2^24 + 1) + -1: left to right the first add rounds to 2^24 (half to even) and the sum is 2^24 - 1; any other order gives 2^24
    codes = [np.array([[2.0 ** 24]], dtype=np.float32), np.array([[1.0]], dtype=np.float32), np.array([[-1.0]], dtype=np.float32)]
    idx = np.zeros((3, 1), dtype=np.int64)
    assert Q.reconstruct(idx, codes)[0][0, 0] == np.float32(2.0 ** 24 - 1)
    assert np.float32(2.0 ** 24) + (np.float32(1.0) + np.float32(-1.0)) == np.float32(2.0 ** 24)
    # one cast behind the adds: 1 + 2^-8 + 2^-8 = 1 + 2^-7 is a bf16 value; casting every term or every partial sum first loses it
    codes = [np.array([[1.0]], dtype=np.float32), np.array([[2.0 ** -8]], dtype=np.float32), np.array([[2.0 ** -8]], dtype=np.float32)]
    assert Q.reconstruct(idx, codes, bf16=True)[0][0, 0] == np.float32(1 + 2.0 ** -7)
    assert Q.to_bf16(Q.to_bf16(np.float32(1 + 2.0 ** -8)) + np.float32(2.0 ** -8)) == np.float32(1.0)
    assert Q.to_bf16(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -1 - 2.0 ** -8, 0.1], np.float32)).tolist() == \
        [1.0, 1 + 2.0 ** -6, -1.0, 0.10009765625]                          # half to even, both ways


def test_host_reconstruct_equals_the_definition():
    from zs_amd.rvq import ResidualCodebook
    rs = np.random.RandomState(2)
    vec = (rs.standard_normal((3, 5, 7)) * np.array([4.0, 1.0, 1e-3])[:, None, None]).astype(np.float32)
    cb = ResidualCodebook(vec)
    idx = rs.randint(0, 5, size=(3, 40))
    idx[1, 3], idx[2, 9], idx[0, 11] = 5, -1, 2 ** 30
    for s_use in (1, 2, 3):
        want, _ = Q.reconstruct(idx, list(vec), s_use)
        got = cb.reconstruct(idx, stages=s_use)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(cb.reconstruct(idx[:s_use]), want)
    assert (cb.reconstruct(idx)[[3, 9, 11]] == 0).all() and (cb.reconstruct(idx, 1)[3] != 0).any()
    assert np.array_equal(cb.reconstruct(idx[0]), cb.reconstruct(idx, 1))  # one plane given flat
    # the order is pinned on the product too
    big = ResidualCodebook(np.array([[[2.0 ** 24]], [[1.0]], [[-1.0]]], dtype=np.float32))
    assert big.reconstruct(np.zeros((3, 1), np.int64))[0, 0] == np.float32(2.0 ** 24 - 1)
    for bad in (np.zeros((4, 2), np.int64), np.zeros((3, 2)), np.zeros((1, 2, 2), np.int64)):
        with pytest.raises(ValueError, match='reconstruct'):
            cb.reconstruct(bad)
    with pytest.raises(ValueError, match=r'stages must be in \[1, S = 2\]'):
        cb.reconstruct(idx[:2], stages=3)


def test_the_reference_fit_lowers_the_distortion_stage_by_stage():
    """The greedy fit of the definition: the summed distance after stage s is at most that after stage s - 1 (a stage's means
    minimise what it leaves), and on a planted mixture of two scales two stages of K beat one stage of K."""
    for n, E, K, S in ((600, 8, 4, 3), (1000, 20, 37, 2)):
        x = R.planted(n, E, 8, 1.0, 21)
        codes, stages = Q.fit(x, K, S, iters=40, seed=0)
        totals = [float(st['dist'].sum()) for st in stages]
        print(n, E, K, S, totals, [st['near'] for st in stages])
        assert all(b <= a for a, b in zip(totals, totals[1:])) and len(codes) == S
        assert np.array_equal(stages[1]['rows'], Q.residual(x, stages[0]['idx'], codes[0])[0])
    x = Q.planted2(1200, 8, 8, 0.05, 31)
    codes, stages = Q.fit(x, 8, 2, iters=40, seed=0)
    one, two = float(stages[0]['dist'].sum()), float(stages[1]['dist'].sum())
    print('planted mixture: one stage %.6g, two stages %.6g' % (one, two))
    assert two < 0.5 * one


# ---- the file -------------------------------------------------------------------------------------------------------------------------
def test_residual_codebook_file_round_trip_and_refusals(tmp_path):
    from zs_amd.codebook import FORMAT_VERSION
    from zs_amd.rvq import ResidualCodebook
    S, K, E = 3, 5, 20
    vec = np.stack([R.planted(K, E, 2, 0.3, s) for s in range(S)])
    meta = {'enc_mode': 'continues', 'n_rows': 77, 'seed': 3, 'bits_per_unit': 4.5,
            'stages': [{'history': [[10.5, 77, 0]], 'shift': 30, 'summed_distance': 8.0, 'symbols_used': 5, 'bits_per_unit': 1.5}] * 3}
    cb = ResidualCodebook(vec, meta)
    assert (cb.kind, cb.S, cb.K, cb.E) == ('residual', S, K, E) and cb.cnorm.shape == (S, K) and cb.cnorm.dtype == np.float32
    assert all(np.array_equal(cb.cnorm[s], R.cnorm(vec[s])) for s in range(S))
    assert ResidualCodebook.default_path('ck', 1024, 4) == os.path.join('ck', 'codebooks', 'K1024x4.rvq.npz')
    path = str(tmp_path / 'K5x3.rvq.npz')
    cb.save(path)
    assert sorted(np.load(path).files) == sorted(['kind', 'format_version', 'K', 'E', 'S', 'vectors', 'meta'])
    back = ResidualCodebook.load(path, E=E)
    assert (back.S, back.K, back.E) == (S, K, E) and np.array_equal(back.vectors, vec) and back.meta == meta
    with pytest.raises(ValueError, match=r'field E is 20.*c_in\) is 8'):
        ResidualCodebook.load(path, E=8)
    two = back.with_stages(2)
    assert two.stages == 2 and back.stages is None and two.vectors is back.vectors and two._dev is back._dev
    for s in (0, 4, -1):
        with pytest.raises(ValueError, match=r'--rvq_stages must be in \[1, S = 3\]'):
            back.with_stages(s)
    good = dict(kind=np.array('residual'), format_version=np.int64(FORMAT_VERSION), K=np.int64(K), E=np.int64(E), S=np.int64(S), vectors=vec,
                meta=np.array('{}'))

    def refused(match, **change):
        d = {k: v for k, v in dict(good, **change).items() if v is not None}
        p = str(tmp_path / 'bad.npz')
        with open(p, 'wb') as f:
            np.savez(f, **d)
        with pytest.raises(ValueError, match=match):
            ResidualCodebook.load(p)

    refused("'vectors' is missing", vectors=None)
    refused("'kind' is missing", kind=None)
    refused("kind must be 'residual'", kind=np.array('vector'))
    refused("'S' is missing", S=None)
    refused("'S' must be one integer", S=np.array([3, 3]))
    refused('S is 2 but vectors has 3 stages', S=np.int64(2))
    refused("'E' is missing", E=None)
    refused('format_version is 99', format_version=np.int64(99))
    refused('K is 6', K=np.int64(6))
    refused('E is 21', E=np.int64(21))
    refused('vectors', vectors=vec.astype(np.float64))
    refused('vectors.*float32 \\[S, K, E\\]', vectors=vec[0])
    refused('meta', meta=np.array('[1, 2'))
    nan = vec.copy()
    nan[1, 2, 3] = np.nan
    refused('vectors.*not finite', vectors=nan)
    for v, match in ((vec[:1], r'S must be in \[2, 8\]'), (np.zeros((9, 2, 2), np.float32), r'S must be in \[2, 8\]'),
                     (vec[:, :0], r'K must be in \[1, 65536\]'), (np.zeros((2, 2, 1025), np.float32), r'E must be in \[1, 1024\]'),
                     (np.zeros((2, 2, 0), np.float32), 'E must be'), (vec.astype(np.float64), 'float32'), (vec[0], 'float32')):
        with pytest.raises(ValueError, match='residual codebook: .*' + match):
            ResidualCodebook(v)


def _three_kinds(tmp_path):
    from zs_amd.codebook import Codebook
    from zs_amd.rvq import ResidualCodebook
    from zs_amd.vq import VectorCodebook
    r, v, b = str(tmp_path / 'K4x2.rvq.npz'), str(tmp_path / 'K4.vq.npz'), str(tmp_path / 'K4.codebook.npz')
    ResidualCodebook(np.stack([R.planted(4, 8, 2, 0.3, 1), R.planted(4, 8, 2, 0.03, 2)])).save(r)
    VectorCodebook(R.planted(4, 8, 2, 0.3, 1)).save(v)
    Codebook(BR.planted(4, 8, 2, 0.3, 1), 8).save(b)
    return r, v, b


def test_load_codebook_dispatches_over_the_three_kinds(tmp_path):
    from zs_amd.codebook import Codebook
    from zs_amd.rvq import ResidualCodebook
    from zs_amd.vq import VectorCodebook, load_codebook
    r, v, b = _three_kinds(tmp_path)
    got = load_codebook(r, 'continues', 8)
    assert isinstance(got, ResidualCodebook) and (got.S, got.K, got.E) == (2, 4, 8)
    assert type(load_codebook(v, 'continues', 8)) is VectorCodebook and type(load_codebook(b, 'multilabel_binary', 8)) is Codebook
    for mode in ('multilabel_binary', 'one_hot', 'binary', 'gumbel_t'):
        with pytest.raises(ValueError, match=r"residual codebook \(kind 'residual'\).*'continues'.*%s" % mode):
            load_codebook(r, mode, 8)
        with pytest.raises(ValueError, match=r"vector codebook \(kind 'vector'\).*'continues'.*%s" % mode):
            load_codebook(v, mode, 8)                                       # the vector kind's words, unchanged
        assert type(load_codebook(b, mode, 8)) is Codebook
    with pytest.raises(ValueError, match=r"enc_mode 'continues' has no units to pack \(its encodings are not 0 / 1\)"):
        load_codebook(b, 'continues', 8)
    with pytest.raises(ValueError, match=r'field E is 8.*c_in\) is 16'):
        load_codebook(r, 'continues', 16)
    with pytest.raises(ValueError, match="kind must be 'vector'"):          # the vector class's own refusal of a foreign kind
        VectorCodebook.load(r)
    with pytest.raises(ValueError, match="kind must be 'residual'"):
        ResidualCodebook.load(v)
    with pytest.raises(ValueError, match=r"a residual codebook serves enc_mode 'continues': this model's enc_mode is 'binary'"):
        ResidualCodebook.check_mode('binary')
    ResidualCodebook.check_mode('continues')


# ---- the unit files -------------------------------------------------------------------------------------------------------------------
def test_index_rows_round_trip_and_refusals(tmp_path):
    from zs_amd import convert as cv
    p = str(tmp_path / 'a.idx.txt')
    rows = np.array([[3, 0, 15], [1, 2, 3], [15, 15, 0]], dtype=np.int32)
    cv.write_index_rows(p, rows)
    assert open(p).read() == '3 0 15\n1 2 3\n15 15 0\n'
    back = cv.read_index_rows(p, 16, 3)
    assert back.dtype == np.int32 and np.array_equal(back, rows) and np.array_equal(cv.read_index_rows(p, 16, 8), rows)
    cv.write_index_rows(p, rows[:, :1])
    assert open(p).read() == '3\n1\n15\n' and cv.read_indices(p, 16).tolist() == [3, 1, 15]       # one column: the vector kind's file
    assert cv.read_index_rows(p, 16, 2).tolist() == [[3], [1], [15]]
    for text, match in (('3 1\n1\n', 'line 2: 1 values where line 1 has 2'), ('3 1\n1 2 3\n', 'line 2: 3 values where line 1 has 2'),
                        ('1 2 3\n', r'line 1: 3 values, expected 1 to S = 2'), ('\n1 2\n', 'line 1: 0 values'),
                        ('3 1\n1 16\n', r'line 2: index 16 is outside \[0, K = 16\)'), ('-1 0\n', 'line 1: index -1'),
                        ('3 x\n', r"line 1: 'x' is not an integer"), ('1.5 2\n', 'is not an integer'), ('', 'no indices')):
        open(p, 'w').write(text)
        with pytest.raises(ValueError, match=('a.idx.txt.*' + match) if text else match):
            cv.read_index_rows(p, 16, 2)
    for bad in (np.zeros(3, np.int32), np.zeros((3, 0), np.int32), np.zeros((3, 2), np.float32)):
        with pytest.raises(ValueError, match='write_index_rows'):
            cv.write_index_rows(p, bad)
    # the one-column reader is as it was
    open(p, 'w').write('3 1\n')
    with pytest.raises(ValueError, match='line 1: 2 values, expected one index'):
        cv.read_indices(p, 16)


def test_residual_units_read_cut_and_refuse_by_columns(tmp_path):
    from zs_amd import convert as cv
    from zs_amd.rvq import ResidualCodebook
    cb = ResidualCodebook(np.stack([R.planted(16, 8, 2, 0.3, s) for s in range(3)]))
    p = str(tmp_path / 'w0.idx.txt')
    cv.write_index_rows(p, np.array([[3, 0], [1, 2]], dtype=np.int32))
    side = cb.units()
    assert isinstance(side, cv._ResidualUnits) and side.s_use == 3 and side.unit_glob == '*.idx.txt' and side.spoken_stem('w0.idx') == 'w0'
    assert side.read_unit_file(p, 8).tolist() == [[3, 0], [1, 2]]          # no s' given: the file's own columns
    assert cb.with_stages(1).units().read_unit_file(p, 8).tolist() == [[3], [1]] and cb.units(2).s_use == 2
    with pytest.raises(ValueError, match=r'w0\.idx\.txt holds c = 2 indices per line, fewer than the s = 3 stages asked for'):
        cb.with_stages(3).units().read_unit_file(p, 8)
    with pytest.raises(ValueError, match='--rvq_stages must be in'):
        cb.units(4)
    side.write_spoken(str(tmp_path / 'out'), np.array([[1, 2, 3]], np.int32), 8)
    assert open(str(tmp_path / 'out.idx.txt')).read() == '1 2 3\n'
    # the folder report of this kind: a histogram and a distance per stage, the totals over them
    st = cv._CodebookStats(cb.with_stages(2), 'f.rvq.npz')
    st.add([np.array([[0, 1], [0, 2], [1, 1]], np.int32), np.array([[0, 1]], np.int32)], np.array([8.0, 2.0]))
    m = st.manifest()
    assert m['S'] == 3 and len(m['stages']) == 2 and m['stages'][0]['mean_distance'] == 2.0 and m['mean_distance'] == 0.5
    assert [s['symbols_used'] for s in m['stages']] == [2, 2] and m['symbols_used'] == 2
    assert abs(m['entropy_bits_per_unit'] - 2 * 0.8112781244591328) < 1e-12
    from zs_amd.vq import VectorCodebook
    plain = cv._CodebookStats(VectorCodebook(R.planted(4, 8, 2, 0.3, 1)), 'f.vq.npz')
    plain.add([np.array([0, 1, 1], np.int32)], 3.0)
    assert plain.manifest() == {'file': 'f.vq.npz', 'K': 4, 'symbols_used': 2, 'entropy_bits_per_unit': plain.manifest()['entropy_bits_per_unit'],
                                'mean_distance': 1.0}


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def test_rvq_flags_are_refused_before_anything_is_built(tmp_path, monkeypatch, capsys):
    import main as M
    r, v, b = _three_kinds(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    for argv in (['--rvq', '1'], ['--rvq', '9'], ['--rvq', 'x'], ['--rvq_stages', '0'], ['--rvq_stages', '9'], ['--rvq_stages', '1.5']):
        with pytest.raises(SystemExit):
            M.build_parser().parse_args(argv)
        assert argv[0] + ' must be' in capsys.readouterr().err
    cont = ['--hps_path', HPS, '--enc_mode', 'continues']
    for argv, match in ((['--rvq', '2'], '--rvq needs --fit_codebook'),
                        (['--rvq', '2', '--convert_dir', 'd', '--codebook', r], '--rvq needs --fit_codebook'),
                        (['--rvq_stages', '1'], '--rvq_stages needs --codebook'),
                        (['--rvq_stages', '1', '--fit_codebook', '8', '--fit_dir', 'd'], '--rvq_stages needs --codebook'),
                        (['--fit_codebook', '8', '--fit_dir', 'd', '--rvq', '2', '--hps_path', HPS],
                         r"--rvq fits a residual codebook.*'continues'.*multilabel_binary"),
                        (['--fit_codebook', '8', '--fit_dir', 'd', '--rvq', '2', '--hps_path', HPS, '--enc_mode', 'one_hot'], "--rvq fits.*one_hot"),
                        (['--convert_dir', 'd', '--codebook', r, '--hps_path', HPS], r"--codebook .*residual codebook.*'continues'.*multilabel_binary"),
                        (['--synth_dir', 'd', '--codebook', r, '--rvq_stages', '1', '--hps_path', HPS, '--enc_mode', 'binary'],
                         r"--codebook .*residual codebook.*'continues'.*binary"),
                        (['--convert_dir', 'd', '--codebook', r, '--rvq_stages', '3'] + cont, r'--rvq_stages 3: .* has S = 2 stages'),
                        (['--test_encode', '--codebook', v, '--rvq_stages', '1'] + cont, r'--rvq_stages needs a residual codebook .*K4\.vq\.npz is none'),
                        (['--synth_dir', 'd', '--codebook', b, '--rvq_stages', '1', '--hps_path', HPS], '--rvq_stages needs a residual codebook'),
                        (['--train_ae', '--synthetic', '--vq_train', r, '--hps_path', os.path.join(ROOT, 'hps', 'zerospeech_english.json'),
                          '--enc_mode', 'continues'], '--vq_train: '),
                        ):
        with pytest.raises(ValueError, match=match):
            M.argument_runner(argv)
    with pytest.raises(SystemExit):                                        # --rvq_stages with --codebook but no mode: --codebook's own refusal
        M.argument_runner(['--codebook', r, '--rvq_stages', '1'])
    assert '--codebook needs --convert_dir, --synth_dir or --test_encode' in capsys.readouterr().err


def test_vq_train_refuses_a_residual_codebook(tmp_path, monkeypatch):
    from zs_amd.vq_train import check_vq_train
    import main as M
    r, v, _ = _three_kinds(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    args = M.build_parser().parse_args(['--train_ae', '--vq_train', r])
    assert check_vq_train(args) is None                                    # the flag combination alone is fine
    with pytest.raises(ValueError, match=r"--vq_train: .*K4x2\.rvq\.npz is a residual codebook \(kind 'residual'\): training through a residual"):
        check_vq_train(args, 'continues', 8)
    with pytest.raises(ValueError, match="--vq_train needs enc_mode 'continues'"):                  # the mode comes first, in its own words
        check_vq_train(args, 'binary', 8)
    args = M.build_parser().parse_args(['--train_ae', '--vq_train', v])
    assert check_vq_train(args, 'continues', 8).kind == 'vector'


def test_accepted_combinations(tmp_path, monkeypatch):
    import main as M
    r, v, _ = _three_kinds(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    cont = ['--hps_path', HPS, '--enc_mode', 'continues']
    args, _ = M.argument_runner(['--fit_codebook', '8', '--fit_dir', 'd', '--rvq', '2'] + cont)
    assert (args.rvq, args.fit_codebook, args.rvq_stages) == (2, 8, None)
    args, _ = M.argument_runner(['--fit_codebook', '8', '--fit_dir', 'd', '--rvq', '8', '--codebook_out', 'x.rvq.npz'] + cont)
    assert args.rvq == 8
    for mode in (['--convert_dir', 'd'], ['--synth_dir', 'd'], ['--test_encode']):
        for extra in ([], ['--rvq_stages', '1'], ['--rvq_stages', '2']):
            args, _ = M.argument_runner(mode + ['--codebook', r] + extra + cont)
            assert args.rvq_stages == (int(extra[1]) if extra else None) and args.rvq is None
    args, _ = M.argument_runner(['--convert_dir', 'd', '--codebook', v] + cont)                    # a vector codebook: as it was
    assert args.rvq_stages is None
    args, _ = M.argument_runner(['--fit_codebook', '8', '--fit_dir', 'd'] + cont)
    assert args.rvq is None


def test_header_declares_the_two_entry_points():
    from zs_amd import _lib as L, rvq as Q2
    assert L.ENUMS['ZS_ABI_VERSION'] == 1 and L.ENUMS['ZS_RVQ_MAX_S'] == 8 == Q2.MAX_S
    assert {'zs_rvq_residual', 'zs_rvq_gather'} <= set(L.FUNCTIONS) and {'ZsRvqResidual', 'ZsRvqGather'} <= set(L.STRUCTS)
    assert [f for f, _ in L._STRUCT_FIELDS['ZsRvqGather']][:6] == ['dtype', 'idx', 'n_idx', 'ld_idx', 'S', 's_use']
    assert L.PROTOS['zs_rvq_residual'][2] == 'ZsRvqResidual' and L.PROTOS['zs_rvq_gather'][2] == 'ZsRvqGather'
