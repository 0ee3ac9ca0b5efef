"""--segment without a GPU: the fp32 definition of tests/segment_ref.py against exhaustive enumeration, the host half of
zs_amd.segment (runs / expand, <name>.seg.txt, check_lambda, the score budget) and main.py's refusals, which come before anything is
loaded."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import segment_ref as R  # noqa: E402


def _int_scores(rs, T, K):
    """Integer scores in [0, 4] with ties planted: equal neighbours in a row and a repeated row."""
    s = rs.randint(0, 5, size=(T, K)).astype(np.int64)
    if K > 1:
        s[::2, 1] = s[::2, 0]
    if T > 2:
        s[2] = s[1]
    return s


@pytest.mark.parametrize('K', [1, 2, 3])
@pytest.mark.parametrize('T', [1, 2, 3, 4, 5, 6])
def test_fp32_recurrence_is_the_optimum_on_integer_scores(K, T):
    rs = np.random.RandomState(100 * K + T)
    for trial in range(3):
        s = _int_scores(rs, T, K)
        for lam in (0, 1, 2, 100):
            idx, n_seg, cost = R.viterbi32(s.astype(np.float32), np.float32(lam))
            assert idx.min() >= 0 and idx.max() < K
            want = R.brute(s, lam)
            assert R.objective(s, lam, idx) == want                       # Python integers: exact
            assert R.viterbi64(s, lam)[0] == want
            assert cost == want                                           # the renormalised minima add up to the optimum
            assert n_seg == len(R.runs(idx))


def test_lambda_zero_is_the_lowest_argmin():
    rs = np.random.RandomState(0)
    for s in (rs.standard_normal((40, 7)).astype(np.float32), rs.randint(0, 3, size=(40, 5)).astype(np.float32)):
        idx, n_seg, cost = R.viterbi32(s, 0.0)
        assert np.array_equal(idx, s.argmin(1))
        assert cost == float(s.min(1).astype(np.float64).sum())


def test_large_lambda_is_one_segment():
    s = np.random.RandomState(1).standard_normal((30, 6)).astype(np.float32)
    idx, n_seg, _ = R.viterbi32(s, 1e30)
    assert n_seg == 1 and (idx == idx[0]).all()


def test_runs_and_expand_round_trip():
    from zs_amd import segment as S
    rs = np.random.RandomState(2)
    for T in (0, 1, 2, 17, 200):
        idx = rs.randint(0, 3, size=T).astype(np.int32)
        r = S.runs(idx)
        assert r.shape == (len(R.runs(idx)), 2) and [tuple(x) for x in r.tolist()] == R.runs(idx)
        assert np.array_equal(S.expand(r), idx) and S.expand(r).dtype == np.int32
        assert R.expand(R.runs(idx)) == idx.tolist()
        assert T == 0 or (r[:, 1] >= 1).all() and (np.diff(r[:, 0]) != 0).all()
    idx = np.asarray([4, 4, 1, 1, 1, 2], dtype=np.int32)
    per = S.runs(idx, [0, 0, 2, 6, 6])
    assert [p.tolist() for p in per] == [[], [[4, 2]], [[1, 3], [2, 1]], []]
    with pytest.raises(ValueError):
        S.expand([[1, 0]])


def test_segment_files(tmp_path):
    from zs_amd import segment as S
    p = str(tmp_path / 'a.seg.txt')
    r = np.asarray([[3, 2], [0, 1], [3, 7]], dtype=np.int64)
    S.write_segments(p, r)
    assert open(p).read() == '3 2\n0 1\n3 7\n'
    assert np.array_equal(S.read_segments(p, 4), r)
    S.write_segments(p, np.zeros((0, 2), dtype=np.int64))
    assert S.read_segments(p, 4).shape == (0, 2)
    assert S.seg_path('/x/name.txt') == '/x/name.seg.txt'
    for bad in ('3\n', '3 2 1\n', 'a 2\n', '3 b\n', '3 2.5\n', '4 1\n', '-1 1\n', '3 0\n', '3 -2\n', '\n'):
        with open(p, 'w') as f:
            f.write('1 1\n' + bad)
        with pytest.raises(ValueError) as e:
            S.read_segments(p, 4)
        assert p in str(e.value) and 'line 2' in str(e.value), bad


def test_check_lambda():
    from zs_amd import segment as S
    assert S.check_lambda(None) is None
    assert S.check_lambda(0) == 0.0 and S.check_lambda(2) == 2.0
    assert S.check_lambda(0.37) == float(np.float32(0.37))
    for bad in (-1, -1e-9, float('nan'), float('inf'), -float('inf'), 1e39, '1', None.__class__, [1], True):
        with pytest.raises(ValueError):
            S.check_lambda(bad)


def test_budget_and_work_size():
    from zs_amd import segment as S
    assert S.SCORE_BUDGET == 4 << 30
    assert S.check_budget(1000, 64) == 256000
    with pytest.raises(ValueError) as e:
        S.check_budget(1 << 20, 4096)
    assert 'smaller batch' in str(e.value) and str(1 << 20) in str(e.value) and '4096' in str(e.value)
    assert S.work_bytes(10, 64) == 10 * 12 and S.work_bytes(10, 65) == 10 * 20 and S.work_bytes(3, 4096) == 3 * (64 * 8 + 4)


def test_codebooks_that_cannot_be_segmented():
    from zs_amd import segment as S
    from zs_amd.rvq import ResidualCodebook
    from zs_amd.vq import VectorCodebook
    rs = np.random.RandomState(0)
    with pytest.raises(ValueError) as e:
        ResidualCodebook(rs.standard_normal((2, 4, 3)).astype(np.float32)).scores_(None, None)
    assert '--segment' in str(e.value)
    with pytest.raises(ValueError) as e:
        VectorCodebook(rs.standard_normal((S.MAX_K + 1, 2)).astype(np.float32)).scores_(None, None)
    assert '--segment' in str(e.value) and str(S.MAX_K) in str(e.value)
    with pytest.raises(ValueError):
        S.check_codebook(None)


# ---- the command line --------------------------------------------------------------------------------------------------------------
HPS = os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')          # seg_len 128, enc_mode multilabel_binary


def test_parse_without_segment_is_unchanged():
    import main as M
    a = M.build_parser().parse_args(['--convert_dir', 'd'])
    b = M.build_parser().parse_args(['--convert_dir', 'd', '--segment', '2.5'])
    assert a.segment is None and a.segments is False and b.segment == 2.5
    va, vb = dict(vars(a)), dict(vars(b))
    assert va.pop('segment') is None and vb.pop('segment') == 2.5 and va == vb            # nothing else moves
    M.check_segment(a)
    M.check_segment(a, 'continues')                                   # absent: nothing to refuse
    with pytest.raises(SystemExit):
        M.build_parser().parse_args(['--convert_dir', 'd', '--segment', 'x'])
    with pytest.raises(SystemExit):
        M.build_parser().parse_args(['--convert_dir', 'd', '--segment'])


def test_check_segment_refusals_come_before_anything_is_loaded(monkeypatch, tmp_path):
    import main as M
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    p = M.build_parser()
    cbk = ['--codebook', 'K4.codebook.npz']

    def refused(argv, match):
        with pytest.raises(ValueError, match=match):
            M.check_segment(p.parse_args(argv))
        with pytest.raises(ValueError, match=match):
            M.argument_runner(argv + ['--hps_path', HPS])             # no checkpoint, no file: refused before either is looked for

    for v in ('-1', 'nan', 'inf', '-inf', '1e39'):
        refused(['--convert_dir', 'd', '--segment=' + v] + cbk, '--segment: lambda must be finite and >= 0')
    refused(['--segment', '1'] + cbk[:0], '--segment needs --convert_dir or --test_encode')
    refused(['--segment', '1', '--train_ae'], '--segment needs --convert_dir or --test_encode')
    refused(['--segment', '1', '--test', '--enc_only'], '--segment needs --convert_dir or --test_encode')
    refused(['--synth_dir', 'd', '--segment', '1'] + cbk, '--segment needs --convert_dir or --test_encode')
    for other in (['--synth_dir', 'e'], ['--test'], ['--cross_test'], ['--test_single'], ['--test_classify']):
        refused(['--convert_dir', 'd', '--segment', '1'] + cbk + other, '--segment serves --convert_dir and --test_encode alone.*--%s' % other[0][2:])
    refused(['--convert_dir', 'd', '--segment', '1'], '--segment needs --codebook')
    refused(['--test_encode', '--segment', '1'], '--segment needs --codebook')
    refused(['--convert_dir', 'd', '--segment', '1', '--codebook', 'K8x2.rvq.npz'], '--segment does not segment the stages of a residual codebook')
    refused(['--convert_dir', 'd', '--segment', '1', '--rvq_stages', '1'] + cbk, 'residual codebook|--rvq_stages')
    refused(['--convert_dir', 'd', '--segments'] + cbk, '--segments needs --synth_dir')
    refused(['--synth_dir', 'd', '--segments'], '--segments needs --codebook')
    refused(['--synth_dir', 'd', '--segments', '--codebook', 'K8x2.rvq.npz'], '--segments does not segment the stages of a residual codebook')
    refused(['--convert_dir', 'd', '--synth_dir', 'e', '--segment', '1', '--segments'] + cbk, 'two commands')
    # a residual codebook under another name is told by its fields once hps is read
    from zs_amd.rvq import ResidualCodebook
    path = str(tmp_path / 'plain_name.npz')
    ResidualCodebook(np.random.RandomState(0).standard_normal((2, 4, 1024)).astype(np.float32)).save(path)
    a = p.parse_args(['--convert_dir', 'd', '--segment', '1', '--codebook', path])
    M.check_segment(a)
    with pytest.raises(ValueError, match='residual codebook'):
        M.check_segment(a, 'continues')
    # accepted
    for argv in (['--convert_dir', 'd', '--segment', '0'] + cbk, ['--test_encode', '--segment', '3.5'] + cbk,
                 ['--convert_dir', 'd', '--segment', '1', '--overlap', '16'] + cbk, ['--synth_dir', 'd', '--segments'] + cbk):
        M.check_segment(p.parse_args(argv))
        M.check_segment(p.parse_args(argv), 'multilabel_binary')
    args, hps = M.argument_runner(['--convert_dir', 'd', '--segment', '2'] + cbk + ['--hps_path', HPS])
    assert args.segment == 2.0 and args.segments is False


def test_manifests_gain_segment_only_when_given(tmp_path):
    from zs_amd import convert as cv, segment as S
    base = dict(in_dir='i', out_dir='o', t_speakers=['V001'], enc_only=True, items=[], skipped=[], stats=None, voices=None, speaker2id={})
    for name in ('convert_dir.json', 'synth_dir.json'):
        m0 = cv._write_manifest(str(tmp_path / ('a_' + name)), **base)
        m2 = cv._write_manifest(str(tmp_path / ('c_' + name)), segment=None, **base)
        assert 'segment' not in m0 and m0 == m2
        assert (tmp_path / ('a_' + name)).read_bytes() == (tmp_path / ('c_' + name)).read_bytes()
        assert list(m0) == ['in_dir', 'out_dir', 'targets', 'sr', 'enc_only', 'items', 'skipped']
    st = S.SegmentStats(1.5, 4)
    st.add([[0, 3], [2, 1]])
    st.add([[2, 4]])
    m1 = cv._write_manifest(str(tmp_path / 'b.json'), segment=st, overlap=16, **base)
    assert list(m1) == list(m0) + ['overlap', 'segment']
    seg = m1['segment']
    assert list(seg) == ['lambda', 'units', 'segments', 'mean_run_units', 'entropy_bits_per_segment', 'bits_per_second']
    assert seg['lambda'] == 1.5 and seg['units'] == 8 and seg['segments'] == 3 and seg['mean_run_units'] == 8 / 3
    ent = -(1 / 3 * np.log2(1 / 3) + 2 / 3 * np.log2(2 / 3))
    assert abs(seg['entropy_bits_per_segment'] - ent) < 1e-12
    assert abs(seg['bits_per_second'] - 3 / (8 * S.seconds_per_unit()) * ent) < 1e-9
    from zs_amd.hps import hp
    assert S.seconds_per_unit() == 8.0 * hp.hop_length / hp.sr


def test_entry_points_are_declared():
    from zs_amd import _lib
    assert _lib.SEGMENT_FUNCTIONS == ['zs_vq_scores', 'zs_code_scores', 'zs_seg_viterbi']            # include/zs_amd_segment.h, in its order
    for fn, st in (('zs_vq_scores', 'ZsVqScores'), ('zs_code_scores', 'ZsCodeScores'), ('zs_seg_viterbi', 'ZsSegViterbi')):
        assert _lib.PROTOS[fn][2] == st and st in _lib.SEGMENT_STRUCTS and st not in _lib.STRUCTS and fn not in _lib.FUNCTIONS
    assert [f for f, _ in _lib._SEGMENT_STRUCT_FIELDS['ZsSegViterbi']] == ['scores', 'n_rows', 'ld_s', 'uoffs', 'n_utt', 'row', 'n_units', 'lam', 'K',
                                                                    'work', 'work_bytes', 'idx', 'n_seg', 'cost', 'bad']
    assert _lib.ENUMS['ZS_SEG_MAX_K'] == 4096 and _lib.ZS_SEG_MAX_K == 4096
    assert len(_lib.FUNCTIONS) + len(_lib.SEGMENT_FUNCTIONS) == len(_lib.PROTOS) == 101
    if os.path.exists(_lib.LIB_PATH):                                 # a built tree: the library exports what the header declares
        assert all(hasattr(_lib.lib(), f) for f in _lib.SEGMENT_FUNCTIONS)


def test_segment_header_matches_the_c_compiler(tmp_path):
    """The layout and signature checks tests/test_host_logic.py makes for include/zs_amd.h, for include/zs_amd_segment.h: gcc's sizeof
    and offsetof of every struct against the generated ctypes Structures, the size of every parameter against the generated argtypes,
    and the work-size macro against zs_amd.segment.work_bytes."""
    import ctypes
    import subprocess
    from zs_amd import _lib, segment as S
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){\n' % _lib.SEGMENT_HEADER
    for n in _lib.SEGMENT_STRUCTS:
        src += 'printf("%s %%zu\\n", sizeof(%s));\n' % (n, n)
        for f, _ in _lib._SEGMENT_STRUCT_FIELDS[n]:
            src += 'printf("%s.%s %%zu\\n", offsetof(%s,%s));\n' % (n, f, n, f)
    cases = [(0, 1), (1, 1), (10, 64), (10, 65), (3, 4096), (2 ** 31 - 1, 4096)]
    for n, K in cases:
        src += 'printf("work %%lld\\n", (long long)ZS_SEG_WORK_BYTES(%dLL, %d));\n' % (n, K)
    src += 'return 0;}\n'
    c = tmp_path / 'seg.c'
    c.write_text(src)
    subprocess.check_call(['gcc', str(c), '-o', str(tmp_path / 'seg')])
    work = []
    for line in subprocess.check_output([str(tmp_path / 'seg')]).decode().split('\n'):
        if not line:
            continue
        k, v = line.split()
        if k == 'work':
            work.append(int(v))
        elif '.' in k:
            n, f = k.split('.')
            assert getattr(_lib.SEGMENT_STRUCTS[n], f).offset == int(v), k
        else:
            assert ctypes.sizeof(_lib.SEGMENT_STRUCTS[k]) == int(v), k
    assert work == [S.work_bytes(n, K) for n, K in cases]
    for fn in _lib.SEGMENT_FUNCTIONS:
        res, args, st = _lib.PROTOS[fn]
        assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_void_p] and st in _lib.SEGMENT_STRUCTS
