"""Overlapped decode windows on the host (no GPU): convert.unit_windows and the cross-fade weights against the numpy statement
(tests/xfade_ref.py), the plan of zs_xfade_gather (convert._xfade_tables) against a brute-force loop over frames, and what
main.py --overlap refuses before anything is built."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import xfade_ref as X  # noqa: E402
import zs_amd  # noqa: E402,F401
from zs_amd import convert as cv  # noqa: E402

HPS = os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')          # seg_len 128, enc_mode multilabel_binary
SEGS = [32, 128]


def _accepted(seg):
    return [v for v in range(0, seg + 9) if X.accepted(v, seg)]


def test_accepted_values():
    assert _accepted(32) == [0, 8, 16] and _accepted(128) == [0, 8, 16, 24, 32, 40, 48, 56, 64]


@pytest.mark.parametrize('seg', SEGS)
def test_overlap_zero_is_unit_fragments(seg):
    Lu = seg // 8
    for n in range(1, 12 * Lu + 1):
        wins = cv.unit_windows(n, seg, 0)
        assert [b - a for a, b in wins] == cv.unit_fragments(n, seg)
        assert wins[0][0] == 0 and wins[-1][1] == n and all(p[1] == q[0] for p, q in zip(wins, wins[1:]))


@pytest.mark.parametrize('seg', SEGS)
def test_window_rule(seg):
    Lu = seg // 8
    for V in _accepted(seg):
        Vu = V // 8
        for n in range(1, 12 * Lu + 1):
            wins = cv.unit_windows(n, seg, V)
            assert wins == X.windows(n, seg, V)
            cover = np.zeros(n, dtype=np.int64)
            for a, b in wins:
                assert 0 <= a < b <= n
                cover[a:b] += 1
            assert cover.min() >= 1 and cover.max() <= 2              # the union is [0, n); no unit lies in three windows
            assert all(p[1] - q[0] == Vu and q[0] > p[0] for p, q in zip(wins, wins[1:]))      # exactly Vu shared units
            assert all(b - a == Lu for a, b in wins[:-1])
            tail = wins[-1][1] - wins[-1][0]
            if n <= 2 * Lu:
                assert wins == [(0, n)]
            else:
                assert len(wins) >= 2 and Lu + Vu < tail <= 2 * Lu


@pytest.mark.parametrize('seg', SEGS)
def test_refused_values(seg):
    Lu = seg // 8
    bad = [4, 12, 8 * (Lu // 2) + 8, -8, 1, 7, 9, seg, 2 * seg, 8.5, '8', None, True]
    bad += [v for v in range(0, seg + 9) if not X.accepted(v, seg)]
    for v in bad:
        with pytest.raises(ValueError, match=r'overlap must be 0 or a multiple of 8 in \[8, %d\] frames' % (8 * (Lu // 2))) as e:
            cv.unit_windows(3 * Lu, seg, v)
        assert repr(v) in str(e.value)
        with pytest.raises(ValueError, match='overlap'):
            cv.check_overlap_value(v, seg)
    for v in _accepted(seg):
        assert cv.check_overlap_value(v, seg) == v
    with pytest.raises(ValueError, match='n_units >= 1'):
        cv.unit_windows(0, seg, 8)


def test_weights_are_symmetric_and_rounded_once():
    for seg in SEGS:
        for V in _accepted(seg)[1:]:
            w, u = cv.xfade_weights(V)
            rw, ru = X.weights(V)
            assert w.dtype == np.float32 and u.dtype == np.float32 and w.shape == (V,) and u.shape == (V,)
            assert np.array_equal(w.view(np.int32), rw.view(np.int32)) and np.array_equal(u.view(np.int32), ru.view(np.int32))
            for j in range(V):
                assert w[j].view(np.int32) == u[V - 1 - j].view(np.int32), (V, j)                # w_j == u_{V-1-j}, bitwise
                assert w[j] == np.float32((2 * j + 1) / (2.0 * V)) and 0 < w[j] < 1
            assert np.all(np.diff(w) > 0)


# ---- the plan ----------------------------------------------------------------------------------------------------------------------
SEG = 32
LU = SEG // 8
UNITS = [3, 2 * LU, 2 * LU + 1, 37, 2, 5 * LU + 3, 2 * LU + 1]       # short, exactly 2 Lu, 2 Lu + 1 (twice), long ones


def _plan(V, max_batch):
    items = [it for u, n in enumerate(UNITS) for it in cv._window_items(u, n, SEG, V)]
    chunks = cv._split_chunks(items, LU, max_batch)
    # a source table as the decoded chunks laid end to end: chunk ci holds len(chunk) windows of 8 * (its longest) rows each
    first, total = [], 0
    for chunk, _ in chunks:
        ld = 8 * max(it.n for it in chunk)
        first += [total + i * ld for i in range(len(chunk))]
        total += len(chunk) * ld
    return items, chunks, first, total


@pytest.mark.parametrize('max_batch', [256, 3])
@pytest.mark.parametrize('V', [8, 16])
def test_plan_tables_against_a_loop_over_frames(V, max_batch):
    items, chunks, first, total = _plan(V, max_batch)
    for u, n in enumerate(UNITS):
        assert [(it.a, it.b) for it in items if it.u == u] == X.windows(n, SEG, V)
    flat = cv._flat(chunks)
    row = {(it.u, it.k): r0 for it, r0 in zip(flat, first)}
    where = {(it.u, it.k): ci for ci, (chunk, _) in enumerate(chunks) for it in chunk}
    if max_batch == 3:                                               # the two windows of one join lie in different chunks
        assert any(where[(u, k)] != where[(u, k + 1)] for (u, k) in where if (u, k + 1) in where)
    Tm, ulens, i0, i1, w0, w1 = cv._xfade_tables(chunks, first, len(UNITS))
    assert ulens == [8 * n for n in UNITS] and Tm == max(ulens)
    assert i0.dtype == np.int32 and i1.dtype == np.int32 and w0.dtype == np.float32 and w1.dtype == np.float32
    assert i0.shape == i1.shape == w0.shape == w1.shape == (len(UNITS) * Tm,)
    i0, i1, w0, w1 = (t.reshape(len(UNITS), Tm) for t in (i0, i1, w0, w1))
    blended = 0
    for u, n in enumerate(UNITS):
        wins = X.windows(n, SEG, V)
        for t in range(Tm):
            if t >= 8 * n:
                assert i0[u, t] == -1 and i1[u, t] == -1
                continue
            ks = [k for k, (a, b) in enumerate(wins) if 8 * a <= t < 8 * b]
            k = ks[0]
            assert 0 <= i0[u, t] < total and i0[u, t] == row[(u, k)] + t - 8 * wins[k][0]
            if len(ks) == 1:
                assert i1[u, t] == -1
            else:
                j = t - 8 * wins[k + 1][0]
                w, uw = X.weights(V)
                assert ks == [k, k + 1] and 0 <= j < V and i1[u, t] == row[(u, k + 1)] + j
                assert w0[u, t].view(np.int32) == uw[j].view(np.int32) and w1[u, t].view(np.int32) == w[j].view(np.int32)
                blended += 1
    assert blended == V * sum(len(X.windows(n, SEG, V)) - 1 for n in UNITS) > 0
    # applied to a table of distinct values, the plan and the reference's blend of the windows agree bit for bit
    rng = np.random.RandomState(V + max_batch)
    src = rng.rand(total, 5).astype(np.float32)
    out = X.gather(src, i0.reshape(-1), i1.reshape(-1), w0.reshape(-1), w1.reshape(-1), 5).reshape(len(UNITS), Tm, 5)
    for u, n in enumerate(UNITS):
        wins = X.windows(n, SEG, V)
        decoded = [src[row[(u, k)]:row[(u, k)] + 8 * (b - a)] for k, (a, b) in enumerate(wins)]
        assert np.array_equal(out[u, :8 * n], X.blend_windows(wins, decoded)) and not out[u, 8 * n:].any()


def test_plan_refuses_windows_that_do_not_join():
    It = cv._Item
    with pytest.raises(ValueError, match='first unit'):
        cv._xfade_tables([([It(0, 0, 1, 5, None)], True)], [0], 1)
    with pytest.raises(ValueError, match='does not continue'):
        cv._xfade_tables([([It(0, 0, 0, 4, None), It(0, 1, 5, 9, None)], True)], [0, 32], 1)
    with pytest.raises(ValueError, match='three windows'):
        cv._xfade_tables([([It(0, 0, 0, 4, None), It(0, 1, 2, 6, None), It(0, 2, 3, 8, None)], True)], [0, 32, 64], 1)


# ---- the command line --------------------------------------------------------------------------------------------------------------
def test_parse_without_overlap_is_unchanged():
    import main as M
    a = M.build_parser().parse_args(['--synth_dir', 'd'])
    assert a.overlap is None
    b = M.build_parser().parse_args(['--synth_dir', 'd', '--overlap', '16'])
    assert b.overlap == 16
    va, vb = dict(vars(a)), dict(vars(b))
    assert va.pop('overlap') is None and vb.pop('overlap') == 16 and va == vb         # nothing else moves
    M.check_overlap(a)
    M.check_overlap(a, 128, 'continues')                             # absent: nothing to refuse
    with pytest.raises(SystemExit):
        M.build_parser().parse_args(['--synth_dir', 'd', '--overlap', 'x'])


def test_check_overlap_refusals_and_accepted_combinations(monkeypatch):
    import main as M
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    p = M.build_parser()
    for argv in (['--overlap', '16'], ['--overlap', '16', '--test', '--enc_only'], ['--overlap', '0', '--cross_test'],
                 ['--overlap', '16', '--test_single'], ['--overlap', '16', '--train_ae']):
        with pytest.raises(ValueError, match='--overlap needs --synth_dir or --convert_dir'):
            M.check_overlap(p.parse_args(argv))
        with pytest.raises(ValueError, match='--overlap needs --synth_dir or --convert_dir'):
            M.argument_runner(argv + ['--hps_path', HPS])
    for mode in ('--synth_dir', '--convert_dir'):
        for v in ('4', '12', '72', '-8', '128'):                       # seg_len 128: multiples of 8 in [8, 64]
            a = p.parse_args([mode, 'd', '--overlap', v])
            M.check_overlap(a)                                       # the range needs seg_len: not refused before hps is read
            with pytest.raises(ValueError, match=r'--overlap: overlap must be 0 or a multiple of 8 in \[8, 64\] frames for seg_len 128 \(got %s\)' % v):
                M.check_overlap(a, 128, 'multilabel_binary')
            with pytest.raises(ValueError, match='--overlap: overlap must be'):
                M.argument_runner([mode, 'd', '--overlap', v, '--hps_path', HPS])
        for v in ('0', '8', '32', '64'):
            M.check_overlap(p.parse_args([mode, 'd', '--overlap', v]), 128, 'multilabel_binary')
        a = p.parse_args([mode, 'd', '--overlap', '24'])
        with pytest.raises(ValueError, match='--overlap'):
            M.check_overlap(a, 32, 'multilabel_binary')              # seg_len 32 stops at 16
    args, hps = M.argument_runner(['--synth_dir', 'd', '--overlap', '64', '--hps_path', HPS])
    assert args.overlap == 64 and hps.seg_len == 128
    # --convert_dir on a 'continues' model: only with a codebook; --synth_dir reads index files and is refused by its own check
    cont = p.parse_args(['--convert_dir', 'd', '--overlap', '16'])
    with pytest.raises(ValueError, match="--overlap with --convert_dir .*'continues'.*--codebook"):
        M.check_overlap(cont, 128, 'continues')
    with pytest.raises(ValueError, match="--overlap with --convert_dir .*'continues'"):
        M.argument_runner(['--convert_dir', 'd', '--overlap', '16', '--hps_path', HPS, '--enc_mode', 'continues'])
    M.check_overlap(p.parse_args(['--convert_dir', 'd', '--overlap', '0']), 128, 'continues')       # 0: today's path, nothing is spoken from units
    M.check_overlap(p.parse_args(['--convert_dir', 'd', '--overlap', '16', '--codebook', 'K4.vq.npz']), 128, 'continues')
    M.check_overlap(p.parse_args(['--synth_dir', 'd', '--overlap', '16']), 128, 'continues')
    M.check_overlap(p.parse_args(['--convert_dir', 'd', '--overlap', '16']), 128, 'one_hot')


def test_manifest_gains_overlap_only_when_given(tmp_path):
    base = dict(in_dir='i', out_dir='o', t_speakers=['V001'], enc_only=True, items=[], skipped=[], stats=None, voices=None, speaker2id={})
    m0 = cv._write_manifest(str(tmp_path / 'a.json'), **base)
    m1 = cv._write_manifest(str(tmp_path / 'b.json'), overlap=16, **base)
    m2 = cv._write_manifest(str(tmp_path / 'c.json'), overlap=None, **base)
    assert 'overlap' not in m0 and m1 == dict(m0, overlap=16)
    assert (tmp_path / 'a.json').read_bytes() == (tmp_path / 'c.json').read_bytes()
    assert list(m0) == ['in_dir', 'out_dir', 'targets', 'sr', 'enc_only', 'items', 'skipped']


def test_unit_counts_follow_the_encoder_rule():
    frames = [5, 9, 32, 33, 63, 64, 65, 95, 97, 129, 200]
    specs = [np.zeros((n, 513), dtype=np.float32) for n in frames]
    want = []
    for n in frames:
        m = max(n, cv.MIN_LEN)
        want.append(cv.MIN_LEN // 8 if n < cv.MIN_LEN else sum(cv._t8(b - a) for a, b in ([(0, m)] if m <= SEG else cv.fragments(m, SEG))))
    assert cv._unit_counts(specs, SEG) == want and want[0] == 1


def test_entry_point_is_declared():
    from zs_amd import _lib
    assert 'zs_xfade_gather' in _lib.FUNCTIONS and _lib.PROTOS['zs_xfade_gather'][2] == 'ZsXfadeGather'
    assert [f for f, _ in _lib._STRUCT_FIELDS['ZsXfadeGather']] == ['src', 'src_rows', 'ld_src', 'i0', 'i1', 'w0', 'w1', 'out', 'rows', 'out_ld',
                                                                     'cols', 'denorm']
    assert len(_lib.FUNCTIONS) == 98
