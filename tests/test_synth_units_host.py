"""Speech from unit files without a GPU: the packed form of the units (the definition zs_units_pack / zs_units_unpack are tested
against), the fragment rule on unit counts against the rule on frames, the parser of unit files, the work plan of --synth_dir and the
command line."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HPS = os.path.join(ROOT, 'hps', 'zerospeech_english.json')

import zs_amd  # noqa: E402,F401
from zs_amd import convert as cv  # noqa: E402


# ---- packed units --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E', [1, 6, 8, 9, 64, 1000, 1024])
def test_pack_units_round_trip_and_bit_order(E):
    rng = np.random.RandomState(E)
    u = (rng.rand(13, E) < 0.5).astype(np.float32)
    u[0], u[1] = 0.0, 1.0                                            # an empty row and a full one
    p = cv.pack_units(u)
    assert p.dtype == np.uint8 and p.shape == (13, (E + 7) // 8)
    assert np.array_equal(p, np.packbits(u.astype(bool), axis=1, bitorder='little'))
    for r, c in ((2, 0), (3, E - 1), (4, E // 2)):                   # bit j of byte k is column 8k + j
        one = np.zeros((1, E), dtype=np.float32)
        one[0, c] = 1.0
        q = cv.pack_units(one)
        assert q[0, c // 8] == 1 << (c % 8) and int(q.astype(np.int64).sum()) == 1 << (c % 8)
    if E % 8:                                                        # the unused high bits of a row's last byte are zero
        assert not (p[:, -1] >> (E % 8)).any()
        assert p[1, -1] == (1 << (E % 8)) - 1
    back = cv.unpack_units(p, E)
    assert back.dtype == np.float32 and back.shape == u.shape and np.array_equal(back, u)
    assert np.array_equal(cv.pack_units(u.astype(np.int64)), p) and np.array_equal(cv.pack_units(u.astype(bool)), p)
    assert cv.pack_units(np.zeros((0, E))).shape == (0, (E + 7) // 8)


def test_pack_units_refuses_other_values_and_shapes():
    u = np.zeros((3, 8), dtype=np.float32)
    for bad in (2, 0.5, -1, float('nan')):
        v = u.copy()
        v[1, 3] = bad
        with pytest.raises(ValueError, match='0 or 1'):
            cv.pack_units(v)
    with pytest.raises(ValueError):
        cv.pack_units(np.zeros(8))
    with pytest.raises(ValueError):
        cv.unpack_units(np.zeros((3, 2), dtype=np.uint8), 8)         # two bytes for eight columns
    with pytest.raises(ValueError):
        cv.unpack_units(np.zeros((3, 1), dtype=np.int32), 8)


# ---- the fragment rule in units -------------------------------------------------------------------------------------------------
def _frame_rule(n, seg_len):
    """The unit lengths fragments() and _t8 give an utterance of n >= MIN_LEN frames (convert() / _enqueue_encode)."""
    if n <= seg_len:
        return [cv._t8(n)]
    return [cv._t8(b - a) for a, b in cv.fragments(n, seg_len)]


@pytest.mark.parametrize('seg_len', [32, 64, 128])
def test_unit_fragments_against_the_frame_rule(seg_len):
    Lu = seg_len // 8
    mismatch = set()
    for n in range(cv.MIN_LEN, 10 * seg_len):
        want = _frame_rule(n, seg_len)
        got = cv.unit_fragments(sum(want), seg_len)
        assert sum(got) == sum(want) and all(1 <= g <= 2 * Lu for g in got) and all(g == Lu for g in got[:-1])
        if got != want:
            mismatch.add(n)
            assert want[-2:] == [Lu, Lu] and got == want[:-2] + [2 * Lu]          # one boundary fewer, nothing else
    expected = {n for n in range(cv.MIN_LEN, 10 * seg_len)
                if (n % seg_len == 1 and n >= 2 * seg_len + 1) or (n % seg_len == 0 and n >= 3 * seg_len)}
    assert mismatch == expected and expected


def test_unit_fragments_rule_itself():
    assert cv.unit_fragments(1, 32) == [1] and cv.unit_fragments(8, 32) == [8] and cv.unit_fragments(9, 32) == [4, 5]
    assert cv.unit_fragments(12, 32) == [4, 8] and cv.unit_fragments(13, 32) == [4, 4, 5]
    assert cv.unit_fragments(100, 128) == [16] * 5 + [20]
    for bad in (0, -3):
        with pytest.raises(ValueError):
            cv.unit_fragments(bad, 32)
    with pytest.raises(ValueError):
        cv.unit_fragments(5, 4)


# ---- unit files ------------------------------------------------------------------------------------------------------------------------
def test_read_units_reads_what_write_encodings_writes(tmp_path):
    rng = np.random.RandomState(0)
    for E in (1, 8, 20):
        u = (rng.rand(11, E) < 0.5).astype(np.float32)
        path = str(tmp_path / ('u%d.txt' % E))
        cv.write_encodings(path, u)
        got = cv.read_units(path, E)
        assert got.dtype == np.float32 and np.array_equal(got, u)


def test_read_units_names_file_and_line(tmp_path):
    def write(name, text):
        p = tmp_path / name
        p.write_text(text)
        return str(p)
    good = '0 1 0 1\n1 1 0 0\n'
    assert cv.read_units(write('good.txt', good), 4).shape == (2, 4)
    cases = [('narrow.txt', good + '0 1 0\n', 3), ('wide.txt', '0 1 0 1 1\n' + good, 1), ('token.txt', good + '0 2 0 1\n', 3),
             ('real.txt', '0 1 0 1\n0.5 1 0 0\n', 2), ('blank.txt', '0 1 0 1\n\n1 1 0 0\n', 2), ('word.txt', 'a b c d\n', 1)]
    for name, text, line in cases:
        path = write(name, text)
        with pytest.raises(ValueError) as e:
            cv.read_units(path, 4)
        assert path in str(e.value) and 'line %d' % line in str(e.value), (name, str(e.value))
    path = write('empty.txt', '')
    with pytest.raises(ValueError) as e:
        cv.read_units(path, 4)
    assert path in str(e.value) and 'empty' in str(e.value)
    with pytest.raises(ValueError, match='line 1'):
        cv.read_units(write('good8.txt', good), 8)                   # a file of another encoder width


# ---- the plan of --synth_dir ------------------------------------------------------------------------------------------------------
def _items(plan):
    return [it for g in plan['groups'] for it in g]


def test_synth_dir_plan_sorts_by_units_and_pairs_every_file_with_every_target():
    files = ['/in/c.txt', '/in/a.txt', '/in/b.txt', '/in/d.txt']
    plan = cv.synth_dir_plan(files, [30, 10, 20, 10], ['V001', 'V002'], '/out')
    items = _items(plan)
    assert [(it['stem'], it['target']) for it in items] == [('a', 'V001'), ('a', 'V002'), ('d', 'V001'), ('d', 'V002'), ('b', 'V001'),
                                                            ('b', 'V002'), ('c', 'V001'), ('c', 'V002')]
    assert [it['units'] for it in items] == [10, 10, 10, 10, 20, 20, 30, 30]
    assert len(plan['groups']) == 1 and plan['skipped'] == []
    for it in items:
        assert it['wav'] == os.path.join('/out', it['target'], it['stem'] + '.wav') and it['file'] == '/in/%s.txt' % it['stem']
    rng = np.random.RandomState(0)
    files = ['/in/u%03d.txt' % i for i in range(37)]
    units = [int(n) for n in rng.randint(2, 9, size=37)]             # many equal lengths: the path breaks the ties
    ref = cv.synth_dir_plan(files, units, ['V001', 'V002'], '/out', batch=8, max_batch_units=40)
    for seed in range(3):
        perm = np.random.RandomState(seed + 1).permutation(37)
        assert cv.synth_dir_plan([files[i] for i in perm], [units[i] for i in perm], ['V001', 'V002'], '/out', batch=8,
                                 max_batch_units=40) == ref


def test_synth_dir_plan_caps_skips_and_refusals():
    files = ['/in/f%02d.txt' % i for i in range(10)]
    units = [10 * (i + 1) for i in range(10)]
    plan = cv.synth_dir_plan(files, units, ['V001'], '/out', batch=4)
    assert [len(g) for g in plan['groups']] == [4, 4, 2]
    plan = cv.synth_dir_plan(files, units, ['V001'], '/out', max_batch_units=120)
    assert [[it['units'] for it in g] for g in plan['groups']] == [[10, 20, 30], [40, 50], [60], [70], [80], [90], [100]]
    plan = cv.synth_dir_plan(['/in/a.txt', '/in/b.txt', '/in/c.txt'], [10, 500, 20], ['V001'], '/out', max_batch_units=100)
    assert [[it['stem'] for it in g] for g in plan['groups']] == [['a', 'c'], ['b']]       # above the cap: a group of its own
    plan = cv.synth_dir_plan(files, units, ['V001', 'V002', 'V003'], '/out', batch=4)
    assert all(len(g) <= 4 for g in plan['groups'])
    assert sorted((it['stem'], it['target']) for it in _items(plan)) == sorted(('f%02d' % i, t) for i in range(10)
                                                                                for t in ('V001', 'V002', 'V003'))
    plan = cv.synth_dir_plan(['/in/one.txt', '/in/ok.txt', '/in/two.txt'], [1, 5, 2], ['V001'], '/out')
    assert [it['stem'] for it in _items(plan)] == ['two', 'ok']
    assert [(s['file'], 'fewer than 2 units' in s['reason']) for s in plan['skipped']] == [('/in/one.txt', True)]
    with pytest.raises(ValueError, match='same outputs'):
        cv.synth_dir_plan(['/a/x.txt', '/b/x.txt'], [5, 5], ['V001'], '/out')
    for args in ((['/a/x.txt'], [5, 6], ['V001']), (['/a/x.txt'], [5], []), (['/a/x.txt'], [5], ['V001', 'V001'])):
        with pytest.raises(ValueError):
            cv.synth_dir_plan(*args, out_dir='/out')


def test_synth_dir_checks_targets_before_reading(tmp_path):
    s2i = tmp_path / 's2i.json'
    s2i.write_text(json.dumps({'S015': 0, 'V001': 1}))
    with pytest.raises(ValueError, match='V009'):
        cv.synth_dir(None, 128, str(tmp_path / 'missing_dir'), str(s2i), str(tmp_path / 'out'), ['V001', 'V009'], True)
    assert not (tmp_path / 'out').exists()


# ---- command line ----------------------------------------------------------------------------------------------------------------------
def test_command_line_accepts_synth_dir():
    import main
    p = main.build_parser()
    assert p.parse_args([]).synth_dir is None
    args, _ = main.argument_runner(['--synth_dir', 'd', '--t_speaker', 'V001,V002', '--hps_path', HPS])
    assert args.synth_dir == 'd' and args.convert_dir is None and args.t_speakers == ['V001', 'V002']
    args, _ = main.argument_runner(['--synth_dir', 'd', '--enc_only', '--hps_path', HPS])     # the default target
    assert args.t_speakers == ['V002'] and args.enc_only
    args, _ = main.argument_runner(['--synth_dir', 'd', '--convert_dir', 'w', '--t_speaker', 'V001', '--hps_path', HPS])
    assert (args.synth_dir, args.convert_dir, args.t_speakers) == ('d', 'w', ['V001'])       # both in one command
    # refused in argument_runner, i.e. before main() builds a model (the hps file does not exist)
    for bad in ('', ',', 'V001,', 'V001,,V002', 'V001,V001'):
        with pytest.raises(ValueError, match='t_speaker'):
            main.argument_runner(['--synth_dir', 'd', '--t_speaker', bad, '--hps_path', '/nonexistent/hps.json'])
    with pytest.raises(SystemExit):
        p.parse_args(['--synth_dir'])
    main.check_ema(p.parse_args(['--use_ema', '--synth_dir', 'X']))
    with pytest.raises(ValueError, match='--use_ema needs a mode that loads a checkpoint'):
        main.check_ema(p.parse_args(['--use_ema']))
    with pytest.raises(ValueError, match='--ema'):
        main.check_ema(p.parse_args(['--synth_dir', 'X', '--ema', '0.9']))
    assert main.OUT_OF_SCOPE == ['train_al', 'train_t', 'test_asr', 'encode']


def test_units_entry_points_are_declared_and_exported():
    from zs_amd import _lib
    assert {'zs_units_unpack', 'zs_units_pack'} <= set(_lib.FUNCTIONS)
    assert {'ZsUnitsUnpack', 'ZsUnitsPack'} <= set(_lib.STRUCTS)
    assert _lib.ENUMS['ZS_UNITS_MAX_FRAG'] == 1 << 20
    L = _lib.lib()
    assert hasattr(L, 'zs_units_unpack') and hasattr(L, 'zs_units_pack')
