"""--convert_dir without a GPU: the work plan (sorting, group caps, pairs per target, output paths, what is refused or skipped),
the command line, the wav header reader, and the reflection of zs_trim's ABI comment against np.pad."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HPS = os.path.join(ROOT, 'hps', 'zerospeech_english.json')

import zs_amd  # noqa: E402,F401
from zs_amd import convert as cv  # noqa: E402
import trim_ref  # noqa: E402


def _items(plan):
    return [it for g in plan['groups'] for it in g]


def test_plan_sorts_by_duration_and_pairs_every_file_with_every_target():
    files = ['/in/c.wav', '/in/a.wav', '/in/b.wav']
    plan = cv.convert_dir_plan(files, [3.0, 1.0, 2.0], ['V001', 'V002'], '/out', batch=64)
    items = _items(plan)
    assert [(it['stem'], it['target']) for it in items] == [('a', 'V001'), ('a', 'V002'), ('b', 'V001'), ('b', 'V002'), ('c', 'V001'),
                                                            ('c', 'V002')]
    assert [it['duration'] for it in items] == [1.0, 1.0, 2.0, 2.0, 3.0, 3.0]
    assert len(plan['groups']) == 1 and plan['skipped'] == []
    for it in items:
        assert it['wav'] == os.path.join('/out', it['target'], it['stem'] + '.wav')
        assert it['txt'] == os.path.join('/out', it['target'], it['stem'] + '.txt')
        assert it['file'] == '/in/%s.wav' % it['stem']


def test_plan_group_caps():
    files = ['/in/f%02d.wav' % i for i in range(10)]
    durs = [float(i + 1) for i in range(10)]
    # at most `batch` items
    plan = cv.convert_dir_plan(files, durs, ['V001'], '/out', batch=4)
    assert [len(g) for g in plan['groups']] == [4, 4, 2]
    # at most max_batch_seconds of padded audio, items x the longest
    plan = cv.convert_dir_plan(files, durs, ['V001'], '/out', batch=64, max_batch_seconds=12.0)
    for g in plan['groups']:
        assert len(g) == 1 or len(g) * max(it['duration'] for it in g) <= 12.0
    assert [[it['duration'] for it in g] for g in plan['groups']] == [[1.0, 2.0, 3.0], [4.0, 5.0], [6.0], [7.0], [8.0], [9.0], [10.0]]
    assert len(_items(plan)) == 10
    # a single file above the cap is a group of its own, and is not dropped
    plan = cv.convert_dir_plan(['/in/a.wav', '/in/b.wav', '/in/c.wav'], [1.0, 50.0, 2.0], ['V001'], '/out', max_batch_seconds=10.0)
    assert [[it['stem'] for it in g] for g in plan['groups']] == [['a', 'c'], ['b']]
    # both caps with several targets: a file's items may be split over two groups, never lost or repeated
    plan = cv.convert_dir_plan(files, durs, ['V001', 'V002', 'V003'], '/out', batch=4)
    assert all(len(g) <= 4 for g in plan['groups'])
    assert sorted((it['stem'], it['target']) for it in _items(plan)) == sorted(('f%02d' % i, t) for i in range(10)
                                                                                for t in ('V001', 'V002', 'V003'))


def test_plan_refuses_duplicate_stems_and_bad_arguments():
    with pytest.raises(ValueError, match='same outputs'):
        cv.convert_dir_plan(['/a/x.wav', '/b/x.wav'], [1.0, 1.0], ['V001'], '/out')
    with pytest.raises(ValueError):
        cv.convert_dir_plan(['/a/x.wav'], [1.0, 2.0], ['V001'], '/out')
    with pytest.raises(ValueError):
        cv.convert_dir_plan(['/a/x.wav'], [1.0], [], '/out')
    with pytest.raises(ValueError):
        cv.convert_dir_plan(['/a/x.wav'], [1.0], ['V001', 'V001'], '/out')


def test_plan_skips_over_long_and_empty_files():
    plan = cv.convert_dir_plan(['/in/long.wav', '/in/ok.wav', '/in/empty.wav'], [1801.0, 5.0, 0.0], ['V001'], '/out')
    assert [it['stem'] for it in _items(plan)] == ['ok']
    assert sorted(s['file'] for s in plan['skipped']) == ['/in/empty.wav', '/in/long.wav']
    reasons = {s['file']: s['reason'] for s in plan['skipped']}
    assert 'max_seconds' in reasons['/in/long.wav'] and 'no samples' in reasons['/in/empty.wav']
    assert cv.convert_dir_plan(['/in/long.wav'], [1801.0], ['V001'], '/out', max_seconds=3600)['skipped'] == []


def test_plan_is_deterministic_under_file_order():
    rng = np.random.RandomState(0)
    files = ['/in/u%03d.wav' % i for i in range(37)]
    durs = [float(d) for d in rng.randint(1, 9, size=37)]          # many equal durations: the path breaks the ties
    ref = cv.convert_dir_plan(files, durs, ['V001', 'V002'], '/out', batch=8, max_batch_seconds=40.0)
    for seed in range(3):
        perm = np.random.RandomState(seed + 1).permutation(37)
        got = cv.convert_dir_plan([files[i] for i in perm], [durs[i] for i in perm], ['V001', 'V002'], '/out', batch=8, max_batch_seconds=40.0)
        assert got == ref


def test_command_line_accepts_convert_dir_and_refuses_an_unusable_target():
    import main
    p = main.build_parser()
    assert p.parse_args([]).convert_dir is None
    args, _ = main.argument_runner(['--convert_dir', 'd', '--t_speaker', 'V001,V002', '--hps_path', HPS])
    assert args.convert_dir == 'd' and args.t_speakers == ['V001', 'V002']
    args, _ = main.argument_runner(['--convert_dir', 'd', '--hps_path', HPS])                 # the default target
    assert args.t_speakers == ['V002']
    args, _ = main.argument_runner(['--convert_dir', 'd', '--t_speaker', 'V001', '--enc_only', '--hps_path', HPS])
    assert args.t_speakers == ['V001'] and args.enc_only
    # --test_single keeps the single name, whatever it holds
    args, _ = main.argument_runner(['--test_single', '--t_speaker', 'V001,V002', '--hps_path', HPS])
    assert args.t_speaker == 'V001,V002' and args.t_speakers is None
    # refused in argument_runner, i.e. before main() builds a model
    for bad in ('', ',', 'V001,', 'V001,,V002', 'V001,V001'):
        with pytest.raises(ValueError, match='t_speaker'):
            main.argument_runner(['--convert_dir', 'd', '--t_speaker', bad, '--hps_path', HPS])
    with pytest.raises(SystemExit):
        p.parse_args(['--convert_dir'])


def test_convert_dir_checks_targets_before_reading(tmp_path):
    import json
    s2i = tmp_path / 's2i.json'
    s2i.write_text(json.dumps({'S015': 0, 'V001': 1}))
    with pytest.raises(ValueError, match='V009'):
        cv.convert_dir(None, 128, str(tmp_path / 'missing_dir'), str(s2i), str(tmp_path / 'out'), ['V001', 'V009'], True)
    assert not (tmp_path / 'out').exists()


@pytest.mark.parametrize('n', [1, 2, 3, 700, 1024, 1025])
def test_triangle_wave_reflection_is_numpy_reflect(n):
    """The refl of zs_trim's ABI comment, for the pad of frame_length / 2 = 1024 on either side, whatever n is."""
    y = np.arange(n, dtype=np.float64)                              # the value is the index
    want = np.pad(y, 1024, mode='reflect').astype(np.int64)
    got = trim_ref.refl(np.arange(-1024, n + 1024), n)
    assert np.array_equal(got, want)


@pytest.mark.parametrize('n', [1, 2, 3, 700, 1024, 1025, 2049, 9000])
def test_restated_trim_equals_convert_trim(n):
    rng = np.random.RandomState(n)
    y = (rng.randn(n) * 0.1).astype(np.float32)
    y[:n // 3] = 0.0
    assert trim_ref.trim_bounds(y) == cv.trim(y)[1]
    assert trim_ref.trim_bounds(np.zeros(n, np.float32)) == cv.trim(np.zeros(n, np.float32))[1] == (0, n)
    assert trim_ref.trim_bounds(np.full(n, 1e-6, np.float32)) == (0, n)           # under the 1e-10 floor: everything is kept


def test_wav_info_reads_headers_without_the_audio(tmp_path):
    from scipy.io import wavfile
    from zs_amd.preprocess import read_wav, wav_info
    rng = np.random.RandomState(0)
    cases = {'i16.wav': (16000, (rng.randn(1234) * 3000).astype(np.int16)),
             'f32.wav': (22050, (rng.randn(777) * 0.1).astype(np.float32)),
             'st.wav': (44100, (rng.randn(501, 2) * 3000).astype(np.int16)),
             'u8.wav': (8000, rng.randint(0, 255, size=333).astype(np.uint8)),
             'one.wav': (16000, np.zeros(1, np.int16))}
    for name, (sr, data) in cases.items():
        path = str(tmp_path / name)
        wavfile.write(path, sr, data)
        assert wav_info(path) == (sr, data.shape[0]) == (read_wav(path)[1], len(read_wav(path)[0]))
    bad = tmp_path / 'bad.wav'
    bad.write_bytes(b'this is not a wav file at all')
    with pytest.raises(ValueError):
        wav_info(str(bad))
    (tmp_path / 'short.wav').write_bytes(b'RIFF')
    with pytest.raises(ValueError):
        wav_info(str(tmp_path / 'short.wav'))
