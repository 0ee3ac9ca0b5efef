"""Band-limited resampling without a GPU (zs_amd.resample): the polyphase bank against the direct fp64 sum of the definition
(tests/resample_ref.py), the filter against sampled sines, the length law, plan errors, the wav reader and the --out_sr flag.
PARITY UNPINNED with resampy / librosa.load: neither is available; the definition in zs_amd/resample.py is what is checked."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resample_ref as RR  # noqa: E402

HPS = os.path.join(ROOT, 'hps', 'zerospeech_english.json')
PAIRS = [(48000, 16000), (44100, 16000), (22050, 16000), (12345, 16000), (8000, 16000), (16000, 44100)]


def _R():
    import zs_amd  # noqa: F401
    from zs_amd import resample
    return resample


def apply_bank(x, bank, sr_in, sr_out, dtype):
    """The polyphase form of the definition in NumPy: y[t] = sum_j bank[p][j + H] * x[q + j], accumulated in `dtype`."""
    n = len(x)
    n_phase, n_tap = bank.shape
    H = (n_tap - 1) // 2
    g = math.gcd(sr_in, sr_out)
    no = RR.n_out(n, sr_in, sr_out)
    xp = np.concatenate([np.zeros(H, dtype), np.asarray(x, dtype), np.zeros(H + 1, dtype)])
    t = np.arange(no, dtype=np.int64)
    q, r = (t * sr_in) // sr_out, (t * sr_in) % sr_out
    win = xp[q[:, None] + np.arange(n_tap)[None, :]]                    # x[q - H .. q + H]
    acc = np.zeros(no, dtype)
    for j in range(n_tap):                                              # the device's order
        acc = (acc + bank[r // g, j].astype(dtype) * win[:, j]).astype(dtype)
    return acc


def test_table_and_bank_shapes():
    R = _R()
    tab = R.filter_table()
    assert tab.shape == (32769,) and tab.dtype == np.float64 and tab[0] == R.ROLLOFF
    assert np.array_equal(tab, RR.table())
    for (a, b), shape in {(48000, 16000): (1, 385), (44100, 16000): (160, 355), (22050, 16000): (320, 179), (8000, 16000): (2, 129),
                          (96000, 16000): (1, 769), (12345, 16000): (3200, 129)}.items():
        pl = R.plan(a, b)
        assert pl.bank.shape == shape == (pl.n_phase, pl.n_tap) and pl.bank.dtype == np.float32 and pl.n_tap == 2 * pl.H + 1
        assert R.plan(a, b) is pl                                       # cached
        dl = R.device_layout(pl, a, b)                                  # [tap][t mod n_phase]
        assert dl.shape == shape[::-1]
        g = math.gcd(a, b)
        for t in (0, 1, 7, shape[0] - 1, shape[0] + 3):
            assert np.array_equal(dl[:, t % shape[0]], pl.bank[((t * a) % b) // g])


@pytest.mark.parametrize('sr_in,sr_out', PAIRS)
def test_bank_equals_direct_sum(sr_in, sr_out):
    R = _R()
    x = np.random.RandomState(sr_in % 977).uniform(-1, 1, 3000)
    ref, A = RR.resample_ref(x, sr_in, sr_out)
    pl = R.plan(sr_in, sr_out)
    y64 = apply_bank(x, pl.bank64, sr_in, sr_out, np.float64)
    assert y64.shape == ref.shape
    e = np.abs(y64 - ref).max()
    print('%d -> %d: fp64 bank vs direct sum %.3g' % (sr_in, sr_out, e))
    assert e <= 1e-12
    # the bank rounded once to fp32, applied exactly: every tap is off by at most 2^-24 relative
    y32 = apply_bank(x, pl.bank.astype(np.float64), sr_in, sr_out, np.float64)
    ratio = (np.abs(y32 - ref) / (2.0 ** -24 * A)).max()
    print('%d -> %d: fp32-rounded bank, error / (2^-24 A) = %.3f' % (sr_in, sr_out, ratio))
    assert (np.abs(y32 - ref) <= 2.0 ** -24 * A).all()


@pytest.mark.parametrize('sr_in', [48000, 44100, 32000, 22050, 11025, 8000])
def test_filter_reconstructs_band_limited_sines(sr_in):
    """An independent check of the filter itself: a band-limited signal resampled to 16 kHz is that signal sampled at 16 kHz."""
    sr_out = 16000
    rng = np.random.RandomState(sr_in % 991)
    nyq = 0.5 * min(sr_in, sr_out)
    f = rng.uniform(50.0, 0.8 * nyq, 8)
    amp = rng.uniform(0.02, 0.1, 8)
    ph = rng.uniform(0, 2 * np.pi, 8)

    def sig(t):
        return (amp[None, :] * np.sin(2 * np.pi * f[None, :] * t[:, None] + ph[None, :])).sum(axis=1)

    n = sr_in // 2
    y, _ = RR.resample_ref(sig(np.arange(n) / float(sr_in)), sr_in, sr_out)
    s = min(1.0, sr_out / sr_in)
    edge = int(math.ceil(math.ceil(64 / s) * sr_out / sr_in)) + 2
    want = sig(np.arange(len(y)) / float(sr_out))
    e = np.abs(y - want)[edge:len(y) - edge].max()
    print('%d -> 16000: max |resampled - sines| away from the edges %.3g' % (sr_in, e))
    assert len(y) - 2 * edge > 1000 and e <= 2e-6
    # ... and the module's own polyphase bank gives the same signal
    R = _R()
    y2 = apply_bank(sig(np.arange(n) / float(sr_in)), R.plan(sr_in, sr_out).bank64, sr_in, sr_out, np.float64)
    assert np.abs(y2 - want)[edge:len(y) - edge].max() <= 2e-6


def test_length_law():
    R = _R()
    for sr_in, sr_out in PAIRS + [(96000, 16000)]:
        for n in (1, 2, 3, 441, 44100, 44101):
            want = int(math.ceil(n * sr_out / sr_in))
            assert R.out_length(n, sr_in, sr_out) == want == RR.n_out(n, sr_in, sr_out)
    assert len(RR.resample_ref(np.ones(441), 44100, 16000)[0]) == 160
    assert len(RR.resample_ref(np.ones(442), 44100, 16000)[0]) == 161


def test_plan_errors():
    R = _R()
    for a, b in ((16000, 16000 * 32 + 1), (16000 * 32 + 1, 16000), (100, 16000), (0, 16000), (16000, -1)):
        with pytest.raises(ValueError):
            R.plan(a, b)
    R.plan(500, 16000)
    R.plan(16000, 500)                                                  # the ends of the range are inside
    with pytest.raises(ValueError) as ei:
        R.plan(31991, 999983)                                           # coprime: 999983 phases x 129 taps
    assert '999983' in str(ei.value) and '129' in str(ei.value)
    with pytest.raises(ValueError):
        R.resample_batch([np.zeros(4)], 100, 16000, device='cpu')


def test_resample_batch_without_a_rate_change_needs_no_gpu():
    R = _R()
    a, b = np.arange(5, dtype=np.float64) / 8, np.arange(3, dtype=np.float32)
    out = R.resample_batch([a, b], 16000, device='cpu')
    assert [o.dtype for o in out] == [np.float32, np.float32] and np.array_equal(out[0], a) and np.array_equal(out[1], b)
    assert R.resample_batch([], 44100) == []


def test_read_wav_and_load_wav(tmp_path):
    from scipy.io import wavfile
    import zs_amd  # noqa: F401
    from zs_amd import preprocess as P
    rng = np.random.RandomState(2)
    i16 = rng.randint(-32768, 32768, 1000).astype(np.int16)
    u8 = rng.randint(0, 256, 1000).astype(np.uint8)
    f32 = rng.uniform(-1, 1, 1000).astype(np.float32)
    st = rng.randint(-32768, 32768, (1000, 2)).astype(np.int16)
    f64 = rng.uniform(-1, 1, 1000)
    cases = {'i16': (i16, i16.astype(np.float32) / 32768.0), 'u8': (u8, (u8.astype(np.float32) - 128.0) / 128.0), 'f32': (f32, f32),
             'st': (st, (st.astype(np.float64) / 32768.0).mean(axis=1).astype(np.float32)), 'f64': (f64, f64.astype(np.float32))}
    for sr in (44100, 8000, 16000):
        for name, (data, want) in cases.items():
            path = str(tmp_path / ('%s_%d.wav' % (name, sr)))
            wavfile.write(path, sr, data)
            got, got_sr = P.read_wav(path)
            assert got_sr == sr and isinstance(got_sr, int) and got.dtype == np.float32 and got.ndim == 1
            assert np.array_equal(got, want), name
            if sr == 16000:                                             # a file at hp.sr: as read, no GPU
                assert np.array_equal(P.load_wav(path), got)


def test_cli_out_sr(monkeypatch):
    import importlib.util
    spec = importlib.util.spec_from_file_location('zs_main_for_out_sr', os.path.join(ROOT, 'main.py'))
    main = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(main)
    import zs_amd  # noqa: F401
    from zs_amd import convert as cv
    from zs_amd.hps import hp
    saved = hp.out_sr
    try:
        assert hp.out_sr is None and cv.out_rate() == 16000
        main.argument_runner(['--test', '--hps_path', HPS])
        assert hp.out_sr is None                                        # a flag that is not given leaves hp as it is
        args, _ = main.argument_runner(['--test', '--out_sr', '44100', '--hps_path', HPS])
        assert args.out_sr == 44100 and hp.out_sr == 44100 and cv.out_rate() == 44100
        for bad in ('0', 'abc', '100', '-16000', '512001', '2.5'):
            with pytest.raises(SystemExit):
                main.build_parser().parse_args(['--out_sr', bad])
        assert main.build_parser().parse_args(['--out_sr', '500']).out_sr == 500
        # None and hp.sr: the helper hands back the very objects, without a device
        wavs = [np.zeros(10, np.float32)]
        hp.out_sr = None
        assert cv.to_out_sr(wavs) is wavs
        hp.out_sr = 16000
        assert cv.to_out_sr(wavs) is wavs and cv.out_rate() == 16000
    finally:
        hp.out_sr = saved
