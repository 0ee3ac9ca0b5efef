"""zs_resample (band-limited sample-rate conversion, zs_amd.resample) on the GPU against the direct fp64 sum of its definition
(tests/resample_ref.py), element by element, and the paths that use it: load_wav / get_spectrograms at any file rate, mixed-rate
batches, preprocess() and the --out_sr helper.  PARITY UNPINNED with resampy / librosa.load (see zs_amd/resample.py).

The per-element bound is resample_ref.bound: (n_tap + 4) * 2^-24 * A[t] + 1e-12, A[t] = s * sum_m |x[m] h(...)| -- the rounding of
an fp32 sum of n_tap rounded products in any order.  It is derived, not fitted."""
import ctypes
import math
import os
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resample_ref as RR  # noqa: E402

# (12345 -> 16000 has 3200 phases and 16000 -> 500 a 147 KB tile span at four outputs per thread: the kernel's one-output path)
PAIRS = [(48000, 16000), (44100, 16000), (22050, 16000), (12345, 16000), (8000, 16000), (16000, 44100), (96000, 16000), (16000, 500)]
ROWS = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097]
SENTINEL = -777.0


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


def _tile(sr_in, sr_out):
    """Outputs per workgroup of resample_kernel (the rule of zs_resample in csrc/zs_resample.hip, restated): NT threads, the first
    multiple of n_phase from 256 on, times 4 outputs each while n_phase <= 512 and the input span fits 64 KB; else 256 x 1."""
    n_phase = sr_out // math.gcd(sr_in, sr_out)
    H = -((-64 * sr_in) // sr_out) if sr_in > sr_out else 64
    if n_phase <= 512:
        nt = n_phase * -(-256 // n_phase)
        if -((-(nt * 4 - 1) * sr_in) // sr_out) + 2 * H + 2 <= 16 * 1024:
            return nt * 4
    return 256


def _rows(sr_in, sr_out):
    """The ten ragged rows plus the input lengths whose outputs end one short of, on and one past the kernel's tile."""
    tile = _tile(sr_in, sr_out)
    return ROWS + [max(1, k * sr_in // sr_out) for k in (tile - 1, tile, tile + 1)]


_CASE = {}


def _case(sr_in, sr_out):
    """Inputs and fp64 references of one rate pair, computed once and shared (never modified)."""
    key = (sr_in, sr_out)
    if key not in _CASE:
        rng = np.random.RandomState(sr_in % 1009 + sr_out % 17)
        xs = [rng.uniform(-1, 1, n).astype(np.float32) for n in _rows(sr_in, sr_out)]
        refs = [RR.resample_ref(x, sr_in, sr_out) for x in xs]
        _CASE[key] = (xs, refs)
    return _CASE[key]


def _launch(dev, xs, sr_in, sr_out, dst_ld=None, src_slack=3):
    """One zs_resample launch over the rows xs: NaN in the slack of every source row, a sentinel in dst.  Returns dst (host)."""
    from zs_amd import resample as R
    lens = np.array([len(x) for x in xs], dtype=np.int32)
    src_ld = int(lens.max()) + src_slack
    host = np.full((len(xs), src_ld), np.nan, dtype=np.float32)
    for i, x in enumerate(xs):
        host[i, :len(x)] = x
    n_out = [RR.n_out(n, sr_in, sr_out) for n in lens]
    dst_ld = dst_ld or max(n_out) + 5
    src = torch.from_numpy(host).to(dev)
    n_in = torch.from_numpy(lens).to(dev)
    from zs_amd import _lib as L
    pl = R.plan(sr_in, sr_out)
    bank = R.device_bank(sr_in, sr_out, dev)
    dst = torch.full((len(xs), dst_ld), SENTINEL, dtype=torch.float32, device=dev)
    L.call('zs_resample', 'ZsResample', torch.cuda.current_stream(dev).cuda_stream, src=L.ptr(src), src_ld=src_ld, n_in=L.ptr(n_in),
           n_utt=len(xs), sr_in=sr_in, sr_out=sr_out, bank=L.ptr(bank), n_phase=pl.n_phase, n_tap=pl.n_tap, dst=L.ptr(dst), dst_ld=dst_ld,
           n_in_max=int(lens.max()))
    return dst.cpu().numpy(), n_out


def _check_rows(got_rows, refs, n_tap, what):
    worst = 0.0
    for u, (g, (ref, A)) in enumerate(zip(got_rows, refs)):
        assert len(g) == len(ref), (what, u, len(g), len(ref))
        err, lim = np.abs(g.astype(np.float64) - ref), RR.bound(n_tap, A)
        worst = max(worst, float((err / lim).max()))
        assert (err <= lim).all(), (what, u, float((err / lim).max()))
    print('%s: largest error / bound %.4f' % (what, worst))
    return worst


@pytest.mark.parametrize('sr_in,sr_out', PAIRS)
def test_kernel_vs_fp64_per_element(dev, sr_in, sr_out):
    from zs_amd import resample as R
    xs, refs = _case(sr_in, sr_out)
    pl = R.plan(sr_in, sr_out)
    got, n_out = _launch(dev, xs, sr_in, sr_out)
    assert max(n_out) > _tile(sr_in, sr_out)                           # more than one workgroup per row
    assert not np.isnan(got).any()
    for u, n in enumerate(n_out):
        assert (got[u, n:] == 0).all() and got.shape[1] > n           # the rest of every row is written as zeros
    _check_rows([got[u, :n] for u, n in enumerate(n_out)], refs, pl.n_tap, '%d -> %d' % (sr_in, sr_out))
    # the same launch again: bitwise equal
    again, _ = _launch(dev, xs, sr_in, sr_out)
    assert np.array_equal(got, again)
    # a row's result does not depend on its neighbours: each row alone (n_utt = 1) equals its row of the batch
    for u in range(len(xs)):
        one, _ = _launch(dev, [xs[u]], sr_in, sr_out, dst_ld=got.shape[1])
        assert np.array_equal(one[0], got[u]), u


def test_argument_errors_launch_nothing(dev):
    from zs_amd import _lib as L, resample as R
    sr_in, sr_out = 44100, 16000
    pl = R.plan(sr_in, sr_out)
    bank = R.device_bank(sr_in, sr_out, dev)
    src = torch.zeros(2, 1000, dtype=torch.float32, device=dev)
    n_in = torch.tensor([1000, 500], dtype=torch.int32, device=dev)
    dst = torch.full((2, 400), SENTINEL, dtype=torch.float32, device=dev)
    fn = L.lib().zs_resample
    st = torch.cuda.current_stream(dev).cuda_stream
    good = dict(src=L.ptr(src), src_ld=1000, n_in=L.ptr(n_in), n_utt=2, sr_in=sr_in, sr_out=sr_out, bank=L.ptr(bank), n_phase=pl.n_phase,
                n_tap=pl.n_tap, dst=L.ptr(dst), dst_ld=400, n_in_max=1000)

    def rc(**kw):
        d = dict(good)
        d.update(kw)
        s = L.STRUCTS['ZsResample'](**{k: v for k, v in d.items() if v is not None})
        return fn(ctypes.addressof(s), st)

    bad = [dict(src=None), dict(n_in=None), dict(bank=None), dict(dst=None), dict(sr_in=0), dict(sr_out=-16000), dict(sr_in=16000 * 32 + 1),
           dict(sr_in=499), dict(n_tap=pl.n_tap + 2), dict(n_tap=129), dict(n_phase=pl.n_phase + 1), dict(n_phase=1), dict(dst_ld=362),
           dict(src_ld=999), dict(n_utt=-1), dict(n_utt=65536)]
    for kw in bad:
        assert rc(**kw) == L.ENUMS['ZS_EINVAL'], kw
        assert L.last_error().startswith('zs_resample'), kw
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == SENTINEL).all()                         # nothing was launched
    assert rc(n_utt=0) == 0 and rc(n_utt=0, src=None, dst=None, n_in=None, bank=None) == 0
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == SENTINEL).all()
    assert rc(dst_ld=363) == 0                                           # ceil(1000 * 16000 / 44100) = 363: exactly enough
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out.reshape(-1)[:363] == 0).all() and (out.reshape(-1)[2 * 363:] == SENTINEL).all()


def test_resample_batch(dev, monkeypatch):
    from zs_amd import _lib as L, resample as R
    sr_in = 44100
    xs, refs = _case(sr_in, 16000)
    order = [9, 0, 5, 12, 3]
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda fname, *a, **kw: (calls.append(fname), real(fname, *a, **kw))[1])
    out = R.resample_batch([xs[i] for i in order], sr_in)                # sr_out defaults to hp.sr
    assert calls == ['zs_resample']                                      # one launch for the batch
    assert [o.dtype for o in out] == [np.float32] * len(order)
    _check_rows(out, [refs[i] for i in order], R.plan(sr_in, 16000).n_tap, 'resample_batch 44100 -> 16000')
    dst, lens = R.resample_batch([xs[i] for i in order], sr_in, 16000, device=dev, to_host=False)
    assert dst.device.type == 'cuda' and dst.shape == (len(order), max(lens)) and list(lens) == [len(o) for o in out]
    dst = dst.cpu().numpy()
    for k, o in enumerate(out):
        assert np.array_equal(dst[k, :lens[k]], o) and (dst[k, lens[k]:] == 0).all()
    del calls[:]
    same = R.resample_batch([xs[3], xs[4].astype(np.float64)], 16000, 16000)
    assert calls == [] and np.array_equal(same[0], xs[3]) and np.array_equal(same[1], xs[4]) and same[1].dtype == np.float32
    assert R.resample_batch([], sr_in) == [] and calls == []


# ---- sound files at other rates -------------------------------------------------------------------------------------

FILES = [(44100, 35280, 4000), (8000, 9000, 0), (48000, 40000, 5000)]    # (rate, samples, silenced samples at either end)


@pytest.fixture(scope='module')
def wav_files(tmp_path_factory):
    from scipy.io import wavfile
    d = tmp_path_factory.mktemp('resample_wavs')
    rng = np.random.RandomState(11)
    paths = []
    for sr, n, sil in FILES:
        path = str(d / ('tone_%d.wav' % sr))
        wavfile.write(path, sr, (RR.tone_wav(rng, n, sr, sil) * 32767).astype(np.int16))
        paths.append((path, sr))
    return paths


def test_load_wav_and_spectrograms_of_files(dev, wav_files):
    import zs_oracle as O
    from zs_amd import preprocess as P, resample as R
    for path, sr in wav_files:
        data, got_sr = P.read_wav(path)
        assert got_sr == sr
        y = P.load_wav(path)
        assert y.dtype == np.float32
        _check_rows([y], [RR.resample_ref(data, sr, 16000)], R.plan(sr, 16000).n_tap, 'load_wav %d' % sr)
        mel, mag = P.get_spectrograms(path)
        mel2, mag2 = P.get_spectrograms_batch([y])[0]
        assert np.array_equal(mel, mel2) and np.array_equal(mag, mag2)
        omel, omag = O.get_spectrograms(y)                               # the same audio through the oracle: never two resamplers
        assert mag.shape == omag.shape and mel.shape == omel.shape
        e = (np.abs(mag - omag).max(), np.abs(mel - omel).max(), np.abs(mag - omag).mean())
        print('%d Hz file: mag max %.3g, mel max %.3g, mag mean %.3g' % ((sr,) + e))
        assert e[0] < 2e-3 and e[1] < 2e-3 and e[2] < 5e-5


def test_mixed_rate_batch(dev, monkeypatch):
    from zs_amd import _lib as L, preprocess as P
    rng = np.random.RandomState(12)
    w16, w44, w8, w16b = (RR.tone_wav(rng, 16000, 16000), RR.tone_wav(rng, 30000, 44100, 3000), RR.tone_wav(rng, 7000, 8000),
                          RR.tone_wav(rng, 9999, 16000, 1000))
    w44b = RR.tone_wav(rng, 20000, 44100)
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda fname, *a, **kw: (calls.append(fname), real(fname, *a, **kw))[1])
    wavs, rates = [w16, w44, w8, w16b, w44b], [16000, 44100, 8000, 16000, 44100]
    got = P.get_spectrograms_batch(wavs, sr=rates)
    assert calls.count('zs_resample') == 2 and calls.count('zs_pre_spectrogram') == 1     # one resampling launch per distinct rate
    for w, r, (mel, mag) in zip(wavs, rates, got):
        mel1, mag1 = P.get_spectrograms_batch([w], sr=r)[0]
        assert np.array_equal(mel, mel1) and np.array_equal(mag, mag1)
    del calls[:]
    today = P.get_spectrograms_batch([w16, w16b])
    for (mel, mag), (mel0, mag0) in zip((got[0], got[3]), today):
        assert np.array_equal(mel, mel0) and np.array_equal(mag, mag0)
    same = P.get_spectrograms_batch([w16, w16b], sr=16000)
    assert all(np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0]) for a, b in zip(same, today))
    assert 'zs_resample' not in calls
    magd, frames = P.get_spectrograms_device(wavs, sr=rates)
    for i, (_, mag) in enumerate(got):
        assert frames[i] == len(mag) and np.array_equal(magd[i, :frames[i]].cpu().numpy(), mag)
    with pytest.raises(ValueError):
        P.get_spectrograms_batch(wavs, sr=[16000, 44100])


def test_preprocess_end_to_end_at_other_rates(dev, tmp_path):
    """2 source speakers x 2 utterances at 44.1 kHz, the target speakers at 16 kHz, a test file at 8 kHz -> container -> batch."""
    from scipy.io import wavfile
    from zs_amd import dataloader as D, preprocess as P
    from zs_amd.convert import trim
    rng = np.random.RandomState(5)
    dirs = {k: tmp_path / k for k in ('source', 'target', 'test')}
    for d in dirs.values():
        d.mkdir()
    files = {}

    def put(kind, name, sr, n, pad):
        path = str(dirs[kind] / (name + '.wav'))
        wavfile.write(path, sr, (RR.tone_wav(rng, n, sr) * 32767).astype(np.int16))
        spk, utt = name.split('_')
        files['%s/%s/%s' % ('test' if kind == 'test' else 'train', spk, utt)] = (path, pad)

    for spk in ('S015', 'S020'):
        for utt in ('0001', '0002'):
            put('source', '%s_%s' % (spk, utt), 44100, 44100 + int(rng.randint(0, 22050)), True)
    for utt in ('0001', '0002'):
        put('target', 'V001_%s' % utt, 16000, 20000, True)
        put('target', 'V002_%s' % utt, 16000, 3000, True)                # short: padded
    put('test', 'S015_0099', 8000, 6000, False)
    ds_path = str(tmp_path / 'dataset_english.npz')
    paths = [str(tmp_path / n) for n in ('index.json', 'index_source.json', 'index_target.json', 'speaker2id.json')]
    P.preprocess(str(dirs['source']), str(dirs['target']), str(dirs['test']), ds_path, paths[0], paths[1], paths[2], paths[3],
                 seg_len=64, n_samples=16, dset='train', remake=True)
    store = D.NpzStore(ds_path, 'r')
    for key, (path, pad) in files.items():
        T = 1 + len(trim(P.load_wav(path))[0]) // 200
        if pad and T <= 64:
            T = 65                                                        # preprocess.py:95-100
        assert store[key + '/lin'].shape == (T, 513) and store[key + '/mel'].shape == (T, 80), key
    assert store['train/V002/0001/lin'].shape[0] == 65 and store['train/S015/0001/lin'].shape[0] > 64
    c, x = next(D.DataLoader(D.Dataset(ds_path, paths[0], dset='train', seg_len=64), 4))
    assert tuple(x.shape) == (4, 64, 513) and float(x.max()) <= 1.0


def test_to_out_sr(dev, tmp_path):
    from zs_amd import convert as cv, resample as R
    from zs_amd.hps import hp
    rng = np.random.RandomState(13)
    wavs = [rng.uniform(-0.5, 0.5, n).astype(np.float32) for n in (5000, 1234)]
    saved = hp.out_sr
    try:
        hp.out_sr = None
        assert cv.to_out_sr(wavs) is wavs and cv.out_rate() == 16000
        hp.out_sr = 16000
        assert cv.to_out_sr(wavs) is wavs
        hp.out_sr = 22050
        out = cv.to_out_sr(wavs)
        assert [len(o) for o in out] == [int(math.ceil(n * 22050 / 16000)) for n in (5000, 1234)]
        _check_rows(out, [RR.resample_ref(w, 16000, 22050) for w in wavs], R.plan(16000, 22050).n_tap, 'to_out_sr 22050')
        path = str(tmp_path / 'out.wav')
        cv.write_wav(path, out[0], cv.out_rate())
        with wave.open(path) as f:
            assert (f.getframerate(), f.getnframes(), f.getsampwidth(), f.getnchannels()) == (22050, len(out[0]), 2, 1)
    finally:
        hp.out_sr = saved
