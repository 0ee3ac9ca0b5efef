"""A folder of sound files converted end to end on the device (--convert_dir):

* zs_trim against convert.trim(), the definition, bound for bound, on lengths around every rule of the reflection and the frames;
* zs_pre_spectrogram reading a window in place (ZsPreSpec.start) against the same launch on host-sliced copies, bit for bit;
* get_spectrograms_device(trim_on='device') against trim_on='host';
* convert_wavs against get_spectrograms_batch + resynth_batch, bit for bit, with and without the generator, deferred too;
* convert_dir / main.py --convert_dir on a temporary folder."""
import json
import os
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trim_ref  # noqa: E402

SEG = 32                                                          # a small seg_len keeps the audio of the fragment cases short
TRIM_LENS = [1, 2, 3, 700, 1024, 1025, 1537, 2047, 2048, 2049, 5000, 9000, 16037, 40001]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


# ---- signals -----------------------------------------------------------------------------------------------------------------------
def _body(rng, n):
    """Tone plus noise between leading and trailing digital silence, 4000 and 5000 samples of it at n = 16037."""
    t = np.arange(n) / 16000.0
    y = 0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.02 * rng.randn(n)
    lead, trail = n * 4000 // 16037, n * 5000 // 16037
    y[:lead] = 0.0
    y[n - trail:] = 0.0
    return y


def _floor(rng, n, db):
    """White noise `db` below the body's level (0.3 / sqrt(2) RMS)."""
    return (0.3 / np.sqrt(2.0)) * 10.0 ** (db / 20.0) * rng.randn(n)


def trim_cases():
    """[(name, float32 signal)]: every content at every length of TRIM_LENS, and the burst."""
    out = []
    for n in TRIM_LENS:
        rng = np.random.RandomState(n)
        body = _body(rng, n)
        out += [('noise/%d' % n, 0.1 * rng.randn(n)), ('silence/%d' % n, body), ('floor-45/%d' % n, body + _floor(rng, n, -45.0)),
                ('floor-75/%d' % n, body + _floor(rng, n, -75.0)), ('floor-90/%d' % n, body + _floor(rng, n, -90.0)),
                ('zero/%d' % n, np.zeros(n)), ('quiet/%d' % n, np.full(n, 1e-6))]
    burst = np.zeros(8000)
    burst[4046:4146] = 0.5 * np.random.RandomState(5).randn(100)
    out.append(('burst/8000', burst))
    return [(name, y.astype(np.float32)) for name, y in out]


KNOWN_BOUNDS = {'floor-45/16037': (0, 16037), 'floor-75/16037': (3072, 12288), 'burst/8000': (3072, 5632)}


def _padded_nan(rows, ld):
    host = np.full((len(rows), ld), np.nan, dtype=np.float32)
    for i, y in enumerate(rows):
        host[i, :len(y)] = y
    return host


def _voiced(rng, n, lead, trail, f0=300.0, sr=16000):
    t = np.arange(n) / float(sr)
    y = 0.3 * np.sin(2 * np.pi * f0 * t) + 0.1 * np.sin(2 * np.pi * 2.7 * f0 * t) + 0.01 * rng.randn(n)
    y[:lead] = 0.0
    if trail:
        y[n - trail:] = 0.0
    return y.astype(np.float32)


# ---- zs_trim -------------------------------------------------------------------------------------------------------------------------
def test_trim_equals_convert_trim(dev):
    """One batch of every case, the slack of each row filled with NaN (wav_ld is odd and longer than every row, so the 16-byte
    loads and the scalar ones both run): the bounds are convert.trim()'s exactly, twice in a row.
    The exact comparison rests on a condition checked here on the host: every frame of every case is at least 0.01 dB from the
    -60 dB threshold, so the last bits in which the device's sums differ from the host's cumulative sums cannot move a bound."""
    from zs_amd import convert as cv, preprocess as P
    cases = trim_cases()
    for name, y in cases:
        assert trim_ref.margin_db(y) >= 0.01, (name, trim_ref.margin_db(y))
    want = np.array([cv.trim(y)[1] for _, y in cases], dtype=np.int32)
    for i, (name, y) in enumerate(cases):
        kind = name.split('/')[0]
        if kind in ('zero', 'quiet'):
            assert tuple(want[i]) == (0, len(y)), name
        if name in KNOWN_BOUNDS:
            assert tuple(want[i]) == KNOWN_BOUNDS[name], name
        assert tuple(want[i]) == trim_ref.trim_bounds(y), name
    ld = 40101
    wav = torch.from_numpy(_padded_nan([y for _, y in cases], ld)).to(dev)
    ns = torch.tensor([len(y) for _, y in cases], dtype=torch.int32, device=dev)
    got = P.trim_device(wav, ns)
    again = P.trim_device(wav, ns)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(cases), 2)
    g = got.cpu().numpy()
    bad = [(cases[i][0], tuple(g[i]), tuple(want[i])) for i in range(len(cases)) if tuple(g[i]) != tuple(want[i])]
    assert not bad, bad[:8]
    assert torch.equal(got, again)
    # a row's bounds do not depend on the rows around it, nor on the row pitch (another alignment of every row)
    pick = [i for i, (name, _) in enumerate(cases) if name.endswith('/16037') or name.endswith('/2049')][::-1]
    wav2 = torch.from_numpy(_padded_nan([cases[i][1] for i in pick], 16040)).to(dev)
    got2 = P.trim_device(wav2, ns[torch.tensor(pick, device=dev)].contiguous())
    assert np.array_equal(got2.cpu().numpy(), want[pick])


def test_trim_empty_rows_and_lengths_past_the_pitch(dev):
    """n <= 0 gives (0, 0) and reads nothing (the row is NaN); n_samples above wav_ld is clamped to the row."""
    from zs_amd import convert as cv, preprocess as P
    rng = np.random.RandomState(3)
    y = (0.1 * rng.randn(3000)).astype(np.float32)
    host = np.full((4, 3000), np.nan, dtype=np.float32)
    host[1] = y
    host[3] = y
    ns = torch.tensor([0, 3000, -5, 99999], dtype=torch.int32, device=dev)
    got = P.trim_device(torch.from_numpy(host).to(dev), ns).cpu().numpy()
    b = cv.trim(y)[1]
    assert [tuple(r) for r in got] == [(0, 0), b, (0, 0), b]


def test_trim_argument_errors_launch_nothing(dev):
    from zs_amd import _lib as L
    wav = torch.zeros(2, 4096, device=dev)
    ns = torch.tensor([4096, 100], dtype=torch.int32, device=dev)
    bounds = torch.full((2, 2), -7, dtype=torch.int32, device=dev)
    nbytes = L.lib().zs_trim_workspace_bytes(2, 4096, 2048, 512)
    assert nbytes == 2 * (4096 // 512 + 4) * 8
    assert L.lib().zs_trim_workspace_bytes(2, 4096, 2048, 0) == 0 and L.lib().zs_trim_workspace_bytes(2, 4096, 1000, 512) == 0
    work = torch.zeros(nbytes // 8, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    ok = dict(wav=L.ptr(wav), wav_ld=4096, n_samples=L.ptr(ns), n_utt=2, frame_length=2048, hop=512, top_db=60.0, bounds=L.ptr(bounds),
              work=L.ptr(work), work_bytes=nbytes)
    for change in (dict(wav=None), dict(n_samples=None), dict(bounds=None), dict(work=None), dict(hop=0), dict(hop=-512),
                   dict(frame_length=0), dict(frame_length=2048 + 256), dict(frame_length=512, hop=1024), dict(work_bytes=nbytes - 8),
                   dict(wav_ld=0), dict(n_utt=-1), dict(top_db=0.0), dict(top_db=float('nan'))):
        with pytest.raises(L.ZsError, match='zs_trim'):
            L.call('zs_trim', 'ZsTrim', st, **dict(ok, **change))
    torch.cuda.synchronize()
    assert (bounds == -7).all() and (work == 0).all()
    L.call('zs_trim', 'ZsTrim', st, **dict(ok, n_utt=0))              # an empty batch succeeds and launches nothing
    torch.cuda.synchronize()
    assert (bounds == -7).all()
    L.call('zs_trim', 'ZsTrim', st, **ok)
    assert bounds.cpu().tolist() == [[0, 4096], [0, 100]]            # all-zero rows keep every frame


# ---- zs_pre_spectrogram with start -----------------------------------------------------------------------------------------------
def test_pre_spectrogram_reads_a_window_in_place(dev):
    """Windows at start {0, 1, 513, 4096} of lengths around the frame rules inside NaN rows: mag and amp are bit-equal to the same
    launch on host-sliced copies with start = NULL, and no NaN reaches the output."""
    from zs_amd import _lib as L
    from zs_amd.hps import hp
    rng = np.random.RandomState(11)
    combos = [(s, n) for s in (0, 1, 513, 4096) for n in (2, 199, 200, 201, 1023, 4000)]
    ld = 8197
    host = np.full((len(combos), ld), np.nan, dtype=np.float32)
    sliced = np.full((len(combos), 4000), np.nan, dtype=np.float32)
    for i, (s, n) in enumerate(combos):
        y = (0.2 * rng.randn(n)).astype(np.float32)
        host[i, s:s + n] = y
        sliced[i, :n] = y
    start = torch.tensor([s for s, _ in combos], dtype=torch.int32, device=dev)
    ns = torch.tensor([n for _, n in combos], dtype=torch.int32, device=dev)
    T_max = 1 + 4000 // 200
    st = torch.cuda.current_stream().cuda_stream

    def run(wav, start):
        mag = torch.zeros(len(combos), T_max, 513, device=dev)
        amp = torch.zeros(len(combos), T_max, 513, device=dev)
        L.call('zs_pre_spectrogram', 'ZsPreSpec', st, wav=L.ptr(wav), wav_ld=wav.shape[1], n_samples=L.ptr(ns), n_utt=len(combos),
               T_max=T_max, preemph=hp.preemphasis, ref_db=float(hp.ref_db), max_db=float(hp.max_db), mag=L.ptr(mag), mag_ld=513,
               amp=L.ptr(amp), start=L.ptr(start))
        return mag, amp
    mag, amp = run(torch.from_numpy(host).to(dev), start)
    mag0, amp0 = run(torch.from_numpy(sliced).to(dev), None)
    assert torch.isfinite(mag).all() and torch.isfinite(amp).all()
    assert torch.equal(mag, mag0) and torch.equal(amp, amp0)
    for i, (_, n) in enumerate(combos):                               # the frames of each row were written, the rows behind were not
        T = 1 + n // 200
        assert (mag[i, :T] > 0).all() and (mag[i, T:] == 0).all()


# ---- feature extraction --------------------------------------------------------------------------------------------------------------
def _four_wavs():
    rng = np.random.RandomState(21)
    rates = [16000, 22050, 8000, 16000]
    wavs = [_voiced(rng, 21000, 3000, 4000, sr=16000), _voiced(rng, 30000, 6000, 2500, sr=22050), _voiced(rng, 9000, 1500, 2000, sr=8000),
            _voiced(rng, 12345, 2048, 700, sr=16000)]
    return wavs, rates


def test_device_trim_features_equal_host_trim_features(dev):
    from zs_amd import preprocess as P
    wavs, rates = _four_wavs()
    mag_h, frames_h = P.get_spectrograms_device(wavs, device=dev, sr=rates)
    mag_d, frames_d = P.get_spectrograms_device(wavs, device=dev, sr=rates, trim_on='device')
    assert np.array_equal(frames_h, frames_d) and frames_d.dtype == np.int64
    assert len(set(int(f) for f in frames_d)) > 1
    for i, T in enumerate(frames_d):
        assert torch.equal(mag_d[i, :T], mag_h[i, :T]) and (mag_d[i, :T] > 0).all()
        assert (mag_d[i, T:] == 0).all()
    # one rate for all, and no trim: no bounds are fetched, the values are the host path's
    for kw in (dict(sr=None), dict(sr=16000, do_trim=False), dict(sr=8000)):
        sub = [wavs[0], wavs[3]]
        a, fa = P.get_spectrograms_device(sub, device=dev, **kw)
        b, fb = P.get_spectrograms_device(sub, device=dev, trim_on='device', **kw)
        assert np.array_equal(fa, fb) and torch.equal(a, b)
    with pytest.raises(ValueError, match='too short after trimming'):
        P.get_spectrograms_device([wavs[0], np.zeros(1, np.float32)], device=dev, trim_on='device')
    with pytest.raises(ValueError, match='trim_on'):
        P.get_spectrograms_device(wavs, device=dev, trim_on='gpu')


# ---- convert_wavs ------------------------------------------------------------------------------------------------------------------
def _trainer(tmp_path, seed=0):
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    torch.manual_seed(seed)
    hps = make_hps(enc_size=8, emb_size=32, n_speakers=4, n_target_speakers=2, seg_len=SEG)
    return Trainer(hps, None, 'targeted_residual', 'multilabel_binary', log_dir=str(tmp_path / 'log'), dtype='fp32',
                   device=torch.device('cuda:0')), hps


def _field_noise(E, seed=1234, T=64):
    """noise_fn whose every batch position reads the same field: a fragment's noise does not depend on where it is batched."""
    U = torch.rand(T, E, 2, generator=torch.Generator().manual_seed(seed))
    base = (-torch.log(-torch.log(U + 1e-20) + 1e-20)).cuda()

    def noise_fn(n, t, e):
        assert e == E and t <= base.shape[0]
        return base[:t].unsqueeze(0).expand(n, t, E, 2).contiguous()
    return noise_fn


def _fragment_wavs():
    """After trimming: more than 2 SEG frames, between SEG and 2 SEG, fewer than MIN_LEN = 9 frames (an input that short has no
    room for silence: the trim's grain is 512 samples)."""
    rng = np.random.RandomState(31)
    rates = [22050, 16000, 8000]
    wavs = [_voiced(rng, 30000, 4000, 3000, sr=22050), _voiced(rng, 13000, 2000, 2500, sr=16000), _voiced(rng, 700, 0, 0, sr=8000)]
    return wavs, rates


@pytest.mark.parametrize('enc_only', [True, False])
def test_convert_wavs_equals_features_then_resynth(dev, tmp_path, enc_only):
    from zs_amd import convert as cv, preprocess as P
    tr, _ = _trainer(tmp_path, seed=3)
    wavs, rates = _fragment_wavs()
    spk = [2, 3, 2]
    noise_fn = _field_noise(8)
    specs = [m for _, m in P.get_spectrograms_batch(wavs, sr=rates)]
    T = [len(s) for s in specs]
    assert T[0] > 2 * SEG and SEG < T[1] <= 2 * SEG and T[2] < cv.MIN_LEN, T
    e0, w0 = cv.resynth_batch(specs, tr, SEG, spk, n_iter=4, noise_fn=noise_fn, enc_only=enc_only)
    e1, w1, info = cv.convert_wavs(wavs, rates, tr, SEG, spk, enc_only=enc_only, n_iter=4, noise_fn=noise_fn)
    assert [i['frames'] for i in info] == T
    for a, b, w, w2, i in zip(e0, e1, w0, w1, info):
        assert np.array_equal(a, b) and w2.dtype == np.float32 and np.array_equal(w, w2) and len(w2) > 0
        assert i['frames'] == 1 + (i['bounds'][1] - i['bounds'][0]) // 200
    assert info[0]['bounds'][0] > 0 and info[2]['bounds'][0] == 0
    # enqueued twice before the first wait
    fa = cv.convert_wavs(wavs, rates, tr, SEG, spk, enc_only=enc_only, n_iter=4, noise_fn=noise_fn, defer=True)
    fb = cv.convert_wavs(wavs[:2], rates[:2], tr, SEG, spk[:2], enc_only=enc_only, n_iter=4, noise_fn=noise_fn, defer=True)
    ea, wa, ia = fa()
    eb, wb, ib = fb()
    assert ia == info and ib == info[:2]
    assert all(np.array_equal(a, b) for a, b in zip(e1, ea)) and all(np.array_equal(a, b) for a, b in zip(w1, wa))
    assert all(np.array_equal(a, b) for a, b in zip(e1[:2], eb)) and all(np.array_equal(a, b) for a, b in zip(w1[:2], wb))


def test_convert_wavs_refuses_a_too_short_input_before_the_network(dev, tmp_path):
    from zs_amd import convert as cv
    tr, _ = _trainer(tmp_path)
    wavs, rates = _fragment_wavs()
    with pytest.raises(ValueError, match='utterance too short after trimming'):
        cv.convert_wavs(wavs + [np.zeros(1, np.float32)], rates + [16000], tr, SEG, [2, 3, 2, 3], n_iter=4)
    with pytest.raises(RuntimeError, match='can only convert to target speakers'):
        cv.convert_wavs(wavs, rates, tr, SEG, [2, 0, 3], enc_only=False, n_iter=4)


# ---- convert_dir -------------------------------------------------------------------------------------------------------------------
def _folder(tmp_path):
    from scipy.io import wavfile
    rng = np.random.RandomState(41)
    d = tmp_path / 'in'
    d.mkdir()
    wavfile.write(str(d / 'a16.wav'), 16000, (_voiced(rng, 15000, 2000, 1500, sr=16000) * 32767).astype(np.int16))
    wavfile.write(str(d / 'b22.wav'), 22050, _voiced(rng, 12000, 1000, 3000, sr=22050))
    st = _voiced(rng, 30000, 5000, 4000, sr=44100)
    wavfile.write(str(d / 'c44.wav'), 44100, (np.stack([st, 0.5 * st], axis=1) * 32767).astype(np.int16))
    wavfile.write(str(d / 'one.wav'), 16000, np.array([1000], dtype=np.int16))
    (d / 'text.wav').write_bytes(b'not a sound file\n' * 8)
    (d / 'notes.txt').write_text('ignored: not a *.wav')
    s2id = tmp_path / 'speaker2id.json'
    s2id.write_text(json.dumps({'S015': 0, 'S020': 1, 'V001': 2, 'V002': 3}))
    return d, str(s2id)


def _check_outputs(out, manifest, targets, rate):
    good = ['a16', 'b22', 'c44']
    for t in targets:
        assert sorted(os.listdir(os.path.join(out, t))) == sorted([s + '.wav' for s in good] + [s + '.txt' for s in good])
        for s in good:
            with wave.open(os.path.join(out, t, s + '.wav'), 'rb') as f:
                assert (f.getframerate(), f.getsampwidth(), f.getnchannels()) == (rate, 2, 1) and f.getnframes() > 0
            rows = open(os.path.join(out, t, s + '.txt')).read().split('\n')
            assert rows[-1] == '' and len(rows) > 1
            assert all(len(r.split(' ')) == 8 and set(r.split(' ')) <= {'0', '1'} for r in rows[:-1])
    assert sorted(os.listdir(out)) == sorted(list(targets) + ['convert_dir.json'])
    assert json.load(open(os.path.join(out, 'convert_dir.json'))) == manifest
    assert sorted((os.path.basename(i['input']), i['target']) for i in manifest['items']) == sorted((s + '.wav', t) for s in good
                                                                                                    for t in targets)
    for i in manifest['items']:
        assert i['wav'] == os.path.join(out, i['target'], os.path.basename(i['input'])[:-4] + '.wav') and os.path.exists(i['txt'])
    skipped = {os.path.basename(s['input']): s['reason'] for s in manifest['skipped']}
    assert sorted(skipped) == ['one.wav', 'text.wav']
    assert 'too short after trimming' in skipped['one.wav'] and 'cannot be read' in skipped['text.wav']


def test_convert_dir_on_a_folder(dev, tmp_path, monkeypatch, capsys):
    sys.path.insert(0, ROOT)
    import main as M
    from zs_amd import convert as cv, preprocess as P
    from zs_amd.hps import hp
    d, s2id = _folder(tmp_path)
    tr, hps = _trainer(tmp_path, seed=5)
    hps_path = str(tmp_path / 'hps.json')
    json.dump(hps._asdict(), open(hps_path, 'w'))
    tr.save_model(str(tmp_path / 'model.pth'), 's2', 1)
    monkeypatch.setattr(hp, 'n_iter', 4)
    # a target outside the generator's range: refused before any file is written
    with pytest.raises(RuntimeError, match='can only convert to target speakers'):
        cv.convert_dir(tr, SEG, str(d), s2id, str(tmp_path / 'refused'), ['V001', 'S015'], False)
    assert not (tmp_path / 'refused').exists()
    # the command line, with the generator, two targets
    res = tmp_path / 'result'
    M.main(['--convert_dir', str(d), '--t_speaker', 'V001,V002', '--hps_path', hps_path, '--speaker2id_path', s2id,
            '--ckpt_pth', str(tmp_path / 'model.pth-s2-1'), '--result_dir', str(res), '--g_mode', 'targeted_residual'])
    out = os.path.join(os.path.join(str(res), './english/'), 'convert')       # {result_dir}/{sub_result_dir}/convert, as main.py joins them
    manifest = json.load(open(os.path.join(out, 'convert_dir.json')))
    _check_outputs(out, manifest, ['V001', 'V002'], 16000)
    printed = capsys.readouterr().out
    assert 'skipped' in printed and 'one.wav' in printed and 'text.wav' in printed
    # bounds and frames are those of a direct convert_wavs call on the files
    read = {n: P.read_wav(str(d / n)) for n in ('a16.wav', 'b22.wav', 'c44.wav')}
    names = sorted(read)
    _, _, info = cv.convert_wavs([read[n][0] for n in names], [read[n][1] for n in names], tr, SEG, [2, 2, 2], n_iter=4)
    for i in manifest['items']:
        n = os.path.basename(i['input'])
        ref = info[names.index(n)]
        assert tuple(i['bounds']) == tuple(ref['bounds']) and i['frames'] == ref['frames']
        assert i['rate'] == read[n][1] and i['samples'] == len(read[n][0])
    # --out_sr: the wavs at another rate; several groups (batch=2) with one group in flight while the previous one is written
    monkeypatch.setattr(hp, 'out_sr', 22050)
    out2 = str(tmp_path / 'out2')
    m2 = cv.convert_dir(tr, SEG, str(d), s2id, out2, ['V002', 'V001'], True, batch=2, n_iter=4)
    _check_outputs(out2, m2, ['V002', 'V001'], 22050)
    assert {(os.path.basename(i['input']), tuple(i['bounds']), i['frames']) for i in m2['items']} == \
           {(os.path.basename(i['input']), tuple(i['bounds']), i['frames']) for i in manifest['items']}
