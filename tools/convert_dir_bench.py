"""What the device trim saves in waveform-to-waveform conversion: two paths over the same inputs, in one process,
alternated repetition by repetition,
  (a) convert_wavs                                   resampled audio stays in HBM, zs_trim, zs_pre_spectrogram in place, resynth_batch
  (b) get_spectrograms_batch, then resynth_batch     host trim; audio (when resampled) and spectrograms come back to the host
on 64 synthetic utterances of 2-7 s with silence at both ends, once at 16 kHz and once at 44.1 kHz, full-size english model
(random weights, bf16), Griffin-Lim n_iter = 300, enc_only.  Host clock around each call (both end in a wait for their last
copy); medians, minima and maxima over the repetitions.  The zs_trim launches alone are timed with HIP events on the 16 kHz batch.
    python tools/convert_dir_bench.py [--utts 64] [--reps 7] [--warmup 2] [--n-iter 300] [--out profiles/convert_dir_bench.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zs_amd  # noqa: E402,F401
from zs_amd import convert as cv, preprocess as P  # noqa: E402
from zs_amd.hps import make_hps  # noqa: E402
from zs_amd.trainer import Trainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--dtype', default='bf16'); ap.add_argument('--utts', type=int, default=64); ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--warmup', type=int, default=2); ap.add_argument('--n-iter', type=int, default=300)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'convert_dir_bench.json'))
a = ap.parse_args()
if a.reps < 7 or a.warmup < 2:
    ap.error('at least 7 repetitions after 2 warm-ups')
if not torch.cuda.is_available():
    sys.exit('convert_dir_bench needs an MI355X: a timing taken anywhere else says nothing about it')
dev = torch.device('cuda:0')


def synth(rate, rng):
    """2-7 s of a drifting harmonic tone with noise, 0.2-0.5 s of digital silence at either end."""
    n = int(rng.uniform(2.0, 7.0) * rate)
    t = np.arange(n) / float(rate)
    f0 = rng.uniform(90, 250)
    y = sum(0.25 / k * np.sin(2 * np.pi * k * f0 * t * (1 + 0.02 * np.sin(2 * np.pi * 0.7 * t))) for k in (1, 2, 3, 5))
    y = y * (0.6 + 0.4 * np.sin(2 * np.pi * 2.1 * t) ** 2) + 0.01 * rng.randn(n)
    lead, trail = int(rng.uniform(0.2, 0.5) * rate), int(rng.uniform(0.2, 0.5) * rate)
    y[:lead] = 0.0
    y[n - trail:] = 0.0
    return y.astype(np.float32)


hps = make_hps(enc_size=1024, emb_size=1024, n_speakers=102)
torch.manual_seed(0)
tr = Trainer(hps, None, 'naive', 'multilabel_binary', log_dir=tempfile.mkdtemp(), dtype=a.dtype, device=dev)
spk = [100 + (i % 2) for i in range(a.utts)]


def path_a(wavs, rate):
    return cv.convert_wavs(wavs, rate, tr, hps.seg_len, spk, n_iter=a.n_iter)[:2]


def path_b(wavs, rate):
    specs = [m for _, m in P.get_spectrograms_batch(wavs, sr=rate)]
    return cv.resynth_batch(specs, tr, hps.seg_len, spk, n_iter=a.n_iter)


def stats(ms):
    return {'median_ms': round(float(np.median(ms)), 2), 'min_ms': round(min(ms), 2), 'max_ms': round(max(ms), 2),
            'all_ms': [round(x, 2) for x in ms]}


record = {'utts': a.utts, 'n_iter': a.n_iter, 'dtype': a.dtype, 'reps': a.reps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0),
          'paths': {'a': 'convert_wavs', 'b': 'get_spectrograms_batch + resynth_batch'}, 'rates': {}}
for rate in (16000, 44100):
    rng = np.random.RandomState(rate)
    wavs = [synth(rate, rng) for _ in range(a.utts)]
    times = {'a': [], 'b': []}
    shapes = {}
    for rep in range(a.warmup + a.reps):
        for name, fn in ((('a', path_a), ('b', path_b)) if rep % 2 == 0 else (('b', path_b), ('a', path_a))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(wavs, rate)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= a.warmup:
                times[name].append(dt)
            if rep == 0:                                              # both paths cut the same fragments (the noise differs: no noise_fn)
                shapes[name] = [e.shape for e in out[0]]
    sa, sb = stats(times['a']), stats(times['b'])
    diff = sb['median_ms'] - sa['median_ms']
    spread = max(sa['max_ms'] - sa['min_ms'], sb['max_ms'] - sb['min_ms'])
    record['rates'][str(rate)] = {
        'audio_seconds': round(sum(len(w) for w in wavs) / float(rate), 1), 'a': sa, 'b': sb,
        'b_minus_a_median_ms': round(diff, 2), 'largest_spread_ms': round(spread, 2),
        'a_faster_beyond_spread': bool(diff > spread), 'ranges_overlap': bool(sa['max_ms'] >= sb['min_ms'] and sb['max_ms'] >= sa['min_ms']),
        'utts_per_s': {'a': round(a.utts / sa['median_ms'] * 1e3, 1), 'b': round(a.utts / sb['median_ms'] * 1e3, 1)},
        'same_unit_shapes': shapes['a'] == shapes['b']}
    print('%d Hz: (a) convert_wavs %.1f ms [%.1f, %.1f]   (b) features + resynth %.1f ms [%.1f, %.1f]   b - a = %.1f ms' %
          (rate, sa['median_ms'], sa['min_ms'], sa['max_ms'], sb['median_ms'], sb['min_ms'], sb['max_ms'], diff))

# zs_trim alone: HIP events around the call (two launches) on the 16 kHz batch, resident on the device
rng = np.random.RandomState(16000)
wavs = [synth(16000, rng) for _ in range(a.utts)]
wav, lens = P._device_audio(wavs, None, dev)
ns = torch.from_numpy(lens).to(dev)
for _ in range(3):
    P.trim_device(wav, ns)
ev = []
for _ in range(20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    P.trim_device(wav, ns)
    e1.record()
    ev.append((e0, e1))
torch.cuda.synchronize()
us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
t0 = time.perf_counter()
for w in wavs:
    cv.trim(w)
host_ms = (time.perf_counter() - t0) * 1e3
nbytes = int(lens.sum()) * 4
record['zs_trim'] = {'rows': a.utts, 'wav_ld': int(wav.shape[1]), 'samples': int(lens.sum()), 'median_us': round(us[len(us) // 2], 1),
                     'min_us': round(us[0], 1), 'max_us': round(us[-1], 1),
                     'note': 'events around one trim_device call: workspace allocation from the caching allocator, two launches',
                     'GBps_at_median': round(nbytes / (us[len(us) // 2] * 1e-6) / 1e9, 1), 'host_trim_same_batch_ms': round(host_ms, 2)}
print('zs_trim on %d rows, %d samples: %.1f us median [%.1f, %.1f]; host trim of the same batch %.1f ms' %
      (a.utts, int(lens.sum()), us[len(us) // 2], us[0], us[-1], host_ms))
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, 'w') as f:
    json.dump(record, f, indent=1)
print(json.dumps({k: record['rates'][k]['b_minus_a_median_ms'] for k in record['rates']}))
