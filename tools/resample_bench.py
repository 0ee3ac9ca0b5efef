"""Cost of resampling in feature extraction: 64 synthetic utterances of 2-7 s, as tools/preprocess_bench.py
uses, generated at 48 kHz and at 44.1 kHz.  In one process, in alternating rounds:
  * the zs_resample launch alone and the zs_pre_spectrogram launch over the same batch at 16 kHz (HIP events around each launch, on
    buffers that are already on the device);
  * get_spectrograms_batch(wavs, sr=rate) against get_spectrograms_batch of the same audio already at 16 kHz (host clock around
    calls that end in a device-to-host copy): the difference is the whole cost of resampling, the host round trip included.
Medians of the rounds.  Also the largest error of the launch over the per-element bound of tests/resample_ref.py on a sample of rows.
  python tools/resample_bench.py [--utts 64] [--rounds 15] [--json profiles/resample_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import zs_amd  # noqa: E402,F401
from zs_amd import _lib as L, preprocess as P, resample as R  # noqa: E402
from zs_amd.hps import hp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--utts', type=int, default=64)
ap.add_argument('--rounds', type=int, default=15)
ap.add_argument('--check-rows', type=int, default=2, help='rows compared with the fp64 direct sum per rate')
ap.add_argument('--json', default=None)
a = ap.parse_args()

dev = torch.device('cuda:0')
rng = np.random.RandomState(0)
secs = rng.uniform(2.0, 7.0, size=a.utts)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def med(v):
    return float(np.median(v))


result = {'utterances': a.utts, 'rounds': a.rounds, 'seconds_of_audio': float(secs.sum()), 'rates': {}}
for rate in (48000, 44100):
    wavs = [(0.1 * rng.randn(int(s * rate))).astype(np.float32) for s in secs]
    wavs16 = R.resample_batch(wavs, rate, hp.sr)                       # the same audio at 16 kHz (also the warm-up of the launch)
    pl = R.plan(rate, hp.sr)
    # device-resident operands of the two launches
    lens = np.array([len(w) for w in wavs], dtype=np.int32)
    host = np.zeros((a.utts, int(lens.max())), dtype=np.float32)
    for i, w in enumerate(wavs):
        host[i, :len(w)] = w
    src, n_in = torch.from_numpy(host).to(dev), torch.from_numpy(lens).to(dev)
    dst_ld = max(len(w) for w in wavs16)
    lens16 = np.array([len(w) for w in wavs16], dtype=np.int32)
    host16 = np.zeros((a.utts, dst_ld), dtype=np.float32)
    for i, w in enumerate(wavs16):
        host16[i, :len(w)] = w
    wav16, ns16 = torch.from_numpy(host16).to(dev), torch.from_numpy(lens16).to(dev)
    T_max = 1 + dst_ld // hp.hop_length
    mag = torch.zeros(a.utts, T_max, 513, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def launch_resample():
        return R.resample_device(src, n_in, rate, hp.sr, dst_ld, n_in_max=int(lens.max()))

    def launch_spec():
        L.call('zs_pre_spectrogram', 'ZsPreSpec', st, wav=L.ptr(wav16), wav_ld=dst_ld, n_samples=L.ptr(ns16), n_utt=a.utts, T_max=T_max,
               preemph=hp.preemphasis, ref_db=float(hp.ref_db), max_db=float(hp.max_db), mag=L.ptr(mag), mag_ld=513, amp=None)

    def feats_sr():
        return P.get_spectrograms_batch(wavs, sr=rate)

    def feats_16():
        return P.get_spectrograms_batch(wavs16)

    for fn in (launch_resample, launch_spec, feats_sr, feats_16):      # warm every shape the timed rounds use
        fn()
    torch.cuda.synchronize()
    t = {'resample_launch_ms': [], 'pre_spectrogram_launch_ms': [], 'features_with_sr_ms': [], 'features_at_16k_ms': []}
    for _ in range(a.rounds):                                          # alternating rounds: both sides see the same machine state
        t['resample_launch_ms'].append(event_ms(launch_resample))
        t['pre_spectrogram_launch_ms'].append(event_ms(launch_spec))
        t['features_with_sr_ms'].append(host_ms(feats_sr))
        t['features_at_16k_ms'].append(host_ms(feats_16))
    r = {k: med(v) for k, v in t.items()}
    r.update({k.replace('_ms', '_min_max_ms'): [float(min(v)), float(max(v))] for k, v in t.items()})
    r['resampling_cost_ms'] = med(np.array(t['features_with_sr_ms']) - np.array(t['features_at_16k_ms']))
    out_samples = int(lens16.sum())
    r.update(bank=[pl.n_phase, pl.n_tap], input_samples=int(lens.sum()), output_samples=out_samples,
             launch_gmacs_per_s=out_samples * pl.n_tap / (r['resample_launch_ms'] * 1e-3) / 1e9)
    if a.check_rows:
        import resample_ref as RR
        worst = 0.0
        for i in np.argsort(lens)[:a.check_rows]:                      # the shortest rows: the fp64 direct sum is host work
            ref, A = RR.resample_ref(wavs[i], rate, hp.sr)
            worst = max(worst, float((np.abs(wavs16[i].astype(np.float64) - ref) / RR.bound(pl.n_tap, A)).max()))
        r['largest_error_over_bound'] = worst
    result['rates'][str(rate)] = r
    print('%d -> %d Hz (%d x %d bank): zs_resample %.3f ms, zs_pre_spectrogram %.3f ms; get_spectrograms_batch %.1f ms with sr, %.1f ms at '
          '16 kHz: resampling costs %.1f ms; error / bound %s' % (rate, hp.sr, pl.n_phase, pl.n_tap, r['resample_launch_ms'],
                                                               r['pre_spectrogram_launch_ms'], r['features_with_sr_ms'],
                                                               r['features_at_16k_ms'], r['resampling_cost_ms'],
                                                               r.get('largest_error_over_bound')))
print(json.dumps(result))
if a.json:
    with open(a.json, 'w') as f:
        json.dump(result, f, indent=1)
