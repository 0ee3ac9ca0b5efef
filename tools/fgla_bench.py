"""Fast Griffin-Lim (momentum) against the plain loop on BASELINE config 4's shape: 64 utterances of U{200..700} frames
(RandomState(0), as bench.py --mode resynth), one GPU.
  * vocoder: griffin_lim_batch at (300 it, alpha 0), (300 it, alpha 0.99), (100 it, alpha 0.99), timed with device events, the
    variants alternated round by round; ms per iteration and the momentum / plain per-iteration ratio;
  * end to end: resynth_batch utt/s (full-size english model, bf16 network, spectrograms resident in HBM) at (300, 0) against
    (100, 0.99), alternated;
  * quality: spectral convergence against iterations for the utterances of tests/golden/fgla_speech.npz (SC on the host from the
    GPU waveforms, zs_oracle.stft).
usage: python tools/fgla_bench.py [--out FILE.json] [--rounds R]
       python tools/fgla_bench.py --gl-only R     (just the three vocoder variants R times each: the run to profile)"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)
import zs_amd  # noqa: E402,F401
from zs_amd import _lib as L, convert as cv  # noqa: E402

GL_VARIANTS = [(300, 0.0), (300, 0.99), (100, 0.99)]
E2E_VARIANTS = [(300, 0.0), (100, 0.99)]
SC_ITERS = [25, 50, 75, 100, 150, 200, 300]


def config4():
    rng = np.random.RandomState(0)
    lens = rng.randint(200, 701, size=64)
    specs = [np.clip(rng.rand(int(n), 513).astype(np.float32), 1e-8, 1) for n in lens]
    spk = [int(rng.randint(0, 102)) for _ in specs]
    return lens, specs, spk


def gl_inputs(specs):
    """The vocoder's input for the batch: de-normalised amplitudes [n, T_max, 513] on the device (what resynth hands it)."""
    dev = torch.device('cuda:0')
    n, Tm = len(specs), max(s.shape[0] for s in specs)
    t = torch.zeros(n, Tm, 513, device=dev)
    for i, s in enumerate(specs):
        t[i, :s.shape[0]] = torch.from_numpy(s).to(dev)
    amp = torch.empty_like(t)
    L.check(L.lib().zs_gl_denormalize(L.ptr(t), L.ptr(amp), t.numel(), torch.cuda.current_stream().cuda_stream), 'zs_gl_denormalize')
    return amp, [int(s.shape[0]) for s in specs]


def time_gl(amp, lens, rounds):
    def once(n_iter, alpha):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        cv.griffin_lim_batch(None, n_iter=n_iter, mag_padded=(amp, lens), momentum=alpha)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e)
    for v in GL_VARIANTS:                                     # warm-up: tables, side streams, chain probe, allocator
        once(*v)
        once(*v)
    ms = {v: [] for v in GL_VARIANTS}
    for _ in range(rounds):
        for v in GL_VARIANTS:
            ms[v].append(once(*v))
    return ms


def time_e2e(specs, spk, rounds):
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    dev = torch.device('cuda:0')
    torch.manual_seed(1)
    hps = make_hps(enc_size=1024, emb_size=1024, n_speakers=102)
    tr = Trainer(hps, None, 'targeted_residual', 'multilabel_binary', log_dir=tempfile.mkdtemp(), dtype='bf16', device=dev)
    specs_dev = [torch.from_numpy(s).to(dev) for s in specs]

    def once(n_iter, alpha):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cv.resynth_batch(specs_dev, tr, 128, spk, n_iter=n_iter, do_trim=True, momentum=alpha)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for v in E2E_VARIANTS:
        once(*v)
        once(*v)
    sec = {v: [] for v in E2E_VARIANTS}
    for _ in range(rounds):
        for v in E2E_VARIANTS:
            sec[v].append(once(*v))
    return sec


def quality():
    import fgla_ref as F
    S = F.fixture_amplitudes()
    _, names = F.fixture_waves()
    table = {}
    for alpha in (0.0, 0.99):
        for n_iter in SC_ITERS:
            wav, _, lens = cv.griffin_lim_batch(S, n_iter=n_iter, momentum=alpha)
            w = wav.cpu().numpy()
            table['alpha=%g,n_iter=%d' % (alpha, n_iter)] = [round(F.spectral_convergence(w[i, :200 * (T - 1)], S[i]), 5)
                                                             for i, T in enumerate(lens)]
    return {'utterances': ['%s (%d frames)' % (n, s.shape[1]) for n, s in zip(names, S)], 'sc': table}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--gl-only', type=int, default=0)
    args = ap.parse_args()
    lens, specs, spk = config4()
    amp, ulens = gl_inputs(specs)
    if args.gl_only:
        for v in GL_VARIANTS:
            for _ in range(args.gl_only):
                cv.griffin_lim_batch(None, n_iter=v[0], mag_padded=(amp, ulens), momentum=v[1])
        torch.cuda.synchronize()
        print('chains used: %d' % L.lib().zs_gl_chains_used())
        return
    ms = time_gl(amp, ulens, args.rounds)
    chains = int(L.lib().zs_gl_chains_used())
    gl = {}
    for (n_iter, alpha), v in ms.items():
        med = float(np.median(v))
        gl['n_iter=%d,alpha=%g' % (n_iter, alpha)] = {'ms_median': round(med, 3), 'ms_min': round(float(np.min(v)), 3),
                                                      'ms_max': round(float(np.max(v)), 3), 'ms_per_iteration': round(med / n_iter, 4)}
    plain, mom, fast = (gl['n_iter=%d,alpha=%g' % v]['ms_median'] for v in GL_VARIANTS)
    out = {
        'shape': '64 utterances, RandomState(0) lengths U{200..700} (%d frames), one MI355X' % int(np.sum(lens)),
        'gl_launch_chains': chains,
        'griffin_lim_batch': gl,
        'momentum_over_plain_per_iteration': round(mom / plain, 4),
        'fgla100_over_plain300_wall': round(fast / plain, 4),
        'acceptance_fgla100_over_plain300_le_0.6': bool(fast / plain <= 0.6),
    }
    print(json.dumps(out, indent=1), flush=True)
    sec = time_e2e(specs, spk, max(3, args.rounds // 2))
    out['resynth_batch'] = {'n_iter=%d,alpha=%g' % k: {'utt_per_s_median': round(64 / float(np.median(v)), 1),
                                                     's_median': round(float(np.median(v)), 5)} for k, v in sec.items()}
    out['quality'] = quality()
    print(json.dumps(out, indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
