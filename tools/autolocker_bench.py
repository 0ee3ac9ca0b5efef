"""The stage-2 autolocker step (AutolockerStep.al_step, trainer.py:563-611) on one MI355X: ms per iteration (al step + the
target-guided step of --train_al's target_guided run) at B = 16 (the reference's batch) and B = 128, bf16, english hps with
enc_size 6 and 1024; and, at each shape, the encoder's input-gradient pass alone (EncoderEngine.backward_input) next to its full
backward (EncoderEngine.backward: weight + data gradients) on the re-encode's tape.  Prints one line per shape and one JSON line.
  python tools/autolocker_bench.py [--sizes 6,1024] [--batches 16,128] [--iters 5] [--rounds 3]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zs_amd  # noqa: E402,F401
from zs_amd import layers  # noqa: E402
from zs_amd.hps import make_hps  # noqa: E402
from zs_amd.trainer import Trainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--sizes', default='6,1024'); ap.add_argument('--batches', default='16,128')
ap.add_argument('--iters', type=int, default=5); ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--dtype', default='bf16'); ap.add_argument('--g_mode', default='targeted_residual')
a = ap.parse_args()
dev = torch.device('cuda:0')


def timed(fn, iters, rounds):
    """median over rounds of the mean ms of `iters` back-to-back calls."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        layers.join_side(dev)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / iters * 1e3)
    return sorted(ts)[len(ts) // 2]


out = {}
for E in [int(v) for v in a.sizes.split(',')]:
    for B in [int(v) for v in a.batches.split(',')]:
        hps = make_hps(enc_size=E, batch_size=B)
        tr = Trainer(hps, None, a.g_mode, hps.enc_mode, log_dir='/tmp/zs_al_log', dtype=a.dtype, device=dev)
        s2 = tr.stage2(autolocker=True)
        g = torch.Generator().manual_seed(0)
        x_s = torch.rand(B, hps.seg_len, 513, generator=g).to(dev); x_t = torch.rand(B, hps.seg_len, 513, generator=g).to(dev)
        c_t = torch.randint(hps.n_speakers - hps.n_target_speakers, hps.n_speakers, (B,), generator=g).to(dev)
        al_ms = timed(lambda: s2.al_step(x_s, c_t), a.iters, a.rounds)
        it_ms = timed(lambda: (s2.al_step(x_s, c_t), s2.tg_step(x_t, c_t)), a.iters, a.rounds)
        s2.al_step(x_s, c_t, update=False)                       # leaves the re-encode's tape and its dlogits
        ee = tr.Encoder._engine()
        tp = ee.tapes['al']
        dlog = ee.ctx.act('e_dlog_al' + tp['tag'], B, tp['T4'], ee.n_lin)
        in_ms = timed(lambda: ee.backward_input(dlogits=dlog, tape='al'), a.iters, a.rounds)
        full_ms = timed(lambda: ee.backward(None, dlog), a.iters, a.rounds)
        layers.check_status(dev)
        key = 'E%d_B%d' % (E, B)
        out[key] = dict(al_step_ms=round(al_ms, 3), iteration_tg_ms=round(it_ms, 3), enc_backward_input_ms=round(in_ms, 3),
                        enc_backward_full_ms=round(full_ms, 3))
        print('[al] enc_size %4d B %3d %s: al step %.2f ms, al + tg iteration %.2f ms; encoder input gradient %.2f ms, full encoder '
              'backward %.2f ms' % (E, B, a.dtype, al_ms, it_ms, in_ms, full_ms), flush=True)
        del tr, s2, ee
        torch.cuda.empty_cache()
print(json.dumps(dict(bench='autolocker', dtype=a.dtype, g_mode=a.g_mode, **out)))
