"""Stage 2 at BASELINE config 5 on one MI355X for two generator modes side by side: B = 128, bf16, english hps with enc_size =
emb_size = 1024.  One iteration = n_patch_steps (5) discriminator steps + one generator step + the target-guided step
(trainer.py:467-560, --train_tgat).  Both trainers live in one process and are timed in alternating rounds, so clocks and
neighbours are shared.  Prints one line per mode and one JSON line.
  python tools/s2_gmode_bench.py [--modes targeted_residual,spectrogram] [--iters 3] [--rounds 3]"""
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
ap.add_argument('--modes', default='targeted_residual,spectrogram'); ap.add_argument('--iters', type=int, default=3)
ap.add_argument('--rounds', type=int, default=3); ap.add_argument('--batch', type=int, default=128); ap.add_argument('--dtype', default='bf16')
a = ap.parse_args()
dev = torch.device('cuda:0')
B = a.batch
hps = make_hps(enc_size=1024, emb_size=1024, batch_size=B)
g = torch.Generator().manual_seed(0)
x_s = torch.rand(B, 128, 513, generator=g).to(dev); x_t = torch.rand(B, 128, 513, generator=g).to(dev)
c_t = torch.randint(hps.n_speakers - hps.n_target_speakers, hps.n_speakers, (B,), generator=g).to(dev)
runs = {}
for mode in a.modes.split(','):
    tr = Trainer(hps, None, mode, hps.enc_mode, log_dir='/tmp/zs_s2_log', dtype=a.dtype, device=dev)
    runs[mode] = (tr, tr.stage2())


def iteration(s2):
    for _ in range(hps.n_patch_steps):
        s2.d_step(x_s, x_t, c_t)
    r = s2.g_step(x_s, x_t, c_t)
    return r, s2.tg_step(x_t, c_t)


times = {m: [] for m in runs}
last = {}
for m, (_, s2) in runs.items():
    iteration(s2)                                                   # warm-up: buffers, packs, kernels
torch.cuda.synchronize()
for _ in range(a.rounds):
    for m, (_, s2) in runs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            last[m] = iteration(s2)
        torch.cuda.synchronize()
        times[m].append((time.perf_counter() - t0) / a.iters * 1e3)
        layers.check_status(dev)
out = {}
for m, (_, s2) in runs.items():
    torch.cuda.synchronize(); t1 = time.perf_counter(); s2.g_step(x_s, x_t, c_t); s2.tg_step(x_t, c_t); torch.cuda.synchronize()
    gt = (time.perf_counter() - t1) * 1e3
    out[m] = {'ms_per_iteration': sorted(times[m]), 'g_plus_tg_ms': gt, 'loss_adv': last[m][0]['loss_adv'].item(),
              'tg_rec': last[m][1].item()}
    print('stage 2 %s (%s, B=%d, 5 D + 1 G + tg): %s ms per iteration (rounds, sorted); G + tg step alone %.1f ms' %
          (m, a.dtype, B, ', '.join('%.1f' % t for t in sorted(times[m])), gt), flush=True)
print(json.dumps({'workload': 'stage 2 config 5, B=%d %s' % (B, a.dtype), 'iters': a.iters, 'rounds': a.rounds, 'modes': out}), flush=True)
