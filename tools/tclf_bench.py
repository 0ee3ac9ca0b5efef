"""Target speaker classifier on one GPU: the --train_c step (TclfStep: forward with Dropout2d, CE, backward to the parameters, clip +
Adam) at two batch sizes, and --test_classify's scoring throughput, classify_batch (one fragment gather, batched eval forwards)
against one Trainer.classify call per fragment (the reference's loop, convert.py:388-393).  Prints one JSON line.

    python tools/tclf_bench.py [--dtype bf16|fp32] [--steps 20] [--warmup 5] [--utts 64] [--frames 700]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step_ms(T, B, steps, warmup, dev):
    from zs_amd.trainer import TclfStep
    step = TclfStep(T, 1e-4, 5.0, 100)
    g = torch.Generator(device=dev).manual_seed(B)
    x = torch.rand(B, 128, 513, generator=g, device=dev)
    c = torch.randint(95, 102, (B,), generator=g, device=dev)
    for _ in range(warmup):
        step.step(x, c)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step.step(x, c)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtype', choices=['fp32', 'bf16'], default='bf16')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--utts', type=int, default=64)
    ap.add_argument('--frames', type=int, default=700)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    import zs_amd  # noqa: F401
    from zs_amd import convert as cv
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    hps = make_hps(enc_size=16, emb_size=32, n_speakers=102, n_target_speakers=2)      # the classifier's size does not depend on these
    tr = Trainer(hps, None, 'targeted_residual', 'multilabel_binary', log_dir='/tmp/tclf_bench_log', dtype=a.dtype, device=dev)
    res = {'dtype': a.dtype}
    for B in (16, 128):
        res['step_ms_b%d' % B] = round(step_ms(tr.TargetClassifier, B, a.steps, a.warmup, dev), 3)
    rng = np.random.RandomState(1)
    lengths = [int(rng.randint(a.frames // 2, a.frames + 1)) for _ in range(a.utts)]
    T_max = max(lengths)
    mag = torch.rand(a.utts, T_max, 513, device=dev)
    plan = cv.tclf_plan(lengths, 128)
    n_frag = len(plan)
    cv.classify_batch((mag, lengths), tr, 128)                                            # warm-up (buffers, code objects)
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(a.reps):
        t0 = time.perf_counter()
        lg, _ = cv.classify_batch((mag, lengths), tr, 128)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    frags = [mag[u, s:s + 128].unsqueeze(0).contiguous() for u, s in plan]
    tr.classify(frags[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for f in frags:
        tr.classify(f)                                                                    # one host sync per fragment (.cpu())
    loop = time.perf_counter() - t0
    res.update(n_frag=n_frag, batched_frag_per_s=round(n_frag / best, 1), per_fragment_frag_per_s=round(n_frag / loop, 1))
    res['speedup'] = round(res['batched_frag_per_s'] / res['per_fragment_frag_per_s'], 2)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
