"""train_ae step time per encoder mode at the bench configuration (hps/zerospeech_english_1024.json: seg_len 128, 513 bins,
emb_size 1024, 102 speakers; B = 256, bf16, graph-captured step on a resident batch, as bench.py measures multilabel_binary):
multilabel_binary, one_hot and continues at enc_size 1024 and binary at enc_size 32 (32^2 = 1024 linear columns).

The modes are built side by side and measured interleaved: R rounds, each timing K steps of every mode in turn (order rotated
per round), after a warm-up per mode; the median and spread over the rounds are reported per mode.  bench.py does not call
this.  Prints one JSON line.
    python tools/encmode_bench.py [--rounds 7] [--steps 10] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

MODES = [('multilabel_binary', 1024), ('one_hot', 1024), ('continues', 1024), ('binary', 32)]


def build(mode, E, dev, dtype, B):
    from zs_amd.hps import Hps
    from zs_amd.model import Decoder, Encoder
    from zs_amd.trainer import AEStep
    hps = Hps(os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')).get_tuple()
    seg_len, F, nspk = hps.seg_len, 513, 102
    torch.manual_seed(1234)
    enc = Encoder(ns=hps.ns, dp=hps.enc_dp, enc_size=E, seg_len=seg_len, enc_mode=mode, dtype=dtype).to(dev)
    dec = Decoder(ns=hps.ns, c_in=E, c_h=hps.emb_size, c_a=nspk, seg_len=seg_len, dtype=dtype).to(dev)
    ae = AEStep(enc, dec, lr=1e-4, max_grad_norm=5.0, use_graph=True)
    g = torch.Generator().manual_seed(99)
    xs, cs = ae.static_inputs(B, seg_len, F)
    xs.copy_(torch.rand(B, seg_len, F, generator=g) * (1 - 1e-8) + 1e-8)
    cs.copy_(torch.randint(0, nspk, (B,), generator=g))
    return ae, xs, cs


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--batch', type=int, default=256)
    p.add_argument('--dtype', default='bf16')
    args = p.parse_args()
    import zs_amd  # noqa: F401
    from zs_amd import layers
    dev = torch.device('cuda:0')
    runs = {}
    for mode, E in MODES:
        ae, xs, cs = build(mode, E, dev, args.dtype, args.batch)
        for _ in range(3 + args.warmup):                   # 2 eager steps + the capture, then warm-up replays
            ae.step(xs, cs)
        torch.cuda.synchronize()
        runs[mode] = (ae, xs, cs, E)
        sys.stderr.write('[encmode_bench] %s E=%d built, loss %.4f\n' % (mode, E, ae._loss.item()))
    ms = {m: [] for m, _ in MODES}
    names = [m for m, _ in MODES]
    for r in range(args.rounds):
        order = names[r % len(names):] + names[:r % len(names)]
        for mode in order:
            ae, xs, cs, _ = runs[mode]
            ae.step(xs, cs)                                # one untimed replay after switching modes
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ae.step(xs, cs)
            torch.cuda.synchronize()
            ms[mode].append((time.perf_counter() - t0) * 1e3 / args.steps)
    layers.check_status(dev)
    out = {'metric': 'train_ae_step_ms_by_enc_mode', 'batch': args.batch, 'dtype': args.dtype, 'rounds': args.rounds,
           'steps_per_round': args.steps, 'device': torch.cuda.get_device_name(dev), 'modes': {}}
    for mode, E in MODES:
        v = ms[mode]
        out['modes'][mode] = {'enc_size': E, 'linear_cols': runs[mode][0].Encoder.n_lin, 'median_ms': round(statistics.median(v), 3),
                              'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3),
                              'final_loss': round(float(runs[mode][0]._loss.item()), 5)}
    base = out['modes']['multilabel_binary']['median_ms']
    for mode in out['modes']:
        out['modes'][mode]['vs_multilabel_binary'] = round(out['modes'][mode]['median_ms'] / base, 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
