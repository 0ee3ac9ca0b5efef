"""What the weight average (--ema) costs the counted train_ae step, and that it costs nothing when off: the B = 256
bf16 graph-captured step of the bench configuration (hps/zerospeech_english_1024.json, a resident batch, as bench.py measures it)
of three builds side by side:
    parent   a built copy of the parent commit (--parent DIR: a tree with its own libzs_amd.so)
    off      this tree, no average
    ema      this tree, AEStep(ema=0.999)
Each is a worker process of its own (a build is a Python package plus its shared library) that captures its step, warms up and
then times K replays whenever the driver tells it to over its stdin; the driver alternates the three, R rounds, order rotated per
round, so that drift of the machine lands on all three alike.  Medians and spreads (max - min over the rounds) go to one JSON
line and to --out.  "off costs nothing" holds when median(off) - median(parent) <= the larger of the two spreads.
    python tools/ema_bench.py --parent DIR [--rounds 7] [--steps 20] [--warmup 5] [--out profiles/ema_step_ms.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(args):
    sys.path.insert(0, args.tree)
    import torch
    import zs_amd  # noqa: F401
    from zs_amd import layers
    from zs_amd.hps import Hps
    from zs_amd.model import Decoder, Encoder
    from zs_amd.trainer import AEStep
    dev = torch.device('cuda:0')
    hps = Hps(os.path.join(args.tree, 'hps', 'zerospeech_english_1024.json')).get_tuple()
    seg_len, F, nspk, B = hps.seg_len, 513, 102, args.batch
    torch.manual_seed(1234)
    enc = Encoder(ns=hps.ns, dp=hps.enc_dp, enc_size=hps.enc_size, seg_len=seg_len, enc_mode='multilabel_binary', dtype=args.dtype).to(dev)
    dec = Decoder(ns=hps.ns, c_in=hps.enc_size, c_h=hps.emb_size, c_a=nspk, seg_len=seg_len, dtype=args.dtype).to(dev)
    kw = {} if args.ema is None else {'ema': args.ema}            # (the parent's AEStep has no such argument)
    ae = AEStep(enc, dec, lr=1e-4, max_grad_norm=5.0, use_graph=True, **kw)
    g = torch.Generator().manual_seed(99)
    xs, cs = ae.static_inputs(B, seg_len, F)
    xs.copy_(torch.rand(B, seg_len, F, generator=g) * (1 - 1e-8) + 1e-8)
    cs.copy_(torch.randint(0, nspk, (B,), generator=g))
    for _ in range(3 + args.warmup):                              # 2 eager steps + the capture, then warm-up replays
        ae.step(xs, cs)
    torch.cuda.synchronize()
    print(json.dumps({'ready': True, 'loss': float(ae._loss.item()), 'graphs': len(ae._graphs)}), flush=True)
    for line in sys.stdin:
        if line.strip() != 'go':
            break
        ae.step(xs, cs)                                           # one untimed replay after the other builds had the GPU
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            ae.step(xs, cs)
        torch.cuda.synchronize()
        print(json.dumps({'ms': (time.perf_counter() - t0) * 1e3 / args.steps}), flush=True)
    layers.check_status(dev)
    print(json.dumps({'done': True, 'loss': float(ae._loss.item())}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent', default=None, help="a built tree of the parent commit (its own package and libzs_amd.so)")
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--batch', type=int, default=256)
    p.add_argument('--dtype', default='bf16')
    p.add_argument('--decay', type=float, default=0.999)
    p.add_argument('--out', default=None)
    p.add_argument('--worker', action='store_true', help=argparse.SUPPRESS)
    p.add_argument('--tree', default=HERE, help=argparse.SUPPRESS)
    p.add_argument('--ema', type=float, default=None, help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.worker:
        return worker(args)
    if args.rounds < 5:
        p.error('--rounds must be at least 5')
    if args.parent is None or not os.path.isdir(args.parent):
        p.error('--parent DIR: a built tree of the parent commit is needed')
    builds = [('parent', os.path.abspath(args.parent), None), ('off', HERE, None), ('ema', HERE, args.decay)]
    procs = {}

    def say(name):
        while True:                                               # (the package prints lines of its own, e.g. the hps loader's)
            line = procs[name].stdout.readline()
            if not line:
                raise RuntimeError('%s worker ended (exit code %r)' % (name, procs[name].wait()))
            if line.startswith('{'):
                return json.loads(line)

    try:
        for name, tree, ema in builds:                            # one after the other: each captures with the GPU to itself
            cmd = [sys.executable, os.path.abspath(__file__), '--worker', '--tree', tree, '--steps', str(args.steps), '--warmup',
                   str(args.warmup), '--batch', str(args.batch), '--dtype', args.dtype] + (['--ema', repr(ema)] if ema is not None else [])
            env = dict(os.environ)
            env.pop('ZS_LIB_PATH', None)                          # each tree loads the library beside its own package
            procs[name] = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=tree, env=env)
            sys.stderr.write('[ema_bench] %s ready: %r\n' % (name, say(name)))
        names = [b[0] for b in builds]
        ms = {n: [] for n in names}
        for r in range(args.rounds):
            for name in names[r % 3:] + names[:r % 3]:
                procs[name].stdin.write('go\n')
                procs[name].stdin.flush()
                ms[name].append(say(name)['ms'])
            sys.stderr.write('[ema_bench] round %d: %s\n' % (r, ', '.join('%s %.3f' % (n, ms[n][-1]) for n in names)))
        final = {}
        for name in names:
            procs[name].stdin.close()
            final[name] = say(name)['loss']
            procs[name].wait()
    finally:
        for pr in procs.values():
            if pr.poll() is None:
                pr.kill()
                pr.wait()
    out = {'metric': 'train_ae_step_ms_parent_vs_ema_off_vs_ema_on', 'batch': args.batch, 'dtype': args.dtype, 'decay': args.decay,
           'rounds': args.rounds, 'steps_per_round': args.steps, 'order': 'alternating parent/off/ema, rotated per round, one GPU job',
           'builds': {}}
    for name in names:
        v = ms[name]
        out['builds'][name] = {'ms': [round(x, 3) for x in v], 'median_ms': round(statistics.median(v), 3),
                               'spread_ms': round(max(v) - min(v), 3), 'final_loss': final[name]}
    b = out['builds']
    out['off_minus_parent_ms'] = round(b['off']['median_ms'] - b['parent']['median_ms'], 3)
    out['larger_spread_ms'] = max(b['off']['spread_ms'], b['parent']['spread_ms'])
    out['off_costs_nothing'] = out['off_minus_parent_ms'] <= out['larger_spread_ms']
    out['ema_minus_off_ms'] = round(b['ema']['median_ms'] - b['off']['median_ms'], 3)
    out['losses_equal'] = final['parent'] == final['off'] == final['ema']
    text = json.dumps(out)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
