"""What held-out validation (--valid_every) costs, and that it costs the training step nothing when off.  Three measurements
at the bench configuration (hps/zerospeech_english_1024.json, B = 256, bf16, graph-captured), one JSON line and --out:
  step      the counted train_ae step of a built copy of the parent commit (--parent DIR: a tree with its own libzs_amd.so) and of this
            tree with validation off, as tools/ema_bench.py measures it: one worker process per build, the driver alternates them, R
            rounds, order rotated.  "off costs nothing" holds when median(off) - median(parent) <= the larger of the two spreads
            (max - min over the rounds): off adds no launch.
  pass      one validation (M = 8 batches: the replayed hipGraph of 8 x (Encoder + Decoder forward + zs_eval_accum), the table's D2H
            copy included) against the replayed graph of the same 8 x (Encoder + Decoder forward) alone, alternating.
  kernel    zs_eval_accum alone: 40 calls captured into one hipGraph, the replay timed by device events (no host launch cost in it).
            The whole call; the call without the unit statistics (the L1 pass + the finishing kernel); the same at T = F = 1 (the
            finishing kernel behind an empty L1 launch), which splits the L1 pass off; cycling over 8 operand pairs (1.07 GB: HBM)
            and on one pair (134 MB: it fits the 256 MiB Infinity Cache).  GB/s = the bytes a part
            must read (2 B T F floats; B T4 E for the units) / its time.
    python tools/valid_bench.py --parent DIR [--rounds 7] [--steps 20] [--warmup 5] [--out profiles/valid_step_ms.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY_GBPS = 6290.0                                       # GB/s of a plain float4 copy kernel on an MI355X (79 % of the 8 TB/s datasheet rate): the yardstick of DESIGN 25


def _nets(args, dev):
    import torch
    from zs_amd.hps import Hps
    from zs_amd.model import Decoder, Encoder
    from zs_amd.trainer import AEStep
    hps = Hps(os.path.join(args.tree, 'hps', 'zerospeech_english_1024.json')).get_tuple()
    torch.manual_seed(1234)
    enc = Encoder(ns=hps.ns, dp=hps.enc_dp, enc_size=hps.enc_size, seg_len=hps.seg_len, enc_mode='multilabel_binary', dtype=args.dtype).to(dev)
    dec = Decoder(ns=hps.ns, c_in=hps.enc_size, c_h=hps.emb_size, c_a=102, seg_len=hps.seg_len, dtype=args.dtype).to(dev)
    return hps, AEStep(enc, dec, lr=1e-4, max_grad_norm=5.0, use_graph=True)


def step_worker(args):
    sys.path.insert(0, args.tree)
    import torch
    import zs_amd  # noqa: F401
    from zs_amd import layers
    dev = torch.device('cuda:0')
    hps, ae = _nets(args, dev)
    seg_len, F, B = hps.seg_len, 513, args.batch
    g = torch.Generator().manual_seed(99)
    xs, cs = ae.static_inputs(B, seg_len, F)
    xs.copy_(torch.rand(B, seg_len, F, generator=g) * (1 - 1e-8) + 1e-8)
    cs.copy_(torch.randint(0, 102, (B,), generator=g))
    for _ in range(3 + args.warmup):                              # 2 eager steps + the capture, then warm-up replays
        ae.step(xs, cs)
    torch.cuda.synchronize()
    print(json.dumps({'ready': True, 'loss': float(ae._loss.item())}), flush=True)
    for line in sys.stdin:
        if line.strip() != 'go':
            break
        ae.step(xs, cs)                                           # one untimed replay after the other build had the GPU
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            ae.step(xs, cs)
        torch.cuda.synchronize()
        print(json.dumps({'ms': (time.perf_counter() - t0) * 1e3 / args.steps}), flush=True)
    layers.check_status(dev)
    print(json.dumps({'done': True, 'loss': float(ae._loss.item())}), flush=True)


def valid_worker(args):
    sys.path.insert(0, args.tree)
    import functools
    import torch
    import zs_amd  # noqa: F401
    from zs_amd import _lib as L
    from zs_amd import layers, validation
    from zs_amd.dataloader import SyntheticDataset
    from zs_amd.trainer import ValidStep
    dev = torch.device('cuda:0')
    hps, ae = _nets(args, dev)
    M, B, T, F = args.valid_batches, args.batch, hps.seg_len, 513
    vset = validation.ValidSet.from_dataset(SyntheticDataset(M * B, seg_len=T, n_speakers=102, seed=3), M, B, 102)
    vs = ValidStep(ae, vset, M, 102)
    first, second = vs.run(), vs.run()                             # eager, then the capture and its first replay
    assert first['spk_sum'].tobytes() == second['spk_sum'].tobytes()
    rec = validation.finish(second, T, F)

    def forward_only(m):                                           # ValidStep._batch without the accumulation
        bits, _, _ = ae.Encoder._engine().forward(vs.x[m], False, noise_kind=2, seed=validation.VALID_SEED + m, tape='valid')
        ae.Decoder._engine().forward(bits, vs.c[m], False)
    fwd = ae._capture_plan([('run', functools.partial(forward_only, m)) for m in range(M)])[1]

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps
    runs = {'pass': vs.run, 'forwards': lambda: ae._execute(fwd)}
    ms = {k: [] for k in runs}
    for r in range(args.rounds):
        for k in (('pass', 'forwards') if r % 2 == 0 else ('forwards', 'pass')):
            ms[k].append(timed(runs[k]))

    # the kernel alone
    E, T4 = hps.enc_size, T // 8
    g = torch.Generator().manual_seed(7)
    xd = [torch.rand(B, T, 520, generator=g).to(dev) for _ in range(M)]                      # rows padded to 520 floats (16-byte aligned), as an activation buffer pads them
    bits = [(torch.rand(B, T4, E, generator=g) < 0.5).float().to(dev) for _ in range(M)]

    def accum(m, units, T=T, F=F):
        L.call('zs_eval_accum', 'ZsEvalAccum', torch.cuda.current_stream(dev).cuda_stream, x_dec=L.ptr(xd[m]), ld_dec=520, x=L.ptr(vs.x[m]),
               ldx=513, c=L.ptr(vs.c[m]), B=B, T=T, F=F, n_speakers=102, work=L.ptr(vs.work), spk_sum=vs._word('spk_sum'),
               spk_cnt=vs._word('spk_cnt'), bad=vs._word('bad'), bits_f32=L.ptr(bits[m]) if units else None, T4=T4, E=E,
               ones=vs._word('ones'), flips=vs._word('flips'), rows=vs._word('rows'), pairs=vs._word('pairs'))

    def kernel_us(calls=40, **kw):
        """us per call of `calls` calls captured into one hipGraph and replayed: the host's launch cost is not in it."""
        cycle = kw.pop('cycle')
        graph = ae._capture_plan([('run', lambda: [accum(i % M if cycle else 0, **kw) for i in range(calls)])])[1]
        ae._execute(graph)
        us = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ae._execute(graph)
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / calls)
        us.sort()
        return round(us[2], 2), round(us[-1] - us[0], 2)
    l1_bytes, unit_bytes = 2 * B * T * F * 4, B * T4 * E * 4
    kern = {}
    for name, kw in (('call_hbm', dict(units=True, cycle=True)), ('l1_finish_hbm', dict(units=False, cycle=True)),
                     ('call_cached', dict(units=True, cycle=False)), ('l1_finish_cached', dict(units=False, cycle=False)),
                     ('empty_l1_finish', dict(units=False, cycle=True, T=1, F=1))):      # the finishing kernel behind an L1 launch of one float a sample
        us, spread = kernel_us(**kw)
        kern[name] = {'us': us, 'spread_us': spread}
    kern['l1_part_us'] = round(kern['l1_finish_hbm']['us'] - kern['empty_l1_finish']['us'], 2)
    kern['l1_part_gbps'] = round(l1_bytes / kern['l1_part_us'] / 1e3, 1)
    kern['l1_finish_gbps'] = round(l1_bytes / kern['l1_finish_hbm']['us'] / 1e3, 1)
    kern['units_part_us'] = round(kern['call_hbm']['us'] - kern['l1_finish_hbm']['us'], 2)
    kern['units_part_gbps'] = round(unit_bytes / kern['units_part_us'] / 1e3, 1)
    kern.update(l1_bytes=l1_bytes, unit_bytes=unit_bytes, copy_gbps=COPY_GBPS)
    layers.check_status(dev)
    out = {name: {'ms': [round(x, 3) for x in v], 'median_ms': round(statistics.median(v), 3), 'spread_ms': round(max(v) - min(v), 3)}
           for name, v in ms.items()}
    out.update(valid_batches=M, valid_loss_rec=rec['valid_loss_rec'], kernel=kern,
               accum_share_ms=round(out['pass']['median_ms'] - out['forwards']['median_ms'], 3))
    print(json.dumps({'valid': out}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent', default=None, help='a built tree of the parent commit (its own package and libzs_amd.so)')
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--batch', type=int, default=256)
    p.add_argument('--valid_batches', type=int, default=8)
    p.add_argument('--dtype', default='bf16')
    p.add_argument('--out', default=None)
    p.add_argument('--worker', default=None, choices=['step', 'valid'], help=argparse.SUPPRESS)
    p.add_argument('--tree', default=HERE, help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.worker == 'step':
        return step_worker(args)
    if args.worker == 'valid':
        return valid_worker(args)
    if args.rounds < 5:
        p.error('--rounds must be at least 5')
    if args.parent is None or not os.path.isdir(args.parent):
        p.error('--parent DIR: a built tree of the parent commit is needed')
    builds = [('parent', os.path.abspath(args.parent)), ('off', HERE)]
    procs = {}
    common = ['--steps', str(args.steps), '--warmup', str(args.warmup), '--batch', str(args.batch), '--dtype', args.dtype,
              '--rounds', str(args.rounds), '--valid_batches', str(args.valid_batches)]
    env = dict(os.environ)
    env.pop('ZS_LIB_PATH', None)                                  # each tree loads the library beside its own package

    def say(pr, name):
        while True:                                               # (the package prints lines of its own, e.g. the hps loader's)
            line = pr.stdout.readline()
            if not line:
                raise RuntimeError('%s worker ended (exit code %r)' % (name, pr.wait()))
            if line.startswith('{'):
                return json.loads(line)

    try:
        for name, tree in builds:                                 # one after the other: each captures with the GPU to itself
            cmd = [sys.executable, os.path.abspath(__file__), '--worker', 'step', '--tree', tree] + common
            procs[name] = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=tree, env=env)
            sys.stderr.write('[valid_bench] %s ready: %r\n' % (name, say(procs[name], name)))
        names = [b[0] for b in builds]
        ms = {n: [] for n in names}
        for r in range(args.rounds):
            for name in names[r % 2:] + names[:r % 2]:
                procs[name].stdin.write('go\n')
                procs[name].stdin.flush()
                ms[name].append(say(procs[name], name)['ms'])
            sys.stderr.write('[valid_bench] round %d: %s\n' % (r, ', '.join('%s %.3f' % (n, ms[n][-1]) for n in names)))
        final = {}
        for name in names:
            procs[name].stdin.close()
            final[name] = say(procs[name], name)['loss']
            procs[name].wait()
        # the validation pass and the kernel, with the GPU to itself again
        cmd = [sys.executable, os.path.abspath(__file__), '--worker', 'valid', '--tree', HERE] + common
        procs['valid'] = subprocess.Popen(cmd, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, text=True, cwd=HERE, env=env)
        valid = say(procs['valid'], 'valid')['valid']
        procs['valid'].wait()
    finally:
        for pr in procs.values():
            if pr.poll() is None:
                pr.kill()
                pr.wait()
    out = {'metric': 'train_ae_step_ms_parent_vs_validation_off, validation_pass_ms, zs_eval_accum_us', 'batch': args.batch,
           'dtype': args.dtype, 'rounds': args.rounds, 'steps_per_round': args.steps,
           'order': 'alternating parent/off, rotated per round; then pass/forwards alternating; one GPU job', 'builds': {}}
    for name in names:
        v = ms[name]
        out['builds'][name] = {'ms': [round(x, 3) for x in v], 'median_ms': round(statistics.median(v), 3),
                               'spread_ms': round(max(v) - min(v), 3), 'final_loss': final[name]}
    b = out['builds']
    out['off_minus_parent_ms'] = round(b['off']['median_ms'] - b['parent']['median_ms'], 3)
    out['larger_spread_ms'] = max(b['off']['spread_ms'], b['parent']['spread_ms'])
    out['off_costs_nothing'] = out['off_minus_parent_ms'] <= out['larger_spread_ms']
    out['losses_equal'] = final['parent'] == final['off']
    out['validation'] = valid
    text = json.dumps(out)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
