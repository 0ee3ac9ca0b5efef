"""What the unit codebook costs, in one GPU job:
  assign    zs_code_assign alone at n = 2^20, K = 1024, E = 1024 and at one inference chunk (256 x 16 rows): HIP events around a replayed
            graph of launches (the host's launch cost is not in it), and beside it, as context, the same argmin through plain torch on the
            same device: unpacked bf16 operands and one matmul
  fit       one full k-modes iteration at the large size (assign, accum, update, the D2H copy of the counters), by the host clock
  convert   convert_wavs with a K = 1024 codebook against without, alternating, on the workload of tools/convert_dir_bench.py at 16 kHz
  parent    (--parent DIR, a built tree of the parent commit) convert_wavs without a codebook in this build against the parent's, one
            worker process each, alternating round by round, both spreads reported: "off costs nothing" holds when
            median(off) - median(parent) <= the larger spread
    python tools/codebook_bench.py [--parent DIR] [--rounds 7] [--utts 64] [--n-iter 300] [--out profiles/codebook_bench.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synth(rate, rng):
    """tools/convert_dir_bench.py's utterance: 2-7 s of a drifting harmonic tone with noise, silence at either end."""
    import numpy as np
    n = int(rng.uniform(2.0, 7.0) * rate)
    t = np.arange(n) / float(rate)
    f0 = rng.uniform(90, 250)
    y = sum(0.25 / k * np.sin(2 * np.pi * k * f0 * t * (1 + 0.02 * np.sin(2 * np.pi * 0.7 * t))) for k in (1, 2, 3, 5))
    y = y * (0.6 + 0.4 * np.sin(2 * np.pi * 2.1 * t) ** 2) + 0.01 * rng.randn(n)
    lead, trail = int(rng.uniform(0.2, 0.5) * rate), int(rng.uniform(0.2, 0.5) * rate)
    y[:lead] = 0.0
    y[n - trail:] = 0.0
    return y.astype(np.float32)


def _workload(args, tree):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    import zs_amd  # noqa: F401
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    dev = torch.device('cuda:0')
    hps = make_hps(enc_size=1024, emb_size=1024, n_speakers=102)
    torch.manual_seed(0)
    tr = Trainer(hps, None, 'naive', 'multilabel_binary', log_dir=tempfile.mkdtemp(), dtype=args.dtype, device=dev)
    rng = np.random.RandomState(16000)
    wavs = [synth(16000, rng) for _ in range(args.utts)]
    spk = [100 + (i % 2) for i in range(args.utts)]
    return dev, hps, tr, wavs, spk


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(v):
    return {'ms': [round(x, 3) for x in v], 'median_ms': round(statistics.median(v), 3), 'spread_ms': round(max(v) - min(v), 3)}


def convert_worker(args):
    """convert_wavs without a codebook in the tree given: one timed call per line on stdin."""
    dev, hps, tr, wavs, spk = _workload(args, args.tree)
    from zs_amd import convert as cv
    run = lambda: cv.convert_wavs(wavs, 16000, tr, hps.seg_len, spk, n_iter=args.n_iter)
    for _ in range(2):
        run()
    print(json.dumps({'ready': True}), flush=True)
    for _ in sys.stdin:
        print(json.dumps({'ms': _timed(run)}), flush=True)
    print(json.dumps({'done': True}), flush=True)


def kernels(args, out):
    import numpy as np
    import torch
    from zs_amd import _lib as L, codebook as C
    dev = torch.device('cuda:0')
    E, K, rb = 1024, 1024, 128
    g = torch.Generator().manual_seed(0)
    code = torch.randint(0, 256, (K, rb), dtype=torch.uint8, generator=g).to(dev)
    out['assign'] = {}
    for name, n, calls in (('n_2p20', 1 << 20, 4), ('chunk_256x16', 256 * 16, 40)):
        near = torch.randint(0, K, (n,), generator=g)
        flip = (torch.rand(n, rb, generator=g) < 0.03).to(torch.uint8) * torch.randint(0, 256, (n, rb), dtype=torch.uint8, generator=g)
        units = (code.cpu()[near] ^ flip).to(dev)
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        dist = torch.empty(n, dtype=torch.int32, device=dev)
        launch = lambda: C.assign(units, code, E, idx=idx, dist=dist)
        launch()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(calls):
                launch()
        graph.replay()
        us = []
        for _ in range(7):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graph.replay()
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1e3 / calls)
        us.sort()
        # context: the same argmin in plain torch -- bf16 0 / 1 operands, one matmul (its bf16 output rounds distances above 256)
        ub = torch.from_numpy(np.unpackbits(units.cpu().numpy(), axis=1, bitorder='little')).to(dev, torch.bfloat16)
        cb = torch.from_numpy(np.unpackbits(code.cpu().numpy(), axis=1, bitorder='little')).to(dev, torch.bfloat16)
        c1 = cb.float().sum(1)

        def plain():
            return (c1[None, :] - 2.0 * (ub @ cb.t()).float()).argmin(1)
        ref = plain()
        tus = []
        for _ in range(7):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            plain()
            b.record()
            torch.cuda.synchronize()
            tus.append(a.elapsed_time(b) * 1e3)
        tus.sort()
        pairs = float(n) * K
        out['assign'][name] = {'n': n, 'K': K, 'E': E, 'launches_per_replay': calls, 'us': round(us[3], 2), 'spread_us': round(us[-1] - us[0], 2),
                               'pairs_per_s': round(pairs / (us[3] * 1e-6), 0), 'xor_popc_dwords_per_s': round(pairs * 32 / (us[3] * 1e-6), 0),
                               'torch_bf16_matmul_argmin_us': round(tus[3], 2), 'torch_spread_us': round(tus[-1] - tus[0], 2),
                               'torch_agrees_on': round(float((ref.int() == idx).float().mean()), 6),
                               'mean_dist': round(float(dist.float().mean()), 2)}
        if n == 1 << 20:                                             # one full fit iteration at this size, by the host clock
            stats = torch.empty(4 + K, dtype=torch.int32, device=dev)
            ones = torch.empty(K, E, dtype=torch.int32, device=dev)
            code2 = code.clone()
            st = torch.cuda.current_stream().cuda_stream

            def iteration():
                stats.zero_()
                ones.zero_()
                C.assign(units, code2, E, idx=idx, dist=dist, total=stats[0:2])
                L.call('zs_code_accum', 'ZsCodeAccum', st, units=L.ptr(units), idx=L.ptr(idx), n=n, row_bytes=rb, K=K, E=E, cnt=L.ptr(stats, 4),
                       ones=L.ptr(ones), bad=L.ptr(stats, 3))
                L.call('zs_code_update', 'ZsCodeUpdate', st, code=L.ptr(code2), K=K, code_bytes=rb, E=E, cnt=L.ptr(stats, 4), ones=L.ptr(ones),
                       changed=L.ptr(stats, 2))
                return stats.cpu()
            iteration()
            ms = [_timed(iteration) for _ in range(7)]
            parts = {}
            for part, fn in (('accum', lambda: L.call('zs_code_accum', 'ZsCodeAccum', st, units=L.ptr(units), idx=L.ptr(idx), n=n, row_bytes=rb,
                                                      K=K, E=E, cnt=L.ptr(stats, 4), ones=L.ptr(ones), bad=L.ptr(stats, 3))),
                             ('update', lambda: L.call('zs_code_update', 'ZsCodeUpdate', st, code=L.ptr(code2), K=K, code_bytes=rb, E=E,
                                                       cnt=L.ptr(stats, 4), ones=L.ptr(ones), changed=L.ptr(stats, 2)))):
                ev = []
                for _ in range(7):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    torch.cuda.synchronize()
                    ev.append(a.elapsed_time(b) * 1e3)
                ev.sort()
                parts[part + '_us'] = round(ev[3], 2)
            out['fit_iteration'] = dict(_stats(ms), n=n, K=K, E=E, **parts)


def convert_with_and_without(args, out):
    import torch
    dev, hps, tr, wavs, spk = _workload(args, HERE)
    from zs_amd import codebook as C, convert as cv
    units, _ = cv.encode_batch([w for w in cv._wav_features(wavs, 16000, dev)[0]], tr, hps.seg_len, packed=True, units_on_device=True)
    cb = C.fit(torch.cat(units).contiguous(), 1024, iters=5, E=1024)
    runs = {'off': lambda: cv.convert_wavs(wavs, 16000, tr, hps.seg_len, spk, n_iter=args.n_iter),
            'K1024': lambda: cv.convert_wavs(wavs, 16000, tr, hps.seg_len, spk, n_iter=args.n_iter, codebook=cb)}
    for fn in runs.values():
        fn()
        fn()
    ms = {k: [] for k in runs}
    for r in range(-1, args.rounds):                              # round -1 alternates as the others do and is not counted
        for k in (('off', 'K1024') if r % 2 == 0 else ('K1024', 'off')):
            t = _timed(runs[k])
            if r >= 0:
                ms[k].append(t)
    out['convert_wavs'] = {k: _stats(v) for k, v in ms.items()}
    out['convert_wavs'].update(utts=args.utts, n_iter=args.n_iter, units=int(sum(len(u) for u in units)), fit_history=cb.meta['history'],
                               K1024_minus_off_ms=round(statistics.median(ms['K1024']) - statistics.median(ms['off']), 3))


def against_parent(args, out):
    builds = [('parent', os.path.abspath(args.parent)), ('off', HERE)]
    env = dict(os.environ)
    env.pop('ZS_LIB_PATH', None)                                  # each tree loads the library beside its own package
    common = ['--utts', str(args.utts), '--n-iter', str(args.n_iter), '--dtype', args.dtype]
    procs = {}

    def say(pr, name):
        while True:
            line = pr.stdout.readline()
            if not line:
                raise RuntimeError('%s worker ended (exit code %r)' % (name, pr.wait()))
            if line.startswith('{'):
                return json.loads(line)
    try:
        for name, tree in builds:
            cmd = [sys.executable, os.path.abspath(__file__), '--worker', '--tree', tree] + common
            procs[name] = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=tree, env=env)
            say(procs[name], name)
        names = [b[0] for b in builds]
        ms = {n: [] for n in names}
        for r in range(-1, args.rounds):                          # round -1 alternates as the others do and is not counted
            for name in names[r % 2:] + names[:r % 2]:
                procs[name].stdin.write('go\n')
                procs[name].stdin.flush()
                t = say(procs[name], name)['ms']
                if r >= 0:
                    ms[name].append(t)
        for name in names:
            procs[name].stdin.close()
            say(procs[name], name)
            procs[name].wait()
    finally:
        for pr in procs.values():
            if pr.poll() is None:
                pr.kill()
                pr.wait()
    rec = {n: _stats(ms[n]) for n in names}
    rec['off_minus_parent_ms'] = round(rec['off']['median_ms'] - rec['parent']['median_ms'], 3)
    rec['larger_spread_ms'] = max(rec['off']['spread_ms'], rec['parent']['spread_ms'])
    rec['off_costs_nothing'] = rec['off_minus_parent_ms'] <= rec['larger_spread_ms']
    out['convert_wavs_off_vs_parent'] = rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent', default=None, help='a built tree of the parent commit (its own package and libzs_amd.so)')
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--utts', type=int, default=64)
    p.add_argument('--n-iter', type=int, default=300, dest='n_iter')
    p.add_argument('--dtype', default='bf16')
    p.add_argument('--out', default=os.path.join(HERE, 'profiles', 'codebook_bench.json'))
    p.add_argument('--worker', default=False, action='store_true', help=argparse.SUPPRESS)
    p.add_argument('--tree', default=HERE, help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.worker:
        return convert_worker(args)
    if args.rounds < 5:
        p.error('--rounds must be at least 5')
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        sys.exit('codebook_bench needs an MI355X: a timing taken anywhere else says nothing about it')
    import zs_amd  # noqa: F401
    out = {'device': torch.cuda.get_device_name(0), 'dtype': args.dtype, 'rounds': args.rounds,
           'order': 'warm-up, one uncounted alternating round, then alternating rounds, order rotated per round; one GPU job'}
    if args.parent is not None:                                   # first, while this process holds no GPU memory
        against_parent(args, out)
    kernels(args, out)
    convert_with_and_without(args, out)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
