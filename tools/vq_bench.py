"""What the vector codebook costs, in one GPU job:
  assign    zs_vq_assign alone at n = 2^20, K = 1024, E = 1024 (fp32 rows, the fit's shape) and at one inference chunk (256 x 16 rows,
            bf16, both decompositions): HIP events around a replayed graph of launches, and beside it, as context and not as a bar, the
            same argmin through torch's fp32 `x @ code.T` + argmin on the same device
  fit       one full k-means iteration at the large size (assign, accum, update, the D2H copy of the counters), by the host clock
  convert   convert_wavs of a 'continues' model with a K = 1024 vector codebook against without, alternating, on the workload of
            tools/convert_dir_bench.py at 16 kHz
  parent    (--parent DIR, a built tree of the parent commit) the paths this feature must not slow, this build against the parent's,
            alternating round by round, both spreads reported: `bench.py --gpus 1 --steps 20 --warmup 5` (one process per run) and
            convert_wavs without a codebook (one worker process each).  "Unchanged" means median(new) - median(parent) <= the larger spread
  sweep     (--sweep, alone) both decompositions of zs_vq_assign at n = 2048 .. ZS_VQ_SPLIT_N - 1 for three K x E, median of 9 launches
            by HIP events -> profiles/vq_split_sweep.json: what the threshold in the header is judged by
    python tools/vq_bench.py [--parent DIR] [--rounds 7] [--utts 64] [--n-iter 300] [--out profiles/vq_bench.json]
    python tools/vq_bench.py --sweep"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, 'tools'))

from codebook_bench import _stats, _timed, synth  # noqa: E402  (the workload and the clocks of the bit codebook's bench)


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
    tr = Trainer(hps, None, 'naive', 'continues', log_dir=tempfile.mkdtemp(), dtype=args.dtype, device=dev)
    rng = np.random.RandomState(16000)
    wavs = [synth(16000, rng) for _ in range(args.utts)]
    spk = [100 + (i % 2) for i in range(args.utts)]
    return dev, hps, tr, wavs, spk


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


def _events(fn, reps=7, per=1):
    import torch
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / per)
    us.sort()
    return us


def kernels(args, out):
    import torch
    from zs_amd import _lib as L, vq as V
    dev = torch.device('cuda:0')
    E, K = 1024, 1024
    g = torch.Generator().manual_seed(0)
    code = torch.randn(K, E, generator=g).to(dev)
    cnorm = (code.double() ** 2).sum(1).float()
    out['assign'] = {}
    for name, n, calls, dt in (('n_2p20_fp32', 1 << 20, 2, torch.float32), ('chunk_256x16_bf16', 256 * 16, 40, torch.bfloat16)):
        x = (code[torch.randint(0, K, (n,), generator=g).to(dev)] + torch.randn(n, E, device=dev)).to(dt)
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        dist = torch.empty(n, dtype=torch.float32, device=dev)
        work = V.workspace(dev)
        rec = {'n': n, 'K': K, 'E': E, 'dtype': str(dt), 'launches_per_replay': calls}
        for path, w in (('split', work), ('rows', None)) if n < V.SPLIT_N else (('rows', None),):
            launch = lambda: V.assign(x, code, cnorm, idx=idx, dist=dist, work=w)
            launch()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(calls):
                    launch()
            graph.replay()
            us = _events(graph.replay, per=calls)
            rec[path] = {'us': round(us[3], 2), 'spread_us': round(us[-1] - us[0], 2),
                         'tflops': round(2.0 * n * K * E / (us[3] * 1e-6) / 1e12, 2)}
        xf = x.float()
        plain = lambda: (cnorm[None, :] - 2.0 * (xf @ code.t())).argmin(1)
        ref = plain()
        tus = _events(plain)
        rec.update(torch_fp32_matmul_argmin_us=round(tus[3], 2), torch_spread_us=round(tus[-1] - tus[0], 2),
                   torch_agrees_on=round(float((ref.int() == idx).float().mean()), 6))
        out['assign'][name] = rec
        if n == 1 << 20:                                             # one full fit iteration at this size, by the host clock
            shift = V.vq_shift(n, float(x.abs().amax()))
            stats = torch.empty(6 + K, dtype=torch.int32, device=dev)
            sums = torch.empty(K, E, dtype=torch.int64, device=dev)
            code2, cn2 = code.clone(), cnorm.clone()
            st = torch.cuda.current_stream().cuda_stream
            accum = lambda: L.call('zs_vq_accum', 'ZsVqAccum', st, x=L.ptr(x), idx=L.ptr(idx), n=n, ld_x=E, K=K, E=E, shift=shift,
                                   cnt=L.ptr(stats, 6), sum=L.ptr(sums), bad=L.ptr(stats, 4))
            update = lambda: L.call('zs_vq_update', 'ZsVqUpdate', st, code=L.ptr(code2), ld_code=E, cnorm=L.ptr(cn2), K=K, E=E, shift=shift,
                                    cnt=L.ptr(stats, 6), sum=L.ptr(sums), changed=L.ptr(stats, 3))

            def iteration():
                stats.zero_()
                sums.zero_()
                V.assign(x, code2, cn2, idx=idx, dist=dist, moved=stats[2:3])
                stats[0:2].view(torch.float64).copy_(dist.sum(dtype=torch.float64))
                accum()
                update()
                return stats.cpu()
            iteration()
            ms = [_timed(iteration) for _ in range(5)]
            out['fit_iteration'] = dict(_stats(ms), n=n, K=K, E=E, shift=shift, accum_us=round(_events(accum)[3], 2),
                                        update_us=round(_events(update)[3], 2))
        del x, xf


def sweep(path):
    import torch
    from zs_amd import vq as V
    dev = torch.device('cuda:0')
    out = {}
    for K, E in ((1024, 1024), (256, 1024), (1024, 128)):
        code = torch.randn(K, E, device=dev)
        cn = (code.double() ** 2).sum(1).float()
        for n in (2048, 8192, 16384, 24576, V.SPLIT_N - 1):
            x = torch.randn(n, E, device=dev).bfloat16()
            idx, dist = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, device=dev)
            rec = {}
            for name, w in (('split', V.workspace(dev)), ('rows', None)):
                f = lambda: V.assign(x, code, cn, idx=idx, dist=dist, work=w)
                f()
                torch.cuda.synchronize()
                rec[name] = round(_events(f, reps=9)[4], 1)
            out['K%d_E%d_n%d' % (K, E, n)] = rec
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


def convert_with_and_without(args, out):
    import torch
    dev, hps, tr, wavs, spk = _workload(args, HERE)
    from zs_amd import convert as cv, vq as V
    rows = cv.encode_rows_on_device([w for w in cv._wav_features(wavs, 16000, dev)[0]], tr, hps.seg_len)
    cb = V.fit_vectors(torch.cat(rows).contiguous(), 1024, iters=5)
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
    out['convert_wavs'].update(utts=args.utts, n_iter=args.n_iter, rows=int(sum(len(u) for u in rows)), fit_history=cb.meta['history'],
                               K1024_minus_off_ms=round(statistics.median(ms['K1024']) - statistics.median(ms['off']), 3))


def _verdict(rec, new):
    rec['new_minus_parent_ms'] = round(rec[new]['median_ms'] - rec['parent']['median_ms'], 3)
    rec['larger_spread_ms'] = max(rec[new]['spread_ms'], rec['parent']['spread_ms'])
    rec['unchanged'] = rec['new_minus_parent_ms'] <= rec['larger_spread_ms']
    return rec


def bench_against_parent(args, out):
    """bench.py --gpus 1 --steps 20 --warmup 5 in each tree, a fresh process per run, alternating."""
    builds = [('parent', os.path.abspath(args.parent)), ('new', HERE)]
    env = dict(os.environ)
    env.pop('ZS_LIB_PATH', None)
    ms = {n: [] for n, _ in builds}
    for r in range(-1, args.rounds):
        for name, tree in builds[r % 2:] + builds[:r % 2]:
            txt = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5'], cwd=tree,
                                 env=env, stdout=subprocess.PIPE, text=True, check=True).stdout
            rec = json.loads([ln for ln in txt.splitlines() if ln.startswith('{')][-1])
            step = rec.get('step_ms', rec.get('ms_per_step'))
            if step is None:
                raise RuntimeError('bench.py printed no step time: %s' % sorted(rec))
            print('[vq_bench] bench.py round %d %s: %.3f ms/step' % (r, name, float(step)), file=sys.stderr, flush=True)
            if r >= 0:
                ms[name].append(float(step))
    out['bench_vs_parent'] = _verdict({n: _stats(v) for n, v in ms.items()}, 'new')


def convert_against_parent(args, out):
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
    out['convert_wavs_off_vs_parent'] = _verdict({n: _stats(ms[n]) for n in names}, 'off')


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent', default=None, help='a built tree of the parent commit (its own package and libzs_amd.so)')
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--utts', type=int, default=64)
    p.add_argument('--n-iter', type=int, default=300, dest='n_iter')
    p.add_argument('--dtype', default='bf16')
    p.add_argument('--out', default=os.path.join(HERE, 'profiles', 'vq_bench.json'))
    p.add_argument('--sweep', default=False, action='store_true', help='only the sweep of both assign decompositions below the threshold')
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
        sys.exit('vq_bench needs an MI355X: a timing taken anywhere else says nothing about it')
    import zs_amd  # noqa: F401
    if args.sweep:
        return sweep(os.path.join(HERE, 'profiles', 'vq_split_sweep.json'))
    out = {'device': torch.cuda.get_device_name(0), 'dtype': args.dtype, 'rounds': args.rounds,
           'order': 'warm-up, one uncounted alternating round, then alternating rounds, order rotated per round; one GPU job'}
    if args.parent is not None:                                   # first, while this process holds no GPU memory
        bench_against_parent(args, out)
        convert_against_parent(args, out)
    for part in (kernels, convert_with_and_without):
        print('[vq_bench] %s' % part.__name__, file=sys.stderr, flush=True)
        part(args, out)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
