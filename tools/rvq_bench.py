"""What the residual vector codebook costs, in one GPU job on one MI355X, bf16, K = E = 1024:
  launches  zs_rvq_residual and zs_rvq_gather alone, each at one inference chunk (256 x 16 rows) and at the fit's shape (2^20 rows): HIP
            events around a replayed graph of launches, median with min and max, beside the bytes each must move -- residual
            n E (in + 4 + 4), gather rows (s_use E 4 + ld elt) -- and zs_vq_assign at the same shapes, the search the glue sits around
  fit       one stage of fit_residual at 2^20 rows beyond its k-means: the assignment under the fitted codebook and the residual
  convert   convert_wavs of a 'continues' model on the workload of tools/convert_dir_bench.py at 16 kHz with no codebook, a vector
            codebook and a residual one at S = 2 and 4, alternating
  parent    (--parent DIR, a built tree of the parent commit) the paths that launch nothing new, this build against the parent's,
            alternating round by round: `bench.py --gpus 1 --steps 20 --warmup 5` (one process per run) and convert_wavs without a
            codebook (one worker process each).  The bar: the two ranges overlap
    python tools/rvq_bench.py [--parent DIR] [--rounds 3] [--utts 64] [--n-iter 300] [--out profiles/rvq_bench.json]"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, 'tools'))

from codebook_bench import _timed  # noqa: E402
from vq_bench import _workload, bench_against_parent, convert_against_parent, convert_worker  # noqa: E402  (the workload and the parent runs)


def _mmm(v, unit, digits=2):
    return {'median_' + unit: round(statistics.median(v), digits), 'min_' + unit: round(min(v), digits), 'max_' + unit: round(max(v), digits)}


def _replayed(launch, calls, reps=9):
    """us per launch: `calls` launches captured in one graph, replayed `reps` times between HIP events."""
    import torch
    launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(calls):
            launch()
    graph.replay()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / calls)
    return us


def launches(args, out):
    import torch
    from zs_amd import rvq as Q, vq as V
    dev = torch.device('cuda:0')
    E, K, S = 1024, 1024, 4
    g = torch.Generator().manual_seed(0)
    code = torch.randn(S, K, E, generator=g).to(dev)
    cnorm = (code.double() ** 2).sum(2).float()
    out['launches'] = {}
    for name, n, calls, dt in (('chunk_256x16_bf16', 256 * 16, 40, torch.bfloat16), ('n_2p20_fp32', 1 << 20, 2, torch.float32)):
        x = torch.randn(n, E, device=dev).to(dt)
        idx = torch.randint(0, K, (S, n), generator=g).int().to(dev)
        dist = torch.empty(n, dtype=torch.float32, device=dev)
        r = torch.empty(n, E, dtype=torch.float32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        rec = {'n': n, 'K': K, 'E': E, 'dtype': str(dt), 'launches_per_replay': calls}
        work = V.workspace(dev) if n < V.SPLIT_N else None
        for what, src, fn in (('residual_first', x, lambda: Q.residual(x, idx[0], code[0], r, bad)),
                              ('residual_in_place', r, lambda: Q.residual(r, idx[1], code[1], r, bad)),
                              ('assign', x, lambda: V.assign(x, code[0], cnorm[0], idx=idx[2], dist=dist, work=work))):
            us = _replayed(fn, calls)
            rec[what] = _mmm(us, 'us')
            if what != 'assign':
                nbytes = n * E * (src.element_size() + 4 + 4)
                rec[what].update(bytes=nbytes, tb_per_s=round(nbytes / (statistics.median(us) * 1e-6) / 1e12, 3))
        del x, r
        if n == 256 * 16:                                            # the operand of one inference chunk: 256 fragments of 16 frames
            start = (torch.arange(256, dtype=torch.int64) * 16).to(dev)
            length = torch.full((256,), 16, dtype=torch.int32, device=dev)
            dst = torch.empty(256, 16, E, dtype=torch.bfloat16, device=dev)
            i1 = idx[0].contiguous()
            us = _replayed(lambda: V.gather(i1, code[0], start, length, 16, dst, bad), calls)
            rec['vq_gather'] = dict(_mmm(us, 'us'), bytes=n * (E * 4 + E * 2))
            for s_use in (1, 2, 4):
                us = _replayed(lambda: Q.gather(idx, s_use, code, start, length, 16, dst, bad), calls)
                nbytes = n * (s_use * E * 4 + E * 2)
                rec['gather_s%d' % s_use] = dict(_mmm(us, 'us'), bytes=nbytes, tb_per_s=round(nbytes / (statistics.median(us) * 1e-6) / 1e12, 3))
        else:                                                        # what a fit stage adds to its k-means at this size, by the host clock
            cb = V.VectorCodebook(code[0].cpu().numpy())
            x = torch.randn(n, E, device=dev)
            r = torch.empty(n, E, dtype=torch.float32, device=dev)

            def stage_tail():
                i, _ = cb.snap(x)
                Q.residual(x, i, cb.to(dev)[0], r, bad)
            stage_tail()
            out['fit_stage_tail'] = dict(_mmm([_timed(stage_tail) for _ in range(5)], 'ms', 3), n=n, K=K, E=E,
                                         note='the assignment under the fitted codebook and the residual; the k-means before it is '
                                              "vq_bench's fit_iteration per iteration")
            del x, r
        out['launches'][name] = rec


def convert_kinds(args, out):
    import torch
    dev, hps, tr, wavs, spk = _workload(args, HERE)
    from zs_amd import convert as cv, rvq as Q, vq as V
    rows = torch.cat(cv.encode_rows_on_device([w for w in cv._wav_features(wavs, 16000, dev)[0]], tr, hps.seg_len)).contiguous()
    cbs = {'off': None, 'vector_K1024': V.fit_vectors(rows, 1024, iters=3)}
    full = Q.fit_residual(rows, 1024, 4, iters=3)
    cbs.update(residual_S2=full.with_stages(2), residual_S4=full)
    runs = {k: (lambda c=c: cv.convert_wavs(wavs, 16000, tr, hps.seg_len, spk, n_iter=args.n_iter, codebook=c)) for k, c in cbs.items()}
    for fn in runs.values():
        fn()
        fn()
    names, ms = list(runs), {k: [] for k in runs}
    for r in range(-1, max(args.rounds, 5)):                      # round -1 rotates as the others do and is not counted
        for k in names[r % len(names):] + names[:r % len(names)]:
            t = _timed(runs[k])
            if r >= 0:
                ms[k].append(t)
    out['convert_wavs'] = {k: _mmm(v, 'ms', 3) for k, v in ms.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    out['convert_wavs'].update(utts=args.utts, n_iter=args.n_iter, rows=int(rows.shape[0]), stages=full.meta['stages'],
                               minus_off_ms={k: round(med[k] - med['off'], 3) for k in names if k != 'off'})


def _ranges(rec, new):
    """min / max beside vq_bench's median and spread, and the bar: the two ranges overlap."""
    for k in (new, 'parent'):
        rec[k].update(min_ms=min(rec[k]['ms']), max_ms=max(rec[k]['ms']))
    rec['ranges_overlap'] = rec[new]['min_ms'] <= rec['parent']['max_ms'] and rec['parent']['min_ms'] <= rec[new]['max_ms']
    return rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent', default=None, help='a built tree of the parent commit (its own package and libzs_amd.so)')
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--utts', type=int, default=64)
    p.add_argument('--n-iter', type=int, default=300, dest='n_iter')
    p.add_argument('--dtype', default='bf16')
    p.add_argument('--out', default=os.path.join(HERE, 'profiles', 'rvq_bench.json'))
    p.add_argument('--worker', default=False, action='store_true', help=argparse.SUPPRESS)
    p.add_argument('--tree', default=HERE, help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.worker:
        return convert_worker(args)
    if args.rounds < 3:
        p.error('--rounds must be at least 3')
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        sys.exit('rvq_bench needs an MI355X: a timing taken anywhere else says nothing about it')
    import zs_amd  # noqa: F401
    out = {'device': torch.cuda.get_device_name(0), 'dtype': args.dtype, 'rounds': args.rounds,
           'order': 'warm-up, one uncounted alternating round, then alternating rounds, order rotated per round; one GPU job'}
    if args.parent is not None:                                   # first, while this process holds no GPU memory
        bench_against_parent(args, out)
        convert_against_parent(args, out)
        _ranges(out['bench_vs_parent'], 'new')
        _ranges(out['convert_wavs_off_vs_parent'], 'off')
    for part in (launches, convert_kinds):
        print('[rvq_bench] %s' % part.__name__, file=sys.stderr, flush=True)
        part(args, out)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
