"""What --score_units costs, in one GPU job:
  dtw       zs_abx_dtw on every unordered pair of the tokens of one score tile of 2048 frames, at the length mixes 1..4, 1..16 and
            32..64 and E = 64 and 1024, bucketed by W as the planner emits them: pairs per second, bytes of S per second (4 La Lb per
            pair, against 6.29 TB/s, what a copy reaches of the card's HBM), the lanes that hold a column and the cell-steps that do
            work, with __shfl_up and with the DPP shift; the score kernel of the tile beside it; hamming and angular
  count     zs_abx_count in comparisons per second on sets of 500 and on sets of 4
  numpy     the float32 reference of tests/abx_ref.py in pairs per second on this host, for scale only
  run       a synthetic whole run: random bit units, 20 contexts x 4 speakers x 8 phones x 3 tokens of 1..8 rows, plan and driver
  parent    (--parent DIR, a built tree of the parent commit) `bench.py --gpus 1 --steps 20 --warmup 5`, this build against the
            parent's, a fresh process per run, alternating: the scoring path launches nothing there
    python tools/abx_bench.py [--parent DIR] [--rounds 5] [--out profiles/abx_bench.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 6.29e12                                          # MI355X HBM3E, measured with a float4 copy (8.0e12 is the spec)


def _summary(v):
    """median (min - max), as the measuring guide asks for."""
    return {'values': [round(x, 3) for x in v], 'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}


def _events(fn, reps=7):
    import torch
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return us


def _tile_tokens(rs, lo, hi, frames):
    import numpy as np
    lens = []
    while sum(lens) + hi <= frames:
        lens.append(int(rs.randint(lo, hi + 1)))
    return np.asarray(lens, dtype=np.int64)


def _utilisation(buckets):
    """(lanes that hold a column / lanes of the waves launched, cells / lane-steps of the sweeps) over the buckets of a tile."""
    import numpy as np
    lanes = held = cells = lane_steps = 0
    for W, rec in buckets.items():
        per = 64 // W
        n_waves = (rec.size + per - 1) // per
        lanes += 64 * n_waves
        held += int(rec['Lb'].sum())
        cells += int((rec['La'].astype(np.int64) * rec['Lb']).sum())
        slabs = (rec['La'] + 15) // 16                              # a record is swept in slabs of 16 rows, Lb - 1 idle steps each
        steps = rec['La'] + slabs * (rec['Lb'] - 1)
        pad = np.concatenate([steps, np.zeros(n_waves * per - rec.size, dtype=steps.dtype)]).reshape(n_waves, per)
        lane_steps += 64 * int(pad.max(1).sum())
    return held / lanes, cells / lane_steps


def dtw(args, out):
    import numpy as np
    import torch
    from zs_amd import abx
    dev = torch.device('cuda:0')
    res = {}
    for lo, hi in ((1, 4), (1, 16), (32, 64)):
        rs = np.random.RandomState(hi)
        lens = _tile_tokens(rs, lo, hi, args.frames)
        blk = abx.Block(0, np.arange(lens.size), lens)
        blk.chunks = [(0, blk.n)]
        buckets = blk.tile_pairs(0, 0)
        n_pairs = sum(r.size for r in buckets.values())
        s_bytes = 4 * sum(int((r['La'].astype(np.int64) * r['Lb']).sum()) for r in buckets.values())
        held, work = _utilisation(buckets)
        recs = {W: abx.to_device(r, dev) for W, r in buckets.items()}
        D = torch.empty(blk.n * blk.n, dtype=torch.float32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        F = blk.frames
        for E in (64, 1024):
            bits = torch.from_numpy(rs.randint(0, 256, size=(F, E // 8)).astype(np.uint8)).to(dev)
            x = torch.from_numpy(rs.standard_normal((F, E)).astype(np.float32)).to(dev)
            S = torch.empty(F, F, dtype=torch.float32, device=dev)
            zero = torch.zeros(F, dtype=torch.float32, device=dev)
            entry = {'tokens': blk.n, 'frames': F, 'pairs': n_pairs, 'bytes_of_S_read': s_bytes, 'buckets': {str(W): int(r.size) for W, r in buckets.items()},
                     'lanes_holding_a_column': round(held, 4), 'cell_steps_doing_work': round(work, 4)}
            for metric in ('hamming', 'angular'):
                rows = bits if metric == 'hamming' else x
                rinv = abx.rownorm(x) if metric == 'angular' else None
                entry['scores_%s_us' % metric] = _summary(_events(lambda: abx.scores_tile(rows, rows, S, metric, E, zero)))
                for dpp in (0, 1):
                    def launch():
                        for W, r in recs.items():
                            abx.dtw(S, F, r, D, bad, metric, E, width=W, rinv_row=rinv, rinv_col=rinv, dpp=dpp)
                    us = _events(launch)
                    med = statistics.median(us)
                    entry['%s_%s' % (metric, 'dpp' if dpp else 'shfl')] = {
                        'us': _summary(us), 'pairs_per_s': round(n_pairs / med * 1e6), 'bytes_per_s': round(s_bytes / med * 1e6),
                        'fraction_of_hbm': round(s_bytes / med * 1e6 / HBM_BYTES_PER_S, 5)}
            assert int(bad.item()) == 0
            res['len_%d_%d_E%d' % (lo, hi, E)] = entry
            print('[abx_bench] dtw %d..%d E %d: %s' % (lo, hi, E, json.dumps(entry)), file=sys.stderr, flush=True)
    out['dtw'] = res


def count(args, out):
    import numpy as np
    import torch
    from zs_amd import abx
    dev = torch.device('cuda:0')
    rs = np.random.RandomState(0)
    res = {}
    for name, n, size, n_jobs in (('sets_of_500', 4096, 500, 1 << 14), ('sets_of_4', 4096, 4, 1 << 18)):
        D = torch.from_numpy(rs.standard_normal((n, 4096)).astype(np.float32)).to(dev)
        jobs = np.zeros(n_jobs, dtype=abx.JOB_DTYPE)
        jobs['x'] = rs.randint(0, n, n_jobs)
        jobs['a0'] = rs.randint(0, 2048 - size, n_jobs)
        jobs['b0'] = 2048 + rs.randint(0, 2048 - size, n_jobs)
        jobs['a1'], jobs['b1'], jobs['skip'] = jobs['a0'] + size, jobs['b0'] + size, -1
        jd = abx.to_device(jobs, dev)
        wins = torch.zeros(n_jobs, dtype=torch.int64, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        us = _events(lambda: abx.count(D, 4096, jd, wins, bad))
        comps = n_jobs * size * size
        res[name] = {'jobs': n_jobs, 'comparisons': comps, 'us': _summary(us), 'comparisons_per_s': round(comps / statistics.median(us) * 1e6),
                     'jobs_per_s': round(n_jobs / statistics.median(us) * 1e6)}
    out['count'] = res


def numpy_reference(args, out):
    import numpy as np
    sys.path.insert(0, os.path.join(HERE, 'tests'))
    import abx_ref as R
    rs = np.random.RandomState(0)
    n = 20000
    La, Lb = rs.randint(1, 5, n), rs.randint(1, 5, n)
    G = rs.randint(0, 9, size=(n, 4, 4)).astype(np.float32) / np.float32(8)
    t0 = time.perf_counter()
    R.dtw_batch(G, La, Lb, np.float32)
    dt = time.perf_counter() - t0
    out['numpy_reference'] = {'pairs': n, 'lengths': '1..4', 'seconds': round(dt, 4), 'pairs_per_s': round(n / dt),
                              'cpus': os.cpu_count(), 'note': 'tests/abx_ref.dtw_batch, vectorised over the pairs, one thread: for scale only'}


def run(args, out):
    import numpy as np
    import torch
    from zs_amd import abx
    rs = np.random.RandomState(1)
    E, n_ctx, n_spk, n_ph, per = 64, 20, 4, 8, 3
    ctx, spk, ph = np.meshgrid(np.arange(n_ctx), np.arange(n_spk), np.arange(n_ph), indexing='ij')
    ctx, spk, ph = (np.repeat(a.reshape(-1), per) for a in (ctx, spk, ph))
    lens = rs.randint(1, 9, ctx.size)
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    tokens = abx.Tokens(start, lens, ph, ctx, spk, ['p%d' % k for k in range(n_ph)], [('c%d' % k, 'x') for k in range(n_ctx)],
                        ['s%d' % k for k in range(n_spk)], {})
    rows = rs.randint(0, 256, size=(int(lens.sum()), E // 8)).astype(np.uint8)
    t0 = time.perf_counter()
    plan = abx.plan(tokens)
    t_plan = time.perf_counter() - t0
    secs = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wins = abx.cell_wins(plan, abx.run(plan, rows, 'hamming', E))
        res = abx.aggregate(plan, wins)
        secs.append(time.perf_counter() - t0)
    pairs = sum(b.n * (b.n - 1) // 2 for b in plan.blocks)
    out['synthetic_run'] = {'tokens': len(tokens), 'contexts': n_ctx, 'pairs': pairs, 'jobs': plan.n_jobs, 'triplets': int(plan.cell_n.sum()),
                            'cells': int(plan.cell_n.size), 'plan_seconds': round(t_plan, 3), 'run_seconds_first': round(secs[0], 3),
                            'run_seconds': _summary(secs[1:]), 'triplets_per_s': round(int(plan.cell_n.sum()) / statistics.median(secs[1:])),
                            'errors': {t: round(r['error'], 3) for t, r in res.items()},
                            'note': 'random units: the errors sit at 50 % by construction and say nothing about a model'}


def bench_against_parent(args, out):
    builds = [('parent', os.path.abspath(args.parent)), ('new', HERE)]
    env = dict(os.environ)
    env.pop('ZS_LIB_PATH', None)
    vals = {n: [] for n, _ in builds}
    for r in range(-1, args.rounds):
        for name, tree in builds[r % 2:] + builds[:r % 2]:
            txt = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5',
                                  '--no-cpu-baseline', '--no-secondary'], cwd=tree, env=env, stdout=subprocess.PIPE, text=True, check=True).stdout
            rec = json.loads([ln for ln in txt.splitlines() if ln.startswith('{')][-1])
            print('[abx_bench] bench.py round %d %s: %s' % (r, name, rec['value']), file=sys.stderr, flush=True)
            if r >= 0:
                vals[name].append(float(rec['value']))
    res = {n: _summary(v) for n, v in vals.items()}
    res['ranges_overlap'] = res['new']['min'] <= res['parent']['max'] and res['parent']['min'] <= res['new']['max']
    res['unit'] = rec['unit'] + ' (higher is better)'
    out['bench_train_ae'] = res


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent', default=None, help='a built tree of the parent commit (its own package and libzs_amd.so)')
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--frames', type=int, default=2048, help='frames of the score tile of the dtw part')
    p.add_argument('--only', default=None, help='comma-separated parts: parent, dtw, count, numpy_reference, run')
    p.add_argument('--out', default=os.path.join(HERE, 'profiles', 'abx_bench.json'))
    args = p.parse_args()
    if args.rounds < 3:
        p.error('--rounds must be at least 3')
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        sys.exit('abx_bench needs an MI355X: a timing taken anywhere else says nothing about it')
    import zs_amd  # noqa: F401
    only = set(args.only.split(',')) if args.only else None
    out = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds, 'hbm_bytes_per_s': HBM_BYTES_PER_S,
           'order': 'warm-up, then 7 timed calls between HIP events per figure; bench.py: one uncounted alternating round, then alternating '
                    'rounds, order rotated per round; one GPU job; median (min - max)'}
    if args.parent is not None and (only is None or 'parent' in only):       # first, while this process holds no GPU memory
        bench_against_parent(args, out)
    for part in (dtw, count, numpy_reference, run):
        if only is None or part.__name__ in only:
            print('[abx_bench] %s' % part.__name__, file=sys.stderr, flush=True)
            part(args, out)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
