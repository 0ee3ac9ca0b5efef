"""What overlapped decode windows cost, in one GPU job:
  kernel    zs_xfade_gather alone at the config-4 shape (64 utterances of 200-700 frames, overlap 32 of seg_len 128): HIP events around
            a replayed graph of launches, beside the bytes it moves, a device-to-device copy of the same bytes, and the
            `table[idx].float()` gather it stands in for
  synth     synth_units_batch and resynth_batch at overlap 0, 16, 32 and 64 on that workload, alternating
  joins     a report, never a bar: mean |frame[t + 1] - frame[t]| of the spectrogram where overlap 0 cuts against the same figure at the other
            unit edges, at overlap 0 and 32 -- on UNTRAINED nets (there is no trained checkpoint beside this tool)
  parent    (--parent DIR, a built tree of the parent commit) `bench.py --gpus 1 --steps 20 --warmup 5` and `bench.py --mode resynth` (both without the host baseline),
            this build against the parent's, a fresh process per run, alternating: neither launches anything new
    python tools/overlap_bench.py [--parent DIR] [--rounds 5] [--n-iter 60] [--out profiles/overlap_bench.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG, OVERLAPS = 128, (0, 16, 32, 64)


def _summary(v):
    """median (min - max), as the measuring guide asks for."""
    return {'values': [round(x, 3) for x in v], 'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}


def _timed(fn):
    import time
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _events(fn, reps=9, per=1):
    import torch
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / per)
    return us


def _graphed(launch, calls):
    import torch
    launch()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            launch()
    g.replay()
    return _events(g.replay, per=calls)


def _frames(n_utt):
    import numpy as np
    return [int(n) for n in np.random.RandomState(4).randint(200, 701, n_utt)]      # config 4: 64 utterances of 200-700 frames


def kernel(args, out):
    import numpy as np
    import torch
    from zs_amd import _lib as L, convert as cv
    dev = torch.device('cuda:0')
    units = [cv._t8(n) for n in _frames(args.utts)]
    items = [it for u, n in enumerate(units) for it in cv._window_items(u, n, SEG, 32)]
    chunks = cv._split_chunks(items, SEG // 8, 256)
    first, total = [], 0
    for chunk, _ in chunks:                                           # the decoded chunks laid end to end, as _enqueue_synth lays them
        ld = 8 * max(it.n for it in chunk)
        first += [total + i * ld for i in range(len(chunk))]
        total += len(chunk) * ld
    Tm, ulens, i0, i1, w0, w1 = cv._xfade_tables(chunks, first, len(units))
    rows = len(units) * Tm
    src = torch.rand(total, 513, device=dev)
    t = torch.empty(rows, 513, device=dev)
    tab = [torch.from_numpy(a).to(dev) for a in (i0, i1, w0, w1)]
    st = lambda: torch.cuda.current_stream().cuda_stream             # read at launch time: a capture runs on a stream of its own
    single, blended, padding = int(((i0 >= 0) & (i1 < 0)).sum()), int((i1 >= 0).sum()), int((i0 < 0).sum())
    moved = 4 * 513 * (single * 2 + blended * 3 + padding) + 16 * rows            # row reads and writes, and the four table entries
    rec = {'utterances': len(units), 'T_max': Tm, 'rows': rows, 'src_rows': total, 'rows_single': single, 'rows_blended': blended,
           'rows_padding': padding, 'bytes_moved': moved}
    for name, denorm in (('denorm0', 0), ('denorm1', 1)):
        launch = lambda: L.call('zs_xfade_gather', 'ZsXfadeGather', st(), src=L.ptr(src), src_rows=total, ld_src=513, i0=L.ptr(tab[0]),
                                i1=L.ptr(tab[1]), w0=L.ptr(tab[2]), w1=L.ptr(tab[3]), out=L.ptr(t), rows=rows, out_ld=513, cols=513,
                                denorm=denorm)
        us = _graphed(launch, 10)
        rec[name] = dict(_summary(us), unit='us', tb_per_s=round(moved / (statistics.median(us) * 1e-6) / 1e12, 3))
    a, b = torch.empty(moved // 8, device=dev), torch.empty(moved // 8, device=dev)      # a copy that reads and writes `moved` bytes in all
    us = _graphed(lambda: b.copy_(a), 10)
    rec['d2d_copy_same_bytes'] = dict(_summary(us), unit='us', tb_per_s=round(moved / (statistics.median(us) * 1e-6) / 1e12, 3))
    # the gather it stands in for: the cut layout of the same utterances through _gather_index's table and torch's index kernel
    cut = cv._split_chunks([it for u, n in enumerate(units) for it in cv._unit_items(u, n, SEG)], SEG // 8, 256)
    shapes = [(len(c), 8 * max(it.n for it in c)) for c, _ in cut]
    idx, _, zero = cv._gather_index(cut, [[8 * it.n for it in c] for c, _ in cut], shapes, len(units))
    table = torch.rand(zero + 1, 513, device=dev)
    idx_d = torch.from_numpy(idx).to(dev)
    us = _graphed(lambda: table[idx_d].float(), 10)
    rec['torch_index_gather_cut_layout'] = dict(_summary(us), unit='us', rows=int(idx.size))
    out['zs_xfade_gather'] = rec


def _trainer(dtype):
    import torch
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    hps = make_hps(enc_size=1024, emb_size=1024, n_speakers=102)
    torch.manual_seed(0)
    return Trainer(hps, None, 'naive', 'multilabel_binary', log_dir=tempfile.mkdtemp(), dtype=dtype, device=torch.device('cuda:0')), hps


def synth(args, out):
    import numpy as np
    from zs_amd import convert as cv
    tr, hps = _trainer(args.dtype)
    rng = np.random.RandomState(5)
    specs = [(rng.rand(n, 513) * 0.98 + 1e-3).astype(np.float32) for n in _frames(args.utts)]
    spk = [100 + (i % 2) for i in range(args.utts)]
    units, _ = cv.encode_batch(specs, tr, hps.seg_len, packed=True)
    Lu = hps.seg_len // 8
    out['expected_decode_growth'] = {str(v): round(Lu / float(Lu - v // 8), 3) for v in OVERLAPS}
    out['decoded_unit_rows'] = {str(v): int(sum(b - a for u in units for a, b in cv.unit_windows(len(u), hps.seg_len, v))) for v in OVERLAPS}
    runs = {}
    for v in OVERLAPS:
        kw = {'overlap': v} if v else {}
        runs['synth_units_batch/%d' % v] = lambda kw=kw: cv.synth_units_batch(units, tr, hps.seg_len, spk, n_iter=args.n_iter, packed=True, **kw)
        runs['resynth_batch/%d' % v] = lambda kw=kw: cv.resynth_batch(specs, tr, hps.seg_len, spk, n_iter=args.n_iter, **kw)
        runs['decode_only/%d' % v] = lambda kw=kw: cv.synth_units_batch(units, tr, hps.seg_len, spk, n_iter=1, do_trim=False, packed=True, **kw)
    names = list(runs)
    for fn in runs.values():
        fn()
    ms = {k: [] for k in names}
    for r in range(-1, args.rounds):                              # round -1 alternates as the others do and is not counted
        for k in names[r % len(names):] + names[:r % len(names)]:
            t = _timed(runs[k])
            if r >= 0:
                ms[k].append(t)
    out['batches_ms'] = {k: dict(_summary(v), unit='ms') for k, v in ms.items()}
    out['batches_ms'].update(utts=args.utts, n_iter=args.n_iter, dtype=args.dtype,
                             note='decode_only: the same call with n_iter = 1 and no trim, the share that is expected to grow by Lu / Hu')
    # the joins, on untrained nets: a report
    joins = {}
    for v in (0, 32):
        s, _ = cv.synth_units_batch(units, tr, hps.seg_len, spk, n_iter=1, do_trim=False, packed=True, want_specs=True,
                                    **({'overlap': v} if v else {}))
        at, away = [], []
        for u, sp in zip(units, s):
            d = np.abs(np.diff(sp.astype(np.float64), axis=0)).mean(axis=1)            # d[t]: frame t + 1 against frame t
            cuts = [8 * b - 1 for a, b in cv.unit_windows(len(u), hps.seg_len, 0)[:-1]]  # where overlap 0 lays two pieces end to end
            mask = np.zeros(len(d), dtype=bool)
            mask[cuts] = True
            at += d[mask].tolist()
            unit_edge = (np.arange(len(d)) % 8) == 7                   # a cut is always the edge of a unit: compare with the other unit edges
            away += d[unit_edge & ~mask].tolist()
        joins[str(v)] = {'mean_abs_step_at_the_cuts_of_overlap_0': round(float(np.mean(at)), 6), 'mean_abs_step_at_the_other_unit_edges': round(float(np.mean(away)), 6),
                         'cuts': len(at)}
    joins['note'] = 'measured on UNTRAINED nets with random units: a figure about the joins of the spectrogram, not about what speech sounds like'
    out['joins'] = joins


def bench_against_parent(args, out):
    builds = [('parent', os.path.abspath(args.parent)), ('new', HERE)]
    env = dict(os.environ)
    env.pop('ZS_LIB_PATH', None)
    quick = ['--no-cpu-baseline', '--no-secondary']                # the GPU figure alone: the host baseline and the second workload are not what is compared
    for key, extra in (('bench_train_ae', quick), ('bench_resynth', ['--mode', 'resynth'] + quick)):
        vals = {n: [] for n, _ in builds}
        for r in range(-1, args.rounds):
            for name, tree in builds[r % 2:] + builds[:r % 2]:
                txt = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5'] + extra,
                                     cwd=tree, env=env, stdout=subprocess.PIPE, text=True, check=True).stdout
                rec = json.loads([ln for ln in txt.splitlines() if ln.startswith('{')][-1])
                val = rec['value']
                print('[overlap_bench] %s round %d %s: %s' % (key, r, name, val), file=sys.stderr, flush=True)
                if r >= 0:
                    vals[name].append(float(val))
        res = {n: _summary(v) for n, v in vals.items()}
        res['ranges_overlap'] = res['new']['min'] <= res['parent']['max'] and res['parent']['min'] <= res['new']['max']
        res['unit'] = rec['unit'] + ' (higher is better)'
        out[key] = res


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent', default=None, help='a built tree of the parent commit (its own package and libzs_amd.so)')
    p.add_argument('--rounds', type=int, default=5)
    p.add_argument('--utts', type=int, default=64)
    p.add_argument('--n-iter', type=int, default=60, dest='n_iter')
    p.add_argument('--dtype', default='bf16')
    p.add_argument('--out', default=os.path.join(HERE, 'profiles', 'overlap_bench.json'))
    args = p.parse_args()
    if args.rounds < 3:
        p.error('--rounds must be at least 3')
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        sys.exit('overlap_bench needs an MI355X: a timing taken anywhere else says nothing about it')
    import zs_amd  # noqa: F401
    out = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds,
           'order': 'warm-up, one uncounted alternating round, then alternating rounds, order rotated per round; one GPU job; median (min - max)'}
    if args.parent is not None:                                   # first, while this process holds no GPU memory
        bench_against_parent(args, out)
    for part in (kernel, synth):
        print('[overlap_bench] %s' % part.__name__, file=sys.stderr, flush=True)
        part(args, out)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
