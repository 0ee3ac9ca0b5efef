"""What --segment costs, in one GPU job:
  kernels   zs_vq_scores beside zs_vq_assign at the same shape (it is that kernel plus n x K x 4 bytes of stores), zs_code_scores
            beside zs_code_assign, each with the bytes it writes: HIP events around a replayed graph of launches
  viterbi   zs_seg_viterbi in microseconds per frame at K = 64, 1024 and 4096, for 64 utterances of 25 - 88 units and for one
            utterance of 20 000 units, at lambda 0 (a run per frame: the walk back at its worst) and at a lambda that joins frames
  convert   convert_wavs under a vector and under a bit codebook at segment None and 1.0, alternating
  rate      a report, never a bar: segments per second and the mean distance at a few lambda -- on UNTRAINED nets with random data
  parent    (--parent DIR, a built tree of the parent commit) `bench.py --gpus 1 --steps 20 --warmup 5` and `bench.py --mode resynth`,
            this build against the parent's, a fresh process per run, alternating: neither launches anything new
    python tools/segment_bench.py [--parent DIR] [--rounds 5] [--out profiles/segment_bench.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def kernels(args, out):
    import numpy as np
    import torch
    from zs_amd import _lib as L, codebook as C, vq as V
    dev = torch.device('cuda:0')
    st = lambda: torch.cuda.current_stream().cuda_stream             # read at launch time: a capture runs on a stream of its own
    rs = np.random.RandomState(0)
    rec = {}
    for n, K, E in ((16384, 1024, 1024), (4096, 64, 128), (65536, 256, 128)):
        x = torch.from_numpy(rs.standard_normal((n, E)).astype(np.float32)).to(dev)
        code = torch.from_numpy(rs.standard_normal((K, E)).astype(np.float32)).to(dev)
        cn = (code.double() ** 2).sum(1).float()
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        scores = torch.empty(n, K, dtype=torch.float32, device=dev)
        a = _graphed(lambda: V.launch_assign(st(), L.ZS_F32, L.ptr(x), n, E, code, cn, idx=idx), 10)
        s = _graphed(lambda: V.launch_scores(st(), L.ZS_F32, L.ptr(x), n, E, code, cn, L.ptr(scores), K), 10)
        med = statistics.median(s)
        rec['vq n%d K%d E%d' % (n, K, E)] = {
            'zs_vq_assign_rows_us': _summary(a), 'zs_vq_scores_us': _summary(s), 'bytes_written': 4 * n * K,
            'write_gb_per_s_of_the_whole_kernel': round(4 * n * K / (med * 1e-6) / 1e9, 1),
            'zs_vq_assign_workgroups': (n + 127) // 128, 'zs_vq_scores_workgroups': ((n + 127) // 128) * ((K + 127) // 128),
            'ratio': round(med / statistics.median(a), 3)}
    for n, K, E in ((16384, 1024, 1024), (4096, 64, 128)):
        nb = (E + 7) // 8
        units = torch.from_numpy(rs.randint(0, 256, size=(n, nb)).astype(np.uint8)).to(dev)
        code = torch.from_numpy(rs.randint(0, 256, size=(K, nb)).astype(np.uint8)).to(dev)
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        scores = torch.empty(n, K, dtype=torch.float32, device=dev)
        a = _graphed(lambda: C.assign(units, code, E, idx=idx), 10)
        s = _graphed(lambda: L.call('zs_code_scores', 'ZsCodeScores', st(), units=L.ptr(units), n=n, row_bytes=nb, code=L.ptr(code), K=K,
                                    code_bytes=nb, E=E, scores=L.ptr(scores), ld_s=K), 10)
        rec['code n%d K%d E%d' % (n, K, E)] = {
            'zs_code_assign_us': _summary(a), 'zs_code_scores_us': _summary(s), 'bytes_written': 4 * n * K,
            'write_gb_per_s_of_the_whole_kernel': round(4 * n * K / (statistics.median(s) * 1e-6) / 1e9, 1),
            'ratio': round(statistics.median(s) / statistics.median(a), 3)}
    out['score_kernels'] = rec


def viterbi(args, out):
    import numpy as np
    import torch
    from zs_amd import _lib as L, segment as S
    dev = torch.device('cuda:0')
    st = lambda: torch.cuda.current_stream().cuda_stream
    rs = np.random.RandomState(1)
    rec = {}
    for name, lens in (('64 utterances of 25 - 88 units', [int(v) for v in rs.randint(25, 89, 64)]), ('1 utterance of 20000 units', [20000])):
        n = sum(lens)
        uoffs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
        for K in (64, 1024, 4096):
            # scores with structure: a slowly moving best codeword plus noise, so that a lambda joins frames
            best = np.repeat(rs.randint(0, K, n // 5 + 1), 5)[:n]
            s = rs.standard_normal((n, K)).astype(np.float32) ** 2 * 4.0
            s[np.arange(n), best] *= 0.05
            s_d = torch.from_numpy(s).to(dev)
            idx = torch.empty(n, dtype=torch.int32, device=dev)
            n_seg = torch.empty(len(lens), dtype=torch.int32, device=dev)
            cost = torch.empty(len(lens), dtype=torch.float64, device=dev)
            bad = torch.zeros(1, dtype=torch.int32, device=dev)
            work = torch.empty((S.work_bytes(n, K) + 7) // 8, dtype=torch.int64, device=dev)
            for lam in (0.0, 2.0):
                launch = lambda: L.call('zs_seg_viterbi', 'ZsSegViterbi', st(), scores=L.ptr(s_d), n_rows=n, ld_s=K, uoffs=L.ptr(uoffs),
                                        n_utt=len(lens), n_units=n, lam=lam, K=K, work=L.ptr(work), work_bytes=work.numel() * 8,
                                        idx=L.ptr(idx), n_seg=L.ptr(n_seg), cost=L.ptr(cost), bad=L.ptr(bad))
                us = _graphed(launch, 4)
                rec['%s, K %d, lambda %g' % (name, K, lam)] = {
                    'us': _summary(us), 'frames': n, 'longest': max(lens), 'segments': int(n_seg.sum().item()),
                    'us_per_frame_of_the_batch': round(statistics.median(us) / n, 4),
                    'us_per_frame_of_the_longest_utterance': round(statistics.median(us) / max(lens), 4),
                    'score_bytes_read': 4 * n * K}
    out['zs_seg_viterbi'] = rec


def _trainer(enc_mode, dtype):
    import torch
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    hps = make_hps(enc_size=128, emb_size=128, n_speakers=102)
    torch.manual_seed(0)
    return Trainer(hps, None, 'naive', enc_mode, log_dir=tempfile.mkdtemp(), dtype=dtype, device=torch.device('cuda:0')), hps


def convert(args, out):
    import numpy as np
    import torch
    from zs_amd import codebook as C, convert as cv, segment as S, vq
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(5)
    wavs = [(0.1 * rng.standard_normal(int(n))).astype(np.float32) for n in rng.randint(32000, 112000, args.utts)]     # 2 - 7 s at 16 kHz
    spk = [100 + (i % 2) for i in range(args.utts)]
    res, rate = {}, {}
    for kind, enc_mode in (('vector', 'continues'), ('bit', 'multilabel_binary')):
        tr, hps = _trainer(enc_mode, args.dtype)
        specs, _ = cv._wav_features(wavs, None, dev)
        if kind == 'vector':
            rows = torch.cat(cv.encode_rows_on_device(specs, tr, hps.seg_len)).contiguous()
            cb = vq.fit_vectors(rows, 256, iters=8)
        else:
            e = cv.encode_batch(specs, tr, hps.seg_len, packed=True, units_on_device=True)[0]
            cb = C.fit(torch.cat(e).contiguous(), 256, iters=8, E=128)
        runs = {'%s/segment None' % kind: lambda cb=cb, tr=tr, hps=hps: cv.convert_wavs(wavs, None, tr, hps.seg_len, spk, n_iter=args.n_iter, codebook=cb),
                '%s/segment 1.0' % kind: lambda cb=cb, tr=tr, hps=hps: cv.convert_wavs(wavs, None, tr, hps.seg_len, spk, n_iter=args.n_iter, codebook=cb,
                                                                                     segment=1.0)}
        names = list(runs)
        for fn in runs.values():
            fn()
        ms = {k: [] for k in names}
        for r in range(-1, args.rounds):                              # round -1 alternates as the others do and is not counted
            for k in names[r % 2:] + names[:r % 2]:
                t = _timed(runs[k])
                if r >= 0:
                    ms[k].append(t)
        res.update({k: dict(_summary(v), unit='ms') for k, v in ms.items()})
        # the mechanism on untrained nets: segments per second and the mean distance along lambda
        secs = None
        lams = (0.0, 0.5, 1.0, 2.0, 4.0, 16.0) if kind == 'bit' else None
        if lams is None:                                              # in units of the median nearest-codeword distance
            _, _, _, tot = cv.resynth_batch(specs[:8], tr, hps.seg_len, spk[:8], n_iter=1, do_trim=False, codebook=cb, want_idx=True)
            n8 = sum(cv._unit_counts(specs[:8], hps.seg_len))
            lams = tuple(round(f * tot / n8, 6) for f in (0.0, 0.25, 0.5, 1.0, 2.0, 8.0))
        for lam in lams:
            _, _, idx, tot = cv.resynth_batch(specs, tr, hps.seg_len, spk, n_iter=1, do_trim=False, codebook=cb, want_idx=True, segment=lam)
            units = sum(len(i) for i in idx)
            segs = sum(len(S.runs(i)) for i in idx)
            secs = units * S.seconds_per_unit()
            rate['%s/lambda %g' % (kind, lam)] = {'units_per_s': round(units / secs, 3), 'segments_per_s': round(segs / secs, 3),
                                                 'mean_distance': round(float(tot) / units, 6)}
        del tr
        torch.cuda.empty_cache()
    res.update(utts=args.utts, n_iter=args.n_iter, dtype=args.dtype, K=256, E=128)
    out['convert_wavs_ms'] = res
    rate['note'] = ('UNTRAINED nets on noise: a statement about the mechanism (lambda trades segments for distance), not about speech; lambda of '
                    'the vector kind is a multiple of the mean nearest-codeword distance')
    out['rate_distortion_untrained'] = rate


def bench_against_parent(args, out):
    builds = [('parent', os.path.abspath(args.parent)), ('new', HERE)]
    env = dict(os.environ)
    env.pop('ZS_LIB_PATH', None)
    quick = ['--no-cpu-baseline', '--no-secondary']                # the GPU figure alone
    for key, extra in (('bench_train_ae', quick), ('bench_resynth', ['--mode', 'resynth'] + quick)):
        vals = {n: [] for n, _ in builds}
        for r in range(-1, args.rounds):
            for name, tree in builds[r % 2:] + builds[:r % 2]:
                txt = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5'] + extra,
                                     cwd=tree, env=env, stdout=subprocess.PIPE, text=True, check=True).stdout
                rec = json.loads([ln for ln in txt.splitlines() if ln.startswith('{')][-1])
                val = rec['value']
                print('[segment_bench] %s round %d %s: %s' % (key, r, name, val), file=sys.stderr, flush=True)
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
    p.add_argument('--only', default=None, help='comma-separated parts: parent, kernels, viterbi, convert')
    p.add_argument('--out', default=os.path.join(HERE, 'profiles', 'segment_bench.json'))
    args = p.parse_args()
    if args.rounds < 3:
        p.error('--rounds must be at least 3')
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        sys.exit('segment_bench needs an MI355X: a timing taken anywhere else says nothing about it')
    import zs_amd  # noqa: F401
    only = set(args.only.split(',')) if args.only else None
    out = {'device': torch.cuda.get_device_name(0), 'rounds': args.rounds,
           'order': 'warm-up, one uncounted alternating round, then alternating rounds, order rotated per round; one GPU job; median (min - max)'}
    if args.parent is not None and (only is None or 'parent' in only):       # first, while this process holds no GPU memory
        bench_against_parent(args, out)
    for part in (kernels, viterbi, convert):
        if only is None or part.__name__ in only:
            print('[segment_bench] %s' % part.__name__, file=sys.stderr, flush=True)
            part(args, out)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
