"""What training through the vector codebook costs, in one GPU job -> profiles/vq_train_step_ms.json:
  step      the replayed AEStep of a 'continues' model at hps/zerospeech_english_1024.json's sizes with and without the bottleneck
            (K = 1024), at B = 16 and B = 256, on speech-like input ('formants') and on uniform noise (on which the assignment
            collapses to one codeword): after the capture, 7 alternating rounds of `--steps` replays each, by the host clock around
            a device synchronise; median / min / max per step; and the bottleneck's own launches alone on the rows of the last step
  kernels   zs_vq_commit, zs_vq_st_bwd, zs_vq_ema, zs_vq_accum and zs_vq_assign alone at those rows (256 and 4096, E = 1024, K = 1024, the
            step's dtype): HIP events around a replayed graph of launches
  parent    (--parent DIR, a built tree of the parent commit) `bench.py --gpus 1 --steps 20 --warmup 5` in each tree, a fresh process
            per run, alternating, three runs each: the headline path launches nothing new, so the two ranges must overlap
    python tools/vq_train_bench.py [--parent DIR] [--rounds 7] [--steps 10] [--dtype bf16] [--out profiles/vq_train_step_ms.json]
With --restart T the same job measures the restart of dead codewords instead -> profiles/vq_restart_step_ms.json:
  step      the replayed step with the bottleneck, without and with restart=T, alternating as above; the figures of the bottleneck
            (used, perplexity, restarts, dead) at the end of those ~100 steps and again after --long steps in all
  kernels   zs_vq_ema alone, zs_vq_restart alone with nothing dead, and with all but one codeword dead (each launch behind a fill that
            makes them dead again; the fill alone is timed beside it)
  parent    as above
    python tools/vq_train_bench.py --restart 0.01 [--decay 0.99] [--long 1000] [--parent DIR]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 1024


def _stats(ms):
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4), 'runs': len(ms)}


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
    return {'median_us': round(us[len(us) // 2], 2), 'min_us': round(us[0], 2), 'max_us': round(us[-1], 2)}


def _batch(kind, B, T, F, g):
    """The step's input [B, T, F] in (0, 1).  'noise': uniform, as --synthetic (on it the encoder's rows are nearly equal and the
    assignment collapses to one codeword, zs_vq_accum's worst case); 'formants': three spectral peaks per sample that glide over
    time on a tilted floor, so that the rows differ as those of speech do."""
    import torch
    if kind == 'noise':
        return torch.rand(B, T, F, generator=g)
    f = torch.arange(F, dtype=torch.float32).view(1, 1, F)
    t = torch.linspace(0.0, 1.0, T).view(1, T, 1)
    x = 0.05 + 0.1 * torch.rand(B, T, F, generator=g) * (1.0 - f / F)
    for _ in range(3):
        f0 = 20.0 + 400.0 * torch.rand(B, 1, 1, generator=g)
        slope = 200.0 * (torch.rand(B, 1, 1, generator=g) - 0.5)
        wob = 30.0 * torch.sin(6.28 * (t * (1.0 + 3.0 * torch.rand(B, 1, 1, generator=g)) + torch.rand(B, 1, 1, generator=g)))
        width = 8.0 + 25.0 * torch.rand(B, 1, 1, generator=g)
        x = x + (0.3 + 0.5 * torch.rand(B, T, 1, generator=g)) * torch.exp(-((f - f0 - slope * t - wob) / width) ** 2)
    return x.clamp(1e-3, 0.999)


def _pair(hps, dtype, dev, B, with_vq, kind, restart=None, decay=None):
    """An Encoder / Decoder pair of the run's sizes and its captured AEStep on one batch."""
    import torch
    from zs_amd import layers
    from zs_amd.model import Decoder, Encoder
    from zs_amd.trainer import AEStep
    from zs_amd.vq import VectorCodebook
    from zs_amd.vq_train import VqBottleneck, encoded_rows
    torch.manual_seed(0)
    enc = Encoder(ns=hps.ns, dp=hps.enc_dp, enc_size=hps.enc_size, seg_len=hps.seg_len, enc_mode='continues', dtype=dtype).to(dev)
    dec = Decoder(ns=hps.ns, c_in=hps.enc_size, c_h=hps.emb_size, c_a=hps.n_speakers, seg_len=hps.seg_len, dtype=dtype).to(dev)
    g = torch.Generator().manual_seed(1)
    x = _batch(kind, B, hps.seg_len, 513, g).to(dev)
    c = torch.randint(0, hps.n_speakers, (B,), generator=g).to(dev)
    bn = None
    if with_vq:                                                   # codewords around the encoder's own rows of this batch
        enc.train()
        _, z, _ = enc._engine().forward(x, True, seed=0)
        rows = z.reshape(-1, hps.enc_size)
        pick = torch.randint(0, rows.shape[0], (K,), generator=g).to(dev)
        code = (rows[pick] + 0.05 * rows.std() * torch.randn(K, hps.enc_size, device=dev)).float().cpu().numpy()
        more = {} if restart is None else {'restart': restart}
        if decay is not None:
            more['decay'] = decay
        bn = VqBottleneck(VectorCodebook(code, {'enc_mode': 'continues'}), rows=encoded_rows(B, hps.seg_len), ctx=layers.Ctx(dev, dtype), **more)
    ae = AEStep(enc, dec, lr=hps.lr, max_grad_norm=hps.max_grad_norm, use_graph=True, vq=bn)
    for _ in range(ae.graph_warmup + 2):                          # the eager warm-up steps, the capture, one replay
        ae.step(x, c)
    torch.cuda.synchronize()
    assert len(ae._graphs) == 1
    return ae, x, c, bn


def step(args, out):
    import torch
    from zs_amd.hps import Hps
    dev = torch.device('cuda:0')
    hps = Hps(os.path.join(HERE, 'hps', 'zerospeech_english_1024.json')).get_tuple()
    out['step'] = {}
    for kind, B in (('formants', 16), ('formants', 256), ('noise', 16), ('noise', 256)):
        if args.restart is not None:
            restart_step(args, out, hps, dev, kind, B)
            continue
        runs = {'off': _pair(hps, args.dtype, dev, B, False, kind), 'vq_K1024': _pair(hps, args.dtype, dev, B, True, kind)}

        def timed(name):
            ae, x, c, _ = runs[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ae.step(x, c)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.steps
        ms = {k: [] for k in runs}
        for r in range(-1, args.rounds):                          # round -1 alternates as the others do and is not counted
            for name in (('off', 'vq_K1024') if r % 2 == 0 else ('vq_K1024', 'off')):
                t = timed(name)
                if r >= 0:
                    ms[name].append(t)
        bn = runs['vq_K1024'][3]
        rec = {k: _stats(v) for k, v in ms.items()}
        rec.update(rows=bn.rows, K=K, E=hps.enc_size, steps_per_round=args.steps, stats_after=bn.stats(),
                   vq_minus_off_ms=round(rec['vq_K1024']['median_ms'] - rec['off']['median_ms'], 4))
        # the bottleneck's own launches alone, on the encoder's rows of the last step: forward + backward as the step issues them
        bits, dq = bn._bits, bn.ctx.act('bench_dq', bn._bits.B, bn._bits.T, bn.E)
        chain = lambda: (bn.forward(bits), bn.backward(dq))
        chain()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(10):
                chain()
        graph.replay()
        rec['bottleneck_launches_alone'] = _events(graph.replay, per=10)
        out['step']['%s_B%d' % (kind, B)] = rec
        print('[vq_train_bench] step %s B %d: %s' % (kind, B, json.dumps(rec)), file=sys.stderr, flush=True)
        del runs, bn
        torch.cuda.empty_cache()


def restart_step(args, out, hps, dev, kind, B):
    """The replayed step with the bottleneck, without and with restart, and what the codebook looks like afterwards."""
    import torch
    runs = {'vq_K1024': _pair(hps, args.dtype, dev, B, True, kind, decay=args.decay),
            'vq_restart': _pair(hps, args.dtype, dev, B, True, kind, restart=args.restart, decay=args.decay)}
    done = {k: v[0].graph_warmup + 2 for k, v in runs.items()}

    def timed(name):
        ae, x, c, _ = runs[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            ae.step(x, c)
        torch.cuda.synchronize()
        done[name] += args.steps
        return (time.perf_counter() - t0) * 1e3 / args.steps
    ms = {k: [] for k in runs}
    names = tuple(runs)
    for r in range(-1, args.rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            t = timed(name)
            if r >= 0:
                ms[name].append(t)
    rec = {k: _stats(v) for k, v in ms.items()}
    rec.update(rows=runs['vq_K1024'][3].rows, K=K, E=hps.enc_size, steps_per_round=args.steps, restart=args.restart, decay=runs['vq_K1024'][3].decay,
               restart_minus_plain_ms=round(rec['vq_restart']['median_ms'] - rec['vq_K1024']['median_ms'], 4))
    for name, (ae, x, c, bn) in runs.items():
        rec[name]['after_%d_steps' % done[name]] = bn.stats()
        while done[name] < args.long:
            ae.step(x, c)
            done[name] += 1
        rec[name]['after_%d_steps' % done[name]] = bn.stats()
    out['step']['%s_B%d' % (kind, B)] = rec
    print('[vq_train_bench] restart step %s B %d: %s' % (kind, B, json.dumps(rec)), file=sys.stderr, flush=True)
    del runs
    torch.cuda.empty_cache()


def restart_kernels(args, out):
    """zs_vq_ema and zs_vq_restart alone at K = E = 1024 and 256 / 4096 rows: HIP events around a replayed graph of launches."""
    import torch
    from zs_amd import _lib as L
    from zs_amd.vq_train import restart_stride
    dev = torch.device('cuda:0')
    E = 1024
    g = torch.Generator().manual_seed(0)
    code = torch.randn(K, E, generator=g).to(dev)
    out['kernels'] = {}
    for n, calls in ((256, 40), (4096, 20)):
        x = torch.randn(n, E, generator=g).to(dev)
        ia = (torch.arange(n, dtype=torch.int32) % K).to(dev)
        cnt, sums = torch.zeros(K, dtype=torch.int32, device=dev), torch.zeros(K, E, dtype=torch.int64, device=dev)
        N, m, code2, cn2 = torch.ones(K, device=dev), code.clone(), code.clone(), (code.double() ** 2).sum(1).float()
        cnt_live = torch.ones(K, dtype=torch.int32, device=dev)
        cnt_dead = torch.zeros(K, dtype=torch.int32, device=dev)
        cnt_dead[0] = 1
        work, stat = torch.zeros(K + 2, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
        seed_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        st = lambda: torch.cuda.current_stream().cuda_stream
        restart = lambda c: L.call('zs_vq_restart', 'ZsVqRestart', st(), thresh=args.restart, x=L.ptr(x), n=n, ld_x=E, idx_acc=L.ptr(ia),
                                   cnt=L.ptr(c), K=K, E=E, N=L.ptr(N), m=L.ptr(m), code=L.ptr(code2), ld_code=E, cnorm=L.ptr(cn2), seed=1,
                                   seed_ptr=L.ptr(seed_dev), stride=restart_stride(n), work=L.ptr(work), restarted=L.ptr(stat),
                                   skipped=L.ptr(stat, 1))
        kill = lambda: N.fill_(0.5 * args.restart)
        fns = {
            'zs_vq_ema': lambda: L.call('zs_vq_ema', 'ZsVqEma', st(), cnt=L.ptr(cnt), sum=L.ptr(sums), K=K, E=E, shift=20, decay=0.99, N=L.ptr(N),
                                        m=L.ptr(m), code=L.ptr(code2), ld_code=E, cnorm=L.ptr(cn2), used=L.ptr(stat, 3)),
            'zs_vq_restart_nothing_dead': lambda: restart(cnt_live),
            'fill_N_alone': kill,
            'fill_N_then_zs_vq_restart_all_but_one_dead': lambda: (kill(), restart(cnt_dead)),
        }
        rec = {'n': n, 'K': K, 'E': E, 'launches_per_replay': calls}
        for name, fn in fns.items():
            if name == 'zs_vq_restart_nothing_dead':
                N.fill_(1.0)                                      # (zs_vq_ema let it decay)
                stat.zero_()
            fn()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(calls):
                    fn()
            graph.replay()
            rec[name] = _events(graph.replay, per=calls)
            if name == 'zs_vq_restart_nothing_dead':
                assert int(stat[0]) == 0 and int(stat[1]) == 0
        assert int(stat[0]) == (K - 1) * (1 + calls * 8) and int(stat[1]) == 0, stat      # (the eager call, one replay, seven timed ones)
        rec['restart_all_but_one_dead_minus_fill_us'] = round(rec['fill_N_then_zs_vq_restart_all_but_one_dead']['median_us'] -
                                                              rec['fill_N_alone']['median_us'], 2)
        rec['nothing_dead_not_above_ema'] = rec['zs_vq_restart_nothing_dead']['median_us'] <= rec['zs_vq_ema']['median_us']
        out['kernels']['rows%d' % n] = rec
        print('[vq_train_bench] restart kernels rows %d: %s' % (n, json.dumps(rec)), file=sys.stderr, flush=True)


def kernels(args, out):
    import torch
    from zs_amd import _lib as L, layers, vq as V
    from zs_amd.vq_train import MAX_ABS, PARTS
    dev = torch.device('cuda:0')
    E = 1024
    dt_id, dt = layers.DTYPES[args.dtype]
    g = torch.Generator().manual_seed(0)
    code = torch.randn(K, E, generator=g).to(dev)
    cnorm = (code.double() ** 2).sum(1).float()
    out['kernels'] = {}
    for n, calls in ((256, 40), (4096, 20)):
        idx0 = torch.randint(0, K, (n,), generator=g).to(dev)
        z = (code[idx0] + 0.3 * torch.randn(n, E, device=dev)).to(dt)
        idx, ia = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        q, dq, zf = torch.empty(n, E, dtype=dt, device=dev), torch.randn(n, E, device=dev).to(dt), torch.empty(n, E, device=dev)
        part, loss = torch.zeros(PARTS, dtype=torch.float64, device=dev), torch.zeros(1, device=dev)
        stat = torch.zeros(4, dtype=torch.int32, device=dev)
        cnt, sums = torch.zeros(K, dtype=torch.int32, device=dev), torch.zeros(K, E, dtype=torch.int64, device=dev)
        N, m, code2, cn2 = torch.ones(K, device=dev), code.clone(), code.clone(), cnorm.clone()
        work = V.workspace(dev)
        shift = V.vq_shift(n, MAX_ABS)
        st = lambda: torch.cuda.current_stream().cuda_stream
        fns = {
            'zs_vq_assign': lambda: L.call('zs_vq_assign', 'ZsVqAssign', st(), dtype=dt_id, x=L.ptr(z), n=n, ld_x=E, code=L.ptr(code), ld_code=E,
                                           cnorm=L.ptr(cnorm), K=K, E=E, idx=L.ptr(idx), work=L.ptr(work), work_bytes=V.WORK_BYTES),
            'zs_vq_commit': lambda: L.call('zs_vq_commit', 'ZsVqCommit', st(), dtype=dt_id, z=L.ptr(z), n=n, ld_z=E, idx=L.ptr(idx), code=L.ptr(code),
                                           ld_code=E, K=K, E=E, q=L.ptr(q), ld_q=E, z_f32=(L.ptr(zf) if dt != torch.float32 else None), ld_zf=E,
                                           idx_acc=L.ptr(ia), scale=1.0 / (n * E), partial=L.ptr(part), loss=L.ptr(loss), bad=L.ptr(stat),
                                           over=L.ptr(stat, 1)),
            'zs_vq_accum': lambda: L.call('zs_vq_accum', 'ZsVqAccum', st(), x=(L.ptr(zf) if dt != torch.float32 else L.ptr(z)), idx=L.ptr(ia), n=n,
                                          ld_x=E, K=K, E=E, shift=shift, cnt=L.ptr(cnt), sum=L.ptr(sums), bad=L.ptr(stat, 2)),
            'zs_vq_ema': lambda: L.call('zs_vq_ema', 'ZsVqEma', st(), cnt=L.ptr(cnt), sum=L.ptr(sums), K=K, E=E, shift=shift, decay=0.99, N=L.ptr(N),
                                        m=L.ptr(m), code=L.ptr(code2), ld_code=E, cnorm=L.ptr(cn2), used=L.ptr(stat, 3)),
            'zs_vq_st_bwd': lambda: L.call('zs_vq_st_bwd', 'ZsVqStBwd', st(), dtype=dt_id, dq=L.ptr(dq), n=n, ld_dq=E, z=L.ptr(z), ld_z=E,
                                           idx=L.ptr(idx), code=L.ptr(code), ld_code=E, K=K, E=E, g=1e-6, dz=L.ptr(dq), ld_dz=E, bad=L.ptr(stat)),
            'zero_counts_and_sums': lambda: (cnt.zero_(), sums.zero_()),
            'copy_codebook': lambda: (code2.copy_(code), cn2.copy_(cnorm)),
        }
        rec = {'n': n, 'K': K, 'E': E, 'dtype': args.dtype, 'launches_per_replay': calls}
        for name, fn in fns.items():                              # (in the step's order: each reads what the one before wrote)
            fn()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(calls):
                    fn()
            graph.replay()
            rec[name] = _events(graph.replay, per=calls)
        assert int(stat[0]) == 0 and int(stat[1]) == 0
        out['kernels']['rows%d' % n] = rec
        print('[vq_train_bench] kernels rows %d: %s' % (n, json.dumps(rec)), file=sys.stderr, flush=True)


def bench_against_parent(args, out):
    """bench.py --gpus 1 --steps 20 --warmup 5 in each tree, a fresh process per run, alternating, three runs each."""
    builds = [('parent', os.path.abspath(args.parent)), ('new', HERE)]
    env = dict(os.environ)
    env.pop('ZS_LIB_PATH', None)                                  # each tree loads the library beside its own package
    got = {n: [] for n, _ in builds}
    for r in range(3):
        for name, tree in builds[r % 2:] + builds[:r % 2]:
            txt = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5'], cwd=tree,
                                 env=env, stdout=subprocess.PIPE, text=True, check=True).stdout
            rec = json.loads([ln for ln in txt.splitlines() if ln.startswith('{')][-1])
            keep = {k: rec[k] for k in ('metric', 'value', 'unit', 'step_ms', 'ms_per_step') if k in rec}
            print('[vq_train_bench] bench.py run %d %s: %s' % (r, name, json.dumps(keep)), file=sys.stderr, flush=True)
            got[name].append(keep)
    out['bench_vs_parent'] = got
    key = 'value' if all('value' in g for v in got.values() for g in v) else 'step_ms'
    lo = {n: min(float(g[key]) for g in v) for n, v in got.items()}
    hi = {n: max(float(g[key]) for g in v) for n, v in got.items()}
    out['bench_vs_parent_ranges'] = {'key': key, 'parent': [lo['parent'], hi['parent']], 'new': [lo['new'], hi['new']],
                                     'overlap': lo['new'] <= hi['parent'] and lo['parent'] <= hi['new']}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent', default=None, help='a built tree of the parent commit (its own package and libzs_amd.so)')
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--steps', type=int, default=10, help='replays per timed round')
    p.add_argument('--dtype', default='bf16')
    p.add_argument('--only', default=None, choices=['step', 'kernels', 'parent'])
    p.add_argument('--restart', type=float, default=None, metavar='T', help='measure zs_vq_restart at this threshold (DESIGN 32) instead')
    p.add_argument('--decay', type=float, default=None, help='with --restart: the decay of the codebook\'s average (default: the run\'s, 0.99)')
    p.add_argument('--long', type=int, default=1000, help='with --restart: steps in all before the second look at the codebook')
    p.add_argument('--out', default=None)
    args = p.parse_args()
    if args.out is None:
        args.out = os.path.join(HERE, 'profiles', 'vq_train_step_ms.json' if args.restart is None else 'vq_restart_step_ms.json')
    if args.rounds < 5:
        p.error('--rounds must be at least 5')
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        sys.exit('vq_train_bench needs an MI355X: a timing taken anywhere else says nothing about it')
    import zs_amd  # noqa: F401
    out = {'device': torch.cuda.get_device_name(0), 'dtype': args.dtype, 'rounds': args.rounds,
           'order': 'warm-up and capture, one uncounted alternating round, then alternating rounds, order rotated per round; one GPU job'}
    if os.path.exists(args.out):                                  # a part run alone keeps the other parts of an earlier job
        with open(args.out) as f:
            out = dict(json.load(f), **out)
    if args.parent is not None and args.only in (None, 'parent'):  # first, while this process holds no GPU memory
        bench_against_parent(args, out)
    for name, part in (('kernels', kernels if args.restart is None else restart_kernels), ('step', step)):
        if args.only in (None, name):
            part(args, out)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
