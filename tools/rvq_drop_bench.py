"""What quantiser dropout costs, in one GPU job -> profiles/rvq_drop_step_ms.json; bf16, K = E = 1024, S = 4:
  kernels   at 256 and 4096 rows (16 and 256 samples of 16 rows), alternating within the job: zs_rvq_commit behind the first stage beside
            zs_rvq_commit_drop with every count at S and with the counts of a draw at P = 1 (at stage 1, where 3/4 of the samples take
            part on average, and at stage 3, 1/4); zs_rvq_gather beside zs_rvq_gather_frag with every count at S and with those counts;
            zs_rvq_drop_draw alone.  HIP events around a replayed graph of launches; beside every figure the bytes the launch must move
            and the share that is of the 6.29 TB/s of a float4 copy (MI355X_MICROARCH.md)
  step      the replayed AEStep of a 'continues' model at hps/zerospeech_english_1024.json's sizes with --rvq_train's bottleneck at S = 4,
            without dropout and with --rvq_dropout 0.5, at B = 16 and B = 256 on speech-like input (tools/rvq_train_bench.py's workload):
            alternating rounds of `--steps` replays each by the host clock around a device synchronise; `used` and `active` per stage
            afterwards (untrained nets collapse the assignment: such a figure is labelled 'collapsed', as DESIGN 34 labels it)
  parent    (--parent DIR, a built tree of the parent commit) `bench.py --gpus 1 --steps 20 --warmup 5` in each tree, a fresh process
            per run, alternating, three runs each: the headline path launches nothing new, so the two ranges must overlap
    python tools/rvq_drop_bench.py [--parent DIR] [--rounds 7] [--steps 10] [--out profiles/rvq_drop_step_ms.json]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, 'tools'))
from rvq_train_bench import _with_bytes  # noqa: E402
from vq_train_bench import K, _batch, _stats, bench_against_parent  # noqa: E402  (the workload, the clocks and the parent runs)

S = 4


def _alternating(fns, calls, rounds=7):
    """{name: median / min / max us per launch}: every fn captured as a graph of `calls` launches, then `rounds` alternating rounds of
    one replay each between HIP events, the order rotated per round (one uncounted round first)."""
    import torch
    graphs = {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(calls):
                fn()
        g.replay()
        graphs[name] = g
    torch.cuda.synchronize()
    names, us = tuple(graphs), {k: [] for k in graphs}
    for r in range(-1, rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graphs[name].replay()
            b.record()
            torch.cuda.synchronize()
            if r >= 0:
                us[name].append(a.elapsed_time(b) * 1e3 / calls)
    return {k: {'median_us': round(sorted(v)[len(v) // 2], 2), 'min_us': round(min(v), 2), 'max_us': round(max(v), 2)} for k, v in us.items()}


def kernels(args, out):
    import torch
    from zs_amd import _lib as L, layers
    from zs_amd.vq_train import PARTS
    dev = torch.device('cuda:0')
    E, Tq = 1024, 16
    dt_id, dt = layers.DTYPES[args.dtype]
    es = 2 if dt != torch.float32 else 4
    g = torch.Generator().manual_seed(0)
    code = torch.randn(S, K, E, generator=g).to(dev)
    out['kernels'] = {}
    st = lambda: torch.cuda.current_stream().cuda_stream
    for n, calls in ((256, 40), (4096, 20)):
        B = n // Tq
        idx = torch.randint(0, K, (S, n), generator=g).to(torch.int32).to(dev)
        x = torch.randn(n, E, generator=g).to(dev)
        r, a = torch.zeros(n, E, device=dev), torch.zeros(n, E, device=dev)
        ia = torch.empty(n, dtype=torch.int32, device=dev)
        part = torch.zeros(PARTS, dtype=torch.float64, device=dev)
        stat = torch.zeros(4, dtype=torch.int32, device=dev)
        q = torch.zeros(n, E, dtype=dt, device=dev)
        start = torch.arange(B, dtype=torch.int64, device=dev) * Tq
        length = torch.full((B,), Tq, dtype=torch.int32, device=dev)
        full = torch.full((B,), S, dtype=torch.int32, device=dev)
        drawn, active = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(S, dtype=torch.int32, device=dev)

        def draw():
            L.call('zs_rvq_drop_draw', 'ZsRvqDropDraw', st(), seed=1, thr=1 << 24, S=S, n_frag=B, rows_per_frag=Tq, s_use=L.ptr(drawn),
                   active=L.ptr(active))
        draw()
        torch.cuda.synchronize()
        act = [int(v) for v in active.cpu()]

        def commit(s_use, stage):
            kw = dict(dtype=dt_id, src_f32=1, first=0, x=L.ptr(x), n=n, ld_x=E, idx=L.ptr(idx[stage]), code=L.ptr(code[stage]), ld_code=E, K=K, E=E,
                      r=L.ptr(r), ld_r=E, idx_acc=L.ptr(ia), a=L.ptr(a), ld_a=E, partial=L.ptr(part), bad=L.ptr(stat), over=L.ptr(stat, 1))
            if s_use is None:
                L.call('zs_rvq_commit', 'ZsRvqCommit', st(), **kw)
            else:
                L.call('zs_rvq_commit_drop', 'ZsRvqCommitDrop', st(), s_use=L.ptr(s_use), rows_per_frag=Tq, stage=stage, **kw)

        def gather(s_use):
            kw = dict(dtype=dt_id, idx=L.ptr(idx), n_idx=n, ld_idx=n, S=S, code=L.ptr(code), ld_code=E, plane_code=K * E, K=K, E=E, start=L.ptr(start),
                      len=L.ptr(length), n_frag=B, T=Tq, dst=L.ptr(q), ld_dst=E, bad=L.ptr(stat, 2))
            if s_use is None:
                L.call('zs_rvq_gather', 'ZsRvqGather', st(), s_use=S, **kw)
            else:
                L.call('zs_rvq_gather_frag', 'ZsRvqGatherFrag', st(), s_use=L.ptr(s_use), **kw)
        # bytes a launch must move: an active row reads x, the codeword and a and writes r and a (5 fp32 rows), an inactive one reads x and
        # writes r (2); a frame of the operand reads s_use codeword rows and writes one row of the compute dtype
        commit_bytes = lambda rows: E * 4 * (5 * rows + 2 * (n - rows))
        mean_use = float(drawn.float().mean().item())
        t = _alternating({
            'zs_rvq_commit': lambda: commit(None, 1),
            'zs_rvq_commit_drop_all_S': lambda: commit(full, 1),
            'zs_rvq_commit_drop_P1_stage1': lambda: commit(drawn, 1),
            'zs_rvq_commit_drop_P1_stage3': lambda: commit(drawn, 3),
            'zs_rvq_gather': lambda: gather(None),
            'zs_rvq_gather_frag_all_S': lambda: gather(full),
            'zs_rvq_gather_frag_P1': lambda: gather(drawn),
            'zs_rvq_drop_draw': draw,
        }, calls, args.rounds)
        nbytes = {'zs_rvq_commit': commit_bytes(n), 'zs_rvq_commit_drop_all_S': commit_bytes(n), 'zs_rvq_commit_drop_P1_stage1': commit_bytes(act[1]),
                  'zs_rvq_commit_drop_P1_stage3': commit_bytes(act[3]), 'zs_rvq_gather': n * E * (4 * S + es), 'zs_rvq_gather_frag_all_S': n * E * (4 * S + es),
                  'zs_rvq_gather_frag_P1': int(n * E * (4 * mean_use + es))}
        rec = {'n': n, 'samples': B, 'rows_per_sample': Tq, 'K': K, 'E': E, 'S': S, 'dtype': args.dtype, 'launches_per_replay': calls,
               'active_rows_of_the_P1_draw': act, 'mean_s_use_of_the_P1_draw': round(mean_use, 3)}
        for name, v in t.items():
            rec[name] = _with_bytes(v, nbytes[name]) if name in nbytes else v
        rec['commit_drop_all_S_over_commit'] = round(rec['zs_rvq_commit_drop_all_S']['median_us'] / rec['zs_rvq_commit']['median_us'], 4)
        rec['gather_frag_all_S_over_gather'] = round(rec['zs_rvq_gather_frag_all_S']['median_us'] / rec['zs_rvq_gather']['median_us'], 4)
        assert int(stat[0]) == 0 and int(stat[2]) == 0, stat
        out['kernels']['rows%d' % n] = rec
        print('[rvq_drop_bench] kernels rows %d: %s' % (n, json.dumps(rec)), file=sys.stderr, flush=True)


def _pair(hps, dtype, dev, B, dropout):
    """tools/rvq_train_bench.py's pair at S stages, the bottleneck with or without dropout: stage s starts from rows of what stage s - 1
    leaves of the encoder's own rows of this batch."""
    import numpy as np
    import torch
    from zs_amd import layers
    from zs_amd.model import Decoder, Encoder
    from zs_amd.rvq import ResidualCodebook
    from zs_amd.rvq_train import RvqBottleneck
    from zs_amd.trainer import AEStep
    from zs_amd.vq_train import encoded_rows
    torch.manual_seed(0)
    enc = Encoder(ns=hps.ns, dp=hps.enc_dp, enc_size=hps.enc_size, seg_len=hps.seg_len, enc_mode='continues', dtype=dtype).to(dev)
    dec = Decoder(ns=hps.ns, c_in=hps.enc_size, c_h=hps.emb_size, c_a=hps.n_speakers, seg_len=hps.seg_len, dtype=dtype).to(dev)
    g = torch.Generator().manual_seed(1)
    x = _batch('formants', B, hps.seg_len, 513, g).to(dev)
    c = torch.randint(0, hps.n_speakers, (B,), generator=g).to(dev)
    enc.train()
    _, z, _ = enc._engine().forward(x, True, seed=0)
    r = z.reshape(-1, hps.enc_size).float()
    planes = []
    for s in range(S):
        pick = torch.randint(0, r.shape[0], (K,), generator=g).to(dev)
        code = r[pick] + 0.05 * r.std() * torch.randn(K, hps.enc_size, device=dev)
        planes.append(code.cpu().numpy())
        r = r - code[torch.cdist(r, code).argmin(1)]                 # (only to place the next stage's start)
    more = {} if dropout is None else {'dropout': dropout}
    bn = RvqBottleneck(ResidualCodebook(np.stack(planes), {'enc_mode': 'continues'}), rows=encoded_rows(B, hps.seg_len), ctx=layers.Ctx(dev, dtype), **more)
    ae = AEStep(enc, dec, lr=hps.lr, max_grad_norm=hps.max_grad_norm, use_graph=True, vq=bn)
    for _ in range(ae.graph_warmup + 2):                              # the eager warm-up steps, the capture, one replay
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
    for B in (16, 256):
        runs = {'rvq_S4': _pair(hps, args.dtype, dev, B, None), 'rvq_S4_dropout_0.5': _pair(hps, args.dtype, dev, B, 0.5)}
        names = tuple(runs)

        def timed(name):
            ae, x, c, _ = runs[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ae.step(x, c)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.steps
        ms = {k: [] for k in runs}
        for r in range(-1, args.rounds):                              # round -1 alternates as the others do and is not counted
            for name in names[r % len(names):] + names[:r % len(names)]:
                t = timed(name)
                if r >= 0:
                    ms[name].append(t)
        rec = {k: _stats(v) for k, v in ms.items()}
        rec.update(rows=runs['rvq_S4'][3].rows, K=K, S=S, E=hps.enc_size, steps_per_round=args.steps)
        for name in names:
            s = runs[name][3].stats()
            rec[name].update(used=s['used'], loss_vq=s['loss_vq'], assignment=('collapsed' if min(s['used']) <= K // 64 else 'spread'))
            if 'active' in s:
                rec[name].update(active=s['active'], s_use_mean=round(s['s_use_mean'], 3))
            print('[rvq_drop_bench] B %d %s: used per stage %s of %d (%s), active %s' % (B, name, s['used'], K, rec[name]['assignment'], s.get('active')),
                  file=sys.stderr, flush=True)
        rec['dropout_minus_none_ms'] = round(rec[names[1]]['median_ms'] - rec[names[0]]['median_ms'], 4)
        out['step']['formants_B%d' % B] = rec
        print('[rvq_drop_bench] step B %d: %s' % (B, json.dumps(rec)), file=sys.stderr, flush=True)
        del runs
        torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent', default=None, help='a built tree of the parent commit (its own package and libzs_amd.so)')
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--steps', type=int, default=10, help='replays per timed round')
    p.add_argument('--dtype', default='bf16')
    p.add_argument('--only', default=None, choices=['step', 'kernels', 'parent'])
    p.add_argument('--out', default=os.path.join(HERE, 'profiles', 'rvq_drop_step_ms.json'))
    args = p.parse_args()
    if args.rounds < 5:
        p.error('--rounds must be at least 5')
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        sys.exit('rvq_drop_bench needs an MI355X: a timing taken anywhere else says nothing about it')
    import zs_amd  # noqa: F401
    out = {'device': torch.cuda.get_device_name(0), 'dtype': args.dtype, 'rounds': args.rounds,
           'order': 'warm-up and capture, one uncounted alternating round, then alternating rounds, order rotated per round; one GPU job'}
    if os.path.exists(args.out):                                      # a part run alone keeps the other parts of an earlier job
        with open(args.out) as f:
            out = dict(json.load(f), **out)
    if args.parent is not None and args.only in (None, 'parent'):      # first, while this process holds no GPU memory
        bench_against_parent(args, out)
    for name, part in (('kernels', kernels), ('step', step)):
        if args.only in (None, name):
            part(args, out)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
