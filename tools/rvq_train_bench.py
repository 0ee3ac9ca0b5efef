"""What training through the residual codebook costs, in one GPU job -> profiles/rvq_train_step_ms.json; bf16, K = E = 1024:
  kernels   each new launch alone at 256 and 4096 rows -- zs_rvq_commit at the first stage (bf16 rows, the fp32 copy) and behind it (fp32
            rows, a read and written), zs_rvq_loss at S = 4, zs_rvq_st_bwd -- beside the bytes it must move and the share that is of the
            6.29 TB/s of a float4 copy (MI355X_MICROARCH.md), and the unchanged zs_vq_assign (on fp32 residual rows), zs_vq_accum and
            zs_vq_ema of a stage at the same rows: HIP events around a replayed graph of launches
  step      the replayed AEStep of a 'continues' model at hps/zerospeech_english_1024.json's sizes without the bottleneck, with
            --vq_train's and with --rvq_train's at S = 2 and 4, at B = 16 and B = 256 on speech-like input: after the capture, alternating
            rounds of `--steps` replays each, by the host clock around a device synchronise; median / min / max per step; `used` per stage
            afterwards (untrained nets collapse the assignment, zs_vq_accum's worst case: such a figure is labelled 'collapsed'); and the
            bottleneck's own launches alone on the rows of the last step
  parent    (--parent DIR, a built tree of the parent commit) `bench.py --gpus 1 --steps 20 --warmup 5` in each tree, a fresh process
            per run, alternating, three runs each: the headline path launches nothing new, so the two ranges must overlap
    python tools/rvq_train_bench.py [--parent DIR] [--rounds 7] [--steps 10] [--out profiles/rvq_train_step_ms.json]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, 'tools'))
from vq_train_bench import K, _batch, _events, _stats, bench_against_parent  # noqa: E402  (the workload, the clocks and the parent runs)

COPY_TBS = 6.29                      # a float4 copy on one MI355X (MI355X_MICROARCH.md)
STAGES = (2, 4)


def _with_bytes(rec, nbytes):
    rec = dict(rec, bytes=int(nbytes))
    rec['TB_per_s'] = round(nbytes / (rec['median_us'] * 1e-6) / 1e12, 3)
    rec['of_float4_copy'] = round(rec['TB_per_s'] / COPY_TBS, 3)
    return rec


def kernels(args, out):
    import torch
    from zs_amd import _lib as L, layers, vq as V
    from zs_amd.vq_train import MAX_ABS, PARTS
    dev = torch.device('cuda:0')
    E, S = 1024, 4
    dt_id, dt = layers.DTYPES[args.dtype]
    es = 2 if dt != torch.float32 else 4
    g = torch.Generator().manual_seed(0)
    code = torch.randn(K, E, generator=g).to(dev)
    cnorm = (code.double() ** 2).sum(1).float()
    out['kernels'] = {}
    for n, calls in ((256, 40), (4096, 20)):
        idx0 = torch.randint(0, K, (n,), generator=g).to(dev)
        z = (code[idx0] + 0.3 * torch.randn(n, E, device=dev)).to(dt)
        idx, ia = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        res = [torch.zeros(n, E, device=dev), torch.zeros(n, E, device=dev)]
        a, dq = torch.zeros(n, E, device=dev), torch.randn(n, E, device=dev).to(dt)
        part, loss = torch.zeros(S, PARTS, dtype=torch.float64, device=dev), torch.zeros(1 + S, device=dev)
        stat = torch.zeros(4, dtype=torch.int32, device=dev)
        cnt, sums = torch.zeros(K, dtype=torch.int32, device=dev), torch.zeros(K, E, dtype=torch.int64, device=dev)
        N, m, code2, cn2 = torch.ones(K, device=dev), code.clone(), code.clone(), cnorm.clone()
        work = V.workspace(dev)
        shift = V.vq_shift(n, MAX_ABS)
        st = lambda: torch.cuda.current_stream().cuda_stream

        def commit(first):
            L.call('zs_rvq_commit', 'ZsRvqCommit', st(), dtype=dt_id, src_f32=int(not first), first=int(first),
                   x=(L.ptr(z) if first else L.ptr(res[1])), n=n, ld_x=E, idx=L.ptr(idx), code=L.ptr(code), ld_code=E, K=K, E=E,
                   r=L.ptr(res[1] if first else res[0]), ld_r=E, x_f32=(L.ptr(res[0]) if first and es == 2 else None),
                   ld_xf=(E if first and es == 2 else 0), idx_acc=L.ptr(ia), a=L.ptr(a), ld_a=E, partial=L.ptr(part[0 if first else 1]),
                   bad=L.ptr(stat), over=L.ptr(stat, 1))
        spread = torch.randint(0, K, (n,), generator=g).to(torch.int32).to(dev)       # indices uniform over K, as section 30 timed it

        def accum(which):
            L.call('zs_vq_accum', 'ZsVqAccum', st(), x=L.ptr(res[1]), idx=L.ptr(which), n=n, ld_x=E, K=K, E=E, shift=shift, cnt=L.ptr(cnt),
                   sum=L.ptr(sums), bad=L.ptr(stat, 2))
        fns = {                                                     # (in the step's order: each reads what the one before wrote)
            'zs_vq_assign_stage0': (lambda: V.launch_assign(st(), dt_id, L.ptr(z), n, E, code, cnorm, idx=idx, work=work), None),
            'zs_rvq_commit_first': (lambda: commit(True), n * E * (es + 4 + 4 + (4 if es == 2 else 0) + 4)),
            'zs_vq_assign_fp32_rows': (lambda: V.launch_assign(st(), L.ZS_F32, L.ptr(res[1]), n, E, code, cnorm, idx=idx, work=work), None),
            'zs_rvq_commit_later': (lambda: commit(False), n * E * (4 + 4 + 4 + 4 + 4)),
            # (the rows behind stage 0 are here noise around zero: every one is nearest the shortest codeword, zs_vq_accum's worst case)
            'zs_vq_accum_as_assigned': (lambda: accum(ia), None),
            'zs_vq_accum': (lambda: accum(spread), None),
            'zs_vq_ema': (lambda: L.call('zs_vq_ema', 'ZsVqEma', st(), cnt=L.ptr(cnt), sum=L.ptr(sums), K=K, E=E, shift=shift, decay=0.99,
                                         N=L.ptr(N), m=L.ptr(m), code=L.ptr(code2), ld_code=E, cnorm=L.ptr(cn2), used=L.ptr(stat, 3)), None),
            'zs_rvq_loss_S4': (lambda: L.call('zs_rvq_loss', 'ZsRvqLoss', st(), partial=L.ptr(part), S=S, scale=1.0 / (n * E), loss=L.ptr(loss)),
                               S * PARTS * 8),
            'zs_rvq_st_bwd': (lambda: L.call('zs_rvq_st_bwd', 'ZsRvqStBwd', st(), dtype=dt_id, dq=L.ptr(dq), n=n, ld_dq=E, a=L.ptr(a), ld_a=E, E=E,
                                             g=1e-6, dz=L.ptr(dq), ld_dz=E), n * E * (es + 4 + es)),
        }
        rec = {'n': n, 'K': K, 'E': E, 'dtype': args.dtype, 'launches_per_replay': calls}
        for name, (fn, nbytes) in fns.items():
            fn()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(calls):
                    fn()
            graph.replay()
            t = _events(graph.replay, per=calls)
            rec[name] = t if nbytes is None else _with_bytes(t, nbytes)
        assert int(stat[0]) == 0 and int(stat[1]) == 0, stat
        new = rec['zs_rvq_commit_later']['median_us']
        old = rec['zs_vq_assign_fp32_rows']['median_us'] + rec['zs_vq_accum']['median_us'] + rec['zs_vq_ema']['median_us']
        rec['glue_share_of_a_stage'] = round(new / (new + old), 4)  # (zs_vq_accum with spread indices)
        rec['used_as_assigned'] = int(torch.unique(ia).numel())
        out['kernels']['rows%d' % n] = rec
        print('[rvq_train_bench] kernels rows %d: %s' % (n, json.dumps(rec)), file=sys.stderr, flush=True)


def _pair(hps, dtype, dev, B, stages):
    """An Encoder / Decoder pair of the run's sizes and its captured AEStep on one batch.  stages: None (no bottleneck), 1 (--vq_train's)
    or S (--rvq_train's): stage s starts from rows of what stage s - 1 leaves of the encoder's own rows of this batch."""
    import numpy as np
    import torch
    from zs_amd import layers
    from zs_amd.model import Decoder, Encoder
    from zs_amd.rvq import ResidualCodebook
    from zs_amd.rvq_train import RvqBottleneck
    from zs_amd.trainer import AEStep
    from zs_amd.vq import VectorCodebook
    from zs_amd.vq_train import VqBottleneck, encoded_rows
    torch.manual_seed(0)
    enc = Encoder(ns=hps.ns, dp=hps.enc_dp, enc_size=hps.enc_size, seg_len=hps.seg_len, enc_mode='continues', dtype=dtype).to(dev)
    dec = Decoder(ns=hps.ns, c_in=hps.enc_size, c_h=hps.emb_size, c_a=hps.n_speakers, seg_len=hps.seg_len, dtype=dtype).to(dev)
    g = torch.Generator().manual_seed(1)
    x = _batch('formants', B, hps.seg_len, 513, g).to(dev)
    c = torch.randint(0, hps.n_speakers, (B,), generator=g).to(dev)
    bn = None
    if stages is not None:
        enc.train()
        _, z, _ = enc._engine().forward(x, True, seed=0)
        r = z.reshape(-1, hps.enc_size).float()
        planes = []
        for s in range(stages):
            pick = torch.randint(0, r.shape[0], (K,), generator=g).to(dev)
            code = r[pick] + 0.05 * r.std() * torch.randn(K, hps.enc_size, device=dev)
            planes.append(code.cpu().numpy())
            r = r - code[torch.cdist(r, code).argmin(1)]             # (only to place the next stage's start)
        ctx, rows = layers.Ctx(dev, dtype), encoded_rows(B, hps.seg_len)
        if stages == 1:
            bn = VqBottleneck(VectorCodebook(planes[0], {'enc_mode': 'continues'}), rows=rows, ctx=ctx)
        else:
            bn = RvqBottleneck(ResidualCodebook(np.stack(planes), {'enc_mode': 'continues'}), rows=rows, ctx=ctx)
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
    for B in (16, 256):
        runs = {'off': _pair(hps, args.dtype, dev, B, None), 'vq_K1024': _pair(hps, args.dtype, dev, B, 1)}
        for S in STAGES:
            runs['rvq_K1024_S%d' % S] = _pair(hps, args.dtype, dev, B, S)
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
        for r in range(-1, args.rounds):                          # round -1 alternates as the others do and is not counted
            for name in names[r % len(names):] + names[:r % len(names)]:
                t = timed(name)
                if r >= 0:
                    ms[name].append(t)
        rec = {k: _stats(v) for k, v in ms.items()}
        rec.update(rows=runs['vq_K1024'][3].rows, K=K, E=hps.enc_size, steps_per_round=args.steps)
        for name in names[1:]:
            bn = runs[name][3]
            s = bn.stats()
            used = s['used'] if isinstance(s['used'], list) else [s['used']]
            rec[name].update(minus_off_ms=round(rec[name]['median_ms'] - rec['off']['median_ms'], 4), used=used, loss_vq=s['loss_vq'],
                             assignment=('collapsed' if min(used) <= K // 64 else 'spread'))
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
            rec[name]['bottleneck_launches_alone'] = _events(graph.replay, per=10)
            print('[rvq_train_bench] B %d %s: used per stage %s of %d (%s)' % (B, name, used, K, rec[name]['assignment']), file=sys.stderr, flush=True)
        out['step']['formants_B%d' % B] = rec
        print('[rvq_train_bench] step B %d: %s' % (B, json.dumps(rec)), file=sys.stderr, flush=True)
        del runs
        torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--parent', default=None, help='a built tree of the parent commit (its own package and libzs_amd.so)')
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--steps', type=int, default=10, help='replays per timed round')
    p.add_argument('--dtype', default='bf16')
    p.add_argument('--only', default=None, choices=['step', 'kernels', 'parent'])
    p.add_argument('--out', default=os.path.join(HERE, 'profiles', 'rvq_train_step_ms.json'))
    args = p.parse_args()
    if args.rounds < 5:
        p.error('--rounds must be at least 5')
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        sys.exit('rvq_train_bench needs an MI355X: a timing taken anywhere else says nothing about it')
    import zs_amd  # noqa: F401
    out = {'device': torch.cuda.get_device_name(0), 'dtype': args.dtype, 'rounds': args.rounds,
           'order': 'warm-up and capture, one uncounted alternating round, then alternating rounds, order rotated per round; one GPU job'}
    if os.path.exists(args.out):                                  # a part run alone keeps the other parts of an earlier job
        with open(args.out) as f:
            out = dict(json.load(f), **out)
    if args.parent is not None and args.only in (None, 'parent'):  # first, while this process holds no GPU memory
        bench_against_parent(args, out)
    for name, part in (('kernels', kernels), ('step', step)):
        if args.only in (None, name):
            part(args, out)
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
