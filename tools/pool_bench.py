"""Real-data --train_ae rate: the step fed from a dataset in device memory against the host-fed step and the static-input step.

  python tools/pool_bench.py [--out profiles] [--steps 200] [--rounds 3]
      One process, B = 256, bf16, hps/zerospeech_english_1024.json, a synthetic dataset of 9 x 256 segments (8 distinct batches
      under the loader's wrap rule).  After warming all three, alternating windows of
        (a) static    AEStep.step on static_inputs: bench.py's path, no data movement at all
        (b) host_fed  trainer.HostFedStep over DataLoader: what `main.py --train_ae` does without --device_data
        (c) pool_fed  trainer.PoolFedStep over PoolLoader: `main.py --train_ae --device_data`
      ms/step per window (host clock around a device synchronise), the median and spread (max - min) of each arm, and
      next(PoolLoader) against next(DevicePrefetcher) at the stage-2 batch (B = 128) -> <out>/pool_step_ms.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/pool_bench.py --mode kernel [--launches 200]
      Only gathers at B = 256 over the same dataset, for a kernel trace.
  python tools/pool_bench.py --mode stats --csv DIR/.../*_kernel_stats.csv [--out profiles]
      The gather's rows of that trace with bytes/s from the shapes (2 x B x seg_len x F x 4 bytes moved per launch, read + write)
      and the share of the HBM peak -> <out>/pool_kernel_stats.csv
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, SEG, F = 256, 128, 513
BATCH_BYTES = 2 * B * SEG * F * 4              # read + written per gather launch
HBM_PEAK = 8.0e12                              # bytes/s, MI355X


def parse():
    p = argparse.ArgumentParser()
    p.add_argument('--mode', choices=['steps', 'kernel', 'stats'], default='steps')
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles'))
    p.add_argument('--steps', type=int, default=200)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--launches', type=int, default=200)
    p.add_argument('--csv', default=None)
    return p.parse_args()


def stats_main(args):
    rows = [r for r in csv.DictReader(open(args.csv)) if 'pool_gather' in r['Name'] or 'cursor_bump' in r['Name']]
    if not any('pool_gather' in r['Name'] for r in rows):
        sys.exit('pool_bench.py: no pool_gather kernel in %s' % args.csv)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, 'pool_kernel_stats.csv')
    with open(path, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['kernel', 'calls', 'avg_us', 'min_us', 'max_us', 'bytes_per_launch', 'avg_bytes_per_s', 'share_of_hbm_peak_8TBs'])
        for r in rows:
            gather = 'pool_gather' in r['Name']
            avg = float(r['AverageNs'])
            rate = BATCH_BYTES / (avg * 1e-9) if gather else 0.0
            w.writerow([r['Name'].replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0], r['Calls'], '%.2f' % (avg / 1e3),
                        '%.2f' % (float(r.get('MinNs', 'nan')) / 1e3), '%.2f' % (float(r.get('MaxNs', 'nan')) / 1e3), BATCH_BYTES if gather else 8,
                        '%.4g' % rate, '%.3f' % (rate / HBM_PEAK)])
    print(open(path).read())


def main():
    args = parse()
    if args.mode == 'stats':
        return stats_main(args)
    import torch
    import zs_amd  # noqa: F401
    from zs_amd.dataloader import DataLoader, DevicePrefetcher, SyntheticDataset
    from zs_amd.hps import Hps
    from zs_amd.model import Decoder, Encoder
    from zs_amd.pool import DevicePool, PoolLoader
    from zs_amd.trainer import AEStep
    if not torch.cuda.is_available():
        sys.exit('pool_bench.py needs the GPU')
    dev = torch.device('cuda:0')
    hps = Hps(os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')).get_tuple()
    assert hps.seg_len == SEG
    ds = SyntheticDataset(9 * B, seg_len=SEG, n_bins=F, n_speakers=hps.n_speakers, seed=0)     # P = 8 distinct batches
    pool = DevicePool(ds, dev)

    if args.mode == 'kernel':
        loader = PoolLoader(pool, ds, B, n_speakers=hps.n_speakers)
        for _ in range(args.launches):
            next(loader)
        torch.cuda.synchronize()
        print('%d gathers, cursor %d' % (args.launches, int(loader.cursor.item())))
        return

    def make_ae():
        torch.manual_seed(1234)
        enc = Encoder(ns=hps.ns, dp=hps.enc_dp, enc_size=hps.enc_size, seg_len=SEG, enc_mode='multilabel_binary', dtype='bf16').to(dev)
        dec = Decoder(ns=hps.ns, c_in=hps.enc_size, c_h=hps.emb_size, c_a=hps.n_speakers, seg_len=SEG, dtype='bf16').to(dev)
        return AEStep(enc, dec, lr=hps.lr, max_grad_norm=hps.max_grad_norm, use_graph=True)

    ae_a, ae_b, ae_c = make_ae(), make_ae(), make_ae()
    xs, cs = ae_a.static_inputs(B, SEG, F)
    c0, x0 = next(DataLoader(ds, B))
    xs.copy_(x0); cs.copy_(c0)
    host = ae_b.host_feeder(DataLoader(ds, B))
    pooled = ae_c.pool_feeder(PoolLoader(pool, ds, B, n_speakers=hps.n_speakers))
    arms = [('static', lambda: ae_a.step(xs, cs)), ('host_fed', lambda: next(host)), ('pool_fed', lambda: next(pooled))]

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n

    for name, fn in arms:                                   # eager warm-up steps, capture, first replays
        print('warm-up %-9s %.2f ms/step' % (name, window(fn, 12)), flush=True)
    ms = {name: [] for name, _ in arms}
    for r in range(args.rounds):
        for name, fn in arms:
            ms[name].append(window(fn, args.steps))
            print('round %d %-9s %.3f ms/step' % (r, name, ms[name][-1]), flush=True)
    out = {'what': 'train_ae ms/step, B=256 bf16, hps/zerospeech_english_1024.json, %d steps per window, %d alternating rounds, one '
                   'process; host clock around a device synchronise' % (args.steps, args.rounds),
           'dataset': 'SyntheticDataset(%d segments): 8 distinct batches' % (9 * B),
           'pool_bytes': pool.plan.nbytes,
           'arms': {name: {'windows_ms': v, 'median_ms': statistics.median(v), 'spread_ms': max(v) - min(v)} for name, v in ms.items()}}
    a, b, c = (out['arms'][k]['median_ms'] for k in ('static', 'host_fed', 'pool_fed'))
    out['pool_minus_static_ms'] = c - a
    out['host_minus_pool_ms'] = b - c
    out['larger_spread_of_host_and_pool_ms'] = max(out['arms']['host_fed']['spread_ms'], out['arms']['pool_fed']['spread_ms'])
    out['pool_faster_than_host_by_more_than_the_spread'] = bool(b - c > out['larger_spread_of_host_and_pool_ms'])

    # next() of the loaders at the stage-2 batch: enqueue + completion of n batches, nothing else on the GPU
    B2, n2 = 128, 100
    pl = PoolLoader(pool, ds, B2, n_speakers=hps.n_speakers)
    pf = DevicePrefetcher(DataLoader(ds, B2), dev, n_speakers=hps.n_speakers)
    loaders = {}
    for name, it in (('pool_loader', pl), ('device_prefetcher', pf)):
        window(lambda: next(it), 10)
        loaders[name] = [window(lambda: next(it), n2) for _ in range(3)]
        print('next(%s) B=128: %s ms' % (name, ['%.3f' % v for v in loaders[name]]), flush=True)
    out['next_ms_B128'] = {k: {'windows_ms': v, 'median_ms': statistics.median(v)} for k, v in loaders.items()}
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, 'pool_step_ms.json')
    json.dump(out, open(path, 'w'), indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
