"""What a checkpoint costs the --train_ae loop: the stall per checkpoint of the synchronous weights-only save against the resumable
save (weights + train state, written by a worker thread), and the step time between checkpoints with and without --resume.

  python tools/ckpt_bench.py [--out profiles] [--every 300] [--ckpts 3] [--rounds 3] [--ckpt_dir DIR]
      One process, one Trainer at hps/zerospeech_english_1024.json, B = 256, bf16, the captured host-fed step, no logged
      iteration inside a window (ZS_LOG_EVERY large: the host runs ahead of the GPU as in a real run).  A window is
      N = ckpts * every + every / 2 iterations of Trainer._loop's body: the step, the batch count, and at every `every`-th
      iteration the checkpoint of its arm; it ends, as Trainer.train does, by waiting for the writer and the device.  Arms,
      interleaved, `rounds` windows each:
        none        no checkpoint                                     resume=False
        sync        Trainer.save_model (weights only, synchronous)    resume=False: every checkpoint of a run without --resume
        resumable   Trainer._checkpoint_async (weights + state)       resume=True
        counted     no checkpoint falls in the window                 resume=True (the batch counts are the only difference)
      stall of an arm = (its median window - none's median window) / ckpts.  Medians, spreads (max - min), both stalls, the
      ms/iteration of `none` and `counted` and the bytes each kind of checkpoint writes -> <out>/ckpt_stall.json
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 256


def parse():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles'))
    p.add_argument('--every', type=int, default=300)
    p.add_argument('--ckpts', type=int, default=3)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--ckpt_dir', default=None, help='where the checkpoints are written (default: a temporary directory, removed)')
    return p.parse_args()


def main():
    args = parse()
    os.environ['ZS_LOG_EVERY'] = '1000000'
    import torch
    import zs_amd  # noqa: F401
    from zs_amd import resume
    from zs_amd.dataloader import DataLoader, SyntheticDataset
    from zs_amd.hps import Hps
    from zs_amd.trainer import Trainer
    if not torch.cuda.is_available():
        sys.exit('ckpt_bench.py needs the GPU')
    dev = torch.device('cuda:0')
    hps = Hps(os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')).get_tuple()._replace(batch_size=B, max_to_keep=3)
    ds = SyntheticDataset(9 * B, seg_len=hps.seg_len, n_speakers=hps.n_speakers, seed=0)
    ckpt_dir = args.ckpt_dir or tempfile.mkdtemp(prefix='zs_ckpt_bench_')
    os.makedirs(ckpt_dir, exist_ok=True)
    torch.manual_seed(1234)
    tr = Trainer(hps, DataLoader(ds, B), hps.g_mode, hps.enc_mode, log_dir=os.path.join(ckpt_dir, 'log'), dtype='bf16', device=dev)
    feeder = tr.ae.host_feeder(tr.data_loader)
    n_iters = args.ckpts * args.every + args.every // 2
    sizes = {}

    def window(arm, tag):
        """One window of the arm; returns its wall time in seconds."""
        model_path = os.path.join(ckpt_dir, 'model_%s.pth' % tag)
        tr.reset_keep()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(n_iters):
            next(feeder)
            if arm in ('resumable', 'counted'):
                tr._took('data')
            if (it + 1) % args.every == 0:
                if arm == 'sync':
                    tr.save_model(model_path, 'ae', it + 1)
                elif arm == 'resumable':
                    tr._checkpoint_async(model_path, 'ae', it + 1, False, False)
        tr._finish_writer()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        for p in list(tr.model_kept):                                      # bytes written per checkpoint, then free the disk
            sizes.setdefault(arm, {'checkpoint': os.path.getsize(p),
                                   'train_state': os.path.getsize(resume.state_path(p)) if os.path.exists(resume.state_path(p)) else 0})
            resume.remove_checkpoint(p)
        return dt

    arms = ['none', 'sync', 'resumable', 'counted']
    for arm in arms:                                                       # warm-up steps, capture, pinned and snapshot buffers
        print('warm-up %-9s %.2f s' % (arm, window(arm, 'warm')), flush=True)
    secs = {a: [] for a in arms}
    for r in range(args.rounds):
        for arm in arms:
            secs[arm].append(window(arm, 'r%d' % r))
            print('round %d %-9s %.3f s (%d iterations)' % (r, arm, secs[arm][-1], n_iters), flush=True)
    med = {a: statistics.median(v) for a, v in secs.items()}
    spread = {a: max(v) - min(v) for a, v in secs.items()}
    out = {'what': 'wall time of %d --train_ae iterations (captured host-fed step, B=256 bf16, hps/zerospeech_english_1024.json) with a '
                   'checkpoint every %d (%d per window); %d interleaved rounds, one process; host clock around a device synchronise, '
                   'the wait for the checkpoint writer included' % (n_iters, args.every, args.ckpts, args.rounds),
           'arms': {a: {'windows_s': secs[a], 'median_s': med[a], 'spread_s': spread[a]} for a in arms},
           'bytes_per_checkpoint': sizes,
           'stall_ms_per_checkpoint': {a: 1e3 * (med[a] - med['none']) / args.ckpts for a in ('sync', 'resumable')},
           'ms_per_iteration': {a: 1e3 * med[a] / n_iters for a in ('none', 'counted')},
           'ms_per_iteration_spread': {a: 1e3 * spread[a] / n_iters for a in ('none', 'counted')}}
    st = out['stall_ms_per_checkpoint']
    out['resumable_stall_not_above_sync'] = bool(st['resumable'] <= st['sync'])
    os.makedirs(args.out, exist_ok=True)
    json.dump(out, open(os.path.join(args.out, 'ckpt_stall.json'), 'w'), indent=1)
    print(json.dumps(out))
    if args.ckpt_dir is None:
        shutil.rmtree(ckpt_dir, ignore_errors=True)


if __name__ == '__main__':
    main()
