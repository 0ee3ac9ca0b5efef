"""Voice adaptation step time at the bench configuration (hps/zerospeech_english_1024.json: seg_len 128, 513 bins, emb_size and
enc_size 1024, 102 speakers; bf16, B = hps.batch_size):

  (a) the replayed VoiceStep iteration (zs_amd.voice) against AEStep's counted, replayed step at the same B in the same process --
      what fine-tuning every weight would cost per iteration; the ratio is reported, there is no target;
  (b) the VoiceStep iteration with zs_voice_adam against the same iteration with the eight launches it replaces (five
      zs_emb_scatter, the two of zs_sqnorm, one zs_adam_clip over the five rows, which are adjacent in the decoder's flat
      parameter buffer), both captured: ComposedStep below;
  (c) zs_voice_gather alone, as a replayed graph of one call.

Everything is built side by side and measured interleaved: R rounds, each timing K replays of every variant in turn (order rotated
per round), after a warm-up per variant; the median, minimum and maximum over the rounds are reported.  bench.py does not call
this.  Prints one JSON line; --out FILE also writes it there.
    python tools/voice_bench.py [--rounds 7] [--steps 20] [--warmup 5] [--out profiles/voice_step_ms.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def composed_step(voice, L):
    """VoiceStep with the eight launches zs_voice_adam replaces in its place (the A/B baseline; nothing else differs).  Its norm is
    zs_sqnorm's, summed in another order than zs_voice_adam's, so the two runs agree to rounding, not to the bit."""

    class ComposedStep(voice.VoiceStep):
        def adam(self):
            st, n, C, B = self.de.ctx.stream, voice.N_ROWS * self.C, self.C, self.B
            p0 = self.row_params[0].data_ptr()
            if [p.data_ptr() for p in self.row_params] != [p0 + 4 * k * C for k in range(voice.N_ROWS)]:
                raise RuntimeError('the five rows are not adjacent in the flat parameter buffer')
            for k in range(voice.N_ROWS):
                L.call('zs_emb_scatter', 'ZsEmbScatter', st, emb_sum=L.ptr(self.de._embsum, k * B * C), emb_ld=C, idx=L.ptr(self.cidx),
                       B=B, demb=L.ptr(self.g, k * C), demb_ld=C, n_rows=1, C=C, accumulate=0)
            L.check(L.lib().zs_sqnorm(L.ptr(self.g), n, L.ptr(self.part), L.ptr(self.sumsq), st), 'zs_sqnorm')
            L.call('zs_adam_clip', 'ZsAdam', st, p=p0, g=L.ptr(self.g), m=L.ptr(self.m), v=L.ptr(self.v), n=n, lr=self.lr,
                   beta1=self.betas[0], beta2=self.betas[1], eps=1e-8, bc1=1.0, bc2=1.0, sumsq=L.ptr(self.sumsq),
                   max_norm=self.max_norm, step_ptr=L.ptr(self._step_dev))
    return ComposedStep


def build(dev, dtype, B):
    from zs_amd import _lib as L
    from zs_amd import voice
    from zs_amd.hps import Hps
    from zs_amd.model import Decoder, Encoder
    from zs_amd.trainer import AEStep
    hps = Hps(os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')).get_tuple()
    B = B or hps.batch_size
    seg_len, F, E, nspk = hps.seg_len, 513, hps.enc_size, hps.n_speakers
    torch.manual_seed(1234)
    enc = Encoder(ns=hps.ns, dp=hps.enc_dp, enc_size=E, seg_len=seg_len, enc_mode='multilabel_binary', dtype=dtype).to(dev)
    dec = Decoder(ns=hps.ns, c_in=E, c_h=hps.emb_size, c_a=nspk, seg_len=seg_len, dtype=dtype).to(dev)
    ae = AEStep(enc, dec, lr=hps.lr, max_grad_norm=hps.max_grad_norm, use_graph=True)
    g = torch.Generator().manual_seed(99)
    xs, cs = ae.static_inputs(B, seg_len, F)
    xs.copy_(torch.rand(B, seg_len, F, generator=g) * (1 - 1e-8) + 1e-8)
    cs.copy_(torch.randint(0, nspk, (B,), generator=g))
    # a voice's data: 24 utterances of 3 to 6 s (300 to 600 frames), random spectrograms and units
    rng = np.random.RandomState(7)
    lens = rng.randint(300, 601, size=24)
    specs = [(rng.rand(n, F) * 0.98 + 1e-3).astype(np.float32) for n in lens]
    units = [np.packbits(rng.randint(0, 2, size=((n - 1) // 8, E)).astype(bool), axis=1, bitorder='little') for n in lens]
    vset = voice.VoiceSet(specs, units, seg_len, dev, seed=7)
    rows = voice.init_rows(dec.state_dict())
    mk = lambda cls: cls(dec, vset, B, rows, lr=hps.lr, max_grad_norm=hps.max_grad_norm, use_graph=True)
    fused, composed, gat = mk(voice.VoiceStep), mk(composed_step(voice, L)), mk(voice.VoiceStep)
    composed.part = torch.zeros(1024, dtype=torch.float64, device=dev)
    return hps, B, ae, xs, cs, fused, composed, gat


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--batch', type=int, default=0, help='default: hps.batch_size')
    p.add_argument('--dtype', default='bf16')
    p.add_argument('--out', default=None)
    args = p.parse_args()
    import zs_amd  # noqa: F401
    from zs_amd import layers
    dev = torch.device('cuda:0')
    hps, B, ae, xs, cs, fused, composed, gat = build(dev, args.dtype, args.batch)
    gat.gather()                                           # eagerly once: the operand buffer exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        gat.gather()
    variants = {'ae_step': lambda: ae.step(xs, cs), 'voice_step': fused.step, 'voice_step_composed': composed.step,
                'voice_gather': graph.replay}
    for name, fn in variants.items():
        for _ in range(3 + args.warmup):                   # 2 eager iterations + the capture, then warm-up replays
            fn()
        torch.cuda.synchronize()
    names = list(variants)
    ms = {n: [] for n in names}
    for r in range(args.rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:
            fn = variants[name]
            fn()                                           # one untimed replay after switching variants
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    layers.check_status(dev)
    stat = lambda v: {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4)}
    out = {'metric': 'voice_step_ms', 'batch': B, 'dtype': args.dtype, 'seg_len': hps.seg_len, 'c_h': hps.emb_size, 'enc_size': hps.enc_size,
           'rounds': args.rounds, 'steps_per_round': args.steps, 'device': torch.cuda.get_device_name(dev),
           'variants': {n: stat(ms[n]) for n in names}}
    v = out['variants']
    out['voice_step_over_ae_step'] = round(v['voice_step']['median_ms'] / v['ae_step']['median_ms'], 4)
    spread = max(max(ms[n]) - min(ms[n]) for n in ('voice_step', 'voice_step_composed'))
    out['adam'] = {'fused_minus_composed_ms': round(v['voice_step']['median_ms'] - v['voice_step_composed']['median_ms'], 4),
                   'rounds_max_minus_min_ms': round(spread, 4),
                   'keep_fused': bool(v['voice_step']['median_ms'] <= v['voice_step_composed']['median_ms'] + spread)}
    moved = B * hps.seg_len * 513 * 4 * 2 + B * (hps.seg_len // 8) * (hps.enc_size // 8 + hps.enc_size * (4 if args.dtype == 'fp32' else 2))
    out['variants']['voice_gather']['GBps_at_median'] = round(moved / (v['voice_gather']['median_ms'] * 1e-3) / 1e9, 1)
    out['final_loss'] = {'voice_step': float(fused._loss.item()), 'voice_step_composed': float(composed._loss.item())}
    out['iterations'] = {'voice_step': fused.iteration, 'voice_step_composed': composed.iteration}
    drift = max(float(abs(a - b).max()) for a, b in zip(fused.rows(), composed.rows()))
    out['rows_max_abs_diff_fused_vs_composed'] = drift
    out['rows_max_abs_diff_bound_lr_times_iterations'] = hps.lr * fused.iteration        # (no Adam step is longer than about lr)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
