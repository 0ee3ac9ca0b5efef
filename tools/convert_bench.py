"""Voice conversion throughput with the stage-2 generator (convert.py:151-168 with enc_only=False): 64 utterances of 200..700 frames,
full-size english model (enc_size = emb_size = 1024, random weights), bf16, Griffin-Lim n_iter = 300, in utterances/s:
  * resynth_batch(enc_only=True)                            the autoencoder-only path (BASELINE config 4), for comparison
  * resynth_batch(enc_only=False), g_mode targeted_residual and spectrogram
  * the per-utterance convert(enc_only=False) loop            (test_step per fragment, one Griffin-Lim per utterance), on a sample
--old-assembly runs the generator batches with the assembly zs_gen_scatter replaced: the chunk outputs copied out, torch.cat,
the padded gather, zs_gen_combine_fwd, zs_gl_denormalize -- the same launches otherwise, for a kernel-trace comparison.
    python tools/convert_bench.py [--utts 64] [--reps 3] [--loop-utts 4] [--n-iter 300] [--modes ...] [--old-assembly]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zs_amd  # noqa: E402,F401
from zs_amd import _lib as L, convert as cv  # noqa: E402
from zs_amd.hps import hp, make_hps  # noqa: E402
from zs_amd.trainer import Trainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--dtype', default='bf16'); ap.add_argument('--utts', type=int, default=64); ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--loop-utts', type=int, default=4); ap.add_argument('--n-iter', type=int, default=300)
ap.add_argument('--modes', default='targeted_residual,spectrogram'); ap.add_argument('--old-assembly', action='store_true')
a = ap.parse_args()
hps = make_hps(enc_size=1024, emb_size=1024, n_speakers=102)
rng = np.random.RandomState(0)
lens = rng.randint(200, 701, size=a.utts)
specs = [np.clip(rng.rand(int(n), 513).astype(np.float32), 1e-8, 1) for n in lens]
spk = [int(rng.randint(100, 102)) for _ in specs]                      # the two target speakers (n_speakers - 2, n_speakers - 1)


def run_old(tr, n_iter):
    """resynth_batch(enc_only=False) with the assembly zs_gen_scatter replaced: the driver's scatter calls are intercepted, each chunk's
    x_dec / generator rows are copied out (the modules' clone()), then torch.cat, the padded gather, zs_gen_combine_fwd and
    zs_gl_denormalize build the vocoder input."""
    dev = tr.device
    st = torch.cuda.current_stream(dev).cuda_stream
    kept, plans = [], []
    real, real_plan = cv.L.call, cv._plan_scatter

    def plan(*args):                                                   # the destination tables, to build the gather index from
        out = real_plan(*args)
        plans.append(out[2])
        return out

    def hooked(fname, sname, stream, **kw):
        if fname != 'zs_gen_scatter':
            return real(fname, sname, stream, **kw)
        if kw['ld_xd'] == 0:                                           # padding rows: the gather's zero row gives them
            return None
        rows = kw['rows']
        xd = torch.empty(rows, 513, dtype=torch.float32, device=dev)   # the modules' clone() of their outputs
        m = torch.empty(rows, 513, dtype=torch.float32, device=dev)
        for dst_t, src, ld in ((xd, kw['xd'], kw['ld_xd']), (m, kw['m'], kw['ld_m'])):
            L.call('zs_cast_rows', 'ZsCastRows', stream, dtype=L.ZS_F32, src=src, ld_src=ld, src_f32=1, dst=L.ptr(dst_t), ld_dst=513,
                   dst_f32=1, col_off=0, rows=rows, cols=513, fill_cols=513, act=L.ZS_ACT_NONE)
        kept.append((xd, m, rows, kw['mode']))
        return None
    cv.L.call, cv._plan_scatter = hooked, plan
    try:
        q = cv._enqueue_encode(specs, tr, 128, spk, None, 256, dec_to_host=False, enc_only=False, denorm=True)
    finally:
        cv.L.call, cv._plan_scatter = real, real_plan
    n_utt, Tm = q.conv.shape[0], q.conv.shape[1]
    xd_all = torch.cat([k[0] for k in kept] + [torch.zeros(1, 513, device=dev)], dim=0)           # torch.cat of the chunk outputs
    m_all = torch.cat([k[1] for k in kept] + [torch.zeros(1, 513, device=dev)], dim=0)
    idx = torch.full((n_utt * Tm,), xd_all.shape[0] - 1, dtype=torch.int64, device=dev)
    base = 0
    for (_, _, rows, _), dsts in zip(kept, plans[0]):
        ok = dsts >= 0
        idx[dsts[ok].long()] = torch.arange(base, base + rows, device=dev)[ok]
        base += rows
    xg, mg = xd_all[idx], m_all[idx]                                                               # the padded gather
    comb = torch.empty(n_utt * Tm, 513, dtype=torch.float32, device=dev)
    L.check(L.lib().zs_gen_combine_fwd(L.ptr(xg), L.ptr(mg), 513, L.ptr(comb), n_utt * Tm, 513, int(kept[0][3] == 2), st), 'zs_gen_combine_fwd')
    amp = torch.empty_like(comb)
    L.check(L.lib().zs_gl_denormalize(L.ptr(comb), L.ptr(amp), comb.numel(), st), 'zs_gl_denormalize')
    return cv._finish_resynth(q, cv._enqueue_vocoder(amp.view(n_utt, Tm, 513), q.ulens, n_iter, True, dev, amplitudes=True), False)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


result = {'utts': a.utts, 'frames': int(lens.sum()), 'dtype': a.dtype, 'n_iter': a.n_iter, 'assembly': 'old' if a.old_assembly else 'scatter'}
for mode in a.modes.split(','):
    torch.manual_seed(1)
    tr = Trainer(hps, None, mode, 'multilabel_binary', log_dir=tempfile.mkdtemp(), dtype=a.dtype)
    if mode == a.modes.split(',')[0]:
        dt, ts = timed(lambda: cv.resynth_batch(specs, tr, 128, spk, n_iter=a.n_iter))
        result['enc_only_utt_s'] = a.utts / dt
        print('resynth_batch(enc_only=True): %.3f s per batch = %.1f utterances/s  (runs %s)' % (dt, a.utts / dt, ['%.4f' % t for t in ts]), flush=True)
    if a.old_assembly:
        dt, ts = timed(lambda: run_old(tr, a.n_iter))
    else:
        dt, ts = timed(lambda: cv.resynth_batch(specs, tr, 128, spk, n_iter=a.n_iter, enc_only=False))
    result['%s_utt_s' % mode] = a.utts / dt
    print('resynth_batch(enc_only=False, %s, %s assembly): %.3f s per batch = %.1f utterances/s  (runs %s)' %
          (mode, result['assembly'], dt, a.utts / dt, ['%.4f' % t for t in ts]), flush=True)
    if a.loop_utts > 0:
        hp.n_iter = a.n_iter
        s2id = {'S%03d' % i: i for i in range(100)}
        s2id.update({'V001': 100, 'V002': 101})
        tars = ['V001' if s == 100 else 'V002' for s in spk]
        loop = lambda: [cv.convert(tr, 128, specs[i], 'S001', tars[i], str(i), s2id, None, enc_only=False, save=[])   # noqa: E731
                        for i in range(a.loop_utts)]
        loop()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        result['%s_convert_loop_utt_s' % mode] = a.loop_utts / dt
        print('convert(enc_only=False, %s) loop: %d utterances in %.3f s = %.2f utterances/s' % (mode, a.loop_utts, dt, a.loop_utts / dt), flush=True)
    del tr
    torch.cuda.empty_cache()
print(json.dumps(result))
