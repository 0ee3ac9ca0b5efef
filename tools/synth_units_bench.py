"""What speech from units costs: on 64 utterances of 200-700 frames, full-size english model (random weights, bf16),
Griffin-Lim n_iter = 300, enc_only, in one process, alternated repetition by repetition,
  (a) synth_units_batch on the packed units of encode_batch    units in: zs_units_unpack, Decoder, vocoder
  (b) resynth_batch of the same spectrograms                   spectrograms in: Encoder, Decoder, vocoder
  (c) encode_batch, encoder only                               the encoder share of (b)
  (d) encode_batch(packed=True), encoder only                  (c) with zs_units_pack and one D2H copy of the units
The expectation to confirm or refute: (a) costs no more than (b) - (c).  Host clock around each call (all end in a wait for their last
copy); medians, minima and maxima over the repetitions.  The bytes encode_batch copies to the host with and without `packed` are
counted from the chunk shapes.  The two kernels alone are timed with HIP events on one chunk of 256 fragments of seg_len / 8 units.
    python tools/synth_units_bench.py [--utts 64] [--reps 7] [--warmup 2] [--n-iter 300] [--out profiles/synth_units_bench.json]"""
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
from zs_amd.hps import make_hps  # noqa: E402
from zs_amd.trainer import Trainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--dtype', default='bf16'); ap.add_argument('--utts', type=int, default=64); ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--warmup', type=int, default=2); ap.add_argument('--n-iter', type=int, default=300)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'synth_units_bench.json'))
a = ap.parse_args()
if a.reps < 7 or a.warmup < 2:
    ap.error('at least 7 repetitions after 2 warm-ups')
if not torch.cuda.is_available():
    sys.exit('synth_units_bench needs an MI355X: a timing taken anywhere else says nothing about it')
dev = torch.device('cuda:0')

hps = make_hps(enc_size=1024, emb_size=1024, n_speakers=102)
torch.manual_seed(0)
tr = Trainer(hps, None, 'naive', 'multilabel_binary', log_dir=tempfile.mkdtemp(), dtype=a.dtype, device=dev)
E, seg = int(hps.enc_size), int(hps.seg_len)
rng = np.random.RandomState(0)
frames = [int(n) for n in rng.randint(200, 701, size=a.utts)]
specs = [(rng.rand(n, 513) * 0.98 + 1e-3).astype(np.float32) for n in frames]
spk = [100 + (i % 2) for i in range(a.utts)]
units, _ = cv.encode_batch(specs, tr, seg, packed=True)             # what a user holds: E / 8 bytes per unit

paths = {'a': lambda: cv.synth_units_batch(units, tr, seg, spk, n_iter=a.n_iter, packed=True),
         'b': lambda: cv.resynth_batch(specs, tr, seg, spk, n_iter=a.n_iter),
         'c': lambda: cv.encode_batch(specs, tr, seg),
         'd': lambda: cv.encode_batch(specs, tr, seg, packed=True)}


def stats(ms):
    return {'median_ms': round(float(np.median(ms)), 2), 'min_ms': round(min(ms), 2), 'max_ms': round(max(ms), 2),
            'all_ms': [round(x, 2) for x in ms]}


times = {k: [] for k in paths}
order = sorted(paths)
for rep in range(a.warmup + a.reps):
    for name in (order if rep % 2 == 0 else order[::-1]):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        paths[name]()
        torch.cuda.synchronize()
        if rep >= a.warmup:
            times[name].append((time.perf_counter() - t0) * 1e3)
st = {k: stats(v) for k, v in times.items()}
spread = max(s['max_ms'] - s['min_ms'] for s in st.values())
budget = st['b']['median_ms'] - st['c']['median_ms']

# bytes encode_batch brings to the host for the units: fp32 [n, E, T'] per chunk (padded to the chunk's longest member) against
# one buffer of (E + 7) // 8 bytes per unit
n_units = sum(len(u) for u in units)
items = []
for n in frames:
    items += [b_ - a_ for a_, b_ in cv.fragments(n, seg)] if n > seg else [n]
full = [n for n in items if n == seg]
rest = sorted((n for n in items if n != seg), reverse=True)
chunks = [full[lo:lo + 256] for lo in range(0, len(full), 256)] + [rest[lo:lo + 256] for lo in range(0, len(rest), 256)]
plain_bytes = sum(len(c) * cv._t8(max(c)) * E * 4 for c in chunks)
packed_bytes = n_units * ((E + 7) // 8)

# the two kernels alone: one chunk of 256 fragments of seg / 8 units, HIP events around each launch
B, T, ld, rb = 256, seg // 8, (E + 31) // 32 * 32, (E + 7) // 8
zdt, tdt = (L.ZS_BF16, torch.bfloat16) if a.dtype == 'bf16' else (L.ZS_F32, torch.float32)
pk = torch.randint(0, 256, (B * T, rb), dtype=torch.uint8, device=dev)
start = (torch.arange(B, dtype=torch.int64, device=dev) * T).contiguous()
length = torch.full((B,), T, dtype=torch.int32, device=dev)
wide = torch.zeros(B * T * ld, dtype=tdt, device=dev)
out = torch.zeros_like(pk)
stream = torch.cuda.current_stream().cuda_stream


def unpack():
    L.call('zs_units_unpack', 'ZsUnitsUnpack', stream, dtype=zdt, packed=L.ptr(pk), n_units=B * T, row_bytes=rb, E=E, start=L.ptr(start),
           len=L.ptr(length), n_frag=B, T=T, dst=L.ptr(wide), ld_dst=ld)


def pack():
    L.call('zs_units_pack', 'ZsUnitsPack', stream, dtype=zdt, src_f32=0, src=L.ptr(wide), ld_src=ld, n_frag=B, T=T, E=E, start=L.ptr(start),
           len=L.ptr(length), packed=L.ptr(out), n_units=B * T, row_bytes=rb)


def events(fn, n=30):
    for _ in range(5):
        fn()
    ev = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
    return {'median_us': round(us[len(us) // 2], 1), 'min_us': round(us[0], 1), 'max_us': round(us[-1], 1)}


k_un, k_pk = events(unpack), events(pack)
assert torch.equal(out, pk)                                          # pack(unpack(x)) == x at the timed shape
moved = B * T * (ld * wide.element_size() + rb)
record = {'utts': a.utts, 'frames': [min(frames), max(frames)], 'units': n_units, 'n_iter': a.n_iter, 'dtype': a.dtype, 'reps': a.reps,
          'warmup': a.warmup, 'device': torch.cuda.get_device_name(0),
          'paths': {'a': 'synth_units_batch(packed units)', 'b': 'resynth_batch', 'c': 'encode_batch (encoder only)',
                    'd': 'encode_batch(packed=True) (encoder only)'},
          'a': st['a'], 'b': st['b'], 'c': st['c'], 'd': st['d'], 'largest_spread_ms': round(spread, 2),
          'b_minus_c_median_ms': round(budget, 2), 'a_minus_budget_ms': round(st['a']['median_ms'] - budget, 2),
          'a_within_b_minus_c': bool(st['a']['median_ms'] <= budget),
          'a_within_b_minus_c_plus_spread': bool(st['a']['median_ms'] <= budget + spread),
          'd_minus_c_median_ms': round(st['d']['median_ms'] - st['c']['median_ms'], 2),
          'encode_batch_d2h_bytes': {'plain': plain_bytes, 'packed': packed_bytes, 'ratio': round(plain_bytes / float(packed_bytes), 1)},
          'kernels': {'shape': {'n_frag': B, 'T': T, 'E': E, 'ld': ld, 'row_bytes': rb, 'bytes_moved': moved},
                      'zs_units_unpack': dict(k_un, GBps_at_median=round(moved / (k_un['median_us'] * 1e-6) / 1e9, 1)),
                      'zs_units_pack': dict(k_pk, GBps_at_median=round(moved / (k_pk['median_us'] * 1e-6) / 1e9, 1)),
                      'note': 'events around one launch each: the time includes the launch gap'}}
print('(a) synth from units %.1f ms   (b) resynth %.1f ms   (c) encoder %.1f ms   (d) encoder, packed %.1f ms   b - c = %.1f ms' %
      (st['a']['median_ms'], st['b']['median_ms'], st['c']['median_ms'], st['d']['median_ms'], budget))
print('D2H bytes of the units: %d plain, %d packed;  unpack %.1f us, pack %.1f us' % (plain_bytes, packed_bytes, k_un['median_us'],
                                                                                       k_pk['median_us']))
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, 'w') as f:
    json.dump(record, f, indent=1)
print(json.dumps({'a_minus_budget_ms': record['a_minus_budget_ms'], 'largest_spread_ms': record['largest_spread_ms']}))
