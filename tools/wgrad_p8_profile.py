"""Where a launch of gemm_wgrad_p8_kernel spends its cycles: reads the in-kernel stamps of a -DZS_WGP8_PROFILE build.
  hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -DZS_WGP8_PROFILE -shared -o libzs_prof.so zerospeech-tts-without-t_amd/csrc/*.hip
  ZS_LIB_PATH=libzs_prof.so python tools/wgrad_p8_profile.py [--B 256 --T 128 --cin 1024 --cout 1024 --k 1]
Waves 0 and 4 of every workgroup (one per wave group of the ping-pong schedule) stamp the cycle counter; the table is the mean
per workgroup, and per K tile for the phases.  The stamps cost time themselves (a scalar memory-time read and a wait each):
compare the shares, not the total, with an unstamped launch."""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zs_amd  # noqa: E402,F401
from zs_amd import _lib as L, layers  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--B', type=int, default=256); ap.add_argument('--T', type=int, default=128)
ap.add_argument('--cin', type=int, default=1024); ap.add_argument('--cout', type=int, default=1024)
ap.add_argument('--k', type=int, default=1); ap.add_argument('--iters', type=int, default=5)
a = ap.parse_args()
os.environ['ZS_OVERLAP_WGRAD'] = '0'
lib = L.lib()
if not hasattr(lib, 'zs_wgp8_profile_read'):
    sys.exit('this library was built without -DZS_WGP8_PROFILE')
ctx = layers.Ctx('cuda:0', 'bf16')
w = torch.randn(a.cout, a.cin, a.k, device=ctx.device) * 0.02
b = torch.zeros(a.cout, device=ctx.device)
l = layers.ConvLayer(ctx, w, b, torch.zeros_like(w), torch.zeros_like(b))
l.pack()
X = ctx.act('x', a.B, a.T, a.cin); X.t.normal_()
Y = ctx.act('y', a.B, a.T, a.cout); Y.t.normal_()
L.set_option('wgrad_p8', 1)
buf = (ctypes.c_ulonglong * 48)()
l.wgrad(Y, X)
assert lib.zs_wgp8_profile_read(buf, 1) == 0
for _ in range(a.iters):
    l.wgrad(Y, X)
assert lib.zs_wgp8_profile_read(buf, 1) == 0
NAMES = ['prologue'] + ['phase %d %s' % (ph, part) for ph in (1, 2, 3, 4) for part in ('read', 'open barrier', 'mfma', 'close barrier')] + \
        ['drain + bias', 'slab store']
print('wgrad p8 stamps  B%d T%d cin%d cout%d k%d, %d launches' % (a.B, a.T, a.cin, a.cout, a.k, a.iters))
for g in range(2):
    v = [buf[g * 24 + i] for i in range(24)]
    tiles, wgs = v[19], v[20]
    if wgs == 0:
        sys.exit('no stamps: the launch did not take gemm_wgrad_p8_kernel')
    total = float(sum(v[:19]))
    print('wave group %d: %d workgroups, %.1f K tiles each, %.0f cycles per workgroup, %.0f per K tile in the loop'
          % (g, wgs, tiles / wgs, total / wgs, sum(v[1:17]) / max(tiles, 1)))
    for i, n in enumerate(NAMES):
        per = v[i] / max(tiles, 1) if 1 <= i <= 16 else v[i] / wgs
        print('  %-22s %9.0f cycles %s  %5.1f %%' % (n, per, 'per K tile    ' if 1 <= i <= 16 else 'per workgroup ', 100.0 * v[i] / total))
