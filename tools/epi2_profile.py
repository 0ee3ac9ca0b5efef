"""Where the register epilogue of the 256x256 conv GEMM kernel (p8_regs_epilogue) spends its cycles: reads the in-kernel stamps of
a -DZS_EPI2_PROFILE build.
  hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -DZS_EPI2_PROFILE -shared -o libzs_prof.so zerospeech-tts-without-t_amd/csrc/*.hip
  ZS_LIB_PATH=libzs_prof.so python tools/epi2_profile.py [--iters 5]
Waves 0 and 4 of every workgroup stamp the cycle counter around each phase; the table is the mean per workgroup in shader cycles
(about 2 GHz under this load) for the epilogue variants of tools/epi_bench.py at M = 32768, N = K = 1024.  The last phase, `drain`,
is a wait for all of the wave's stores that only this build has: in the product build the wave ends with its stores in flight.
The stamps cost time themselves (a scalar memory-time read and a wait each): compare phases, not totals, with an unstamped launch."""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zs_amd  # noqa: E402,F401
from zs_amd import _lib as L, layers  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=5)
a = ap.parse_args()
lib = L.lib()
if not hasattr(lib, 'zs_epi2_profile_read'):
    sys.exit('this library was built without -DZS_EPI2_PROFILE')
ctx = layers.Ctx('cuda:0', 'bf16')
dev = ctx.device
B, T, C = 256, 128, 1024
w = torch.randn(C, C, device=dev) * 0.02
b = torch.zeros(C, device=dev)
lin = layers.ConvLayer(ctx, w, b, torch.zeros_like(w), torch.zeros_like(b))
lin.pack()


def act(name):
    x = ctx.act(name, B, T, C)
    x.t.normal_()
    return x


X, Y, Y2, D, R = act('x'), act('y'), act('y2'), act('d'), act('r')
emb = torch.randn(102, C, device=dev)
idx = torch.randint(0, 102, (B,), device=dev)
CASES = [
    ('plain (bias + lrelu)', lambda: lin.fwd(X, out=Y, act=L.ZS_ACT_LRELU, slope=0.01)),
    ('dual: + out2 = out + emb[idx]', lambda: lin.fwd(X, out=Y, act=L.ZS_ACT_LRELU, slope=0.01, out2=Y2, vec2=emb, idx=idx)),
    ('dgrad plain', lambda: lin.dgrad(Y, T, D)),
    ("dgrad * lrelu'(dact)", lambda: lin.dgrad(Y, T, D, dact_src=X, slope=0.01)),
    ('dgrad + add_src', lambda: lin.dgrad(Y, T, D, add_src=R)),
    ('dgrad dact + add', lambda: lin.dgrad(Y, T, D, dact_src=X, slope=0.01, add_src=R)),
]
NAMES = ['staging 1', 'barrier', 'copy-out 1 (issue)', 'barrier', 'staging 2', 'barrier', 'copy-out 2 (issue)', 'drain']
buf = (ctypes.c_ulonglong * 24)()
print('p8_regs_epilogue stamps, B%d T%d N%d K%d, %d launches per case; cycles per workgroup, wave group 0 | wave group 1' % (B, T, C, C, a.iters))
for name, fn in CASES:
    fn()
    assert lib.zs_epi2_profile_read(buf, 1) == 0
    for _ in range(a.iters):
        fn()
    assert lib.zs_epi2_profile_read(buf, 1) == 0
    v = [[buf[g * 12 + i] for i in range(12)] for g in range(2)]
    if v[0][8] == 0:
        sys.exit('no stamps: the launch did not take the register epilogue')
    print('%s: %d workgroups per launch' % (name, v[0][8] // a.iters))
    for i, n in enumerate(NAMES):
        print('  %-20s %8.0f | %8.0f' % (n, v[0][i] / v[0][8], v[1][i] / v[1][8]))
    print('  %-20s %8.0f | %8.0f' % ('sum', sum(v[0][:8]) / v[0][8], sum(v[1][:8]) / v[1][8]))
