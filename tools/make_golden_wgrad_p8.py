"""Records what gemm_wgrad_p8_kernel computes for the cases of tests/test_gpu_wgrad_p8.py (GPU):
  python tools/make_golden_wgrad_p8.py [--out tests/golden/wgrad_p8_parent.npz]
Per case: the SHA-256 of the dW and db bytes, and every 97th element as fp32 (a readable diff when a digest fails).
Run it at the commit whose results are the reference (before the kernel is changed); the test then holds later kernels to it."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_gpu_wgrad_p8 as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=T.GOLDEN)
a = ap.parse_args()

import zs_amd  # noqa: E402,F401
from zs_amd import _lib as L, layers  # noqa: E402

L.lib()
out = {}
for name in sorted(T.CASES):
    w, b = T.run_case(L, layers, name)
    w2, b2 = T.run_case(L, layers, name)
    assert (w == w2).all() and (b == b2).all(), '%s: two runs differ' % name
    for key, t in (('dw', w), ('db', b)):
        out['%s.%s_sha256' % (name, key)] = np.array(T.digest(t))
        out['%s.%s_samples' % (name, key)] = T.samples(t)
    print('%-28s %s dW %s db %s' % (name, 'carried' if T.carried_path(T.CASES[name][0]) else 'general', T.digest(w)[:16], T.digest(b)[:16]),
          flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
np.savez_compressed(a.out, **out)
print('wrote %s (%d bytes)' % (a.out, os.path.getsize(a.out)))
