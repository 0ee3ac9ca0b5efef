"""Records what the register epilogue of the 256x256 conv GEMM kernel writes for the cases of tests/test_gpu_epilogue2.py (GPU):
  python tools/make_golden_epilogue2.py [--out tests/golden/epilogue2_parent.npz]
Per case and output buffer (out, out2, colsum; NaN guards included): the SHA-256 of the bytes, and every 97th element's bits (a
readable diff when a digest fails).  Run it at the commit whose results are the reference (before the epilogue is changed); the
test then holds later kernels to it."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_gpu_epilogue2 as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=T.GOLDEN)
a = ap.parse_args()

import zs_amd  # noqa: E402,F401
from zs_amd import _lib as L  # noqa: E402

L.lib()
out = {}
for name in T.NAMES:
    sp, g, d, plan, outs, outs2 = T.run_case(L, name)
    assert plan == ('P8', 1), (name, plan)
    for key in sorted(outs):
        assert T.digest(outs[key]) == T.digest(outs2[key]), '%s %s: two launches differ' % (name, key)
        out['%s.%s_sha256' % (name, key)] = np.array(T.digest(outs[key]))
        out['%s.%s_samples' % (name, key)] = T.samples(outs[key])
    print('%-28s %s' % (name, '  '.join('%s %s' % (k, T.digest(outs[k])[:16]) for k in sorted(outs))), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
np.savez_compressed(a.out, **out)
print('wrote %s (%d bytes)' % (a.out, os.path.getsize(a.out)))
