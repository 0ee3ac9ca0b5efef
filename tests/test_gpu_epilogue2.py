"""The register epilogue of the 256x256 conv GEMM kernel (p8_regs_epilogue in csrc/zs_gemm.hip), forced at small shapes
(gemm_p8 = 1, gemm_p8_min_tiles = 0), in the variants whose order of global loads and stores was rebuilt: two outputs
(out2 = out + vec2[idx], rows and SPLIT2, with pre_vec) and one output with a second operand (dact_src / add_src, with colsum
before and after the mask).
(i) out, out2 and colsum have the bytes recorded from the kernel before that change (tests/golden/epilogue2_parent.npz, written
    by tools/make_golden_epilogue2.py): the fp32 expressions, the zeroed columns and the row mapping are the same, only the order
    of the memory operations moved;
(ii) the same buffers against the fp64 reference at the bound of tests/test_gpu_gemm.py, with its NaN guards: nothing outside
    [rows, out_cols) is written (a failure names the element);
(iii) two launches of a case are bit-equal.
Operands, launch and reference are those of tests/test_gpu_gemm.py (its Spec / Data / launch / reference / check_outputs)."""
import hashlib
import os

import numpy as np
import pytest
import torch

import test_gpu_gemm as G
from test_gpu_gemm import Spec

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'epilogue2_parent.npz')
SAMPLE_EVERY = 97
DTYPE = 'bf16'
PATH = 'P8'

_DG = dict(gather=1, B=5, T=64, N=264)          # 256 % T == 0 (colsum); N: a second column tile of 8 columns
CASES = [
    # samples change inside a wave's 16-row blocks, M = 288 is no multiple of 256, N has a partial 8-group and zero columns
    Spec('out2_rows_vec2', B=18, T=16, N=72, k=1, bias=True, out2='rows', vec2=True),
    # out and out2 both SPLIT2; the second column tile is mostly empty
    Spec('split2_both_vec2', B=17, T=16, N=272, k=3, bias=True, act=True, out='split', out2='split', vec2=True),
    Spec('out2_split_vec2_prevec', B=9, T=32, N=96, k=1, out2='split', vec2=True, pre_vec=True),
    # M = 528, N = 520: three row tiles and three column tiles, the last of each partial
    Spec('out2_rows_vec2_3x3_tiles', B=33, T=16, N=520, k=1, bias=True, act=True, out2='rows', vec2=True),
    Spec('dgrad_dact', dact=True, **_DG),
    Spec('dgrad_add', add='t', **_DG),
    Spec('dgrad_dact_add', dact=True, add='t', **_DG),
    Spec('dgrad_dact_colsum', dact=True, colsum=(16, 0, 1), **_DG),
    Spec('dgrad_add_colsum', add='t', colsum=(0, 0, 1), **_DG),
    Spec('dgrad_dact_colsum_post', dact=True, colsum=(16, 1, 1), **_DG),
]
NAMES = [sp.name for sp in CASES]
BY_NAME = {sp.name: sp for sp in CASES}


def digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.numpy()).tobytes()).hexdigest()


def samples(t):
    """every 97th element's fp32 bits (the buffers hold NaN guards: compared as integers)"""
    return np.ascontiguousarray(t.numpy()).reshape(-1)[::SAMPLE_EVERY].view(np.uint32).copy()


def run_case(L, name):
    """Operands of a case, its plan, and the host copies of two launches' whole output buffers (guards included)."""
    sp = BY_NAME[name]
    g = G.geometry(sp, DTYPE, PATH)
    d = G.Data(sp, DTYPE, g)
    dev = G.Device(sp, DTYPE, d)
    plan, outs = G.launch(L, sp, DTYPE, g, d, dev, PATH)
    plan2, outs2 = G.launch(L, sp, DTYPE, g, d, dev, PATH)
    assert plan == plan2
    return sp, g, d, plan, outs, outs2


@pytest.fixture(scope='module')
def zs():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    from zs_amd import _lib
    _lib.lib()
    return _lib


_RUNS = {}


def _runs(zs, name):
    if name not in _RUNS:
        _RUNS[name] = run_case(zs, name)
    return _RUNS[name]


@pytest.mark.parametrize('name', NAMES)
def test_takes_the_register_epilogue(zs, name):
    _, _, _, plan, _, _ = _runs(zs, name)
    assert plan == ('P8', 1), plan


@pytest.mark.parametrize('name', NAMES)
def test_bytes_equal_parent(zs, name):
    z = np.load(GOLDEN, allow_pickle=False)
    _, _, _, _, outs, _ = _runs(zs, name)
    assert sorted(outs) == sorted(k.split('.')[1][:-7] for k in z.files if k.startswith(name + '.') and k.endswith('_sha256'))
    for key in sorted(outs):
        if digest(outs[key]) != str(z['%s.%s_sha256' % (name, key)]):
            got, want = samples(outs[key]), z['%s.%s_samples' % (name, key)]
            bad = np.flatnonzero(got != want)
            pytest.fail('%s %s: bytes differ from the parent kernel; %d of %d sampled elements differ, first at flat index %s: %r != %r'
                        % (name, key, bad.size, got.size, bad[:1] * SAMPLE_EVERY, got[bad[:1]].view(np.float32), want[bad[:1]].view(np.float32)))


@pytest.mark.parametrize('name', NAMES)
def test_against_fp64_and_guards(zs, name):
    sp, g, d, (path, regs), outs, _ = _runs(zs, name)
    refs = G.reference(sp, DTYPE, g, d, bool(regs))
    G.check_outputs('epilogue2/%s/%s/%s' % (name, path, DTYPE), sp, g, outs, refs, ('epilogue2', path, DTYPE))


@pytest.mark.parametrize('name', NAMES)
def test_two_launches_bit_equal(zs, name):
    _, _, _, _, outs, outs2 = _runs(zs, name)
    for key in sorted(outs):
        assert digest(outs[key]) == digest(outs2[key]), '%s %s differs between two launches' % (name, key)
