"""The 256x256 ping-pong bf16 weight-gradient kernel (gemm_wgrad_p8_kernel), forced (wgrad_p8 = 2) at explicit split counts:
(i) dW / db digests equal those recorded from the kernel before its K-loop address path and slab store were rebuilt
    (tests/golden/wgrad_p8_parent.npz, written by tools/make_golden_wgrad_p8.py): each lane's MFMA sequence is unchanged, so the
    slabs and their reduction are bit-identical at equal splits;
(ii) the same results against the fp64 reference dY^T * gather(X) at the bound of tests/test_gpu_wgrad_dma.py (its _check_ref);
(iii) two runs of a case are bit-equal.
The cases cover both address paths of the K loop: carried pointers (1-D, stride 1, T_out divides 128) and the general one."""
import hashlib
import os

import numpy as np
import pytest
import torch

import test_gpu_wgrad_dma as D

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wgrad_p8_parent.npz')
SAMPLE_EVERY = 97

_K3 = dict(Cout=512, Cin=256, taps=3, pad_left=1)
_LIN = dict(taps=1, pad_left=0, reflect=False, linear=True)
# name: (Case arguments, splits, db given, accumulate)
CASES = {
    'lin256_m2048_s1': (dict(B=32, T_in=64, T_out=64, Cout=256, Cin=256, **_LIN), 1, True, False),
    'lin1024_m32768_s16': (dict(B=256, T_in=128, T_out=128, Cout=1024, Cin=1024, **_LIN), 16, True, False),
    'lin1024_m32768_s16_acc': (dict(B=256, T_in=128, T_out=128, Cout=1024, Cin=1024, **_LIN), 16, True, True),
    'k3_t16_s3': (dict(B=128, T_in=16, T_out=16, **_K3), 3, True, False),
    'k3_t32_s1_nodb': (dict(B=64, T_in=32, T_out=32, **_K3), 1, False, False),
    'k3_t64_s5_short_last': (dict(B=48, T_in=64, T_out=64, **_K3), 5, True, True),        # 4 x 640 rows + 512
    'k3_t128_s3': (dict(B=24, T_in=128, T_out=128, **_K3), 3, True, False),
    'k3_t128_s16_odd_start': (dict(B=24, T_in=128, T_out=128, **_K3), 16, False, True),   # 192-row splits: starts at 64 mod 128
    'k5_stride2_s3': (dict(B=32, T_in=128, T_out=64, Cout=256, Cin=256, taps=5, stride=2, pad_left=2), 3, True, False),
    'k5_stride2_s1_acc': (dict(B=32, T_in=128, T_out=64, Cout=256, Cin=256, taps=5, stride=2, pad_left=2), 1, True, True),
    'co_split2_t40_s3': (dict(B=64, T_in=40, T_out=40, Cout=512, Cin=256, taps=1, pad_left=1, reflect=False, linear=True,
                              co_split2=True), 3, True, False),
    'c1000x520_t32_s3': (dict(B=64, T_in=32, T_out=32, Cout=520, Cin=1000, taps=3, pad_left=1), 3, True, False),
    'c1000x520_t32_s16_nodb': (dict(B=64, T_in=32, T_out=32, Cout=520, Cin=1000, taps=3, pad_left=1), 16, False, False),
    'conv2d_3x3_s3': (dict(B=32, T_in=64, T_out=64, Cout=256, Cin=256, taps=9, pad_left=1, geom2=(8, 8, 8, 8, 3)), 3, True, False),
    'conv2d_3x3_s16_acc': (dict(B=32, T_in=64, T_out=64, Cout=256, Cin=256, taps=9, pad_left=1, geom2=(8, 8, 8, 8, 3)), 16, True, True),
    'k3_t48_s5': (dict(B=64, T_in=48, T_out=48, **_K3), 5, True, False),
}


def carried_path(kw):
    """The kernel's own rule (wgrad_p8_carried in zs_gemm.hip): per-lane source pointers are carried across K tiles."""
    return kw.get('geom2') is None and kw.get('stride', 1) == 1 and 128 % kw['T_out'] == 0


def make_case(name):
    return D.Case(seed=sum(map(ord, name)), **CASES[name][0])


def run_case(L, layers, name, case=None):
    case = case or make_case(name)
    _, splits, bias, accumulate = CASES[name]
    ctx = layers.Ctx('cuda:0', 'bf16')
    return D._with(L, {'wgrad_p8': 2}, lambda: case.run(L, layers, ctx, splits, bias, accumulate))


def digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.numpy()).tobytes()).hexdigest()


def samples(t):
    return t.numpy().reshape(-1)[::SAMPLE_EVERY].astype(np.float32)


@pytest.fixture(scope='module')
def zs():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    from zs_amd import _lib, layers
    _lib.lib()
    return _lib, layers


_RUNS = {}


def _runs(zs, name):
    """(case, first run, second run) of a case, computed once per module"""
    if name not in _RUNS:
        L, layers = zs
        case = make_case(name)
        _RUNS[name] = (case, run_case(L, layers, name, case), run_case(L, layers, name, case))
    return _RUNS[name]


def test_cases_cover_both_address_paths():
    n = sum(carried_path(c[0]) for c in CASES.values())
    assert n >= 3 and len(CASES) - n >= 3, (n, len(CASES) - n)


@pytest.mark.parametrize('name', sorted(CASES))
def test_wgrad_p8_digests_equal_parent(zs, name):
    z = np.load(GOLDEN, allow_pickle=False)
    _, (w, b), _ = _runs(zs, name)
    bias = CASES[name][2]
    for key, t in (('dw', w),) + ((('db', b),) if bias else ()):
        if digest(t) != str(z['%s.%s_sha256' % (name, key)]):
            got, want = samples(t), z['%s.%s_samples' % (name, key)]
            bad = np.flatnonzero(got != want)
            pytest.fail('%s %s: digest differs from the parent kernel; %d of %d sampled elements differ, first at flat index %s: %r != %r'
                        % (name, key, bad.size, got.size, bad[:1] * SAMPLE_EVERY, got[bad[:1]], want[bad[:1]]))


@pytest.mark.parametrize('name', sorted(CASES))
def test_wgrad_p8_against_fp64(zs, name):
    case, (w, b), _ = _runs(zs, name)
    _, splits, bias, accumulate = CASES[name]
    D._check_ref('%s splits %d' % (name, splits), case, w, b, bias, accumulate)


@pytest.mark.parametrize('name', sorted(CASES))
def test_wgrad_p8_two_runs_bit_equal(zs, name):
    _, (w0, b0), (w1, b1) = _runs(zs, name)
    assert torch.equal(w0, w1), '%s: dW differs between two runs' % name
    if CASES[name][2]:
        assert torch.equal(b0, b1), '%s: db differs between two runs' % name
