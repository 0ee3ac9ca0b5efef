"""The stage-2 glue kernels of zs_patch.hip and zs_autolocker.hip (zs_conv2d_gather in both modes, zs_conv2d_fold in both modes,
zs_conv2d_unpad, zs_enc_dx_fold, zs_bce_mbv_bwd, zs_gen_combine_bwd, zs_l1_plain) through the C ABI against the fp64 definitions
of tests/patch_ref.py (which test_patch_ref_host.py holds against F.pad + F.unfold and the adjoint identity), on every path of
each kernel: vector and per-element loads, the interior fast path of the fold with all four tap slots and its general path,
reflection partners on both sides at once (size pad + 1), fill columns, spare gp rows, and one case per kernel just above its
grid cap, where the grid-stride loop runs.  The caps are the kernels' own; the case that crosses one asserts it from its sizes.

Buffers (the conventions and helpers of test_gpu_elem.py): every output lies between NaN guards that are compared bit for bit
with their image before the call; columns in [C, fill_cols) are exactly zero and columns in [fill_cols, ld) keep their bits.
Every input is NaN past its valid columns and rows (ldx > C, ldg > k C, the spare gp_rows row, ld_in > F, ...) and is compared
bit for bit after the call.  References are built from the values the kernel reads (bf16-rounded for bf16 operands).

Tolerances (U = 2^-24; every check prints its measured error beside the bound; "used" below is the largest measured
error / bound over the module's cases on an MI355X.  2^-8 is the unit roundoff of bf16 (8 significant bits): a value just above
a power of two is rounded by up to 2^-8 of itself, so a bf16 output uses up to 0.996 of its bound in every kernel here and the
fp32 figures are the ones that show the headroom of the arithmetic):
  * zs_conv2d_gather, both modes: BIT-EXACT (it moves values; an fp32 source into bf16 takes one round-to-nearest-even, which
    is x.to(torch.bfloat16)); the columns past k C (k k C) up to ldo are +0.
  * zs_conv2d_fold, both modes, zs_conv2d_unpad: (n + 1) U sum|terms| per element, + 2^-8 |ref| for a bf16 output.  The inputs
    are bf16-exact, so every term is exact in fp32 and only the n - 1 additions round (each by at most U times a partial sum
    <= sum|terms|); n = the number of terms of the definition for that element (the transpose applied to ones: at most
    3 ceil(k/s) 3 for the H-only fold, (3 ceil(k/s))^2 for col2im, 9 for the un-padding) plus one for `add`.
    Used, fp32 or fp32 output: fold 0.29, col2im 0.08, unpad 0.13.
  * zs_enc_dx_fold: 4 U sum|terms| (at most 4 terms, 3 additions, fp32 output).  Used: 0.47.
  * zs_gen_combine_bwd: 6 U |ref| + 2^-8 |ref| for bf16.  Roundings: m m (or 1 - m), the difference, dx xd, the product = 4; the
    mask m of the tanh variant is drawn from [-0.7, 0.7] so that the cancellation in 1 - m^2 amplifies the rounding of m^2 by
    m^2 / (1 - m^2) < 1.  Used, fp32: 0.47.
  * zs_bce_mbv_bwd, dlogits: 6 U |ref| + 2^-8 |ref| for bf16 against the definition that takes 1 - x in fp32 and everything else
    in fp64.  The kernel's fp32 chain is ten operations long (x - y, x (1 - x), the quotient, 1 / N, grad_scale / N, their product,
    1 - y0, two products, / tau); N and tau are powers of two in the soft-x cases and grad_scale is 1 or 1/2, so four of them are
    exact and six round.  dlogits[2e + 1] == -dlogits[2e] bit for bit.  Used, fp32: 0.65 (soft x), 0.50 (hard units).
    Loss, soft x: max(8 |BCE_fp32 - BCE_fp64| of torch on the CPU for the same inputs, 16 U mean|l|) as for zs_softmax_ce; the
    measured CPU figures are 2.6e-09 and 5.1e-09 for the two shapes, 8 x which is below the floor 16 U mean|l| = 9.5e-07 and
    9.9e-07, so the floor decides.  Used: 0.07.
    Loss, hard units: np.float32(100 mismatches / N) to within one fp32 ulp (every term is 0 or 100: the double partials are exact).
  * zs_l1_plain: loss N U mean|d| with N = terms per thread + 6 shuffle steps + 4 waves (the chain derived for zs_l1_loss in
    test_gpu_elem.py; the second stage is fp64).  Used: 0.008.  d = sign(a - b) float32(scale) / float32(n) to one ulp (2^-23
    relative), exactly 0 where a == b."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import patch_ref as R  # noqa: E402
from test_gpu_elem import DTYPES, NAN, U, Buf, _dt, check, gen, padded, rnd, same_bits, stream, tdt, zs  # noqa: E402,F401

pytestmark = pytest.mark.gpu

KSP = [(5, 2, 2), (3, 1, 1), (5, 1, 2), (7, 2, 3), (4, 2, 1)]
MODES = [R.REFLECT, R.ZERO]
CAP_ITEMS = 16384 * 256                                       # grid_for(): at most 16384 workgroups of 256 threads = 4 194 304 items
ksp_id = lambda t: 'k%d_s%d_p%d' % t  # noqa: E731


def rup(n, m):
    return (n + m - 1) // m * m


def pm(L, mode):
    return L.ZS_PAD_REFLECT if mode == R.REFLECT else L.ZS_PAD_ZERO


def bf(x):
    """bf16-exact fp32 values"""
    return x.to(torch.bfloat16).float()


def f64(t):
    return t.double().numpy()


def rows_buf(x, ld, dt):
    """[..., C] values -> a guarded device buffer of rows of ld elements, NaN past column C"""
    x2 = x.reshape(-1, x.shape[-1])
    return Buf(x2.shape[0] * ld, dt, init=padded(x2, ld))


def out_rows(name, buf, rows, ld, C, fill):
    """The valid columns [rows, C] of an output image; asserts the guards, zeros in [C, fill) and untouched bits in [fill, ld)."""
    reg = buf.region(name).view(rows, ld)
    before = buf.before[buf.lo:buf.lo + buf.n].view(rows, ld)
    if fill < ld:
        same_bits(name + ': columns at or past fill_cols', reg[:, fill:], before[:, fill:])
    assert (reg[:, C:fill] == 0).all(), name + ': fill columns not exactly 0'
    return reg[:, :C]


def sum_bound(n, sabs, ref, out_bf16):
    return (n + 1) * U * sabs + (2.0 ** -8 * np.abs(ref) if out_bf16 else 0.0)


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- zs_conv2d_gather ------------------------------------------------------------------------------------------------------------
def gather_run(L, dtype, full, ksp, mode, C, x_f32, ldo_extra, H_in, B=2, Wd=17, seed=1, cheap=False):
    k, s, pad = ksp
    H_out, W_out = R.out_len(H_in, k, s, pad), (R.out_len(Wd, k, s, pad) if full else Wd)
    g = gen(seed)
    x = (torch.randint(-120, 121, (B, H_in, Wd, C), generator=g).float() / 16 if cheap else torch.randn(B, H_in, Wd, C, generator=g))
    src_dt = torch.float32 if x_f32 else tdt(dtype)
    xv = x if x_f32 else rnd(x, dtype)                       # the values the kernel reads
    ldx = C + 8 if C % 8 == 0 else C + 3                    # the 16-byte path needs 16-byte rows; the per-element path gets an odd pitch
    bx = rows_buf(xv, ldx, src_dt)
    kc = k * C * (k if full else 1)
    ldo = rup(kc, 8) + 8 * ldo_extra
    rows = B * H_out * W_out
    out = Buf(rows * ldo, tdt(dtype))
    L.call('zs_conv2d_gather', 'ZsConv2dGather', stream(), dtype=_dt(L, dtype), x=bx.ptr(L), ldx=ldx, x_f32=int(x_f32), out=out.ptr(L), ldo=ldo,
           B=B, H_in=H_in, H_out=H_out, Wd=Wd, C=C, k=k, stride=s, pad=pad, pad_mode=pm(L, mode), full=int(full))
    ref = (R.im2col if full else R.gather_h)(f64(xv), k, s, pad, mode)
    exp = torch.zeros(rows, ldo, dtype=torch.float64)
    exp[:, :kc] = t64(ref).reshape(rows, kc)
    name = '%s C %d x_f32 %d ldo %d H_in %d' % ('im2col' if full else 'gather', C, x_f32, ldo, H_in)
    same_bits(name, out.image(), out.expect(exp.float().to(tdt(dtype))))        # fp32 -> bf16: one round-to-nearest-even
    bx.unchanged(name + ': x')
    return rows * (ldo // 8)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ksp', KSP, ids=ksp_id)
@pytest.mark.parametrize('full', [0, 1], ids=['h_only', 'both_axes'])
def test_conv2d_gather(zs, full, ksp, mode, dtype):
    """C = 8, 64: the 16-byte load of the H-only gather (fp32 and T source); C = 1, 12: 8-column groups that straddle two kh blocks,
    and k C not a multiple of 8 (zeros inside the last group); ldo above the rounded k C: whole groups of zeros."""
    k, s, pad = ksp
    salt = KSP.index(ksp) + MODES.index(mode)
    seen = set()
    for i, C in enumerate([1, 8, 12, 64]):
        for j, H_in in enumerate([11, 12, pad + 1]):
            x_f32, extra = divmod((3 * i + j + salt) % 4, 2)
            seen.add((x_f32, extra))
            gather_run(zs, dtype, full, ksp, mode, C, x_f32, extra, H_in, seed=100 * i + j)
    assert len(seen) == 4                                    # x_f32 x (ldo == / > the rounded k C)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('full', [0, 1], ids=['h_only', 'both_axes'])
def test_conv2d_gather_above_the_cap(zs, full, dtype):
    """B H_out W ldo / 8 work items just above 16384 x 256: the first threads take a second item in the grid-stride loop."""
    if full:
        items = gather_run(zs, dtype, 1, (3, 2, 1), R.REFLECT, 1, 1, 0, 16, B=29128, seed=7, cheap=True)           # 8 x 9 rows per image, 2 groups
    else:
        items = gather_run(zs, dtype, 0, (3, 1, 1), R.ZERO, 8, 0, 0, 8, B=5141, Wd=34, seed=8, cheap=True)       # 8 x 34 rows per image, 3 groups
    assert CAP_ITEMS < items < CAP_ITEMS * 1.01, items


# ---- zs_conv2d_fold --------------------------------------------------------------------------------------------------------------
def fold_run(L, dtype, ksp, mode, C, out_f32, fill_extra, gp_kind, add, H_in, Wd, dH, B=2, tight=False, seed=1):
    """non-full fold.  gp_kind 0: gp_rows = 0; 1: gp_rows = Wp; 2: gp_rows = Wp + (Wp & 1).  -> fraction of the bound used"""
    k, s, pad = ksp
    H_out = max(1, R.out_len(H_in, k, s, pad) - dH)
    Wp = Wd + 2 * pad
    gp_rows = [0, Wp, Wp + (Wp & 1)][gp_kind]
    Wr = gp_rows or Wp
    fill = C if out_f32 else rup(C, 8) + fill_extra
    if tight:
        ldg = k * C                                          # the last row of gp ends with the last tap: a fill group has nothing behind it
        assert (k - 1) * C + fill > ldg and C % 8 == 0
    else:
        ldg = max(k * C, (k - 1) * C + fill)
        ldg = rup(ldg, 8) + 8 if C % 8 == 0 else ldg + 3
    g = gen(seed)
    gp = torch.full((B, H_out, Wr, k * C), NAN)
    gp[:, :, :Wp] = bf(torch.randn(B, H_out, Wp, k * C, generator=g))           # a spare row stays NaN
    bgp = rows_buf(gp, ldg, tdt(dtype))
    rows = B * H_in * Wd
    av = bf(torch.randn(B, H_in, Wd, C, generator=g)) if add else None
    badd = rows_buf(av, C + 5, tdt(dtype)) if add else None
    ldo = C + 3 if out_f32 else fill + 8 * (seed % 2)
    out = Buf(rows * ldo, torch.float32 if out_f32 else tdt(dtype))
    L.call('zs_conv2d_fold', 'ZsConv2dFold', stream(), dtype=_dt(L, dtype), gp=bgp.ptr(L), ldg=ldg, out=out.ptr(L), ldo=ldo, out_f32=int(out_f32),
           fill_cols=fill, add=badd.ptr(L) if add else None, ldadd=C + 5, B=B, H_in=H_in, H_out=H_out, Wd=Wd, C=C, k=k, stride=s, pad=pad,
           pad_mode=pm(L, mode), gp_rows=gp_rows, full=0)
    gpn = f64(gp)
    args = (k, s, pad, mode, H_in, Wd)
    ref, sabs, n = R.fold_h(gpn, *args), R.fold_h(np.abs(gpn), *args), R.fold_h(np.ones_like(gpn), *args)
    assert n.max() <= 3 * math.ceil(k / s) * 3
    if add:
        ref, sabs, n = ref + f64(av), sabs + np.abs(f64(av)), n + 1
    name = 'fold C %d out_f32 %d fill %d ldg %d gp_rows %d add %d H_in %d H_out %d Wd %d' % (C, out_f32, fill, ldg, gp_rows, add, H_in, H_out, Wd)
    got = out_rows(name, out, rows, ldo, C, fill)
    check(name, got, t64(ref).reshape(rows, C), t64(sum_bound(n, sabs, ref, dtype == 'bf16' and not out_f32)).reshape(rows, C))
    bgp.unchanged(name + ': gp')
    if add:
        badd.unchanged(name + ': add')
    return int(n.max())


FOLD_C = [(1, 1), (8, 0), (12, 1), (64, 0)]                 # (C, out_f32)


def fold_configs(ksp, mode):
    """Every C with every Wd; the other factors rotate, shifted per (k, s, pad) and padding mode, so that each value of each
    factor occurs in every test case (asserted there) and the combinations differ from case to case."""
    pad = ksp[2]
    salt = KSP.index(ksp) + 2 * MODES.index(mode)
    out = []
    for i, (C, out_f32) in enumerate(FOLD_C):
        for j, Wd in enumerate([pad + 1, 17, 65]):
            t = 3 * i + j + salt
            out.append(dict(C=C, out_f32=out_f32, Wd=Wd, fill=16 * (t % 2), gp=(2 * i + j + salt) % 3, add=(t // 2) % 2,
                            H_in=[pad + 1, pad + 2, 12][(i // 2 + j + salt) % 3], dH=(t // 3) % 2, seed=t))
    return out


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ksp', KSP, ids=ksp_id)
def test_conv2d_fold(zs, ksp, mode, dtype):
    """(7, 2, 3) fills the fourth tap slot of the interior fast path (kh = 0, 2, 4, 6); (5, 1, 2) has five taps per row and sends
    the interior through the general path; H_in, Wd = pad + 1 give every position both reflection partners; H_out one below the
    full count cuts the last taps (ho >= H_out); Wd = 65 x 8 or 10 groups = three workgroups along x, the last one partial."""
    k, s, pad = ksp
    cfgs = fold_configs(ksp, mode)
    for f, want in (('C', 4), ('Wd', 3), ('fill', 2), ('gp', 3), ('add', 2), ('H_in', 3), ('dH', 2)):
        assert len({c[f] for c in cfgs}) == want, f
    assert {(c['C'], c['H_in']) for c in cfgs} >= {(C, H) for C in (8, 64) for H in (pad + 1, 12)}    # the 16-byte path at the smallest and at an interior height
    n_max = 0
    for c in cfgs:
        n_max = max(n_max, fold_run(zs, dtype, ksp, mode, c['C'], c['out_f32'], c['fill'], c['gp'], c['add'], c['H_in'], c['Wd'], c['dH'], seed=c['seed']))
    print('[fold] most terms in one element: %d' % n_max)
    if ksp == (7, 2, 3):
        assert n_max >= 4                                   # four taps along H: the fourth slot of the fast path is in use


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ksp', [(5, 2, 2), (7, 2, 3), (5, 1, 2)], ids=ksp_id)
def test_conv2d_fold_fill_groups_read_nothing(zs, ksp, mode, dtype):
    """ldg == k C with fill_cols = C + 24: the three fill groups of every position lie past the row of the last tap, on the last row of
    gp past the buffer.  They store zeros and load nothing (the NaN guard behind gp is all there is to read)."""
    for C, Wd, H_in in [(8, 17, 12), (64, 5, 12), (8, 65, ksp[2] + 1)]:
        fold_run(zs, dtype, ksp, mode, C, 0, 24, 0, 1, H_in, Wd, 0, tight=True, seed=3)


def col2im_run(L, dtype, ksp, mode, C, out_f32, add, H_in, Wd, dH, B=2, seed=1, cheap=False):
    k, s, pad = ksp
    H_out, W_out = max(1, R.out_len(H_in, k, s, pad) - dH), R.out_len(Wd, k, s, pad)
    kkc = k * k * C
    ldg = kkc + 3
    g = gen(seed)
    gp = (torch.randint(-64, 65, (B, H_out, W_out, kkc), generator=g).float() / 16 if cheap else bf(torch.randn(B, H_out, W_out, kkc, generator=g)))
    bgp = rows_buf(gp, ldg, tdt(dtype))
    rows = B * H_in * Wd
    av = bf(torch.randn(B, H_in, Wd, C, generator=g)) if add else None
    badd = rows_buf(av, C + 5, tdt(dtype)) if add else None
    ldo = C + 3
    out = Buf(rows * ldo, torch.float32 if out_f32 else tdt(dtype))
    L.call('zs_conv2d_fold', 'ZsConv2dFold', stream(), dtype=_dt(L, dtype), gp=bgp.ptr(L), ldg=ldg, out=out.ptr(L), ldo=ldo, out_f32=int(out_f32),
           fill_cols=C, add=badd.ptr(L) if add else None, ldadd=C + 5, B=B, H_in=H_in, H_out=H_out, Wd=Wd, C=C, k=k, stride=s, pad=pad,
           pad_mode=pm(L, mode), gp_rows=0, full=1)
    gpn = f64(gp)
    args = (k, s, pad, mode, H_in, Wd)
    ref, sabs, n = R.col2im(gpn, *args), R.col2im(np.abs(gpn), *args), R.col2im(np.ones_like(gpn), *args)
    assert n.max() <= (3 * math.ceil(k / s)) ** 2
    if add:
        ref, sabs, n = ref + f64(av), sabs + np.abs(f64(av)), n + 1
    name = 'col2im C %d out_f32 %d add %d H_in %d H_out %d Wd %d' % (C, out_f32, add, H_in, H_out, Wd)
    got = out_rows(name, out, rows, ldo, C, C)
    check(name, got, t64(ref).reshape(rows, C), t64(sum_bound(n, sabs, ref, dtype == 'bf16' and not out_f32)).reshape(rows, C))
    bgp.unchanged(name + ': gp')
    return rows * C


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ksp', KSP, ids=ksp_id)
def test_conv2d_fold_full(zs, ksp, mode, dtype):
    k, s, pad = ksp
    for i, (C, out_f32) in enumerate([(1, 1), (8, 0), (8, 1)]):
        for j, (H_in, Wd) in enumerate([(pad + 1, pad + 1), (12, 17), (pad + 2, 9)]):
            col2im_run(zs, dtype, ksp, mode, C, out_f32, (i + j) % 2, H_in, Wd, j % 2, seed=10 * i + j)


@pytest.mark.parametrize('dtype', DTYPES)
def test_conv2d_fold_full_above_the_cap(zs, dtype):
    items = col2im_run(zs, dtype, (3, 2, 1), R.REFLECT, 8, 0, 0, 4, 17, 0, B=7711, seed=5, cheap=True)
    assert CAP_ITEMS < items < CAP_ITEMS * 1.01, items


# ---- zs_conv2d_unpad -------------------------------------------------------------------------------------------------------------
def unpad_run(L, dtype, pad, mode, C, fill, add, H, W, Hp, Wp, B=2, seed=1, cheap=False):
    g = gen(seed)
    ldg, ldo, ldadd = C + 8, fill + 8, C + 16
    cls, bufs = [], []
    for ph in (0, 1):
        for pw in (0, 1):
            Hc, Wc = R.class_shape(Hp, Wp, ph, pw)
            v = torch.randint(-64, 65, (B, Hc, Wc, C), generator=g).float() / 16 if cheap else bf(torch.randn(B, Hc, Wc, C, generator=g))
            cls.append(v)
            bufs.append(rows_buf(v, ldg, tdt(dtype)) if v.numel() else Buf(8, tdt(dtype)))          # four allocations of their own
    rows = B * H * W
    av = bf(torch.randn(B, H, W, C, generator=g)) if add else None
    badd = rows_buf(av, ldadd, tdt(dtype)) if add else None
    out = Buf(rows * ldo, tdt(dtype))
    L.call('zs_conv2d_unpad', 'ZsConv2dUnpad', stream(), dtype=_dt(L, dtype), g00=bufs[0].ptr(L), g01=bufs[1].ptr(L), g10=bufs[2].ptr(L),
           g11=bufs[3].ptr(L), ldg=ldg, B=B, H=H, W=W, C=C, Hp=Hp, Wp=Wp, pad=pad, pad_mode=pm(L, mode), add=badd.ptr(L) if add else None,
           ldadd=ldadd, out=out.ptr(L), ldo=ldo, fill_cols=fill)
    cn = [f64(v) for v in cls]
    args = (pad, mode, H, W, Hp, Wp)
    ref, sabs, n = R.unpad(*cn, *args), R.unpad(*[np.abs(a) for a in cn], *args), R.unpad(*[np.ones_like(a) for a in cn], *args)
    assert n.max() <= 9
    if add:
        ref, sabs, n = ref + f64(av), sabs + np.abs(f64(av)), n + 1
    name = 'unpad C %d fill %d add %d H %d W %d Hp %d Wp %d' % (C, fill, add, H, W, Hp, Wp)
    got = out_rows(name, out, rows, ldo, C, fill)
    check(name, got, t64(ref).reshape(rows, C), t64(sum_bound(n, sabs, ref, dtype == 'bf16')).reshape(rows, C))
    for b in bufs:
        b.unchanged(name + ': class gradient')
    return rows * (fill // 8)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('pad', [1, 2])
def test_conv2d_unpad(zs, pad, mode, dtype):
    """Hp, Wp at H + 2 pad and one below (the positions a stride-2 convolution never reaches): odd and even class sizes; H, W down to
    pad + 1; fill_cols above C; the four classes in four allocations, so that an index into the wrong class lands in a NaN guard."""
    i = 0
    for H, W in [(pad + 1, pad + 1), (pad + 2, 7), (6, 5), (5, pad + 1)]:
        for dh, dw in [(0, 0), (1, 0), (0, 1), (1, 1)]:
            C = [8, 24][i % 2]
            unpad_run(zs, dtype, pad, mode, C, C + 16 * ((i // 2) % 2), (i // 4 + i) % 2, H, W, H + 2 * pad - dh, W + 2 * pad - dw, seed=i)
            i += 1


@pytest.mark.parametrize('dtype', DTYPES)
def test_conv2d_unpad_above_the_cap(zs, dtype):
    items = unpad_run(zs, dtype, 1, R.REFLECT, 8, 64, 0, 6, 5, 7, 7, B=17477, seed=2, cheap=True)    # 30 rows per image x 8 groups
    assert CAP_ITEMS < items < CAP_ITEMS * 1.01, items


# ---- zs_enc_dx_fold --------------------------------------------------------------------------------------------------------------
def enc_dx_run(L, dtype, pad, mode, T, C, with_pass, B=2, seed=1):
    g = gen(seed)
    gv = torch.randn(B, T + 2 * pad, C, generator=g)
    pv = rnd(torch.randn(B, T, C, generator=g), dtype) if with_pass else None
    ldg, ldx, ld_pass = C + 3, C + 2, C + 5
    bg = rows_buf(gv, ldg, torch.float32)
    bp = rows_buf(pv, ld_pass, tdt(dtype)) if with_pass else None
    out = Buf(B * T * ldx, torch.float32)
    L.call('zs_enc_dx_fold', 'ZsEncDxFold', stream(), dtype=_dt(L, dtype), g=bg.ptr(L), ldg=ldg, pass_through=bp.ptr(L) if with_pass else None,
           ld_pass=ld_pass, B=B, T=T, C=C, pad=pad, pad_mode=pm(L, mode), dx=out.ptr(L), ldx=ldx)
    pn = f64(pv) if with_pass else None
    ref = R.enc_dx_fold(f64(gv), pad, mode, pn)
    sabs = R.enc_dx_fold(np.abs(f64(gv)), pad, mode, np.abs(pn) if with_pass else None)
    name = 'enc_dx_fold pad %d T %d C %d pass %d' % (pad, T, C, with_pass)
    got = out_rows(name, out, B * T, ldx, C, C)
    check(name, got, t64(ref).reshape(B * T, C), t64(4 * U * sabs).reshape(B * T, C))
    bg.unchanged(name + ': g')
    return B * T * C


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mode', MODES)
def test_enc_dx_fold(zs, mode, dtype):
    """T = pad + 1: every row but the first has a left partner, every row but the last a right one, and row `pad` mirrors padded
    row 0; T = 2 pad + 1: the middle row is the only one with one partner on each side at distance pad."""
    i = 0
    for pad, Ts in [(3, [4, 5, 7, 40]), (0, [1, 5])]:
        for T in Ts:
            for C in (80, 513):
                enc_dx_run(zs, dtype, pad, mode, T, C, i % 2, seed=i)
                i += 1
    enc_dx_run(zs, dtype, 3, mode, 4, 80, 0, seed=98)          # both values of pass_through at the smallest T
    enc_dx_run(zs, dtype, 3, mode, 5, 513, 1, seed=99)


@pytest.mark.parametrize('dtype', DTYPES)
def test_enc_dx_fold_above_the_cap(zs, dtype):
    items = enc_dx_run(zs, dtype, 3, R.REFLECT, 40, 513, 1, B=52, seed=3)
    assert 4096 * 256 < items < 4096 * 256 * 1.02, items      # at most 4096 workgroups of 256 threads


# ---- zs_bce_mbv_bwd --------------------------------------------------------------------------------------------------------------
BCE_CAP = 1024 * 256                                          # bce_mbv_stage1: at most 1024 workgroups of 256 threads, one item per unit pair


def bce_call(L, dtype, x, y, y0, tau, gs, fill, ld):
    rows, E = x.shape
    bx, by, b0 = (Buf(rows * E, init=v) for v in (x, y, y0))
    dl = Buf(rows * ld, tdt(dtype))
    part, lo = Buf(1024, torch.float64), Buf(1)
    L.call('zs_bce_mbv_bwd', 'ZsBceMbvBwd', stream(), dtype=_dt(L, dtype), bits=bx.ptr(L), y0=b0.ptr(L), target=by.ptr(L), rows=rows, E=E, tau=tau,
           grad_scale=gs, dlogits=dl.ptr(L), ld=ld, fill_cols=fill, partial=part.ptr(L), loss_out=lo.ptr(L))
    for b in (bx, by, b0):
        b.unchanged('bce input')
    nb = min(1024, (rows * (fill // 2) + 255) // 256)
    pr = part.region('partial')
    assert torch.isfinite(pr[:nb]).all() and torch.isnan(pr[nb:]).all(), 'partials: %d expected' % nb
    return lo.region('loss_out')[0], out_rows('dlogits', dl, rows, ld, 2 * E, fill)


BCE_SHAPES = [(5, 20, 46, 49), (32, 16, 40, 40), (4096, 64, 132, 135)]          # (rows, E, fill_cols, ld)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('gs', [0.0, 0.5])
@pytest.mark.parametrize('shape', BCE_SHAPES, ids=lambda s: 'rows%d_E%d_fill%d_ld%d' % s)
def test_bce_mbv_bwd_hard_units(zs, shape, gs, dtype):
    rows, E, fill, ld = shape
    items = rows * (fill // 2)
    assert items < 256 or rows < 4096 or BCE_CAP < items < BCE_CAP * 1.04       # one partial workgroup ... just above the cap
    g = gen(rows)
    y = (torch.rand(rows, E, generator=g) < 0.5).float()
    x = torch.where(torch.rand(rows, E, generator=g) < 0.1, 1 - y, y)
    y0 = torch.rand(rows, E, generator=g) * 0.96 + 0.02
    tau = 0.7
    loss, dl = bce_call(zs, dtype, x, y, y0, tau, gs, fill, ld)
    mis = int((x != y).sum())
    assert mis > 0
    want = np.float32(100.0 * mis / (rows * E))
    print('[bce] hard units: loss %.9g, expected %.9g (%d mismatches of %d)' % (loss.item(), want, mis, rows * E))
    assert abs(np.float32(loss.item()) - want) <= np.spacing(want)
    _, ref = R.bce_mbv(x.numpy(), y.numpy(), y0.numpy(), tau, gs)
    mag = 1e12 / (rows * E) * (gs or 1.0) * f64(y0) * (1 - f64(y0)) / float(np.float32(tau))
    assert np.allclose(np.abs(ref[:, 0::2]), np.where(f64(x) != f64(y), mag, 0.0), rtol=1e-12, atol=0)      # the header's statement
    ref = t64(ref)
    check('dlogits, hard units', dl, ref, (6 * U + (2.0 ** -8 if dtype == 'bf16' else 0.0)) * ref.abs())
    assert (dl[:, 0::2][x == y] == 0).all()
    same_bits('dlogits[2e + 1] == -dlogits[2e]', dl[:, 1::2].contiguous(), (-dl[:, 0::2]).contiguous())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('gs', [0.0, 0.5])
@pytest.mark.parametrize('shape', BCE_SHAPES[1:], ids=lambda s: 'rows%d_E%d_fill%d_ld%d' % s)
def test_bce_mbv_bwd_soft_x(zs, shape, gs, dtype):
    rows, E, fill, ld = shape                                 # N = rows E is a power of two (exact 1 / N), tau = 0.5
    assert (rows * E) & (rows * E - 1) == 0
    g = gen(rows + 1)
    y = (torch.rand(rows, E, generator=g) < 0.5).float()
    x = torch.rand(rows, E, generator=g) * 0.998 + 0.001
    x.view(-1)[:6] = torch.tensor([1e-7, 1 - 2.0 ** -24, 0.5, 1e-7, 1 - 2.0 ** -24, 0.5])
    y.view(-1)[:6] = torch.tensor([0., 0., 0., 1., 1., 1.])
    assert x.max() < 1 and x.min() > 0
    y0 = torch.rand(rows, E, generator=g) * 0.96 + 0.02
    tau = 0.5
    loss, dl = bce_call(zs, dtype, x, y, y0, tau, gs, fill, ld)
    l, ref = R.bce_mbv(x.numpy(), y.numpy(), y0.numpy(), tau, gs)
    ref = t64(ref)
    check('dlogits, soft x', dl, ref, (6 * U + (2.0 ** -8 if dtype == 'bf16' else 0.0)) * ref.abs())
    same_bits('dlogits[2e + 1] == -dlogits[2e]', dl[:, 1::2].contiguous(), (-dl[:, 0::2]).contiguous())
    cpu = abs(F.binary_cross_entropy(x, y).item() - F.binary_cross_entropy(x.double(), y.double()).item())
    tol = max(8 * cpu, 16 * U * float(np.abs(l).mean()))
    print('[bce] |BCE_fp32 - BCE_fp64| on the CPU %.3g; floor %.3g' % (cpu, 16 * U * float(np.abs(l).mean())))
    check('loss, soft x', loss, torch.tensor(float(l.mean()), dtype=torch.float64), tol)


# ---- zs_gen_combine_bwd ----------------------------------------------------------------------------------------------------------
def gen_combine_run(L, dtype, mode, tanh_out, rows, fill, seed=1):
    Fv, ld_in, ld_dx, ldo = 513, 520, 517, fill + 3
    g = gen(seed)
    dxg, xd = torch.randn(rows, Fv, generator=g), torch.rand(rows, Fv, generator=g) + 0.01
    m = torch.rand(rows, Fv, generator=g) * 1.4 - 0.7 if tanh_out else torch.rand(rows, Fv, generator=g) * 0.98 + 0.01
    bdx, bxd, bm = rows_buf(dxg, ld_dx, torch.float32), rows_buf(xd, ld_in, torch.float32), rows_buf(m, ld_in, torch.float32)
    out = Buf(rows * ldo, tdt(dtype))
    L.call('zs_gen_combine_bwd', 'ZsGenCombineBwd', stream(), dtype=_dt(L, dtype), dx_gen=bdx.ptr(L), ld_dx=ld_dx, xd=bxd.ptr(L) if mode else None,
           m=bm.ptr(L), ld_in=ld_in, dpre=out.ptr(L), ldo=ldo, fill_cols=fill, rows=rows, F=Fv, mode=mode, tanh_out=tanh_out)
    ref = t64(R.gen_combine_bwd(f64(dxg), f64(xd), f64(m), mode, tanh_out))
    name = 'gen_combine_bwd mode %d tanh_out %d rows %d fill %d' % (mode, tanh_out, rows, fill)
    got = out_rows(name, out, rows, ldo, Fv, fill)
    check(name, got, ref, (6 * U + (2.0 ** -8 if dtype == 'bf16' else 0.0)) * ref.abs())
    for b in (bdx, bxd, bm):
        b.unchanged(name + ': input')
    return rows * fill


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('fill', [513, 544])
@pytest.mark.parametrize('tanh_out', [0, 1])
@pytest.mark.parametrize('mode', [0, 1])
def test_gen_combine_bwd(zs, mode, tanh_out, fill, dtype):
    gen_combine_run(zs, dtype, mode, tanh_out, 7, fill, seed=4 * mode + 2 * tanh_out)


@pytest.mark.parametrize('dtype', DTYPES)
def test_gen_combine_bwd_above_the_cap(zs, dtype):
    items = gen_combine_run(zs, dtype, 1, 1, 7711, 544, seed=9)
    assert CAP_ITEMS < items < CAP_ITEMS * 1.01, items


# ---- zs_l1_plain -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 4097, 4194304 + 5])
def test_l1_plain(zs, n):
    """4097: two workgroups, the second with one element; 4 194 309: the 1024-workgroup cap, 17 terms for the first five threads."""
    L = zs
    g = gen(n)
    a, b = torch.rand(n, generator=g), torch.rand(n, generator=g)
    b = torch.where(torch.arange(n) % 8 == 3, a, b)          # an eighth of the pairs equal
    if n == 1:
        b = a - 0.25
    scale = 0.3
    nb = min(1024, (n + 4095) // 4096)
    N = (n + nb * 256 - 1) // (nb * 256) + 6 + 4
    assert (nb == 1024 and N == 27) if n > 4194304 else nb == (n + 4095) // 4096
    ref_l, ref_d = R.l1_plain(f64(a), f64(b), scale)
    ba, bb = Buf(n, init=a), Buf(n, init=b)
    losses = []
    for with_d in (1, 0):
        bd, part, lo = Buf(n), Buf(1024), Buf(1)
        L.check(L.lib().zs_l1_plain(ba.ptr(L), bb.ptr(L), n, scale, part.ptr(L), lo.ptr(L), bd.ptr(L) if with_d else None, stream()), 'zs_l1_plain')
        pr = part.region('partial')
        assert torch.isfinite(pr[:nb]).all() and torch.isnan(pr[nb:]).all(), 'partials: %d expected' % nb
        losses.append(lo.region('loss_out'))
        check('loss (N = %d, d %s)' % (N, 'written' if with_d else 'null'), losses[-1][0], torch.tensor(ref_l, dtype=torch.float64),
              N * U * float(np.abs(f64(a) - f64(b)).mean()))
        if with_d:
            d = bd.region('d')
            check('d', d, t64(ref_d), t64(2.0 ** -23 * np.abs(ref_d)))
            assert (d[a == b] == 0).all() and torch.equal(torch.sign(d.double()), t64(np.sign(ref_d)))
            if n > 8:
                assert int((a == b).sum()) >= n // 8
        else:
            bd.unchanged('d (null pointer passed)')
    same_bits('loss with and without d', losses[0], losses[1])
    ba.unchanged('a')
    bb.unchanged('b')


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise(zs):
    L = zs
    src, buf, f32 = Buf(1 << 12, torch.bfloat16, init=torch.zeros(1 << 12)), Buf(1 << 12, torch.bfloat16), Buf(1 << 12, init=torch.full((1 << 12,), 0.5))
    i, p, q = src.ptr(L), buf.ptr(L), f32.ptr(L)              # inputs, T-dtype outputs, fp32 inputs and outputs
    q_out, q_part = L.ptr(f32.t, f32.lo + 2048), L.ptr(f32.t, f32.lo + 3072)
    fold = dict(dtype=L.ZS_BF16, gp=i, ldg=48, out=p, ldo=16, out_f32=0, fill_cols=8, B=1, H_in=6, H_out=3, Wd=9, C=8, k=5, stride=2, pad=2,
                pad_mode=L.ZS_PAD_REFLECT, gp_rows=0, full=0)
    gather = dict(dtype=L.ZS_BF16, x=i, ldx=8, x_f32=0, out=p, ldo=40, B=1, H_in=6, H_out=3, Wd=9, C=8, k=5, stride=2, pad=2, pad_mode=L.ZS_PAD_REFLECT, full=0)
    unpad = dict(dtype=L.ZS_BF16, g00=i, g01=i, g10=i, g11=i, ldg=8, B=1, H=4, W=4, C=8, Hp=6, Wp=6, pad=1, pad_mode=L.ZS_PAD_REFLECT, out=p, ldo=8, fill_cols=8)
    bce = dict(dtype=L.ZS_BF16, bits=q, y0=q, target=q, rows=2, E=4, tau=1.0, grad_scale=0.0, dlogits=p, ld=16, fill_cols=8, partial=q_part, loss_out=q_out)
    enc = dict(dtype=L.ZS_BF16, g=q, ldg=8, B=1, T=4, C=8, pad=3, pad_mode=L.ZS_PAD_REFLECT, dx=q_out, ldx=8)
    good = [('zs_conv2d_fold', 'ZsConv2dFold', fold), ('zs_conv2d_gather', 'ZsConv2dGather', gather), ('zs_conv2d_unpad', 'ZsConv2dUnpad', unpad),
            ('zs_bce_mbv_bwd', 'ZsBceMbvBwd', bce), ('zs_enc_dx_fold', 'ZsEncDxFold', enc)]
    for fn, sn, kw in good:                                   # the base of every refusal below is a call that is accepted
        L.call(fn, sn, stream(), **kw)
    torch.cuda.synchronize()
    bad = [('zs_conv2d_fold', 'ZsConv2dFold', dict(fold, gp_rows=12)),                               # 0 < gp_rows < Wd + 2 pad = 13
           ('zs_conv2d_fold', 'ZsConv2dFold', dict(fold, gp_rows=1)),
           ('zs_conv2d_fold', 'ZsConv2dFold', dict(fold, out=q_out, out_f32=1, ldo=7)),                 # fp32 rows narrower than C
           ('zs_conv2d_fold', 'ZsConv2dFold', dict(fold, H_in=2, H_out=1)),                          # reflect: pad >= H_in
           ('zs_conv2d_fold', 'ZsConv2dFold', dict(fold, Wd=2)),                                     # reflect: pad >= Wd
           ('zs_conv2d_fold', 'ZsConv2dFold', dict(fold, Wd=2, ldg=200, full=1)),
           ('zs_conv2d_gather', 'ZsConv2dGather', dict(gather, ldo=44)),                             # ldo not a multiple of 8
           ('zs_conv2d_gather', 'ZsConv2dGather', dict(gather, ldo=204, full=1)),
           ('zs_conv2d_unpad', 'ZsConv2dUnpad', dict(unpad, C=4)),                                   # C % 8 != 0
           ('zs_conv2d_unpad', 'ZsConv2dUnpad', dict(unpad, C=12, ldg=16, ldo=16, fill_cols=16)),
           ('zs_bce_mbv_bwd', 'ZsBceMbvBwd', dict(bce, fill_cols=9)),                                # odd fill_cols
           ('zs_enc_dx_fold', 'ZsEncDxFold', dict(enc, T=3))]                                        # reflect with T == pad
    for fn, sn, kw in bad:
        with pytest.raises(L.ZsError):
            L.call(fn, sn, stream(), **kw)
        print('[refused] %s: %s' % (fn, L.last_error()))
    # the same sizes are accepted under zero padding, which has no partner to look for
    L.call('zs_conv2d_fold', 'ZsConv2dFold', stream(), **dict(fold, Wd=2, pad_mode=L.ZS_PAD_ZERO))
    L.call('zs_conv2d_fold', 'ZsConv2dFold', stream(), **dict(fold, gp_rows=13))
    L.call('zs_enc_dx_fold', 'ZsEncDxFold', stream(), **dict(enc, T=3, pad_mode=L.ZS_PAD_ZERO))
    torch.cuda.synchronize()
    src.unchanged('bf16 inputs')
    buf.region('bf16 outputs: guards')
    f32.region('fp32 scratch: guards')
