"""The loss, norm, Adam, cross-entropy and row glue kernels of zs_elem.hip (zs_l1_loss, zs_sqnorm / zs_sqnorm_stage1, zs_adam_clip,
zs_softmax_ce, zs_cast_rows, zs_add_rowvec, zs_rows_reverse, zs_copy_vec_batch, zs_host_fetch, zs_step_counters) through the C
ABI, against fp64 (or, where the kernel's expression has one rounding, bit-exact fp32) references on the CPU, at the sizes
where each kernel's grid cap makes it loop and on every alignment switch.  The thresholds are the kernels' own (zs_elem.hip);
each case that is meant to cross one says so in a comment beside it, and asserts it where the API reports it.

Buffers: every output lies between two guards (SLACK elements before, at least SLACK after) of NaN -- a marker value for
integers -- and each test compares the guards, the columns at or past fill_cols and the rows past the last one with their bits
before the call.  Inputs are padded with NaN past their valid columns, so that a read one column too far poisons the result.
Inputs come from seeded CPU generators; references are built from the values the kernel reads (bf16-rounded for bf16 sources).

Tolerances (U = 2^-24, the unit roundoff of fp32; every check prints its measured error beside the bound):
  * zs_l1_loss, loss, dyadic inputs (multiples of 2^-12 in [1/8, 7/8], an eighth of the pairs equal): BIT-EXACT against
    np.float32(fp64 sum / (rows F)).  Every |d| is a multiple of 2^-12, so an fp32 partial sum is exact while it stays below
    2^12 = 4096; the test asserts (terms per workgroup) x max|d| < 4096 from the inputs alone (the interval [1/8, 7/8] keeps
    max|d| <= 3/4: 4101 rows x 513 columns put 8 x 513 = 4104 terms into one workgroup).  The second stage sums and divides in
    fp64 and rounds once, which is the reference's expression.
  * zs_l1_loss, loss, random inputs: |loss - fp64| <= N U mean|d|, N = the longest chain of fp32 additions = terms per lane
    (rows per wave x columns per lane, from the 1024-workgroup cap) + 6 shuffle steps + 4 waves.  The first addition of a chain
    is exact (0 + x), which leaves room for the rounding of d itself and of the result.
  * zs_l1_loss, gradient: fp32 8 U |g_ref| (roundings: rows F, the division, 1 - x_dec, two products); bf16 that plus
    2^-8 |g_ref| (one rounding to 8 significant bits); the sign equals sign(d) exactly; fill columns exactly 0.
  * zs_sqnorm: 2^-23 relative to the fp64 sum (squares exact in double, double sums n 2^-53, one rounding to fp32 = 2^-24, the
    rest is margin); the stage-1 partials summed in fp64: (n + 16) 2^-53 relative.
  * zs_adam_clip: per step and tensor, 4 x max|fp32 restatement - fp64 restatement| of the formula in zs_amd.h, both computed on
    the CPU from the test's inputs (the kernel's output takes no part), floored at 4 U max|tensor|.  The 4 covers the kernel's
    written-out FMA fusions (zs_adam_upd.h), which differ from torch's op-by-op roundings.  Measured fp32-vs-fp64 figures at
    n = 10007, seed 3, three steps (largest over the variants, which is the unclipped run; max|tensor| and the floor beside
    them): p 3.2e-07 (4.15, 9.9e-07), m 4.2e-07 (7.09, 1.7e-06), v 1.5e-06 (17.1, 4.1e-06), clipped g 2.1e-08 (12.3, 2.9e-06),
    the average 2.7e-07 (3.61, 8.6e-07): 4 x the measured figure decides for p and v, the floor for m, g and the average.
    With the clip active |m| <= 0.28 and the floor 6.6e-08 decides.
    Bit relations (no tolerance): max_blocks in {1, 3} = default grid; all buffers one float off 16-byte alignment = aligned.
  * zs_softmax_ce: loss max(8 |CE_fp32 - CE_fp64|, 16 U max|logit|); gradient max(8 max|grad_fp32 - grad_fp64|,
    16 U max|logit| grad_scale / B) -- torch's fp32 cross_entropy against its fp64 one on the same logits (spread over +-30),
    the 8 for library expf / logf that differ by a few ulp.  The floor: l - max is rounded at magnitudes up to 60, which is a
    relative error of up to 60 U in exp(); the gradient's floor carries the gradient's own scale grad_scale / B, which makes it
    tighter than the loss's.  Measured CE_fp32-vs-fp64 figures over the cases: loss <= 4.0e-06 (8 x that is 3.2e-05, the floor
    2.9e-05), gradient <= 5.0e-08 at B = 1 and <= 2.5e-10 at B = 700 (the floor, 2.9e-05 grad_scale / B, decides everywhere).
    correct_out is exact, the first index winning a tie as torch.argmax does.
  * zs_cast_rows, zs_add_rowvec: BIT-EXACT against the kernel's own fp32 expression with one round-to-nearest-even to bf16.
  * zs_rows_reverse, zs_copy_vec_batch, zs_host_fetch, zs_step_counters: exact (they move or count bits)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = ['fp32', 'bf16']
U = 2.0 ** -24
SLACK = 64                      # guard elements on each side of a buffer (a multiple of 16 bytes for every type used)
MARK = -0x5A5A5A5B              # guard value of integer buffers
NAN = float('nan')


@pytest.fixture(scope='module')
def zs():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    from zs_amd import _lib
    _lib.lib()
    return _lib


def _dt(L, dtype):
    return L.ZS_F32 if dtype == 'fp32' else L.ZS_BF16


def tdt(dtype):
    return torch.float32 if dtype == 'fp32' else torch.bfloat16


def rnd(x, dtype):
    """fp32 cpu tensor -> the values the kernel reads (bf16-rounded for bf16), still fp32."""
    return x.float() if dtype == 'fp32' else x.to(torch.bfloat16).float()


def stream():
    return torch.cuda.current_stream().cuda_stream


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def same_bits(name, got, exp):
    """Every element of `got` has the bits of `exp` (NaN guards included: they are copies of one image)."""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (name, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = bits(got) != bits(exp)
    n_bad = int(bad.sum())
    print('[bits] %s: %d of %d elements differ' % (name, n_bad, got.numel()))
    if n_bad:
        i = tuple(int(k) for k in bad.nonzero()[0])
        raise AssertionError('%s: %d of %d elements differ, first at %s: got %r expected %r' %
                             (name, n_bad, got.numel(), i, got[i].item(), exp[i].item()))


class Buf(object):
    """n elements of `dt` on the device between two guards (SLACK elements before, `tail` after; NaN, or MARK for integers).
    `off` shifts the region by that many elements, so that its base leaves the 16-byte (and for bf16 the 4-byte) alignment the
    allocation has.  `before` is the image on the host as it was uploaded."""

    def __init__(self, n, dt=torch.float32, init=None, off=0, tail=SLACK):
        self.n, self.lo = n, SLACK + off
        fill = NAN if dt.is_floating_point else MARK
        self.before = torch.full((self.lo + n + tail,), fill, dtype=dt)
        if init is not None:
            self.before[self.lo:self.lo + n] = init.reshape(-1).to(dt)
        self.t = self.before.to('cuda:0')
        assert self.t.data_ptr() % 16 == 0

    def ptr(self, L):
        return L.ptr(self.t, self.lo)

    def image(self):
        torch.cuda.synchronize()
        return self.t.cpu()

    def region(self, name, img=None):
        """The region of the image after a call; asserts that both guards kept their bits."""
        img = self.image() if img is None else img
        same_bits(name + ': guard before', img[:self.lo], self.before[:self.lo])
        same_bits(name + ': guard after', img[self.lo + self.n:], self.before[self.lo + self.n:])
        return img[self.lo:self.lo + self.n]

    def unchanged(self, name):
        same_bits(name + ': unchanged', self.image(), self.before)

    def expect(self, region):
        """The whole image with the region replaced (exact comparisons: same_bits(name, buf.image(), buf.expect(ref)))."""
        e = self.before.clone()
        e[self.lo:self.lo + self.n] = region.reshape(-1).to(e.dtype)
        return e


def check(name, got, ref, allowed):
    """|got - ref| <= allowed (a number or a tensor), element by element; prints the measured error beside the bound."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), name + ': non-finite output'
    err = (got - ref).abs()
    allowed = torch.zeros_like(err) + allowed
    used = torch.where(err > 0, err / allowed.clamp_min(1e-300), torch.zeros_like(err))
    print('[err] %s: max err %.3g (largest allowance %.3g; %.3f of the allowance used)' %
          (name, err.max().item(), allowed.max().item(), used.max().item()))
    if (err > allowed).any():
        i = np.unravel_index(int((err - allowed).argmax()), err.shape)
        raise AssertionError('%s: err %.4g > allowed %.4g at %s: got %.9g ref %.9g' %
                             (name, err[i].item(), allowed[i].item(), tuple(int(k) for k in i), got[i].item(), ref[i].item()))


def padded(x, ld):
    """[rows, C] -> [rows, ld] with NaN in the columns past C."""
    out = torch.full((x.shape[0], ld), NAN, dtype=x.dtype)
    out[:, :x.shape[1]] = x
    return out


# ---- zs_l1_loss ------------------------------------------------------------------------------------------------------------------
L1_CAP, L1_WAVES = 1024, 4                                    # l1_stage1_kernel: at most 1024 workgroups of 4 waves, a wave per row
L1_ROWS = [1, 3, 50, 4101]                                    # 4101 rows > 4096 = 1024 blocks x 4 waves: waves 0..4 take two rows
# (F, fill_cols, ldg).  (81, 83, 84) is the shape whose paired bf16 store could run one column too far: an odd fill_cols in an even ldg
L1_SHAPES = [(80, 96, 96), (81, 81, 83), (80, 80, 96), (513, 520, 520), (7, 8, 8), (81, 83, 84)]


def l1_grid(rows):
    nb = min(L1_CAP, (rows * 64 + 255) // 256)
    return nb, nb * L1_WAVES


def l1_inputs(rows, Fv, family, seed):
    g = gen(seed)
    if family == 'dyadic':                                    # multiples of 2^-12 in [1/8, 7/8]; an eighth of the pairs equal (d == 0)
        a = torch.randint(512, 3585, (rows, Fv), generator=g)
        b = torch.randint(512, 3585, (rows, Fv), generator=g)
        b = torch.where(torch.rand(rows, Fv, generator=g) < 0.125, a, b)
        assert (a == b).any() or rows * Fv < 16
        return (a.double() / 4096).float(), (b.double() / 4096).float()
    return torch.rand(rows, Fv, generator=g) * 0.98 + 0.01, torch.rand(rows, Fv, generator=g)       # x_dec (1 - x_dec) > 0


def l1_call(L, dtype, xd, x, shape, grad=True, off=0, gs=1.0):
    """-> (loss fp32 scalar tensor, gradient image [rows, ldg] in the kernel dtype or None)"""
    Fv, fill, ldg = shape
    rows = xd.shape[0]
    bxd, bx = Buf(rows * (Fv + 5), init=padded(xd, Fv + 5)), Buf(rows * (Fv + 2), init=padded(x, Fv + 2))
    dl = Buf(rows * ldg, tdt(dtype), off=off) if grad else None
    part, lo = Buf(1024), Buf(1)
    L.call('zs_l1_loss', 'ZsL1Loss', stream(), dtype=_dt(L, dtype), x_dec=bxd.ptr(L), ld_dec=Fv + 5, x=bx.ptr(L), ldx=Fv + 2, rows=rows,
           F=Fv, dlogits=dl.ptr(L) if grad else None, ldg=ldg, fill_cols=fill, partial=part.ptr(L), loss_out=lo.ptr(L), grad_scale=gs)
    bxd.unchanged('x_dec')
    bx.unchanged('x')
    nb = l1_grid(rows)[0]
    pr = part.region('partial')
    assert torch.isfinite(pr[:nb]).all() and torch.isnan(pr[nb:]).all(), 'partials: %d expected' % nb
    return lo.region('loss_out')[0], (dl.region('dlogits').view(rows, ldg) if grad else None)


def l1_check_grad(name, dtype, g, xd, x, shape, gs):
    Fv, fill, ldg = shape
    rows = xd.shape[0]
    d = xd.double() - x.double()
    ref = torch.sign(d) * (float(np.float32(gs)) / (rows * Fv)) * xd.double() * (1 - xd.double())
    assert torch.isnan(g[:, fill:]).all(), name + ': columns at or past fill_cols written'
    assert (g[:, Fv:fill] == 0).all(), name + ': fill columns not exactly 0'
    check(name, g[:, :Fv], ref, (8 * U + (2.0 ** -8 if dtype == 'bf16' else 0.0)) * ref.abs())
    assert torch.equal(torch.sign(g[:, :Fv].double()), torch.sign(d)), name + ': sign'


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rows', L1_ROWS)
@pytest.mark.parametrize('shape', L1_SHAPES, ids=lambda s: 'F%d_fill%d_ldg%d' % s)
def test_l1_loss(zs, dtype, rows, shape):
    """bf16 reaches the paired 4-byte store (even ldg, 4-byte base) and each fallback: odd ldg (81, 81, 83), odd fill_cols
    (81, 83, 84), base off by one element; 513 columns make a lane loop over columns; 4101 rows make a wave loop over rows."""
    L = zs
    Fv, fill, ldg = shape
    nb, nw = l1_grid(rows)
    rows_per_wave = (rows + nw - 1) // nw
    assert (rows_per_wave > 1) == (rows > 4096)
    # (a) dyadic grid: bit-exact loss
    xd, x = l1_inputs(rows, Fv, 'dyadic', 11)
    d = xd.double() - x.double()
    assert rows_per_wave * L1_WAVES * Fv * d.abs().max().item() < 4096          # every fp32 partial sum is exact
    want = np.float32(np.float64(d.abs().sum().item()) / np.float64(rows * Fv))
    loss, g = l1_call(L, dtype, xd, x, shape)
    print('[l1] dyadic loss %.9g, expected %.9g' % (loss.item(), want))
    assert np.float32(loss.item()) == want, ('dyadic loss', loss.item(), float(want))
    l1_check_grad('dyadic gradient', dtype, g, xd, x, shape, 1.0)
    loss0, _ = l1_call(L, dtype, xd, x, shape, grad=False)                      # loss only (dlogits null)
    assert np.float32(loss0.item()) == want, ('dyadic loss without a gradient', loss0.item(), float(want))
    # (b) random values
    xd, x = l1_inputs(rows, Fv, 'uniform', 12)
    d = xd.double() - x.double()
    per_lane = rows_per_wave * (2 * (Fv // 128) + min(2, Fv % 128))             # a lane takes columns 2 lane, 2 lane + 1 (+ 128 k)
    N = per_lane + 6 + L1_WAVES
    ref = d.abs().sum().item() / (rows * Fv)
    runs = [('aligned', 0, 1.0), ('grad_scale', 0, 0.3)] + ([('base + 1 element', 1, 1.0)] if dtype == 'bf16' else [])
    for name, off, gs in runs:
        loss, g = l1_call(L, dtype, xd, x, shape, off=off, gs=gs)
        check('loss, %s (N = %d)' % (name, N), loss, torch.tensor(ref, dtype=torch.float64), N * U * d.abs().mean().item())
        l1_check_grad('gradient, ' + name, dtype, g, xd, x, shape, gs)


# ---- zs_sqnorm -------------------------------------------------------------------------------------------------------------------
SQ_CAP = 1024                                                # sqnorm_stage1_kernel: at most 1024 workgroups of 256 threads


# 1 048 579 = 4 x 262 144 + 3: just past one grid stride of float4 (1024 x 256), so the loop with two loads in flight runs once for
# the first lanes; 2 359 299 = 4 x 589 824 + 3: 2.25 grid strides plus a tail of 3
@pytest.mark.parametrize('off', [0, 1], ids=['aligned', 'base+1'])          # base + 1 float: the all-scalar path (n4 = 0)
@pytest.mark.parametrize('n', [1, 3, 4, 10007, 1048579, 2359299])
def test_sqnorm(zs, n, off):
    L = zs
    g = torch.randn(n, generator=gen(21)) * 3
    ref = (g.double() ** 2).sum().item()
    bg = Buf(n, init=g, off=off)
    assert (bg.ptr(L) % 16 == 0) == (off == 0)
    part, out = Buf(SQ_CAP, torch.float64), Buf(1)
    L.check(L.lib().zs_sqnorm(bg.ptr(L), n, part.ptr(L), out.ptr(L), stream()), 'zs_sqnorm')
    check('sqnorm', out.region('out')[0], torch.tensor(ref, dtype=torch.float64), 2.0 ** -23 * ref)
    part2 = Buf(SQ_CAP, torch.float64)
    nb = L.lib().zs_sqnorm_stage1(bg.ptr(L), n, part2.ptr(L), stream())
    assert nb == min(SQ_CAP, (n + 255) // 256)
    if n > 4 * SQ_CAP * 256:
        assert nb == SQ_CAP                                  # the grid is capped: float4 index i + stride < n4 exists
    bg.unchanged('g')
    for name, b in (('zs_sqnorm', part), ('zs_sqnorm_stage1', part2)):
        pr = b.region(name + ' partials')
        assert torch.isfinite(pr[:nb]).all() and torch.isnan(pr[nb:]).all(), name + ': partials written: %d expected' % nb
        check(name + ' partials, summed in fp64', pr[:nb].sum(), torch.tensor(ref, dtype=torch.float64), (n + 16) * 2.0 ** -53 * ref)


# ---- zs_adam_clip ----------------------------------------------------------------------------------------------------------------
AD = dict(lr=1e-3, beta1=0.5, beta2=0.9, eps=1e-8)
AD_N, AD_STEPS = 10007, 3


def adam_inputs(n, seed=3):
    g = gen(seed)
    p0 = torch.randn(n, generator=g)
    return p0, [torch.randn(n, generator=g) * 3 for _ in range(AD_STEPS)], torch.randn(n, generator=g)


def sumsq32(g):
    return torch.tensor(np.float32((g.double() ** 2).sum().item()))


def adam_ref(dt, p0, gs_list, max_norm=5.0, use_sumsq=True, grad_scale=0.0, step_ptr=False, ema0=None, decay=0.0):
    """The formula of zs_adam_clip (include/zs_amd.h) in dtype dt -- torch.float64: the reference; torch.float32: the same
    statement with every operation rounded to fp32.  Kernel arguments enter as the fp32 values the kernel reads.
    -> per step dict(p, m, v, g (the clipped gradient), ema)."""
    c = lambda x: torch.tensor(x, dtype=torch.float32).to(dt)
    p, m, v = p0.to(dt), torch.zeros_like(p0, dtype=dt), torch.zeros_like(p0, dtype=dt)
    e = ema0.to(dt) if ema0 is not None else None
    b1, b2, one = c(AD['beta1']), c(AD['beta2']), torch.tensor(1.0, dtype=dt)
    out = []
    for t, g in enumerate(gs_list, 1):
        gsc = c(grad_scale if grad_scale else 1.0)
        coef = gsc
        if max_norm > 0 and use_sumsq:
            norm = torch.sqrt(sumsq32(g).to(dt)) * gsc
            coef = gsc * torch.clamp(c(max_norm) / (norm + c(1e-6)), max=1.0)
        if step_ptr:
            bc1, bc2 = one - b1 ** t, one - b2 ** t
        else:
            bc1, bc2 = c(1 - AD['beta1'] ** t), c(1 - AD['beta2'] ** t)
        ge = g.to(dt) * coef
        m = m + (ge - m) * (one - b1)
        v = v * b2 + ge * ge * (one - b2)
        p = p - (c(AD['lr']) / bc1) * (m / (torch.sqrt(v) / torch.sqrt(bc2) + c(AD['eps'])))
        if e is not None:
            e = e + (p - e) * (one - c(decay))
        out.append(dict(p=p, m=m, v=v, g=ge, ema=e))
    return out


def adam_tols(ref64, ref32):
    """Per step and tensor: 4 x the largest fp32-restatement-versus-fp64 difference, floored at 4 U max|tensor|."""
    tols = []
    for a, b in zip(ref64, ref32):
        tols.append({k: max(4 * (a[k] - b[k].double()).abs().max().item(), 4 * U * a[k].abs().max().item()) for k in a if a[k] is not None})
    return tols


def adam_run(L, p0, gs_list, off=0, max_norm=5.0, use_sumsq=True, grad_scale=0.0, wcg=0, step_ptr=False, max_blocks=0, ema0=None,
             decay=0.0):
    """AD_STEPS calls of zs_adam_clip from m = v = 0 -> per step dict(p, m, v, g, ema) of the regions after the call."""
    n = p0.numel()
    z = torch.zeros(n)
    bp, bm, bv = Buf(n, init=p0, off=off), Buf(n, init=z, off=off), Buf(n, init=z, off=off)
    be = Buf(n, init=ema0, off=off) if ema0 is not None else None
    out = []
    for t, g in enumerate(gs_list, 1):
        bg, sq = Buf(n, init=g, off=off), Buf(1, init=sumsq32(g))
        st = Buf(1, torch.int32, init=torch.tensor([t], dtype=torch.int32))
        L.call('zs_adam_clip', 'ZsAdam', stream(), p=bp.ptr(L), g=bg.ptr(L), m=bm.ptr(L), v=bv.ptr(L), n=n,
               bc1=0.0 if step_ptr else 1 - AD['beta1'] ** t, bc2=0.0 if step_ptr else 1 - AD['beta2'] ** t,
               sumsq=sq.ptr(L) if use_sumsq else None, max_norm=max_norm, write_clipped_grad=wcg,
               step_ptr=st.ptr(L) if step_ptr else None, grad_scale=grad_scale, max_blocks=max_blocks,
               ema=be.ptr(L) if be else None, ema_decay=decay, **AD)
        sq.unchanged('sumsq')
        st.unchanged('step')
        if not wcg:
            bg.unchanged('g (write_clipped_grad = 0)')
        out.append(dict(p=bp.region('p'), m=bm.region('m'), v=bv.region('v'), g=bg.region('g'), ema=be.region('ema') if be else None))
    return out


ADAM_VARIANTS = {
    'clip': dict(max_norm=5.0),
    'no_clip': dict(max_norm=0.0),                              # max_norm <= 0: off
    'null_sumsq': dict(max_norm=5.0, use_sumsq=False),          # no norm: no clipping either
    'grad_scale': dict(max_norm=5.0, grad_scale=0.25),          # g holds 4 x the gradient
    'write_clipped': dict(max_norm=5.0, wcg=1),
    'step_ptr': dict(max_norm=5.0, step_ptr=True),              # bc1, bc2 from the device step count
    'step_ptr_grad_scale_write': dict(max_norm=5.0, step_ptr=True, grad_scale=0.25, wcg=1),
}


@pytest.mark.parametrize('variant', list(ADAM_VARIANTS))
def test_adam_clip_against_fp64(zs, variant):
    L = zs
    kw = dict(ADAM_VARIANTS[variant])
    p0, gl, _ = adam_inputs(AD_N)
    if kw.get('grad_scale'):
        gl = [g * 4 for g in gl]
    wcg = kw.pop('wcg', 0)
    ref64, ref32 = adam_ref(torch.float64, p0, gl, **kw), adam_ref(torch.float32, p0, gl, **kw)
    tols = adam_tols(ref64, ref32)
    got = adam_run(L, p0, gl, wcg=wcg, **kw)
    for t in range(AD_STEPS):
        for k in ('p', 'm', 'v'):
            check('%s, step %d: %s' % (variant, t + 1, k), got[t][k], ref64[t][k], tols[t][k])
        if wcg:
            check('%s, step %d: clipped g' % (variant, t + 1), got[t]['g'], ref64[t]['g'], tols[t]['g'])
    if variant == 'clip':
        assert all(sumsq32(g).sqrt().item() > 5.0 for g in gl)                  # the clip is active in every step


def adam_same(name, a, b, keys=('p', 'm', 'v')):
    for t in range(AD_STEPS):
        for k in keys:
            same_bits('%s, step %d: %s' % (name, t + 1, k), a[t][k], b[t][k])


def test_adam_clip_grid_cap_and_alignment_give_the_same_bits(zs):
    """max_blocks 1 and 3 make every thread walk the grid-stride loop (10007 / 4 float4 over 256 and 768 threads); p, g, m, v one
    float off 16-byte alignment take the one-element loop, which the header promises gives the same bits."""
    L = zs
    p0, gl, _ = adam_inputs(AD_N)
    base = adam_run(L, p0, gl, wcg=1)
    for mb in (1, 3):
        adam_same('max_blocks %d' % mb, adam_run(L, p0, gl, wcg=1, max_blocks=mb), base, ('p', 'm', 'v', 'g'))
    adam_same('base + 1 float', adam_run(L, p0, gl, wcg=1, off=1), base, ('p', 'm', 'v', 'g'))
    adam_same('base + 1 float, max_blocks 1', adam_run(L, p0, gl, wcg=1, off=1, max_blocks=1), base, ('p', 'm', 'v', 'g'))
    for n in (1, 2, 3, 5):                                      # 5: one float4 and a tail of one against five single elements
        p0, gl, _ = adam_inputs(n, seed=40 + n)
        adam_same('n = %d, base + 1 float' % n, adam_run(L, p0, gl, wcg=1, off=1), adam_run(L, p0, gl, wcg=1), ('p', 'm', 'v', 'g'))


def test_adam_clip_average_off_alignment_and_under_a_grid_cap(zs):
    """test_gpu_ema.py::test_kernels_average_alike_and_perturb_nothing already asserts, on the default grid: p, g, m, v bit-equal
    with and without the average, the same bits with only the average off alignment, and the average within an ulp of the recursion
    on the kernel's own p.  Left for here: all FIVE buffers off alignment and the capped grid (bit relations), and the average
    against the fp64 restatement of the whole step."""
    L = zs
    p0, gl, e0 = adam_inputs(AD_N)
    kw = dict(ema0=e0, decay=0.9)
    base, on = adam_run(L, p0, gl), adam_run(L, p0, gl, **kw)
    for name, r in (('all five + 1 float', adam_run(L, p0, gl, off=1, **kw)), ('max_blocks 3', adam_run(L, p0, gl, max_blocks=3, **kw)),
                    ('all five + 1 float, max_blocks 1', adam_run(L, p0, gl, off=1, max_blocks=1, **kw))):
        adam_same(name + ' against no average', r, base)
        adam_same(name + ' against the aligned default grid', r, on, ('ema',))
    ref64, ref32 = adam_ref(torch.float64, p0, gl, **kw), adam_ref(torch.float32, p0, gl, **kw)
    tols = adam_tols(ref64, ref32)
    for t in range(AD_STEPS):
        check('average, step %d' % (t + 1), on[t]['ema'], ref64[t]['ema'], tols[t]['ema'])


# ---- zs_softmax_ce ---------------------------------------------------------------------------------------------------------------
def ce_call(L, logits, target, grad=True, correct=True, gs=1.0):
    B, nc = logits.shape
    ld, ldg = nc + 5, nc + 3
    bl, bt = Buf(B * ld, init=padded(logits, ld)), Buf(B, torch.int64, init=target)
    lo, dl, co = Buf(1), Buf(B * ldg) if grad else None, Buf(1, torch.int32) if correct else None
    L.call('zs_softmax_ce', 'ZsSoftmaxCE', stream(), logits=bl.ptr(L), ld=ld, target=bt.ptr(L), B=B, n_class=nc, loss_out=lo.ptr(L),
           dlogits=dl.ptr(L) if grad else None, ldg=ldg, grad_scale=gs, correct_out=co.ptr(L) if correct else None)
    bl.unchanged('logits')
    bt.unchanged('target')
    g = None
    if grad:
        g = dl.region('dlogits').view(B, ldg)
        assert torch.isnan(g[:, nc:]).all(), 'dlogits: columns at or past n_class written'
        g = g[:, :nc]
    return lo.region('loss_out')[0], g, (int(co.region('correct_out')[0]) if correct else None)


def ce_ref(logits, target, gs):
    """-> (loss fp64, grad fp64, loss tolerance, grad tolerance): torch's cross_entropy in fp64, and 8 x its distance from torch's
    fp32 one on the same inputs, floored (module docstring)."""
    res = {}
    for dt in (torch.float64, torch.float32):
        z = logits.detach().clone().to(dt).requires_grad_(True)
        loss = F.cross_entropy(z, target)
        loss.backward()
        res[dt] = (loss.detach().double(), z.grad.double() * float(np.float32(gs)))
    (l64, g64), (l32, g32) = res[torch.float64], res[torch.float32]
    mx, B = logits.abs().max().item(), logits.shape[0]
    dl, dg = (l64 - l32).abs().item(), (g64 - g32).abs().max().item()
    print('[ce] fp32 torch against fp64: loss %.3g, gradient %.3g (floors %.3g, %.3g)' % (dl, dg, 16 * U * mx, 16 * U * mx * gs / B))
    return l64, g64, max(8 * dl, 16 * U * mx), max(8 * dg, 16 * U * mx * gs / B)


@pytest.mark.parametrize('B', [1, 255, 256, 257, 700])          # one workgroup of 256 threads: B > 256 gives a thread a second sample
@pytest.mark.parametrize('nc', [1, 2, 7, 103])
def test_softmax_ce(zs, B, nc):
    L = zs
    g = gen(100 * B + nc)
    logits = (torch.rand(B, nc, generator=g) * 2 - 1) * 30      # spread over +-30: exp() without the max subtracted would overflow
    target = torch.randint(0, nc, (B,), generator=g)
    want_correct = int((torch.argmax(logits, 1) == target).sum())
    for name, grad, correct, gs in (('all outputs', True, True, 1.0), ('loss only', False, False, 1.0), ('grad_scale', True, False, 0.3),
                                    ('no gradient', False, True, 1.0)):
        l64, g64, tol_l, tol_g = ce_ref(logits, target, gs)
        loss, dl, corr = ce_call(L, logits, target, grad, correct, gs)
        check('loss, ' + name, loss, l64, tol_l)
        if grad:
            check('gradient, ' + name, dl, g64, tol_g)
        if correct:
            assert corr == want_correct, (name, corr, want_correct)


def test_softmax_ce_counts_the_first_index_of_a_tie(zs):
    L = zs
    B, nc = 257, 7
    g = gen(5)
    logits = (torch.rand(B, nc, generator=g) * 2 - 1) * 30
    target = torch.randint(0, nc, (B,), generator=g)
    logits[:100, 2] = 31.0                                      # an exact tie for the maximum at indices 2 and 5 in the first 100 rows
    logits[:100, 5] = 31.0
    target[:100:2], target[1:100:2] = 2, 5                      # 50 name the first index (counted), 50 the second (not counted)
    am = torch.argmax(logits, 1)
    assert (am[:100] == 2).all()
    want = int((am == target).sum())
    assert want == 50 + int((am[100:] == target[100:]).sum())
    l64, g64, tol_l, tol_g = ce_ref(logits, target, 1.0)
    loss, dl, corr = ce_call(L, logits, target)
    assert corr == want, (corr, want)
    check('loss', loss, l64, tol_l)
    check('gradient', dl, g64, tol_g)


# ---- zs_cast_rows ----------------------------------------------------------------------------------------------------------------
# name: (dtype, src_f32, dst_f32, source type, destination type); the second destination always has the type of `dtype`
CAST_CONV = {'f32_f32': ('fp32', 0, 0, 'fp32', 'fp32'), 'f32_bf16': ('bf16', 1, 0, 'fp32', 'bf16'),
             'bf16_bf16': ('bf16', 0, 0, 'bf16', 'bf16'), 'bf16_f32': ('bf16', 0, 1, 'bf16', 'fp32')}


def rup8(c):
    return (c + 7) // 8 * 8


# col_off, ld parity, base offset and fill_cols of the first destination, its activation; the same of the second destination or None.
# `pad` columns follow the filled ones in a row (2 keeps ld's parity that of col_off + fill, 3 flips it); they must stay untouched.
def cast_layouts(cols):
    return [
        dict(col_off=0, pad=2 + (cols & 1), off=0, fill=cols, act=None, d2=None),                           # pair1 (bf16): even ld
        dict(col_off=3, pad=2 + ((cols + 3 + 1) & 1), off=0, fill=cols + 1, act=0.01, d2=None),             # odd col_off, even ld
        dict(col_off=2, pad=3, off=0, fill=rup8(cols), act=0.2, d2=None),                                   # odd ld (rup8 is even)
        dict(col_off=0, pad=2 + ((cols + 1) & 1), off=1, fill=cols + 1, act=None,                           # dst base + 1 element;
             d2=dict(col_off=2, pad=2 + (cols & 1), off=0, fill=cols, act=0.01)),                           # fill2 < fill, pair2
        dict(col_off=4, pad=2 + (cols & 1), off=0, fill=cols, act=0.01,                                     # pair1;
             d2=dict(col_off=1, pad=3, off=0, fill=cols + 3, act=None)),                                    # fill2 > fill, odd col_off2
        dict(col_off=0, pad=2 + ((cols + 1) & 1), off=0, fill=cols + 1, act=None,                           # pair1 with a fill column;
             d2=dict(col_off=0, pad=2, off=1, fill=rup8(cols) + 8, act=0.3)),                               # fill2 > fill, dst2 base + 1
    ]


def cast_expect(buf, x, rows, d, ld, dtype):
    y = x if d['act'] is None else torch.where(x > 0, x, x * torch.tensor(d['act'], dtype=torch.float32))   # the kernel's expression
    e = buf.before.clone()
    v = e[buf.lo:buf.lo + rows * ld].view(rows, ld)
    cols = x.shape[1]
    v[:, d['col_off']:d['col_off'] + cols] = y.to(tdt(dtype))                                               # one RNE rounding
    v[:, d['col_off'] + cols:d['col_off'] + d['fill']] = 0
    return e


# 8197 rows > 8192 = 2048 blocks x 4 waves: waves 0..4 take a second row.  130 and 513 columns > 128: a lane loops over columns.
@pytest.mark.parametrize('conv', list(CAST_CONV))
@pytest.mark.parametrize('rows,cols', [(r, c) for r in (1, 5, 8197) for c in (1, 80, 81, 130, 513) if c < 513 or r < 100])
def test_cast_rows(zs, conv, rows, cols):
    L = zs
    dtype, src_f32, dst_f32, st, dt1 = CAST_CONV[conv]
    x = rnd(torch.randn(rows, cols, generator=gen(rows + cols)), st)
    x[x == 0] = 1.0                                             # no -0 (and no NaN): the bits of the reference are then unambiguous
    ld_src = cols + 3
    src = Buf(rows * ld_src, tdt(st), init=padded(x, ld_src))
    for i, d in enumerate(cast_layouts(cols)):
        ld = d['col_off'] + d['fill'] + d['pad']
        dst = Buf(rows * ld, tdt(dt1), off=d['off'])
        kw, d2 = {}, d['d2']
        if d2:
            ld2 = d2['col_off'] + d2['fill'] + d2['pad']
            dst2 = Buf(rows * ld2, tdt(dtype), off=d2['off'])
            kw = dict(dst2=dst2.ptr(L), ld_dst2=ld2, col_off2=d2['col_off'], fill_cols2=d2['fill'],
                      act2=L.ZS_ACT_NONE if d2['act'] is None else L.ZS_ACT_LRELU, slope2=d2['act'] or 0.0)
        L.call('zs_cast_rows', 'ZsCastRows', stream(), dtype=_dt(L, dtype), src=src.ptr(L), ld_src=ld_src, src_f32=src_f32, dst=dst.ptr(L),
               ld_dst=ld, dst_f32=dst_f32, col_off=d['col_off'], rows=rows, cols=cols, fill_cols=d['fill'],
               act=L.ZS_ACT_NONE if d['act'] is None else L.ZS_ACT_LRELU, slope=d['act'] or 0.0, **kw)
        same_bits('layout %d: dst' % i, dst.image(), cast_expect(dst, x, rows, d, ld, dt1))
        if d2:
            same_bits('layout %d: dst2' % i, dst2.image(), cast_expect(dst2, x, rows, d2, ld2, dtype))
    src.unchanged('src')


# ---- zs_add_rowvec ---------------------------------------------------------------------------------------------------------------
def rowvec_case(L, dtype, B, T, C, fill, with_x, ldo, off=0):
    g = gen(B * 1000 + T + C)
    n_vec, vec_ld, unused = 4, C + 3, 2
    vec = torch.randn(n_vec, C, generator=g)
    vec[unused] = NAN                                           # a row that idx never names
    idx = torch.tensor([(0, 3, 3, 1, 0, 3, 1, 1, 0)[b % 9] for b in range(B)])        # repeats
    bvec, bidx = Buf(n_vec * vec_ld, init=padded(vec, vec_ld)), Buf(B, torch.int64, init=idx)
    rows = B * T
    x, bx = None, None
    if with_x:
        x = rnd(torch.randn(rows, fill, generator=g), dtype)
        bx = Buf(rows * (fill + 2), tdt(dtype), init=padded(x, fill + 2))
    out = Buf(rows * ldo, tdt(dtype), off=off)
    L.call('zs_add_rowvec', 'ZsAddRowvec', stream(), dtype=_dt(L, dtype), x=bx.ptr(L) if bx else None, ldx=fill + 2, vec=bvec.ptr(L),
           vec_ld=vec_ld, idx=bidx.ptr(L), out=out.ptr(L), ldo=ldo, B=B, T=T, C=C, fill_cols=fill)
    ref = x.clone() if with_x else torch.zeros(rows, fill)      # columns C <= c < fill: x, or 0 in the broadcast form
    ref[:, :C] += vec[idx].repeat_interleave(T, 0)
    e = out.before.clone()
    e[out.lo:out.lo + rows * ldo].view(rows, ldo)[:, :fill] = ref.to(tdt(dtype))
    same_bits('out', out.image(), e)
    bvec.unchanged('vec')
    bidx.unchanged('idx')
    if bx:
        bx.unchanged('x')


ROWVEC_SHAPES = [(2, 3, 5, 8), (3, 17, 130, 136), (5, 1031, 250, 256)]


# add_rowvec_kernel (x given).  5 x 1031 x 256 = 1 319 680 > 1 048 576 = 4096 blocks x 256 threads: the grid-stride loop runs
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', ROWVEC_SHAPES)
def test_add_rowvec_with_x(zs, dtype, shape):
    B, T, C, fill = shape
    rowvec_case(zs, dtype, B, T, C, fill, True, fill + 3)


# x == null.  bcast8: fill_cols % 8 == 0, ldo % 8 == 0 and a 16-byte base take add_rowvec_bcast8_kernel; each of the three other
# variants breaks one of the conditions and must take add_rowvec_kernel with x == null
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('variant', ['bcast8', 'fill_not_8', 'ldo_not_8', 'base+1'])
@pytest.mark.parametrize('shape', ROWVEC_SHAPES)
def test_add_rowvec_broadcast(zs, dtype, shape, variant):
    B, T, C, fill = shape
    if variant == 'fill_not_8':
        fill += 1
    assert (fill % 8 != 0) == (variant == 'fill_not_8')
    ldo = fill + (8 if variant != 'ldo_not_8' else 5)
    assert (ldo % 8 != 0) == (variant in ('ldo_not_8', 'fill_not_8'))
    rowvec_case(zs, dtype, B, T, C, fill, False, ldo, off=1 if variant == 'base+1' else 0)


@pytest.mark.parametrize('dtype', DTYPES)
def test_add_rowvec_broadcast8_loops(zs, dtype):
    B, T, C, fill = 9, 1025, 1000, 1024
    assert B * T * fill // 8 > 4096 * 256                       # 1 180 800 groups of 8 > 1 048 576: add_rowvec_bcast8_kernel loops
    rowvec_case(zs, dtype, B, T, C, fill, False, fill + 8)


# ---- zs_rows_reverse -------------------------------------------------------------------------------------------------------------
# (6, 1025, 768): 6 x 512 x 768 (fp32) or x 384 (bf16) words > 1 048 576 = 4096 blocks x 256 threads: the grid-stride loop; 1025
# and 9 are odd T (the middle row stays); (1, 1, 4): T < 2 launches nothing
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('use_lengths', [False, True], ids=['full', 'lengths'])
@pytest.mark.parametrize('shape', [(1, 1, 4), (3, 2, 6), (4, 9, 96), (6, 1025, 768)])
def test_rows_reverse(zs, dtype, shape, use_lengths):
    L = zs
    B, T, cols = shape
    col0 = 2
    ld = col0 + cols + 4
    if shape == (6, 1025, 768):
        assert B * (T // 2) * (cols * (4 if dtype == 'fp32' else 2) // 4) > 4096 * 256
    x = rnd(torch.randn(B * T, ld, generator=gen(B + T)), dtype)
    buf = Buf(B * T * ld, tdt(dtype), init=x)
    odd = max(1, (2 * T // 3) | 1) if T > 1 else 1
    lengths = [min(T, v) for v in (0, T, 1, odd, T - 1, 3)][:B]               # 0, T, 1, an odd value, and for B = 6 an even one
    blen = Buf(B, torch.int32, init=torch.tensor(lengths, dtype=torch.int32)) if use_lengths else None
    L.call('zs_rows_reverse', 'ZsRowsReverse', stream(), dtype=_dt(L, dtype), x=buf.ptr(L), ld=ld, col0=col0, cols=cols, B=B, T=T,
           lengths=blen.ptr(L) if blen else None)
    ref = x.clone().view(B, T, ld)
    for b in range(B):
        n = lengths[b] if use_lengths else T
        ref[b, :n, col0:col0 + cols] = x.view(B, T, ld)[b, :n, col0:col0 + cols].flip(0)
    same_bits('x', buf.image(), buf.expect(ref))               # columns outside the block and rows at or past len included
    if blen:
        blen.unchanged('lengths')


# ---- zs_copy_vec_batch -----------------------------------------------------------------------------------------------------------
def test_copy_vec_batch(zs):
    """70 jobs = launches of 32, 32 and 6.  A launch's grid is sized by its longest job and capped at 64 blocks x 256 threads =
    16 384 elements: the 20 000 and 16 385 element jobs loop, and the short jobs beside them run in a grid far wider than they
    are."""
    L = zs
    g = gen(8)
    lens = [int(v) for v in torch.randint(1, 400, (70,), generator=g)]
    lens[0], lens[3], lens[31], lens[32], lens[40], lens[63], lens[64], lens[69] = 1, 20000, 257, 16385, 16384, 1, 256, 5000
    assert max(lens) == 20000 > 64 * 256 and min(lens) == 1
    strides = [((1, 1), (3, 1), (1, 3), (3, 3))[i % 4] for i in range(70)]    # (src_stride, dst_stride)
    so, do, s_at, d_at = 0, 0, [], []
    for n, (ss, ds) in zip(lens, strides):
        s_at.append(so)
        d_at.append(do)
        so += (n - 1) * ss + 1 + 2
        do += (n - 1) * ds + 1 + 2
    src = torch.randn(so, generator=g)
    bsrc, bdst = Buf(so, init=src), Buf(do)
    jobs = [L.STRUCTS['ZsVecCopy'](src=bsrc.ptr(L) + 4 * s, dst=bdst.ptr(L) + 4 * d, len=n, src_stride=ss, dst_stride=ds)
            for n, (ss, ds), s, d in zip(lens, strides, s_at, d_at)]
    arr = (L.STRUCTS['ZsVecCopy'] * len(jobs))(*jobs)
    L.check(L.lib().zs_copy_vec_batch(ctypes.addressof(arr), len(jobs), stream()), 'zs_copy_vec_batch')
    ref = torch.full((do,), NAN)                                # the skipped elements between strided destinations stay NaN
    for n, (ss, ds), s, d in zip(lens, strides, s_at, d_at):
        ref[d:d + (n - 1) * ds + 1:ds] = src[s:s + (n - 1) * ss + 1:ss]
    same_bits('dst', bdst.image(), bdst.expect(ref))
    bsrc.unchanged('src')


# ---- zs_host_fetch, zs_step_counters ---------------------------------------------------------------------------------------------
FETCH_TAIL = 8 * 1024           # guard elements (int32) behind source and destination: more than one grid stride of 16-byte words of
#                                 the largest grid below, so that a loop that ran a stride too far would be seen, not fault


# a lane has 8 loads in flight while i + 7 stride < n16; one workgroup: stride 256, so the unrolled loop starts at n16 = 1793 (lane 0
# only) and 4113 = 2 x 2048 + 17 runs it twice for 17 lanes; 3 workgroups: 768 lanes, 40 001 = 6 x 6144 + 3137; 0 = the default of 32
@pytest.mark.parametrize('wg,n16', [(1, 1), (1, 1791), (1, 1792), (1, 1793), (1, 4113), (3, 40001), (0, 40001)])
def test_host_fetch(zs, wg, n16):
    L = zs
    n = 4 * n16
    assert FETCH_TAIL * 4 // 16 > max(wg, 1) * 256 or wg == 0
    host = torch.full((n + FETCH_TAIL,), 0x5A5A5A5A, dtype=torch.int32)
    host[:n] = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=gen(n16), dtype=torch.int64).to(torch.int32)
    pinned = host.pin_memory()
    assert pinned.is_pinned() and pinned.data_ptr() % 16 == 0
    dst = Buf(n, torch.int32, tail=FETCH_TAIL)
    L.check(L.lib().zs_host_fetch(pinned.data_ptr(), dst.ptr(L), 16 * n16, wg, stream()), 'zs_host_fetch')
    same_bits('dst', dst.image(), dst.expect(host[:n]))        # bytes at or past `bytes` included
    assert torch.equal(pinned, host)


@pytest.mark.parametrize('which', ['seed', 'step', 'both'])
def test_step_counters(zs, which):
    L = zs
    golden = 0x9E3779B97F4A7C15
    to_i64 = lambda u: u - (1 << 64) if u >= (1 << 63) else u
    seeds = [0, 12345, (1 << 64) - 5, (1 << 64) - golden]      # the last two wrap modulo 2^64 (the last one to exactly 0)
    for s0 in seeds:
        seed = Buf(1, torch.int64, init=torch.tensor([to_i64(s0)]))
        step = Buf(1, torch.int32, init=torch.tensor([41], dtype=torch.int32))
        for k in (1, 2):
            L.check(L.lib().zs_step_counters(seed.ptr(L) if which != 'step' else None, step.ptr(L) if which != 'seed' else None, stream()),
                    'zs_step_counters')
            want_seed = to_i64((s0 + k * golden) % (1 << 64)) if which != 'step' else to_i64(s0)
            assert int(seed.region('seed')[0]) == want_seed, (hex(s0), k, int(seed.region('seed')[0]), want_seed)
            assert int(step.region('step')[0]) == (41 + k if which != 'seed' else 41)
    assert any(s0 + golden >= (1 << 64) for s0 in seeds)


# ---- rejections: ZS_EINVAL before any launch --------------------------------------------------------------------------------------
def test_bad_arguments_are_refused(zs):
    L = zs
    assert L.ZS_EINVAL == -1
    st = stream()
    f32, bf = Buf(4096), Buf(4096, torch.bfloat16)
    i64, part, lo = Buf(8, torch.int64, init=torch.zeros(8, dtype=torch.int64)), Buf(1024), Buf(1)
    with pytest.raises(L.ZsError):                              # a bf16 block of an odd number of columns is not made of 4-byte words
        L.call('zs_rows_reverse', 'ZsRowsReverse', st, dtype=L.ZS_BF16, x=bf.ptr(L), ld=8, col0=0, cols=3, B=2, T=4)
    pinned = torch.zeros(64, dtype=torch.int32).pin_memory()
    rc = L.lib().zs_host_fetch(pinned.data_ptr(), f32.ptr(L), 24, 1, st)                      # bytes % 16 != 0
    assert rc == L.ZS_EINVAL
    with pytest.raises(L.ZsError):
        L.check(rc, 'zs_host_fetch')
    with pytest.raises(L.ZsError):                              # bc1 = 0 and no step_ptr
        L.call('zs_adam_clip', 'ZsAdam', st, p=f32.ptr(L), g=f32.ptr(L) + 1024, m=f32.ptr(L) + 2048, v=f32.ptr(L) + 3072, n=16,
               bc1=0.0, bc2=0.1, max_norm=0.0, **AD)
    with pytest.raises(L.ZsError):                              # fill_cols < cols
        L.call('zs_cast_rows', 'ZsCastRows', st, dtype=L.ZS_F32, src=f32.ptr(L), ld_src=8, dst=f32.ptr(L) + 1024, ld_dst=8, rows=2, cols=6,
               fill_cols=5)
    with pytest.raises(L.ZsError):                              # fill_cols < C
        L.call('zs_add_rowvec', 'ZsAddRowvec', st, dtype=L.ZS_F32, vec=f32.ptr(L), vec_ld=8, idx=i64.ptr(L), out=f32.ptr(L) + 1024, ldo=8,
               B=2, T=2, C=6, fill_cols=5)
    with pytest.raises(L.ZsError):                              # partial null
        L.call('zs_l1_loss', 'ZsL1Loss', st, dtype=L.ZS_F32, x_dec=f32.ptr(L), ld_dec=8, x=f32.ptr(L) + 1024, ldx=8, rows=2, F=6,
               loss_out=lo.ptr(L), grad_scale=1.0)
    for name, b in (('f32', f32), ('bf16', bf), ('idx', i64), ('partial', part), ('loss_out', lo)):
        b.unchanged(name)                                       # nothing ran
