"""Stage-2 InstanceNorm2d kernels of zs_patch.hip (zs_in2d_stats, zs_row_moments, zs_in2d_finalize, zs_in2d_fwd / _bwd / _adj)
and the gradient-penalty glue (zs_gp_penalty, zs_lerp_rows), kernel by kernel against the formulas of include/zs_amd.h in fp64.

Tolerances (each check prints its measured error):
  * elementwise outputs: relative to the largest magnitude of the reference -- fp32 F32_TOL = 4e-7 (a few roundings of the
    formula; measured 1.4e-7), bf16 BF16_TOL = 2^-7 (one output rounding is up to 2^-8 of the value; references read the same
    bf16-rounded operands; measured 3.3e-3).
  * statistics are fp32 in both dtypes: |d mean| <= MEAN_K * 2^-24 * max|y| (measured 6.0), |d rstd| / rstd <= RSTD_K * 2^-24 *
    (1 + max|y| * rstd) (measured 1.5; the second term is the mean's own rounding inside the variance: data 100 + N(0, 1) make
    it ~100 units, while a one-pass E[y^2] - E[y]^2 in fp32 would be off by ~10^4 units); the one-pass and the two-pass
    statistics differ by no more than that either (measured 6.3 and 1.9).  Moment sums: |d s| <= MOM_K * 2^-24 * sum |term|
    per (sample, channel) (measured 10.2: s2 of a centred bf16 sum).
  * gradient penalty (units of 2^-24 of the value): s_b is a double sum rounded once (bound 2, measured 0.63), gp a few fp32
    roundings of the kernel's own s_b (2, measured 0.77), gbar likewise (5, measured 1.9), lerp_rows (4, measured 1.9)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = ['fp32', 'bf16']
EPS, SLOPE = 1e-5, 0.2
U = 2.0 ** -24
F32_TOL, BF16_TOL = 4e-7, 2.0 ** -7
MEAN_K, RSTD_K, MOM_K = 16.0, 4.0, 24.0


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


def rnd(x, dtype):
    return x.float() if dtype == 'fp32' else x.to(torch.bfloat16).float()


def tdt(dtype):
    return torch.float32 if dtype == 'fp32' else torch.bfloat16


def dev(x, dtype, ld):
    """[..., C] fp32 cpu -> [rows, ld] device rows in the kernel dtype (columns past C zero), on a buffer with slack."""
    C = x.shape[-1]
    rows = x.numel() // C
    buf = torch.zeros(rows * ld + 256, dtype=tdt(dtype), device='cuda:0')
    v = buf[:rows * ld].view(rows, ld)
    v[:, :C] = x.reshape(rows, C).to(v.device, v.dtype)
    return v


def sentinel(rows, ld, dtype):
    return torch.full((rows * ld + 256,), float('nan'), dtype=tdt(dtype), device='cuda:0')[:rows * ld].view(rows, ld)


def host(v, shape, C):
    h = v.float().cpu()
    if v.shape[1] > C:
        assert torch.isnan(h[:, C:]).all(), 'columns past C written'
    return h[:, :C].double().reshape(*shape, C)


def f32d(t):
    return t.float().contiguous().to('cuda:0')


def stream():
    return torch.cuda.current_stream().cuda_stream


def check(name, got, ref, tol):
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), name + ': non-finite output'
    scale = max(1e-6, ref.abs().max().item())
    err = (got - ref).abs()
    print('[err] %s: %.3g of scale %.3g (bound %.3g)' % (name, err.max().item() / scale, scale, tol))
    if err.max().item() > tol * scale:
        i = np.unravel_index(int(err.argmax()), err.shape)
        raise AssertionError('%s: max err %.4g > %.4g (scale %.3g) at %s: got %.7g ref %.7g' %
                             (name, err[i].item(), tol * scale, scale, tuple(int(k) for k in i), got[i].item(), ref[i].item()))


def check_units(name, err, unit, bound):
    units = (err / unit).max().item()
    print('[err] %s: %.3g units of 2^-24 (bound %g)' % (name, units, bound))
    assert units <= bound, '%s: %.3g units > %g' % (name, units, bound)


def data(g, B, T, C, dtype):
    """Every third channel 100 + N(0, 1) (where a one-pass variance loses its digits), the others mean -3..3, spread 0.5..2."""
    far = (torch.arange(C) % 3 == 0).view(1, 1, C)
    off = torch.where(far, torch.full((1, 1, C), 100.0), torch.rand(1, 1, C, generator=g) * 6 - 3)
    sd = torch.where(far, torch.ones(1, 1, C), torch.rand(1, 1, C, generator=g) * 1.5 + 0.5)
    return rnd(off + sd * torch.randn(B, T, C, generator=g), dtype)


def check_stats(name, mean, rstd, y):
    m64 = y.mean(1)
    r64 = 1.0 / torch.sqrt(((y - m64[:, None]) ** 2).mean(1) + EPS)
    amax = y.abs().amax(1)
    check_units(name + ' mean', (mean - m64).abs(), U * amax, MEAN_K)
    check_units(name + ' rstd', (rstd - r64).abs() / r64, U * (1 + amax * r64), RSTD_K)


def moments_call(L, dtype, u, B, T, C, s1, **kw):
    ws = torch.empty(L.lib().zs_row_moments_workspace(B, T, C) + 64, dtype=torch.uint8, device='cuda:0')
    L.call('zs_row_moments', 'ZsRowMoments', stream(), dtype=_dt(L, dtype), u=u.data_ptr(), ldu=u.shape[1], B=B, T=T, C=C,
           s1=s1.data_ptr(), partial=ws.data_ptr(), partial_bytes=ws.numel(), **kw)


def stat_buf(B, C):
    return torch.full((B * C,), float('nan'), dtype=torch.float32, device='cuda:0')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', [8, 32, 56, 64, 72, 512])
@pytest.mark.parametrize('T', [1, 31, 32, 33, 511, 512, 513, 1040, 16448])
def test_in2d_stats_vs_fp64_and_two_pass(zs, dtype, C, T):
    """zs_in2d_stats (one pass: 512-row slabs, Chan merges of the 32 row groups and of the slabs) across the slab boundaries, up to
    the first critic layer's T = 16448, against fp64 and against the two-pass path (zs_row_moments for sum y, again for the
    centred second moment, zs_in2d_finalize).  Both are held to the fp32 statistics bounds; so is their difference."""
    L = zs
    B = 3 if T * C <= 1 << 19 else 1
    g = torch.Generator().manual_seed(T * 13 + C)
    y = data(g, B, T, C, dtype)
    Y = dev(y, dtype, C)
    mean, rstd = stat_buf(B, C), stat_buf(B, C)
    ws = torch.empty(L.lib().zs_row_moments_workspace(B, T, C) + 64, dtype=torch.uint8, device='cuda:0')
    L.check(L.lib().zs_in2d_stats(_dt(L, dtype), Y.data_ptr(), C, B, T, C, EPS, mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(), ws.numel(),
                                  stream()), 'zs_in2d_stats')
    s1, q, tmp, mean2, rstd2 = (stat_buf(B, C) for _ in range(5))
    moments_call(L, dtype, Y, B, T, C, s1)
    moments_call(L, dtype, Y, B, T, C, tmp, v=Y.data_ptr(), ldv=C, s2=q.data_ptr(), center_sum=s1.data_ptr(), center_scale=1.0 / T)
    L.check(L.lib().zs_in2d_finalize(s1.data_ptr(), q.data_ptr(), mean2.data_ptr(), rstd2.data_ptr(), B * C, T, EPS, stream()), 'zs_in2d_finalize')
    torch.cuda.synchronize()
    yd = y.double()
    tag = '%s B%d T%d C%d' % (dtype, B, T, C)
    m1, r1 = mean.cpu().double().view(B, C), rstd.cpu().double().view(B, C)
    m2, r2 = mean2.cpu().double().view(B, C), rstd2.cpu().double().view(B, C)
    check_stats('in2d_stats ' + tag, m1, r1, yd)
    check_stats('two-pass ' + tag, m2, r2, yd)
    amax = yd.abs().amax(1)
    check_units('one vs two pass mean ' + tag, (m1 - m2).abs(), U * amax, MEAN_K)
    check_units('one vs two pass rstd ' + tag, (r1 - r2).abs() / r2, U * (1 + amax * r2), RSTD_K)


MOM_CASES = ['s1', 'v_eq_u', 'v_ne_u', 'y', 'w', 'center', 'adjoint']


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(3, 33, 56), (2, 1040, 520), (1, 513, 72)])
@pytest.mark.parametrize('case', MOM_CASES)
def test_row_moments_operands_vs_fp64(zs, dtype, shape, case):
    """zs_row_moments, each optional operand on its own -- s2 with v == u and with v != u, the lrelu'(y) weight, s3 = sum u*w,
    center_sum -- and the double backward's combination (y, v != u, w).  Header: u' = u - center_sum*center_scale,
    m = lrelu'(y), s1 = sum u'*m, s2 = sum u'*m*v (v == u: sum u'^2), s3 = sum u*w."""
    L = zs
    B, T, C = shape
    g = torch.Generator().manual_seed(len(case) * 100 + T)
    u = rnd(data(g, B, T, C, dtype) * 0.1, dtype)
    v, y, w = (rnd(torch.randn(B, T, C, generator=g), dtype) for _ in range(3))
    ld = C + 8
    Ud, Vd, Yd, Wd = dev(u, dtype, ld), dev(v, dtype, ld), dev(y, dtype, ld), dev(w, dtype, ld)
    s1, s2, s3 = stat_buf(B, C), stat_buf(B, C), stat_buf(B, C)
    kw, uc, m = {}, u.double(), torch.ones(1, dtype=torch.float64)
    if case == 'center':
        csum = (u.double().sum(1) * (1 + 0.01 * torch.randn(B, C, generator=g).double())).float()
        ctr = (csum * torch.tensor(1.0 / T, dtype=torch.float32)).double()   # the kernel's fp32 centre
        csum_d = f32d(csum)
        kw.update(center_sum=csum_d.data_ptr(), center_scale=1.0 / T, v=Ud.data_ptr(), ldv=ld, s2=s2.data_ptr())
        uc = u.double() - ctr[:, None]
    if case in ('y', 'adjoint'):
        kw.update(y=Yd.data_ptr(), ldy=ld, slope=SLOPE)
        m = torch.where(y > 0, 1.0, SLOPE).double()
    if case == 'v_eq_u':
        kw.update(v=Ud.data_ptr(), ldv=ld, s2=s2.data_ptr())
    if case in ('v_ne_u', 'y', 'adjoint'):
        kw.update(v=Vd.data_ptr(), ldv=ld, s2=s2.data_ptr())
    if case in ('w', 'adjoint'):
        kw.update(w=Wd.data_ptr(), ldw=ld, s3=s3.data_ptr())
    moments_call(L, dtype, Ud, B, T, C, s1, **kw)
    torch.cuda.synchronize()
    tag = '%s %s B%d T%d C%d' % (case, dtype, B, T, C)
    t1 = uc * m
    refs = [('s1', s1, t1)]
    if 's2' in kw:
        refs.append(('s2', s2, t1 * (uc if kw['v'] == Ud.data_ptr() else v.double())))
    if 's3' in kw:
        refs.append(('s3', s3, u.double() * w.double()))
    for nm, got, terms in refs:
        err = (got.cpu().double().view(B, C) - terms.sum(1)).abs()
        check_units('row_moments %s %s' % (nm, tag), err, U * terms.abs().sum(1).clamp_min(1e-30), MOM_K)
    for nm, buf in (('s2', s2), ('s3', s3)):
        if nm not in kw:
            assert torch.isnan(buf.cpu()).all(), nm + ' written without being asked for'


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(1, 16448, 64), (128, 17, 72), (2, 300, 520), (3, 100, 56)])
@pytest.mark.parametrize('drop', [False, True])
def test_in2d_fwd_bwd_adj_vs_fp64(zs, dtype, shape, drop):
    """zs_in2d_fwd, zs_in2d_bwd (without and with ga2 / S2x) and zs_in2d_adj against the header's formulas in fp64, with dm NULL or
    holding dropped maps (dm = 0) next to kept ones (dm = 2), rows with ld > C, and shapes where row_walk_grid clamps (B = 1 at
    T = 16448; B = 128 at T = 17) or the 8-channel groups do not divide 256 threads (C = 56, 72, 520).  The statistics fed in
    are exact fp32 numbers; the reference reads the same operands.  Columns past C are not written."""
    L = zs
    B, T, C = shape
    ld = C + 16
    tol = F32_TOL if dtype == 'fp32' else BF16_TOL
    g = torch.Generator().manual_seed(B * 7 + T + C + drop)
    y = data(g, B, T, C, dtype)
    yd = y.double()
    mean = yd.mean(1).float()
    rstd = (1.0 / torch.sqrt(((yd - yd.mean(1)[:, None]) ** 2).mean(1) + EPS)).float()
    if drop:
        keep = torch.rand(B, C, generator=g) >= 0.5
        keep.view(-1)[0], keep.view(-1)[1] = False, True
        dm = keep.float() * 2.0
    else:
        dm = torch.ones(B, C)
    inv_dm = torch.where(dm > 0, 1.0 / dm.clamp_min(1e-30), torch.zeros(())).double()
    dmd, r64 = dm.double()[:, None], rstd.double()[:, None]
    Yd = dev(y, dtype, ld)
    dm_d, mean_d, rstd_d = f32d(dm), f32d(mean), f32d(rstd)          # (kept alive until the launches have run)
    common = dict(dtype=_dt(L, dtype), rstd=rstd_d.data_ptr(), dm=dm_d.data_ptr() if drop else None, B=B, T=T, C=C)
    tag = '%s B%d T%d C%d%s' % (dtype, B, T, C, ' dropout' if drop else '')
    # forward
    A = sentinel(B * T, ld, dtype)
    L.call('zs_in2d_fwd', 'ZsIn2dFwd', stream(), y=Yd.data_ptr(), ldy=ld, a=A.data_ptr(), lda=ld, mean=mean_d.data_ptr(), **common)
    torch.cuda.synchronize()
    a = host(A, (B, T), C)
    check('in2d_fwd ' + tag, a, (yd - mean.double()[:, None]) * r64 * dmd, tol)
    xhat = a * inv_dm[:, None]
    lr = torch.where(y > 0, 1.0, SLOPE).double()
    # backward, then with the second gradient addend and the rstd adjoint S2x
    ga, ga2 = (rnd(torch.randn(B, T, C, generator=g), dtype) for _ in range(2))
    GA, GA2 = dev(ga, dtype, ld), dev(ga2, dtype, ld)
    for with2 in (False, True):
        gsum = ga.double() + (ga2.double() if with2 else 0.0)
        S1, S2 = gsum.sum(1).float(), (gsum * a).sum(1).float()
        S2x = (torch.randn(B, C, generator=g) * S2.abs().mean()).float() if with2 else torch.zeros(B, C)
        GZ = sentinel(B * T, ld, dtype)
        S1d, S2d, S2xd = f32d(S1), f32d(S2), f32d(S2x)
        L.call('zs_in2d_bwd', 'ZsIn2dBwd', stream(), ga=GA.data_ptr(), ldga=ld, ga2=GA2.data_ptr() if with2 else None, ldga2=ld,
               a=A.data_ptr(), lda=ld, y=Yd.data_ptr(), ldy=ld, S1=S1d.data_ptr(), S2=S2d.data_ptr(),
               S2x=S2xd.data_ptr() if with2 else None, slope=SLOPE, gz=GZ.data_ptr(), ldgz=ld, **common)
        torch.cuda.synchronize()
        s2t = (S2.double() + S2x.double())[:, None]
        ref = (r64 * dmd * (gsum - S1.double()[:, None] / T) - r64 * xhat * s2t / T) * lr
        check('in2d_bwd%s %s' % (' ga2+S2x' if with2 else '', tag), host(GZ, (B, T), C), ref, tol)
    # double backward (adjoint of the backward)
    gbz = rnd(torch.randn(B, T, C, generator=g), dtype)
    gby = gbz.double() * lr
    A1, A2 = gby.sum(1).float(), (gby * a).sum(1).float()
    S2 = (ga.double() * a).sum(1).float()
    GBZ, GBA, XBA = dev(gbz, dtype, ld), sentinel(B * T, ld, dtype), sentinel(B * T, ld, dtype)
    A1d, A2d, S2d = f32d(A1), f32d(A2), f32d(S2)
    L.call('zs_in2d_adj', 'ZsIn2dAdj', stream(), gbz=GBZ.data_ptr(), ldgbz=ld, y=Yd.data_ptr(), ldy=ld, a=A.data_ptr(), lda=ld,
           ga=GA.data_ptr(), ldga=ld, A1=A1d.data_ptr(), A2=A2d.data_ptr(), S2=S2d.data_ptr(), slope=SLOPE,
           gba=GBA.data_ptr(), ldgba=ld, xba=XBA.data_ptr(), ldxba=ld, **common)
    torch.cuda.synchronize()
    idm, a2, a1 = inv_dm[:, None], A2.double()[:, None], A1.double()[:, None]
    ref_gba = dmd * r64 * (gby - a1 / T - xhat * idm * a2 / T)
    ref_xba = -idm * r64 * (gby * S2.double()[:, None] / T + ga.double() * dmd * idm * a2 / T)
    check('in2d_adj gbar_a ' + tag, host(GBA, (B, T), C), ref_gba, tol)
    check('in2d_adj xbar_a ' + tag, host(XBA, (B, T), C), ref_xba, tol)


@pytest.mark.parametrize('B, n', [(1, 1), (1, 3000), (3, 1025), (5, 16448)])
def test_gp_penalty_and_lerp_rows_vs_fp64(zs, B, n):
    """zs_lerp_rows: out[b] = alpha[b]*x[b] + (1 - alpha[b])*y[b].  zs_gp_penalty: s_b = sqrt(1e-12 + sum g_b^2) (double sum, one
    rounding), gp = mean_b (1 - s_b)^2, gbar[b] = scale*(2/B)*(s_b - 1)/s_b*g[b]; n not a multiple of the 1024-thread workgroup,
    and (B > 1) an all-zero sample, whose s_b is 1e-6 and whose gbar row is finite zeros."""
    L = zs
    g = torch.Generator().manual_seed(B * 10 + n)
    x, y = torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)
    alpha = torch.rand(B, generator=g)
    X, Y, AL, OUT = f32d(x), f32d(y), f32d(alpha), torch.full((B * n + 64,), float('nan'), device='cuda:0')
    L.check(L.lib().zs_lerp_rows(X.data_ptr(), Y.data_ptr(), AL.data_ptr(), OUT.data_ptr(), B, n, stream()), 'zs_lerp_rows')
    grad = torch.randn(B, n, generator=g) * (torch.rand(B, 1, generator=g) * 3 / np.sqrt(n))
    if B > 1:
        grad[1] = 0.0
    G = f32d(grad)
    scale = 10.0
    s, gp, gbar = (torch.full((m + 64,), float('nan'), device='cuda:0') for m in (B, 1, B * n))
    L.check(L.lib().zs_gp_penalty(G.data_ptr(), B, n, scale, s.data_ptr(), gp.data_ptr(), gbar.data_ptr(), stream()), 'zs_gp_penalty')
    torch.cuda.synchronize()
    ad, xd, yd = alpha.double()[:, None], x.double(), y.double()
    err = (OUT[:B * n].cpu().double().view(B, n) - (ad * xd + (1 - ad) * yd)).abs()
    check_units('lerp_rows B%d n%d' % (B, n), err, U * ((ad * xd).abs() + ((1 - ad) * yd).abs()).clamp_min(1e-30), 4)
    sg = s[:B].cpu().double()
    s64 = torch.sqrt(1e-12 + (grad.double() ** 2).sum(1))
    check_units('gp s_b B%d n%d' % (B, n), (sg - s64).abs(), U * s64, 2)
    d = (1 - sg) ** 2
    check_units('gp B%d n%d' % (B, n), (gp[0].cpu().double() - d.mean()).abs(), U * d.mean().clamp_min(1e-30), 2)
    ref = scale * (2.0 / B) * ((sg - 1) / sg)[:, None] * grad.double()
    got = gbar[:B * n].cpu().double().view(B, n)
    assert torch.isfinite(got).all()
    check_units('gp gbar B%d n%d' % (B, n), (got - ref).abs(), U * ref.abs().clamp_min(1e-30), 5)
    if B > 1:
        assert sg[1].item() == float(np.float32(1e-6)) and (got[1] == 0).all(), 'all-zero sample'
