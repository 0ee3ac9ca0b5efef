"""InstanceNorm1d kernels (zs_instnorm_fwd, zs_instnorm_bwd, zs_grad_combine) and zs_emb_scatter against fp64 references, in
both decompositions of zs_norm.hip: 32 row groups x 64 channels ("narrow") and 8 row groups x 256 channels ("wide", bf16,
C >= 256, T <= the norm_lim knob of the kernel and <= 64).  zs_norm_decomposition reports which one a launch takes; the tests
assert it for every case that is meant to run the wide one.

Tolerances (bounds relative to the largest magnitude of the reference, `scale`; each check prints its measured error):
  * fp32 outputs of the two normalisations: F32_TOL = 2e-5 -- summation order of fp32 reductions over T against fp64 (measured
    worst without the allowances below: 1.7e-5, the backward at T = 2).  The combine has no reduction in its output: a few fp32
    roundings, COMBINE_F32_TOL = 2.5e-7 (measured 8.9e-8).
  * bf16 outputs: BF16_TOL = 2^-7 -- one rounding to bf16 is up to 2^-8 of the value (8 significant bits); the reference is built
    from the same bf16-rounded inputs.  Measured worst 3.7e-3 of scale: one rounding.
  * x - mean cancels: fp32 cannot represent the mean of a channel better than its rounding, and the normalisation multiplies
    that error by rstd (316 for a constant channel at eps = 1e-5).  Forward outputs therefore also get
    CANCEL_K * 2^-24 * max|x| * rstd per (sample, channel) -- the mean's rounding bound (CANCEL_K = MEAN_K), amplified
    (measured 6.2 units: constant channels at T = 31).  The backward's
    g - mean(g) - xhat * mean(g xhat) cancels the same way (T = 2 cancels it completely) and is multiplied by rstd again:
    BWD_K * 2^-24 * rstd * (|g| + |mean g| + |xhat| |mean g xhat| (1 + max|x| rstd)) per element.
  * statistics (mean, rstd, emb_sum) are fp32 in both dtypes and held to fp32 bounds: |d mean| <= MEAN_K * 2^-24 * max|x|
    (measured 8.5: the 32 canonical partials add in sequence), |d rstd| / rstd <= RSTD_K * 2^-24 * (1 + max|x| * rstd)
    (measured 1.8; the second term is the mean's rounding inside the variance), emb_sum within EMB_K * 2^-24 of
    |emb_sum(0)| + sum_t |v| (measured 3.0)."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = ['fp32', 'bf16']
EPS, SLOPE = 1e-5, 0.01
U = 2.0 ** -24
F32_TOL, COMBINE_F32_TOL, BF16_TOL = 2e-5, 2.5e-7, 2.0 ** -7
MEAN_K, RSTD_K, BWD_K, EMB_K = 24.0, 4.0, 8.0, 8.0
CANCEL_K = MEAN_K
WIDE = dict(norm_wide=1, norm_lim0=64, norm_lim1=64, norm_lim2=64)
NARROW = dict(norm_wide=0)
FWD, BWD, COMBINE = 0, 1, 2
T_WIDE = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64]
T_NARROW = [65, 128, 255, 256]


@pytest.fixture(scope='module')
def zs():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    from zs_amd import _lib
    _lib.lib()
    return _lib


@contextlib.contextmanager
def knobs(L, **kv):
    old = {}
    try:
        for k, v in kv.items():
            old[k] = L.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            L.set_option(k, v)


def _dt(L, dtype):
    return L.ZS_F32 if dtype == 'fp32' else L.ZS_BF16


def decomposition(L, kernel, dtype, T, C):
    rc = L.lib().zs_norm_decomposition(kernel, _dt(L, dtype), T, C)
    assert rc in (0, 1), L.last_error()
    return 'wide' if rc else 'narrow'


def variants(L, kernel, dtype, T, C):
    """(name, knobs) of every decomposition this shape can take: both for bf16 at T <= 64, C >= 256 (asserted), else the one."""
    if dtype == 'bf16' and T <= 64 and C >= 256:
        with knobs(L, **WIDE):
            assert decomposition(L, kernel, dtype, T, C) == 'wide'
        with knobs(L, **NARROW):
            assert decomposition(L, kernel, dtype, T, C) == 'narrow'
        return [('wide', WIDE), ('narrow', NARROW)]
    return [(decomposition(L, kernel, dtype, T, C), {})]


def rnd(x, dtype):
    """fp32 cpu tensor -> the values the kernel reads (bf16-rounded for bf16), still fp32."""
    return x.float() if dtype == 'fp32' else x.to(torch.bfloat16).float()


def dev(x, dtype, ld):
    """[..., C] fp32 cpu -> [rows, ld] device rows in the kernel dtype, columns past C zero (buffer with slack)."""
    C = x.shape[-1]
    rows = x.numel() // C
    buf = torch.zeros(rows * ld + 256, dtype=torch.float32 if dtype == 'fp32' else torch.bfloat16, device='cuda:0')
    v = buf[:rows * ld].view(rows, ld)
    v[:, :C] = x.reshape(rows, C).to(v.device, v.dtype)
    return v


def sentinel(rows, ld, dtype, fill=float('nan')):
    buf = torch.full((rows * ld + 256,), fill, dtype=torch.float32 if dtype == 'fp32' else torch.bfloat16, device='cuda:0')
    return buf[:rows * ld].view(rows, ld)


def f32(n, fill=float('nan')):
    return torch.full((n + 64,), fill, dtype=torch.float32, device='cuda:0')


def host(v, shape, C):
    """device rows -> fp64 cpu [shape..., C] of the valid columns; asserts the columns past C were not written."""
    h = v.float().cpu()
    if v.shape[1] > C:
        assert torch.isnan(h[:, C:]).all(), 'columns past C written'
    return h[:, :C].double().reshape(*shape, C)


def stream():
    return torch.cuda.current_stream().cuda_stream


def check(name, got, ref, tol, extra=0.0):
    """max |got - ref| <= tol * scale (+ a per-element allowance `extra`); prints the measured error beside the bound."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), name + ': non-finite output'
    scale = max(1e-6, ref.abs().max().item())
    err = (got - ref).abs()
    allowed = torch.zeros_like(err) + tol * scale + extra
    worst = (err - allowed).max().item()
    print('[err] %s: max err %.3g = %.3g of scale %.3g (bound %.3g; %.2f of the allowance used)' %
          (name, err.max().item(), err.max().item() / scale, scale, tol, (err / allowed).max().item()))
    if worst > 0:
        i = np.unravel_index(int((err - allowed).argmax()), err.shape)
        raise AssertionError('%s: err %.4g > allowed %.4g (scale %.3g) at %s: got %.7g ref %.7g' %
                             (name, err[i].item(), allowed[i].item(), scale, tuple(int(k) for k in i), got[i].item(), ref[i].item()))


def tol_of(dtype):
    return F32_TOL if dtype == 'fp32' else BF16_TOL


def inputs(g, B, T, C, dtype, const_channels=True):
    """Non-zero channel means (-3..3), spreads 0.2..2; channels 5 and C - 3 constant over T (variance 0)."""
    off = torch.rand(1, 1, C, generator=g) * 6 - 3
    sd = torch.rand(1, 1, C, generator=g) * 1.8 + 0.2
    x = off + sd * torch.randn(B, T, C, generator=g)
    if const_channels:
        x[:, :, 5] = off[0, 0, 5]
        x[:, :, C - 3] = -off[0, 0, C - 3] * 1.7
    return rnd(x, dtype)


def stats64(x):
    """fp64 InstanceNorm statistics over T of [B, T, C]."""
    m = x.mean(1)
    return m, 1.0 / torch.sqrt(((x - m[:, None]) ** 2).mean(1) + EPS)


def check_stats(name, mean, rstd, x):
    m64, r64 = stats64(x)
    amax = x.abs().amax(1)
    dm, dr = (mean - m64).abs(), (rstd - r64).abs() / r64
    print('[err] %s mean: %.3g ulp-units of max|x| (bound %g); rstd: %.3g units (bound %g)' %
          (name, (dm / (U * amax.clamp_min(1e-30))).max().item(), MEAN_K, (dr / (U * (1 + amax * r64))).max().item(), RSTD_K))
    assert (dm <= MEAN_K * U * amax).all(), name + ': mean'
    assert (dr <= RSTD_K * U * (1 + amax * r64)).all(), name + ': rstd'


RES = ['none', 'identity', 'upsample', 'avg_even_reflect', 'avg_odd_reflect', 'avg_even_zero', 'avg_odd_zero']


def res_shape(L, res, T):
    """(mode enum, T_res, pad mode) of a residual, or None where the shape does not allow it."""
    pad = L.ZS_PAD_ZERO if res.endswith('zero') else L.ZS_PAD_REFLECT
    if res == 'none':
        return L.ZS_RES_NONE, T, pad
    if res == 'identity':
        return L.ZS_RES_IDENTITY, T, pad
    if res == 'upsample':
        return (L.ZS_RES_UPSAMPLE2, T // 2, pad) if T % 2 == 0 else None
    Tr = 2 * T if 'even' in res else 2 * T - 1
    return (L.ZS_RES_AVGPOOL2, Tr, pad) if Tr >= 2 else None


def res_ref(res, r):
    """fp64 residual term of r [B, T_res, C] as the forward adds it (model: F.pad(x, (0, T % 2)) + avg_pool1d(2))."""
    if res == 'none':
        return 0.0
    if res == 'identity':
        return r
    if res == 'upsample':
        return r.repeat_interleave(2, dim=1)
    rb = F.pad(r.permute(0, 2, 1), (0, r.shape[1] % 2), mode='constant' if res.endswith('zero') else 'reflect')
    return F.avg_pool1d(rb, 2).permute(0, 2, 1)


def fwd_call(L, dtype, X, out, B, T, C, **kw):
    L.call('zs_instnorm_fwd', 'ZsInstNormFwd', stream(), dtype=_dt(L, dtype), x=X.data_ptr(), ldx=X.shape[1], out=out.data_ptr(),
           ldo=out.shape[1], B=B, T=T, C=C, eps=EPS, **kw)


def _fwd_case(L, dtype, B, T, C, res_modes, seed):
    g = torch.Generator().manual_seed(seed)
    x = inputs(g, B, T, C, dtype)
    xd = x.double()
    m64, r64 = stats64(xd)
    xh = (xd - m64[:, None]) * r64[:, None]
    extra = (CANCEL_K * U * xd.abs().amax(1) * r64)[:, None, :]
    X = dev(x, dtype, C + 8)
    nspk, p = 5, 0.3
    vec2 = torch.randn(nspk, C + 16, generator=g)
    idx = torch.randint(0, nspk, (B,), generator=g)
    vcols = C - 8                                                     # vec2_cols < C: the last 8 channels get no add
    keep = torch.rand(B, T, C, generator=g) >= p
    m8 = keep.to(torch.uint8).reshape(B * T, C).to('cuda:0')
    vec2_d, idx_d = vec2.to('cuda:0'), idx.to('cuda:0')
    residuals = {}
    for res in res_modes:
        rs = res_shape(L, res, T)
        if rs is not None:
            residuals[res] = (rs, rnd(torch.randn(B, rs[1], C, generator=g) * 1.5, dtype))
    tol = tol_of(dtype)
    for vname, kv in variants(L, FWD, dtype, T, C):
        with knobs(L, **kv):
            tag = '%s B%d T%d C%d %s' % (dtype, B, T, C, vname)
            # stats, out2 = out + vec2[idx[b]], no dropout, no residual
            out, out2 = sentinel(B * T, C + 8, dtype), sentinel(B * T, C + 16, dtype)
            mean, rstd = f32(B * C), f32(B * C)
            fwd_call(L, dtype, X, out, B, T, C, out2=out2.data_ptr(), ldo2=out2.shape[1], vec2=vec2_d.data_ptr(), vec2_ld=vec2.shape[1],
                     vec2_cols=vcols, idx=idx_d.data_ptr(), mean=mean.data_ptr(), rstd=rstd.data_ptr(), res_mode=L.ZS_RES_NONE)
            torch.cuda.synchronize()
            check_stats('fwd stats ' + tag, mean[:B * C].double().cpu().view(B, C), rstd[:B * C].double().cpu().view(B, C), xd)
            check('fwd out ' + tag, host(out, (B, T), C), xh, tol, extra)
            e2 = torch.zeros(B, 1, C, dtype=torch.float64)
            e2[:, 0, :vcols] = vec2[idx, :vcols].double()
            check('fwd out2 ' + tag, host(out2, (B, T), C), xh + e2, tol, extra)
            # each residual with mask dropout
            for res, ((mode, Tr, pad), r) in residuals.items():
                R = dev(r, dtype, C + 8)
                out = sentinel(B * T, C + 8, dtype)
                fwd_call(L, dtype, X, out, B, T, C, drop_p=p, mask=m8.data_ptr(), mask_ld=C, res_mode=mode, res=R.data_ptr(),
                         ldres=R.shape[1], T_res=Tr, res_pad_mode=pad)
                torch.cuda.synchronize()
                ref = xh * keep.double() / (1 - p) + res_ref(res, r.double())
                check('fwd %s mask-dropout %s' % (res, tag), host(out, (B, T), C), ref, tol, extra / (1 - p))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', [256, 264, 512, 1024])
@pytest.mark.parametrize('T', T_WIDE + T_NARROW)
def test_instnorm_fwd_vs_fp64(zs, dtype, C, T):
    """Forward at every T around the row-group boundaries (T <= 64 in both decompositions for bf16; C = 264 leaves the second
    256-channel chunk of the wide one a single valid channel group), every residual mode, out2 with vec2_cols < C, the saved
    statistics, mask dropout; inputs with non-zero means and two constant channels.  Columns past C are never written."""
    _fwd_case(zs, dtype, 1 if T % 2 else 3, T, C, RES, T * 1009 + C)


@pytest.mark.parametrize('dtype', ['bf16'])
def test_instnorm_fwd_vs_fp64_full_batch(zs, dtype):
    """The train_ae shape of the widest norms: B = 256, T = 64, C = 1024 in bf16 (wide decomposition by default)."""
    assert decomposition(zs, FWD, dtype, 64, 1024) == 'wide'
    _fwd_case(zs, dtype, 256, 64, 1024, ['identity'], 7)


@pytest.mark.parametrize('res', ['none', 'identity', 'avg_reflect', 'avg_zero'])
def test_instnorm_wide_ragged_batch(zs, res):
    """ZsInstNormFwd.lengths / res_lengths in the wide decomposition (bf16, C = 512, the batched inference of resynth_batch):
    every sample's rows and statistics are bit-identical to the sample launched alone, match fp64 of that sample, and the rows
    past its length are zeros."""
    L = zs
    lens = [64, 1, 17, 32, 33]
    B, Tm, C, dtype = len(lens), max(lens), 512, 'bf16'
    g = torch.Generator().manual_seed(11)
    x = inputs(g, B, Tm, C, dtype)
    if res == 'none':
        mode, rlens, Trm, pad = L.ZS_RES_NONE, lens, Tm, L.ZS_PAD_REFLECT
    elif res == 'identity':
        mode, rlens, Trm, pad = L.ZS_RES_IDENTITY, lens, Tm, L.ZS_PAD_REFLECT
    else:
        mode, Trm = L.ZS_RES_AVGPOOL2, 2 * Tm
        rlens = [max(2, 2 * n - (i + 1) % 2) for i, n in enumerate(lens)]   # odd residual lengths: the pad at the sample's own end
        pad = L.ZS_PAD_REFLECT if res == 'avg_reflect' else L.ZS_PAD_ZERO
    r = rnd(torch.randn(B, Trm, C, generator=g), dtype)
    for n in lens:
        assert decomposition(L, FWD, dtype, n, C) == 'wide'
    X, R = dev(x, dtype, C), dev(r, dtype, C)
    out, mean, rstd = sentinel(B * Tm, C, dtype), f32(B * C), f32(B * C)
    ld_, rl_ = torch.tensor(lens, dtype=torch.int32, device='cuda:0'), torch.tensor(rlens, dtype=torch.int32, device='cuda:0')
    fwd_call(L, dtype, X, out, B, Tm, C, mean=mean.data_ptr(), rstd=rstd.data_ptr(), res_mode=mode, res=R.data_ptr(), ldres=C,
             T_res=Trm, res_pad_mode=pad, lengths=ld_.data_ptr(), res_lengths=rl_.data_ptr() if mode == L.ZS_RES_AVGPOOL2 else None)
    torch.cuda.synchronize()
    got = out.float().cpu().view(B, Tm, C)
    gm, gr = mean[:B * C].cpu().view(B, C), rstd[:B * C].cpu().view(B, C)
    for i, n in enumerate(lens):
        Xi, Ri = dev(x[i:i + 1, :n], dtype, C), dev(r[i:i + 1, :rlens[i]], dtype, C)
        oi, mi, ri = sentinel(n, C, dtype), f32(C), f32(C)
        fwd_call(L, dtype, Xi, oi, 1, n, C, mean=mi.data_ptr(), rstd=ri.data_ptr(), res_mode=mode, res=Ri.data_ptr(), ldres=C,
                 T_res=rlens[i], res_pad_mode=pad)
        torch.cuda.synchronize()
        assert torch.equal(got[i, :n], oi.float().cpu()), 'sample %d (length %d): ragged launch differs from the sample alone' % (i, n)
        assert torch.equal(gm[i], mi[:C].cpu()) and torch.equal(gr[i], ri[:C].cpu()), 'sample %d: statistics' % i
        assert (got[i, n:] == 0).all(), 'sample %d: rows past the length must be zeros' % i
        xi = x[i:i + 1, :n].double()
        m64, r64 = stats64(xi)
        ri_ = res_ref({'none': 'none', 'identity': 'identity', 'avg_reflect': 'avg_odd_reflect', 'avg_zero': 'avg_odd_zero'}[res],
                      r[i:i + 1, :rlens[i]].double())
        ref = (xi - m64[:, None]) * r64[:, None] + ri_
        check('ragged %s sample %d (T %d)' % (res, i, n), got[i:i + 1, :n].double(), ref, BF16_TOL,
              (CANCEL_K * U * xi.abs().amax(1) * r64)[:, None, :])
        check_stats('ragged sample %d' % i, gm[i:i + 1].double(), gr[i:i + 1].double(), xi)


@pytest.mark.parametrize('T', [17, 64])
def test_instnorm_wide_stats_given(zs, T):
    """ZsInstNormFwd.stats_given in the wide decomposition: given the statistics the same call computed, every output bit is the
    same (identity residual, out2, mask dropout)."""
    L, B, C, dtype = zs, 3, 512, 'bf16'
    assert decomposition(L, FWD, dtype, T, C) == 'wide'
    g = torch.Generator().manual_seed(T)
    X = dev(inputs(g, B, T, C, dtype), dtype, C)
    R = dev(rnd(torch.randn(B, T, C, generator=g), dtype), dtype, C)
    vec2, idx = torch.randn(2, C, generator=g).to('cuda:0'), torch.tensor([1, 0, 1], device='cuda:0')
    m8 = (torch.rand(B * T, C, generator=g) >= 0.5).to(torch.uint8).to('cuda:0')
    mean, rstd = f32(B * C), f32(B * C)
    kw = dict(vec2=vec2.data_ptr(), vec2_ld=C, vec2_cols=C, idx=idx.data_ptr(), mean=mean.data_ptr(), rstd=rstd.data_ptr(), drop_p=0.5,
              mask=m8.data_ptr(), mask_ld=C, res_mode=L.ZS_RES_IDENTITY, res=R.data_ptr(), ldres=C, T_res=T)
    o1, o2, p1, p2 = (sentinel(B * T, C, dtype) for _ in range(4))
    fwd_call(L, dtype, X, o1, B, T, C, out2=o2.data_ptr(), ldo2=C, **kw)
    torch.cuda.synchronize()
    m0, r0 = mean.clone(), rstd.clone()
    fwd_call(L, dtype, X, p1, B, T, C, out2=p2.data_ptr(), ldo2=C, stats_given=1, **kw)
    torch.cuda.synchronize()
    assert torch.equal(o1, p1) and torch.equal(o2, p2)
    assert torch.equal(m0[:B * C], mean[:B * C]) and torch.equal(r0[:B * C], rstd[:B * C])         # inputs, not rewritten


# ---- backward ---------------------------------------------------------------------------------------------------------------------
def keep_mask(seed, stream_id, B, T, C, p):
    """Host replica of zs_keep (zs_common.h): the counter-hash keep decision of element (row b*T + t, channel c)."""
    def mix(x):
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x7feb352d)
        x = x ^ (x >> np.uint32(15))
        x = x * np.uint32(0x846ca68b)
        return x ^ (x >> np.uint32(16))
    with np.errstate(over='ignore'):
        idx = np.arange(B * T * C, dtype=np.uint64)
        lo, hi = (idx & np.uint64(0xffffffff)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32)
        s_lo, s_hi, sid = np.uint32(seed & 0xffffffff), np.uint32(seed >> 32), np.uint32(stream_id)
        a = mix(lo ^ s_lo)
        b = mix(hi + s_hi + sid * np.uint32(0x9e3779b9) + a)
        r = mix(a ^ (b * np.uint32(0x85ebca6b)) ^ sid)
    u = (r >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return torch.from_numpy(u >= np.float32(p)).view(B, T, C)


def bwd_ref(x, dout, keep, p):
    """fp64 autograd of dropout(InstanceNorm1d(x)), times lrelu'(x) (x = lrelu(z): the gradient w.r.t. z), and the per-element
    cancellation allowance of the fp32 backward (module docstring)."""
    xv = x.double().clone().requires_grad_(True)
    m = xv.mean(1, keepdim=True)
    y = (xv - m) / torch.sqrt(((xv - m) ** 2).mean(1, keepdim=True) + EPS) * keep.double() / (1 - p)
    y.backward(dout.double())
    dl = torch.where(x > 0, 1.0, SLOPE).double()
    m64, r64 = stats64(x.double())
    xh = (x.double() - m64[:, None]) * r64[:, None]
    g = dout.double() * keep.double() / (1 - p)
    amax_r = (x.double().abs().amax(1) * r64)[:, None]
    extra = BWD_K * U * r64[:, None] * (g.abs() + g.mean(1, keepdim=True).abs() +
                                        xh.abs() * (g * xh).mean(1, keepdim=True).abs() * (1 + amax_r)) * dl
    return xv.grad * dl, extra


def bwd_call(L, dtype, D, X, mean, rstd, dz, B, T, C, **kw):
    L.call('zs_instnorm_bwd', 'ZsInstNormBwd', stream(), dtype=_dt(L, dtype), dout=D.data_ptr(), ldd=D.shape[1], x=X.data_ptr(),
           ldx=X.shape[1], mean=mean.data_ptr(), rstd=rstd.data_ptr(), dz=dz.data_ptr(), ldz=dz.shape[1], B=B, T=T, C=C, slope=SLOPE, **kw)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', [256, 264, 512])
@pytest.mark.parametrize('T', [2, 9, 32, 33, 64, 65, 200])
@pytest.mark.parametrize('drop', ['mask', 'rng'])
def test_instnorm_bwd_vs_fp64(zs, dtype, C, T, drop):
    """Backward in each decomposition the shape can take (norm_lim1 = 64 puts bf16 T <= 64 in the wide one) with the explicit
    mask and with counter-hash dropout (seed, stream_id), against fp64 autograd.  The RNG mask is checked against a host replica
    of the hash through the forward's zeros.  Bound: the output tolerance of the dtype."""
    L = zs
    B, p, seed, sid = 2, 0.4, 1234 + T, 7
    g = torch.Generator().manual_seed(T * 31 + C)
    z = torch.rand(1, 1, C, generator=g) * 2 - 0.5 + torch.randn(B, T, C, generator=g)
    x = rnd(F.leaky_relu(z, SLOPE), dtype)
    dout = rnd(torch.randn(B, T, C, generator=g), dtype)
    if drop == 'mask':
        keep = torch.rand(B, T, C, generator=g) >= p
        m8 = keep.to(torch.uint8).reshape(B * T, C).to('cuda:0')
        dkw = dict(drop_p=p, mask=m8.data_ptr(), mask_ld=C)
    else:
        keep = keep_mask(seed, sid, B, T, C, p)
        dkw = dict(drop_p=p, seed=seed, stream_id=sid)
    X, D = dev(x, dtype, C + 8), dev(dout, dtype, C)
    mean, rstd, out = f32(B * C), f32(B * C), sentinel(B * T, C + 8, dtype)
    fwd_call(L, dtype, X, out, B, T, C, mean=mean.data_ptr(), rstd=rstd.data_ptr(), res_mode=L.ZS_RES_NONE, **dkw)
    torch.cuda.synchronize()
    o = host(out, (B, T), C)
    m64, r64 = stats64(x.double())
    sure = ((x.double() - m64[:, None]) * r64[:, None]).abs() > 1e-2      # elements whose kept output cannot round to zero
    assert (o[~keep] == 0).all() and (o[keep & sure] != 0).all(), 'forward dropout differs from the keep mask'
    ref, extra = bwd_ref(x, dout, keep, p)
    for vname, kv in variants(L, BWD, dtype, T, C):
        with knobs(L, **kv):
            dz = sentinel(B * T, C + 8, dtype)
            bwd_call(L, dtype, D, X, mean, rstd, dz, B, T, C, **dkw)
            torch.cuda.synchronize()
            check('bwd %s %s T%d C%d %s' % (drop, dtype, T, C, vname), host(dz, (B, T), C), ref, tol_of(dtype), extra)


def test_instnorm_fwd_wide_bwd_narrow_same_rng_mask(zs):
    """The encoder's case: bf16, C = 512, T = 64, counter-hash dropout, default limits -- the forward runs the wide decomposition
    and the backward the narrow one.  The keep mask recovered from the forward's zeros is the one the backward applies: its dz
    matches fp64 autograd with that mask."""
    L, dtype = zs, 'bf16'
    B, T, C, p, seed, sid = 4, 64, 512, 0.5, 99, 3
    assert decomposition(L, FWD, dtype, T, C) == 'wide' and decomposition(L, BWD, dtype, T, C) == 'narrow'
    g = torch.Generator().manual_seed(5)
    x = rnd(F.leaky_relu(torch.randn(B, T, C, generator=g) + 0.3, SLOPE), dtype)
    dout = rnd(torch.randn(B, T, C, generator=g), dtype)
    X, D = dev(x, dtype, C), dev(dout, dtype, C)
    mean, rstd, out, dz = f32(B * C), f32(B * C), sentinel(B * T, C, dtype), sentinel(B * T, C, dtype)
    kw = dict(drop_p=p, seed=seed, stream_id=sid)
    fwd_call(L, dtype, X, out, B, T, C, mean=mean.data_ptr(), rstd=rstd.data_ptr(), res_mode=L.ZS_RES_NONE, **kw)
    bwd_call(L, dtype, D, X, mean, rstd, dz, B, T, C, **kw)
    torch.cuda.synchronize()
    keep = host(out, (B, T), C) != 0
    assert abs(keep.double().mean().item() - (1 - p)) < 0.01
    assert torch.equal(keep, keep_mask(seed, sid, B, T, C, p))
    ref, extra = bwd_ref(x, dout, keep, p)
    check('fwd wide -> bwd narrow', host(dz, (B, T), C), ref, BF16_TOL, extra)


# ---- gradient combine -------------------------------------------------------------------------------------------------------------
GC_CFGS = [
    # name, pad_left, pad_right, reflect, residual, dact, unshuffle, emb ('none' | 'acc': += with out | 'only': out = NULL)
    ('p11_identity_dact_emb', 1, 1, True, 'identity', True, False, 'acc'),
    ('p22_avgpool_unshuffle', 2, 2, True, 'avgpool', False, True, 'none'),
    ('p33_upsample_dact_unshuffle_emb', 3, 3, True, 'upsample', True, True, 'acc'),
    ('p32_emb_only', 3, 2, True, 'none', False, False, 'only'),
    ('p22zero_identity_emb', 2, 2, False, 'identity', False, False, 'acc'),
]


def combine_call(L, dtype, GP, B, T, C, pl, pr, pad, out=None, **kw):
    L.call('zs_grad_combine', 'ZsGradCombine', stream(), dtype=_dt(L, dtype), gp=GP.data_ptr(), ldg=GP.shape[1], pad_left=pl,
           pad_right=pr, pad_mode=pad, B=B, T=T, C=C, slope=SLOPE, out=out.data_ptr() if out is not None else None,
           ldo=out.shape[1] if out is not None else 0, **kw)


def combine_ref(gp, T, pl, pr, reflect):
    """fp64 gradient of the padded rows w.r.t. the unpadded ones: autograd through F.pad (reflect or zero)."""
    B, Tp, C = gp.shape
    xv = torch.zeros(B, C, T, dtype=torch.float64, requires_grad=True)
    xp = F.pad(xv, (pl, pr), mode='reflect' if reflect else 'constant')
    (xp * gp.permute(0, 2, 1)).sum().backward()
    return xv.grad.permute(0, 2, 1)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', [256, 264, 512])
@pytest.mark.parametrize('T', [2, 16, 32, 64, 65, 128])
def test_grad_combine_vs_fp64(zs, dtype, C, T):
    """zs_grad_combine, every option (reflect pads (1,1) (2,2) (3,3) (3,2) and zero pads, emb_sum += into a non-zero buffer also
    with out = NULL and emb_cols < C, IDENTITY / AVGPOOL2 / UPSAMPLE2 residual, lrelu' of dact_src, unshuffle), in each
    decomposition the shape can take.  Bounds: the output tolerance of the dtype; emb_sum (fp32) within EMB_K * 2^-24 of
    |emb_sum(0)| + sum_t |v| per (sample, channel)."""
    L = zs
    B = 2
    tol = COMBINE_F32_TOL if dtype == 'fp32' else BF16_TOL
    for name, pl, pr, reflect, res, dact, unshuffle, emb in GC_CFGS:
        if (reflect and max(pl, pr) >= T) or ((res == 'avgpool' or unshuffle) and T % 2):
            continue
        g = torch.Generator().manual_seed(T * 7 + C + pl * 3 + pr)
        Tp = T + pl + pr
        gp = rnd(torch.randn(B, Tp, C, generator=g), dtype)
        GP = dev(gp, dtype, C + 8)
        v = combine_ref(gp.double(), T, pl, pr, reflect)
        ref = v.clone()
        kw = {}
        if res != 'none':
            Tr = {'identity': T, 'avgpool': T // 2, 'upsample': 2 * T}[res]
            r = rnd(torch.randn(B, Tr, C, generator=g), dtype)
            R = dev(r, dtype, C + 8)
            kw.update(res_mode={'identity': L.ZS_RES_IDENTITY, 'avgpool': L.ZS_RES_AVGPOOL2, 'upsample': L.ZS_RES_UPSAMPLE2}[res],
                      res=R.data_ptr(), ldres=R.shape[1])
            rd = r.double()
            if res == 'identity':
                ref = ref + rd
            elif res == 'avgpool':                          # backward of avg_pool1d(2)
                ref = ref + 0.5 * rd.repeat_interleave(2, dim=1)
            else:                                           # backward of nearest x2
                ref = ref + rd[:, 0::2] + rd[:, 1::2]
        Bo, To, Co = (B, T // 2, 2 * C) if unshuffle else (B, T, C)
        ref = ref.reshape(Bo, To, Co)                       # unshuffle: (b, t, c) -> row (b, t/2), column (t & 1) * C + c
        if dact:
            y = rnd(torch.randn(Bo, To, Co, generator=g), dtype)
            Y = dev(y, dtype, Co + 8)
            kw.update(dact_src=Y.data_ptr(), dact_ld=Y.shape[1])
            ref = ref * torch.where(y > 0, 1.0, SLOPE).double()
        emb_ld, emb_cols = C + 8, C - 8
        emb0 = torch.randn(B, emb_ld, generator=g)
        for vname, kv in variants(L, COMBINE, dtype, T, C):
            with knobs(L, **kv):
                tag = '%s %s T%d C%d %s' % (name, dtype, T, C, vname)
                out = None if emb == 'only' else sentinel(Bo * To, Co + 8, dtype)
                ekw = {}
                if emb != 'none':
                    E = emb0.to('cuda:0')
                    ekw = dict(emb_sum=E.data_ptr(), emb_ld=emb_ld, emb_cols=emb_cols)
                combine_call(L, dtype, GP, B, T, C, pl, pr, L.ZS_PAD_REFLECT if reflect else L.ZS_PAD_ZERO, out=out, unshuffle=int(unshuffle),
                             **kw, **ekw)
                torch.cuda.synchronize()
                if out is not None:
                    check('combine ' + tag, host(out, (Bo, To), Co), ref, tol)
                if emb != 'none':
                    e = E.cpu()
                    assert torch.equal(e[:, emb_cols:], emb0[:, emb_cols:]), 'emb_sum columns past emb_cols written'
                    eref = emb0[:, :emb_cols].double() + v.sum(1)[:, :emb_cols]
                    bound = EMB_K * U * (emb0[:, :emb_cols].double().abs() + v.abs().sum(1)[:, :emb_cols])
                    err = (e[:, :emb_cols].double() - eref).abs()
                    print('[err] combine emb_sum %s: %.3g units (bound %g)' % (tag, (err / bound * EMB_K).max().item(), EMB_K))
                    assert (err <= bound).all(), 'emb_sum ' + tag


# ---- one reduction order --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 7, 32, 33, 64])
@pytest.mark.parametrize('C', [264, 1024])
def test_norm_decompositions_bitwise_equal(zs, T, C):
    """The reduction over T has one order in every decomposition (zs_norm.hip, RGN): 32 canonical partials of rows r, r + 32, ...
    summed r = 0..31, each partial over its rows in ascending order.  So the wide and the narrow decomposition give the same bits
    for every output: forward out / out2 / mean / rstd (identity residual, counter-hash dropout), backward dz, and the combine's
    output and emb_sum.  Turning norm_wide off must change no result bit.  The rows and the padded gradient span six decades of
    magnitude: sums of bf16 values of one range are exact in fp32 in any order, so only such data can tell orders apart."""
    L, B, dtype = zs, 3, 'bf16'
    g = torch.Generator().manual_seed(T + C)

    def decades(*shape):
        return rnd(torch.randn(*shape, generator=g) * torch.pow(10.0, torch.rand(*shape, generator=g) * 6 - 3), dtype)
    x = decades(B, T, C) + inputs(g, B, T, C, dtype)
    X = dev(x, dtype, C)
    R = dev(rnd(torch.randn(B, T, C, generator=g), dtype), dtype, C)
    D = dev(rnd(torch.randn(B, T, C, generator=g), dtype), dtype, C)
    vec2, idx = torch.randn(3, C, generator=g).to('cuda:0'), torch.tensor([2, 0, 1], device='cuda:0')
    pl, pr, pad = ((3, 2, L.ZS_PAD_REFLECT) if T > 3 else (1, 1, L.ZS_PAD_REFLECT) if T > 1 else (2, 2, L.ZS_PAD_ZERO))
    GP = dev(decades(B, T + pl + pr, C), dtype, C)
    Y = dev(rnd(torch.randn(B, T, C, generator=g), dtype), dtype, C)
    emb0 = torch.randn(B, C, generator=g).to('cuda:0')
    drop = dict(drop_p=0.5, seed=42, stream_id=5)

    def run():
        out, out2, dz, comb = (sentinel(B * T, C, dtype) for _ in range(4))
        mean, rstd, emb = f32(B * C), f32(B * C), emb0.clone()
        fwd_call(L, dtype, X, out, B, T, C, out2=out2.data_ptr(), ldo2=C, vec2=vec2.data_ptr(), vec2_ld=C, vec2_cols=C, idx=idx.data_ptr(),
                 mean=mean.data_ptr(), rstd=rstd.data_ptr(), res_mode=L.ZS_RES_IDENTITY, res=R.data_ptr(), ldres=C, T_res=T, **drop)
        bwd_call(L, dtype, D, X, mean, rstd, dz, B, T, C, **drop)
        combine_call(L, dtype, GP, B, T, C, pl, pr, pad, out=comb, emb_sum=emb.data_ptr(), emb_ld=C, emb_cols=C,
                     res_mode=L.ZS_RES_IDENTITY, res=R.data_ptr(), ldres=C, dact_src=Y.data_ptr(), dact_ld=C)
        torch.cuda.synchronize()
        return dict(out=out, out2=out2, mean=mean, rstd=rstd, dz=dz, combine=comb, emb_sum=emb)

    got = {}
    for vname, kv in (('wide', WIDE), ('narrow', NARROW)):
        with knobs(L, **kv):
            assert all(decomposition(L, k, dtype, T, C) == vname for k in (FWD, BWD, COMBINE))
            got[vname] = run()
    for k in got['wide']:
        a, b = got['wide'][k], got['narrow'][k]
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                           b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32)), \
            '%s differs between the decompositions (T %d, C %d)' % (k, T, C)


# ---- embedding scatter ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [3, 128, 129, 256, 300])
@pytest.mark.parametrize('accumulate', [0, 1])
def test_emb_scatter_fixed_sample_order(zs, B, accumulate):
    """zs_emb_scatter: demb[r] (+)= sum over the samples b with idx[b] == r, summed left to right in ascending b (several ballot
    rounds of 128 samples for B > 128) -- bit for bit the float32 host sum in that order.  Rows no sample uses are 0 (or keep
    their value when accumulating); columns past C are not written."""
    L = zs
    n_rows, C, emb_ld, demb_ld = 9, 200, 208, 216
    g = torch.Generator().manual_seed(B * 2 + accumulate)
    idx = torch.randint(0, 6, (B,), generator=g)                 # rows 6..8 unused
    idx[:3] = torch.tensor([4, 1, 4])                            # repeated indices
    es = torch.randn(B, emb_ld, generator=g) * torch.pow(10.0, torch.rand(B, 1, generator=g) * 6 - 3)
    demb0 = torch.randn(n_rows, demb_ld, generator=g)
    demb0[:, C:] = 7.0
    E, I, Dm = es.to('cuda:0'), idx.to('cuda:0'), demb0.to('cuda:0')
    L.call('zs_emb_scatter', 'ZsEmbScatter', stream(), emb_sum=E.data_ptr(), emb_ld=emb_ld, idx=I.data_ptr(), B=B, demb=Dm.data_ptr(),
           demb_ld=demb_ld, n_rows=n_rows, C=C, accumulate=accumulate)
    torch.cuda.synchronize()
    e = es[:, :C].numpy()

    def host_sum(order):
        acc = np.zeros((n_rows, C), dtype=np.float32)
        for b in order:
            acc[idx[b]] = acc[idx[b]] + e[b]
        return acc
    acc = host_sum(range(B))
    ref = demb0.numpy().copy()
    ref[:, :C] = (ref[:, :C] + acc) if accumulate else acc
    got = Dm.cpu().numpy()
    assert np.array_equal(got.view(np.int32), ref.view(np.int32)), 'max |d| %g' % np.abs(got - ref).max()
    if B >= 128:                                                  # the data tell the orders apart
        assert not np.array_equal(acc, host_sum(reversed(range(B))))
