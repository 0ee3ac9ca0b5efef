"""The LDS-DMA 128x128 bf16 weight-gradient kernel (gemm_wgrad_dma_kernel) and the Conv1d slab reduce (wgrad_reduce_taps_kernel)
against the kernels they replace (wgrad_dma = 0 / wgrad_reduce_taps = 0: gemm_wgrad_kernel<bf16>, wgrad_reduce_kernel) at equal
split counts, bit for bit, and both against an fp64 reference of dY^T * gather(X)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def zs():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    from zs_amd import _lib, layers
    _lib.lib()
    return _lib, layers


def _rup(x, m):
    return (x + m - 1) // m * m


def _src(s, n, reflect):
    """source index of padded position s along an axis of length n (None: zero padding)"""
    if reflect:
        if s < 0:
            s = -s
        if s >= n:
            s = 2 * (n - 1) - s
        return s
    return s if 0 <= s < n else None


def _gather_1d(x, T_out, j, stride, pad_left, reflect):
    """x [B, T_in, C] -> rows x[b, t*stride + j - pad_left] (zeros where padded) as [B, T_out, C]"""
    B, T_in, C = x.shape
    out = torch.zeros(B, T_out, C, dtype=x.dtype)
    for t in range(T_out):
        s = _src(t * stride + j - pad_left, T_in, reflect)
        if s is not None:
            out[:, t] = x[:, s]
    return out


def _gather_2d(x, H, W, Ho, Wo, kh, kw, stride, pad, reflect):
    B, _, C = x.shape
    xi = x.view(B, H, W, C)
    out = torch.zeros(B, Ho, Wo, C, dtype=x.dtype)
    for ho in range(Ho):
        h = _src(ho * stride + kh - pad, H, reflect)
        if h is None:
            continue
        for wo in range(Wo):
            w = _src(wo * stride + kw - pad, W, reflect)
            if w is not None:
                out[:, ho, wo] = xi[:, h, w]
    return out.view(B, Ho * Wo, C)


class Case(object):
    def __init__(self, B, T_in, T_out, Cout, Cin, taps, stride=1, pad_left=0, reflect=True, linear=False, co_split2=False,
                 geom2=None, seed=0):
        self.__dict__.update(locals())
        del self.__dict__['self']
        g = torch.Generator().manual_seed(seed)
        self.ldy, self.ldx = _rup(Cout, 32), _rup(Cin, 32)
        dy = torch.zeros(B, T_out, self.ldy)
        dy[:, :, :Cout] = torch.randn(B, T_out, Cout, generator=g)
        x = torch.zeros(B, T_in, self.ldx)
        x[:, :, :Cin] = torch.randn(B, T_in, Cin, generator=g)
        self.dy = dy.to(torch.bfloat16)
        self.x = x.to(torch.bfloat16)
        self.W0 = torch.randn(Cout, Cin * taps, generator=g)
        self.b0 = torch.randn(Cout, generator=g)

    def reference(self):
        """fp64 dW [Cout, Cin, taps] and db [Cout] in the caller's channel order"""
        dy = self.dy.double()[:, :, :self.Cout]
        x = self.x.double()[:, :, :self.Cin]
        dW = torch.zeros(self.Cout, self.Cin, self.taps, dtype=torch.float64)
        for j in range(self.taps):
            if self.geom2 is not None:
                H, W, Ho, Wo, taps_h = self.geom2
                xg = _gather_2d(x, H, W, Ho, Wo, j % taps_h, j // taps_h, self.stride, self.pad_left, self.reflect)
            else:
                xg = _gather_1d(x, self.T_out, j, self.stride, self.pad_left, self.reflect)
            dW[:, :, j] = torch.einsum('bto,btc->oc', dy, xg)
        db = dy.sum(dim=(0, 1))
        if self.co_split2:          # kernel channel n = packed position; caller channel co(n): n < C/2 -> 2n, else 2(n - C/2) + 1
            half = self.Cout // 2
            perm = [(co & 1) * half + (co >> 1) for co in range(self.Cout)]
            dW, db = dW[perm], db[perm]
        return dW, db

    def run(self, L, layers, ctx, splits, bias=True, accumulate=False):
        dev = ctx.device
        dY, X = self.dy.to(dev), self.x.to(dev)
        dW = (self.W0.clone() if accumulate else torch.zeros(self.Cout, self.Cin * self.taps)).to(dev)
        db = (self.b0.clone() if accumulate else torch.zeros(self.Cout)).to(dev)
        if self.linear:
            so, si, sj = self.Cin, 1, 0
        else:
            so, si, sj = self.Cin * self.taps, self.taps, 1
        kw = dict(dtype=ctx.dt, dY=dY.data_ptr(), ldy=self.ldy, y_cols=_rup(self.Cout, 8), X=X.data_ptr(), ldx=self.ldx,
                  x_batch_stride=self.T_in * self.ldx, x_cols=_rup(self.Cin, 8), B=self.B, T_in=self.T_in, T_out=self.T_out,
                  taps=self.taps, stride=self.stride, pad_left=self.pad_left, pad_mode=L.ZS_PAD_REFLECT if self.reflect else L.ZS_PAD_ZERO,
                  Cout=self.Cout, Cin=self.Cin, dW=dW.data_ptr(), so=so, si=si, sj=sj, db=(db.data_ptr() if bias else None),
                  co_split2=int(self.co_split2), accumulate=int(accumulate), splits=splits)
        if self.geom2 is not None:
            H, W, Ho, Wo, taps_h = self.geom2
            kw.update(w_in=W, w_out=Wo, taps_h=taps_h)
        layers.wgrad_call(ctx, kw)
        torch.cuda.synchronize()
        return dW.cpu().view(self.Cout, self.Cin, self.taps), db.cpu()


def _with(L, opts, fn):
    old = {k: L.set_option(k, v) for k, v in opts.items()}
    try:
        return fn()
    finally:
        for k, v in old.items():
            L.set_option(k, v)


def _check_ref(name, case, got_w, got_b, bias, accumulate):
    rw, rb = case.reference()
    if accumulate:
        rw = rw + case.W0.double().view(case.Cout, case.Cin, case.taps)
        rb = rb + case.b0.double()
    sw = max(float(rw.abs().max()), 1.0)
    ew = float((got_w.double() - rw).abs().max())
    assert ew <= 2e-5 * sw, '%s dW: max|d| %.3g (scale %.3g)' % (name, ew, sw)
    if bias:
        sb = max(float(rb.abs().max()), 1.0)
        eb = float((got_b.double() - rb).abs().max())
        assert eb <= 2e-5 * sb, '%s db: max|d| %.3g (scale %.3g)' % (name, eb, sb)


CASES = {
    # the encoder's conv bank: C_in 513 -> 128, k = 1..7, reflect padding (k//2, k//2 - 1 + k%2)
    **{'bank_k%d' % k: dict(B=8, T_in=128, T_out=128, Cout=128, Cin=513, taps=k, pad_left=k // 2) for k in range(1, 8)},
    't16_layer': dict(B=64, T_in=16, T_out=16, Cout=384, Cin=256, taps=3, pad_left=1),
    'stride2': dict(B=16, T_in=64, T_out=32, Cout=256, Cin=192, taps=3, stride=2, pad_left=1),
    'gru_3HxH_split2_shift': dict(B=8, T_in=40, T_out=40, Cout=384, Cin=128, taps=1, pad_left=1, reflect=False, linear=True, co_split2=True),
    'conv2d_3x3': dict(B=4, T_in=64, T_out=64, Cout=128, Cin=64, taps=9, pad_left=1, geom2=(8, 8, 8, 8, 3)),
}


@pytest.mark.parametrize('name', sorted(CASES))
@pytest.mark.parametrize('bias,accumulate', [(True, False), (False, False), (True, True)])
def test_wgrad_dma_bitwise_vs_register_staged(zs, name, bias, accumulate):
    L, layers = zs
    case = Case(seed=sum(map(ord, name)), **CASES[name])
    ctx = layers.Ctx('cuda:0', 'bf16')
    M = case.B * case.T_out
    for splits in sorted({1, 3, max(1, M // 416)}):      # 416 rows = 13 chunks of 32: a split that ends half-way through a 64-row stage
        base = {'wgrad_p8': 0, 'wgrad_reduce_taps': 0}
        new_w, new_b = _with(L, dict(base, wgrad_dma=1), lambda: case.run(L, layers, ctx, splits, bias, accumulate))
        old_w, old_b = _with(L, dict(base, wgrad_dma=0), lambda: case.run(L, layers, ctx, splits, bias, accumulate))
        assert torch.equal(new_w, old_w), '%s splits %d: dW differs from gemm_wgrad_kernel' % (name, splits)
        if bias:
            assert torch.equal(new_b, old_b), '%s splits %d: db differs from gemm_wgrad_kernel' % (name, splits)
        _check_ref('%s splits %d' % (name, splits), case, new_w, new_b, bias, accumulate)


@pytest.mark.parametrize('name', ['bank_k3', 'bank_k7', 'conv2d_3x3', 'gru_3HxH_split2_shift', 'stride2'])
@pytest.mark.parametrize('accumulate', [False, True])
def test_wgrad_reduce_taps_bitwise(zs, name, accumulate):
    """The same slabs reduced by wgrad_reduce_taps_kernel and by wgrad_reduce_kernel (linear weights take the latter either way)."""
    L, layers = zs
    case = Case(seed=7, **CASES[name])
    ctx = layers.Ctx('cuda:0', 'bf16')
    for splits in (1, 5, 19):
        new_w, new_b = _with(L, {'wgrad_reduce_taps': 1}, lambda: case.run(L, layers, ctx, splits, True, accumulate))
        old_w, old_b = _with(L, {'wgrad_reduce_taps': 0}, lambda: case.run(L, layers, ctx, splits, True, accumulate))
        assert torch.equal(new_w, old_w) and torch.equal(new_b, old_b), '%s splits %d' % (name, splits)
        _check_ref('%s splits %d' % (name, splits), case, new_w, new_b, True, accumulate)


def test_wgrad_default_plan_matches_reference(zs):
    """Default dispatch (split-K plan for a launch alone and for launches side by side) on a bank layer at the bench's batch."""
    L, layers = zs
    case = Case(B=64, T_in=128, T_out=128, Cout=128, Cin=513, taps=5, pad_left=2, seed=3)
    ctx = layers.Ctx('cuda:0', 'bf16')
    for alone in (0, 1):
        w, b = _with(L, {'wgrad_alone': alone}, lambda: case.run(L, layers, ctx, 0))
        _check_ref('alone %d' % alone, case, w, b, True, False)
