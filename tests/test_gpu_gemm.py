"""zs_gemm_conv (csrc/zs_gemm.hip) against fp64, element by element, on every kernel its dispatch can choose: P8 (256x256 quadrant
ping-pong, with the register epilogue and with the fp32 staging epilogue), RING_PP / RING (256x128 3-stage ring), DMA64 / DMA128
(LDS-DMA, 64- and 128-row tiles) and REG (register-staged), fp32 and bf16, gather 0 (forward) and 1 (data gradient).
zs_gemm_conv_path reports the kernel of a launch from the launch's own plan function; every case asserts it on the struct it
launches, and test_cases_reach_every_path asserts that the cases reach every (path, register epilogue, dtype, gather).

The test lays every operand out itself (no zs_pack_weight, no ConvLayer, except the stride-2 / column-window data gradients, which
are layer logic): activations [B*T_in][lda] with zero pad columns and 512 elements of zeroed slack, the weight as
Wt[n][j*cin_pad + ci] zero padded to n_pad rows and ldw columns.  Outputs (out, out2, colsum) are prefilled with NaN inside guard
rows of NaN; after the launch columns [N, out_cols) must be zeros and everything the launch does not own must still be NaN.

Reference: the source row of every (output row, tap) is computed with the gather rule of zs_amd.h written out in NumPy index
arithmetic (reflect / zero, stride, per-sample lengths, 2-D images, transposed-conv validity); the rows are gathered from the values
the kernel reads (bf16-rounded for bf16) and multiplied in fp64, once for the value and once with absolute values for
S = sum|terms|.  Every element of every case is compared; nothing is sampled.

Bound per element (U = 2^-24, K = taps * cin_pad; each check prints its worst error as a fraction of the bound):
  * accumulation: C_ACC(K) U S.  bf16: C_ACC(K) = K / 16 + 8 (tests/test_gpu_gru.py: the same MFMA shapes; an element is a chain of
    K / 16 MFMA accumulations).  fp32: K / 2 + 8.  With K / 16 + 8 the fp32 cases failed on ALL six kernels with bit-identical
    outputs, one element each in 7 cases, at 1.02 .. 1.20 of that bound (K = 96 .. 320), always an output near 2^9 dominated by one
    product (both factors from the 2^6 end of the magnitude spread) that enters early: every later accumulation then rounds at the
    magnitude of S, and v_mfma_f32_32x32x2_f32 makes a chain of K / 2 of them per element (16x16x4: K / 4), eight times the bf16
    chain.  K / 2 roundings of at most U S each is that chain's worst case; it stays below the textbook (K - 1) U S;
  * each fp32 epilogue operation (bias, pre_vec, activation, mask, add, vec2): C_E = 8 U of the magnitudes involved;
  * a bf16 store: 2^-8 |value|.  The P8 register epilogue stages the tile as bf16 BEFORE the dact_src mask / add_src, so there the
    bound has two roundings, 2^-8 |staged| |mask| + 2^-8 |result|; the regs bit of zs_gemm_conv_path says which applies;
    out_f32 outputs have no bf16 term;
  * colsum: the sum over T_out of the per-term bounds (terms are the staged bf16 values on the register-epilogue path) plus
    (T_out + 2) U sum|terms| for the fp32 sum and the accumulation into the previous content.

Measured worst fractions of the bound on an MI355X (every family, all elements), bf16 / fp32:
  P8 1.00 / 0.35, RING_PP 1.00 / 0.39, RING 1.00 / 0.39, DMA64 1.00 / 0.39, DMA128 1.00 / 0.39, REG 1.00 / 0.39; the production
  shapes under the default knobs (bf16): DMA128 0.99, RING_PP 1.00, P8 0.99, DMA64 0.98.
The bf16 fractions are the output rounding itself (2^-8 of the value is reached just above a power of two); the five
non-P8 kernels give bit-identical fp32 results (the same K order), the P8 kernel's 16x16x4 chain differs in the last bits.

Value-only single-line mutations of zs_gemm.hip / zs_common.h (scratch builds, never committed), the new tests that fail on each,
and what the suite before this file (test_gpu_kernels.py, test_gpu_configs.py) did with them:
  1 bias skipped for the second 128 columns of a P8 tile on the fp32-staging path: test_k_loop (odd nk: bias), test_epilogue
    [bias_second_half, prevec_t24, split2_both_vec2_t24, split2_half_not_8, out_f32] on P8 in both dtypes.  Before: caught in
    fp32 only; no bf16 case reached the staging epilogue with a bias past column 128.
  2 zs_reflect off by one row when t * stride + j - pad_left == T_in: 375 cases of every family with reflect padding.  Before: caught.
  3 n0 = (in_g / GM) * PBN in the P8 tile order: 40 P8 cases (test_tile_grid: 14, NaN left in tiles never computed).
    Before: caught by 4 cases.
  4 lseg of loader piece 3 from r instead of r >> 1: 158 P8 cases.  Before: caught.
  5 len_out without pad_right in conv_row_setup: all 48 test_ragged cases with pad_right > 0.  Before: caught.
  6 dlrelu_f with y >= 0: 84 test_epilogue cases (every dact_src case on every path; the cases put exact zeros into dact_src)
    and the production data gradient.  Before: invisible (no test had a zero in dact_src).
  7 epilogue_finish takes the sample of pre_vec / vec2 from the tile's first row: 80 test_epilogue cases on every path.
    Before: caught.
  8 bsel from m0 / T_out in the P8 register epilogue: test_epilogue[prevec_t16, out2_rows_vec2_t16, split2_both_vec2_t16,
    rows_out2_split] on P8 / bf16 and the production SPLIT2 + out2 launch.  Before: caught by one case.
No kernel bug was found.
"""
import contextlib
import ctypes
import math
import time
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF = 2.0 ** -8
C_E = 8.0
PATHS = ('P8', 'RING_PP', 'RING', 'DMA64', 'DMA128', 'REG')
DTYPES = ('fp32', 'bf16')
SLACK = 512
GUARD = 3
FORCE = {
    'P8': dict(gemm_dma=1, gemm_p8=1, gemm_p8_min_tiles=0),
    'RING_PP': dict(gemm_dma=1, gemm_p8=0, gemm_ring=1, gemm_ring_min_tiles=0, gemm_pp=1),
    'RING': dict(gemm_dma=1, gemm_p8=0, gemm_ring=1, gemm_ring_min_tiles=0, gemm_pp=0),
    'DMA64': dict(gemm_dma=1, gemm_p8=0, gemm_ring=0, gemm_dma64=1, gemm_dma64_max_tiles=1 << 30),
    'DMA128': dict(gemm_dma=1, gemm_p8=0, gemm_ring=0, gemm_dma64=0),
    'REG': dict(gemm_dma=0),
}
STATS = {}          # (family, path, dtype) -> worst fraction of the bound


def c_acc(K, dtype):
    """Accumulation constant: K / 16 + 8 for bf16 (a chain of K / 16 MFMA accumulations), K / 2 + 8 for fp32 (K / 2: see the module
    docstring); both below the textbook K - 1 for every K these kernels admit (K is a multiple of 64 in bf16, of 32 in fp32)."""
    return (K / 2.0 if dtype == 'fp32' else K / 16.0) + 8.0


def rup(x, m):
    return (x + m - 1) // m * m


@pytest.fixture(scope='module')
def zs():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    from zs_amd import _lib, layers
    _lib.lib()
    t0 = time.time()
    yield _lib, layers
    print('\n[gemm] wall time of this module %.1f s; worst fraction of the bound per (family, path, dtype):' % (time.time() - t0))
    for k in sorted(STATS):
        print('[gemm]   %-12s %-8s %-5s %.3f' % (k + (STATS[k],)))
    worst = {}
    for (fam, path, dt), v in STATS.items():
        worst[(path, dt)] = max(worst.get((path, dt), 0.0), v)
    print('[gemm] per path: ' + '  '.join('%s/%s %.2f' % (p, d, worst[(p, d)]) for p, d in sorted(worst)))


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


# ------------------------------------------------------------------------------------------------------------------------------
# a case


class Spec(object):
    """One launch.  Geometry: B samples of T rows (2-D: img = (h_in, w_in, taps_h, taps_w), T = h_in * w_in), C real input
    channels, k taps, stride, padding (pl, pr; default the pad_layer() rule k // 2, k - 1 - k // 2), mode 'reflect' / 'zero',
    gather; chunks: K chunks per tap (default: what C needs); N outputs.  Epilogue: see the keyword names."""

    DEFAULTS = dict(B=2, T=16, C=40, N=48, k=1, stride=1, pl=None, pr=None, mode='reflect', gather=0, chunks=None, ldw_extra=0,
                    lda='pad', img=None, lengths=None, bias=False, pre_vec=False, act=False, out='rows', out_cols='r32', out_f32=False,
                    out2=None, vec2=False, dact=False, add=None, colsum=None, unaligned=False, regs=None)

    def __init__(self, name, **kw):
        self.name = name
        bad = set(kw) - set(self.DEFAULTS)
        assert not bad, bad
        self.__dict__.update(self.DEFAULTS)
        self.__dict__.update(kw)
        if self.pl is None:
            self.pl = 0 if self.gather else self.k // 2
        if self.pr is None:
            self.pr = 0 if self.gather else self.k - 1 - self.k // 2

    def __repr__(self):
        return self.name


def geometry(sp, dtype, path):
    """All integer fields of the ZsGemmConv of a case, and the sizes of its buffers."""
    es = 4 if dtype == 'fp32' else 2
    kc = 128 // es
    g = dict(es=es, kc=kc)
    cin_pad = rup(sp.C, kc) if sp.chunks is None else sp.chunks * kc
    C = sp.C if sp.chunks is None else sp.chunks * kc - 5
    g.update(C=C, cin_pad=cin_pad)
    if sp.img is not None:
        h_in, w_in, th, tw = sp.img
        taps = th * tw
        if sp.gather:
            h_out, w_out = (h_in - 1) * sp.stride + th, (w_in - 1) * sp.stride + tw
        else:
            h_out = (h_in + sp.pl + sp.pr - th) // sp.stride + 1
            w_out = (w_in + sp.pl + sp.pr - tw) // sp.stride + 1
        T_in, T_out = h_in * w_in, h_out * w_out
        g.update(w_in=w_in, w_out=w_out, taps_h=th, h_in=h_in, h_out=h_out)
    else:
        taps, T_in = sp.k, sp.T
        T_out = (T_in - 1) * sp.stride + taps if sp.gather else (T_in + sp.pl + sp.pr - taps) // sp.stride + 1
        g.update(w_in=0, w_out=0, taps_h=0)
    lda = cin_pad if sp.lda == 'pad' else rup(C, 32)
    n_pad = rup(sp.N, 256 if path == 'P8' else 128)
    M = sp.B * T_out
    split = sp.out == 'split'
    half = sp.N // 2
    if split:
        out_cols = half
    elif sp.out_cols == 'r32':
        out_cols = rup(sp.N, 32)
    elif sp.out_cols == 'r8':
        out_cols = rup(sp.N, 8) + (8 if rup(sp.N, 8) % 32 == 0 else 0)
    else:
        out_cols = sp.N
    ldc = rup(out_cols, 8) + 8 + (4 if sp.unaligned else 0)
    g.update(taps=taps, T_in=T_in, T_out=T_out, lda=lda, abs=T_in * lda, n_pad=n_pad, ldw=taps * cin_pad + sp.ldw_extra,
             M=M, K=taps * cin_pad, split=split, half=half, out_cols=out_cols, ldc=ldc, rows=2 * M if split else M)
    if sp.out2 is not None:
        s2 = sp.out2 == 'split'
        o2c = half if s2 else rup(sp.N, 8)
        g.update(split2=s2, out2_cols=o2c, ldc2=rup(o2c, 8) + 16, rows2=2 * M if s2 else M)
    return g


def struct_kw(L, sp, dtype, g, ptr):
    """Keyword arguments of the ZsGemmConv; ptr(name) is the address of an operand."""
    kw = dict(dtype=L.ZS_F32 if dtype == 'fp32' else L.ZS_BF16, A=ptr('A'), lda=g['lda'], a_batch_stride=g['abs'], B=sp.B,
              T_in=g['T_in'], T_out=g['T_out'], taps=g['taps'], stride=sp.stride, pad_left=sp.pl,
              pad_mode=L.ZS_PAD_REFLECT if sp.mode == 'reflect' else L.ZS_PAD_ZERO, gather=sp.gather, cin_pad=g['cin_pad'],
              W=ptr('W'), ldw=g['ldw'], N=sp.N, n_pad=g['n_pad'], act=L.ZS_ACT_LRELU if sp.act else L.ZS_ACT_NONE, slope=0.01 if sp.act or sp.dact else 0.0,
              out=ptr('out'), ldc=g['ldc'], out_f32=int(sp.out_f32), out_cols=g['out_cols'],
              store_mode=L.ZS_STORE_SPLIT2 if g['split'] else L.ZS_STORE_ROWS, groups=1, w_in=g['w_in'], w_out=g['w_out'], taps_h=g['taps_h'])
    if sp.bias:
        kw.update(bias=ptr('bias'))
    if sp.pre_vec:
        kw.update(pre_vec=ptr('pre_vec'), pre_vec_ld=sp.N + 3, vec_idx=ptr('vec_idx'))
    if sp.out2 is not None:
        kw.update(out2=ptr('out2'), ldc2=g['ldc2'], out2_cols=g['out2_cols'], store_mode2=L.ZS_STORE_SPLIT2 if g['split2'] else L.ZS_STORE_ROWS)
        if sp.vec2:
            kw.update(vec2=ptr('vec2'), vec2_ld=sp.N + 5, vec_idx=ptr('vec_idx'))
    if sp.dact:
        kw.update(dact_src=ptr('dact'), dact_ld=rup(sp.N, 8) + 8)
    if sp.add is not None:
        kw.update(add_src=ptr('add'), add_ld=rup(sp.N, 8) + 16, add_f32=int(sp.add == 'f32'))
    if sp.colsum is not None:
        kw.update(colsum=ptr('colsum'), colsum_ld=sp.N - sp.colsum[0] + 5, colsum_col0=sp.colsum[0], colsum_post=int(sp.colsum[1]))
    if sp.lengths is not None:
        kw.update(lengths=ptr('lengths'), pad_right=sp.pr)
    return kw


def query(L, kw):
    s = L.STRUCTS['ZsGemmConv'](**{k: v for k, v in kw.items() if v is not None})
    rc = L.lib().zs_gemm_conv_path(ctypes.addressof(s))
    assert rc >= 0, L.last_error()
    return PATHS[rc & 255], rc >> 8


DUMMY = {n: 0x100000 * (i + 1) for i, n in enumerate(('A', 'W', 'out', 'out2', 'bias', 'pre_vec', 'vec_idx', 'vec2', 'dact', 'add',
                                                      'colsum', 'lengths'))}


def planned(L, sp, dtype, path):
    """(path, regs) the plan gives this case under the knobs that force `path`, from dummy operand addresses with the alignment the
    real ones have."""
    g = geometry(sp, dtype, path)
    off = g['es'] * GUARD * g['ldc'] if sp.unaligned else 0

    def ptr(n):
        return DUMMY[n] + (off if n == 'out' else 0)
    with knobs(L, **FORCE[path]):
        return query(L, struct_kw(L, sp, dtype, g, ptr))


# ------------------------------------------------------------------------------------------------------------------------------
# the gather rule of zs_amd.h in index arithmetic


def axis_rows(gather, reflect, stride, pad_left, T_in, t, j):
    """Source position along one axis for output positions t [P] and taps j [J] -> (pos [P, J], ok [P, J]).  T_in: scalar or [P]."""
    t = t[:, None].astype(np.int64)
    j = j[None, :].astype(np.int64)
    T = np.asarray(T_in, dtype=np.int64)
    T = T[:, None] if T.ndim else T
    if gather == 0:
        s = t * stride + j - pad_left
        if reflect:
            s = np.where(s < 0, -s, s)
            s = np.where(s >= T, 2 * (T - 1) - s, s)
        ok = (s >= 0) & (s < T)
        return np.where(ok, s, 0), ok
    s = t - j
    q = np.floor_divide(s, stride)
    ok = (s >= 0) & (q * stride == s) & (q < T)
    return np.where(ok, q, 0), ok


def source_rows(sp, g, lengths=None):
    """[M, taps] offsets (elements) of the A rows each output row reads, and [M, taps] validity."""
    B, T_out, taps = sp.B, g['T_out'], g['taps']
    reflect = sp.mode == 'reflect'
    b = np.repeat(np.arange(B), T_out)
    t = np.tile(np.arange(T_out), B)
    j = np.arange(taps)
    if sp.img is not None:
        ho, wo = t // g['w_out'], t % g['w_out']
        kw_, kh = j // g['taps_h'], j % g['taps_h']
        h, okh = axis_rows(sp.gather, reflect, sp.stride, sp.pl, g['h_in'], ho, kh)
        w, okw = axis_rows(sp.gather, reflect, sp.stride, sp.pl, g['w_in'], wo, kw_)
        row, ok = h * g['w_in'] + w, okh & okw
    else:
        T = g['T_in']
        if lengths is not None:
            ln = np.asarray(lengths, dtype=np.int64)[b]
            len_out = (ln + sp.pl + sp.pr - taps) // sp.stride + 1
            row, ok = axis_rows(sp.gather, reflect, sp.stride, sp.pl, ln, t, j)
            ok = ok & (t < len_out)[:, None]
        else:
            row, ok = axis_rows(sp.gather, reflect, sp.stride, sp.pl, T, t, j)
    return b[:, None] * g['abs'] + row * g['lda'], ok, b


# ------------------------------------------------------------------------------------------------------------------------------
# data, launch, reference


def spread(shape, gen, scale=1.0):
    """Normal values, a quarter of them scaled by 2^e, e uniform in [-6, 6]: small and large outputs exist."""
    x = torch.randn(shape, generator=gen, dtype=torch.float32) * scale
    e = torch.randint(-6, 7, shape, generator=gen).float()
    pick = torch.rand(shape, generator=gen) < 0.25
    return torch.where(pick, x * torch.exp2(e), x)


def rnd(x, dtype):
    return x if dtype == 'fp32' else x.to(torch.bfloat16).float()


class Data(object):
    """Host operands of a case (fp32 tensors holding exactly the values the kernel reads)."""

    def __init__(self, sp, dtype, g):
        gen = torch.Generator().manual_seed(zlib.crc32(('%s/%s' % (sp.name, dtype)).encode()))
        B, N, C, M = sp.B, sp.N, g['C'], g['M']
        nrows = B * g['abs'] // g['lda']
        A = torch.zeros(nrows, g['lda'])
        A[:, :C] = rnd(spread((nrows, C), gen), dtype)
        self.A = torch.cat([A.reshape(-1), torch.zeros(SLACK)])
        w = rnd(spread((N, g['taps'], C), gen, 1.0 / math.sqrt(C * g['taps'])), dtype)
        W = torch.zeros(g['n_pad'], g['ldw'])
        for j in range(g['taps']):
            W[:N, j * g['cin_pad']:j * g['cin_pad'] + C] = w[:, j]
        self.W = W
        self.nspk = 5
        self.bias = spread((N,), gen) if sp.bias else None
        self.pre_vec = spread((self.nspk, N + 3), gen) if sp.pre_vec else None
        self.vec2 = spread((self.nspk, N + 5), gen) if sp.vec2 else None
        self.vec_idx = torch.randint(0, self.nspk, (B,), generator=gen)
        self.dact = self.add = self.colsum0 = None
        if sp.dact:
            d = rnd(spread((M, rup(N, 8) + 8), gen), dtype)
            d[torch.rand(d.shape, generator=gen) < 0.125] = 0.0           # exact zeros: lrelu' takes the slope there
            self.dact = d
        if sp.add is not None:
            self.add = rnd(spread((M, rup(N, 8) + 16), gen), 'fp32' if sp.add == 'f32' else dtype)
        if sp.colsum is not None:
            c0 = torch.full((GUARD + B + GUARD, N - sp.colsum[0] + 5), float('nan'))
            c0[GUARD:GUARD + B, :N - sp.colsum[0]] = spread((B, N - sp.colsum[0]), gen) if sp.colsum[2] else 0.0
            self.colsum0 = c0


def to_dev(x, dtype, slack=True):
    t = x.reshape(-1)
    if slack:
        t = torch.cat([t, torch.zeros(SLACK)])
    return t.to('cuda', torch.float32 if dtype == 'fp32' else torch.bfloat16)


class Device(object):
    """Device copies of a case's inputs (shared by the launches of the case)."""

    def __init__(self, sp, dtype, d):
        self.t = dict(A=to_dev(d.A, dtype, False), W=to_dev(d.W, dtype))
        for n in ('bias', 'pre_vec', 'vec2'):
            if getattr(d, n) is not None:
                self.t[n] = to_dev(getattr(d, n), 'fp32')
        self.t['vec_idx'] = d.vec_idx.to('cuda', torch.int64)
        if d.dact is not None:
            self.t['dact'] = to_dev(d.dact, dtype)
        if d.add is not None:
            self.t['add'] = to_dev(d.add, 'fp32' if sp.add == 'f32' else dtype)
        if sp.lengths is not None:
            self.t['lengths'] = torch.tensor(sp.lengths, dtype=torch.int32, device='cuda')


def launch(L, sp, dtype, g, d, dev, path, sub=None, force=None):
    """One launch into fresh NaN-filled outputs.  sub = (b, len): the batch-1 launch of sample b of a ragged case.
    force: the knobs to launch under instead of FORCE[path].  Returns ((path, regs), {name: whole host buffer, guards included})."""
    tdt = torch.float32 if dtype == 'fp32' else torch.bfloat16
    M, rows = g['M'], g['rows']
    if sub is not None:
        b, ln = sub
        t_out = (ln + sp.pl + sp.pr - g['taps']) // sp.stride + 1
        M = t_out
        rows = 2 * M if g['split'] else M
    bufs = dict(out=torch.full((GUARD + rows + GUARD, g['ldc']), float('nan'), dtype=torch.float32 if sp.out_f32 else tdt, device='cuda'))
    if sp.out2 is not None:
        bufs['out2'] = torch.full((GUARD + (2 * M if g['split2'] else M) + GUARD, g['ldc2']), float('nan'), dtype=tdt, device='cuda')
    if sp.colsum is not None:
        bufs['colsum'] = d.colsum0.to('cuda')
    off = dict(out=GUARD * g['ldc'], out2=GUARD * g.get('ldc2', 0), colsum=GUARD * (sp.N - sp.colsum[0] + 5) if sp.colsum else 0)

    def ptr(n):
        if n in bufs:
            return L.ptr(bufs[n], off[n])
        return L.ptr(dev.t[n])
    kw = struct_kw(L, sp, dtype, g, ptr)
    if sub is not None:
        kw.update(B=1, T_in=ln, T_out=t_out, A=L.ptr(dev.t['A'], b * g['abs']), lengths=None, pad_right=0, vec_idx=L.ptr(dev.t['vec_idx'], b))
    assert kw['out_cols'] <= kw['ldc'] and kw['n_pad'] % 128 == 0 and kw['ldw'] >= g['K']           # bounds of what the launch may touch
    with knobs(L, **(force if force is not None else FORCE.get(path, {}))):
        s = L.call('zs_gemm_conv', 'ZsGemmConv', torch.cuda.current_stream().cuda_stream, **kw)
        plan = query(L, {f: getattr(s, f) for f, _ in s._fields_})
    torch.cuda.synchronize()
    return plan, {n: t.float().cpu() for n, t in bufs.items()}


def reference(sp, dtype, g, d, regs):
    """{name: (ref, bound)} in fp64 for out [rows, cols], out2 and colsum [B, N - col0]."""
    N, M, cp, K = sp.N, g['M'], g['cin_pad'], g['K']
    offs, ok, b = source_rows(sp, g, sp.lengths)
    A = d.A.double()
    Wn = d.W[:N].double()
    ar = torch.arange(cp)
    acc = torch.zeros(M, N, dtype=torch.float64)
    S = torch.zeros(M, N, dtype=torch.float64)
    for j in range(g['taps']):
        idx = torch.from_numpy(offs[:, j])[:, None] + ar[None, :]
        Ag = A[idx] * torch.from_numpy(ok[:, j])[:, None]
        Wj = Wn[:, j * cp:(j + 1) * cp]
        acc += Ag @ Wj.T
        S += Ag.abs() @ Wj.abs().T
    bf_out = dtype == 'bf16' and not sp.out_f32
    bi = torch.from_numpy(b)
    spk = d.vec_idx[bi]
    v, mag = acc, S
    if sp.bias:
        v = v + d.bias.double()[None, :]
        mag = mag + d.bias.double().abs()[None, :]
    if sp.pre_vec:
        pv = d.pre_vec.double()[spk][:, :N]
        v, mag = v + pv, mag + pv.abs()
    e = c_acc(K, dtype) * U * S
    if sp.bias or sp.pre_vec or sp.act:
        e = e + C_E * U * mag
    if sp.act:
        v = torch.where(v > 0, v, 0.01 * v)
    second = sp.dact or sp.add is not None
    res = {}
    e_pre = e + (BF * (v.abs() + e) if regs else 0.0)          # the staged bf16 tile of the register epilogue
    if second:
        mask = torch.where(d.dact.double()[:, :N] > 0, 1.0, 0.01) if sp.dact else torch.ones_like(v)
        add = d.add.double()[:, :N] if sp.add is not None else torch.zeros_like(v)
        r = v * mask + add
        e_r = (e_pre if regs else e) * mask.abs() + C_E * U * ((v * mask).abs() + add.abs())
    else:
        r, e_r = v, e
    e_out = (e_pre if regs and not second else e_r + (BF * (r.abs() + e_r) if bf_out else 0.0))
    if g['split']:
        res['out'] = (unshuffle(r, g['half']), unshuffle(e_out, g['half']))
    else:
        res['out'] = (r, e_out)
    if sp.out2 is not None:
        if g['split2']:
            r2, e2 = unshuffle(r, g['half']), unshuffle(e_r, g['half'])
            sp2 = spk.repeat_interleave(2)
        else:
            r2, e2, sp2 = r, e_r, spk
        if sp.vec2:
            v2 = d.vec2.double()[sp2][:, :r2.shape[1]]
            e2 = e2 + C_E * U * (r2.abs() + v2.abs())
            r2 = r2 + v2
        res['out2'] = (r2, e2 + (BF * (r2.abs() + e2) if dtype == 'bf16' else 0.0))
    if sp.colsum is not None:
        col0, post, _ = sp.colsum
        if post and second:
            terms, te = r, (e_out if regs else e_r)
        else:
            terms, te = v, e_pre
        T_out = g['T_out']
        c0 = d.colsum0[GUARD:GUARD + sp.B, :N - col0].double()
        tsum = terms.view(sp.B, T_out, N).sum(1)[:, col0:]
        tabs = terms.abs().view(sp.B, T_out, N).sum(1)[:, col0:]
        res['colsum'] = (c0 + tsum, te.view(sp.B, T_out, N).sum(1)[:, col0:] + (T_out + 2) * U * (tabs + c0.abs()))
    return res


def unshuffle(x, half):
    """SPLIT2: (m, n') -> row 2m + (n' >= half), column n' mod half."""
    return x.reshape(x.shape[0], 2, half).reshape(2 * x.shape[0], half)


def compare(name, got, ref, bound, key):
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), name + ': non-finite value where the launch owns the element (%d)' % int((~torch.isfinite(got)).sum())
    err = (got.double() - ref).abs()
    tiny = 1e-300
    frac = err / (bound + tiny)
    worst = frac.max().item() if frac.numel() else 0.0
    STATS[key] = max(STATS.get(key, 0.0), worst)
    print('[gemm] %-60s %-7s worst err / bound %.3f' % (name, '%dx%d' % tuple(got.shape), worst))
    if worst > 1.0:
        i = np.unravel_index(int(frac.argmax()), frac.shape)
        raise AssertionError('%s: err %.4g > bound %.4g at %s (got %.7g, ref %.7g; %d elements over)' %
                             (name, err[i].item(), bound[i].item(), tuple(int(k) for k in i), got[i].item(), ref[i].item(), int((frac > 1).sum())))


def all_nan(x):
    return bool(torch.isnan(x).all())


def check_outputs(tag, sp, g, outs, refs, key):
    """Values against the reference and everything the launch must not touch."""
    N = sp.N
    for n, cols, rows, split in (('out', g['out_cols'], g['rows'], g['split']),) + \
            ((('out2', g['out2_cols'], g['rows2'], g['split2']),) if sp.out2 is not None else ()):
        buf = outs[n]
        assert all_nan(buf[:GUARD]) and all_nan(buf[GUARD + rows:]), '%s %s: guard rows written' % (tag, n)
        own = buf[GUARD:GUARD + rows]
        ref, bound = refs[n]
        if split:
            compare('%s %s' % (tag, n), own[:, :g['half']], ref, bound, key)
            assert all_nan(own[:, g['half']:]), '%s %s: columns past N/2 written' % (tag, n)
        else:
            compare('%s %s' % (tag, n), own[:, :N], ref, bound, key)
            assert (own[:, N:cols] == 0).all(), '%s %s: columns [N, out_cols) must be zeros' % (tag, n)
            assert all_nan(own[:, cols:]), '%s %s: columns past out_cols written' % (tag, n)
    if sp.colsum is not None:
        buf = outs['colsum']
        w = N - sp.colsum[0]
        assert all_nan(buf[:GUARD]) and all_nan(buf[GUARD + sp.B:]) and all_nan(buf[:, w:]), '%s colsum: written outside [0, N - col0)' % tag
        compare('%s colsum' % tag, buf[GUARD:GUARD + sp.B, :w], refs['colsum'][0], refs['colsum'][1], key)


def run_case(L, family, sp, dtype, path, want_path=None):
    g = geometry(sp, dtype, path)
    d = Data(sp, dtype, g)
    dev = Device(sp, dtype, d)
    (got_path, regs), outs = launch(L, sp, dtype, g, d, dev, path)
    tag = '%s/%s/%s/%s%s' % (family, sp.name, path, dtype, '/regs' if regs else '')
    assert got_path == (want_path or path), '%s: the launch took %s' % (tag, got_path)
    if sp.regs is not None and got_path == 'P8' and dtype == 'bf16':
        assert bool(regs) == sp.regs, '%s: register epilogue %d, expected %d' % (tag, regs, sp.regs)
    assert not regs or (got_path == 'P8' and dtype == 'bf16')
    refs = reference(sp, dtype, g, d, bool(regs))
    check_outputs(tag, sp, g, outs, refs, (family, got_path, dtype))
    return g, d, dev, outs


# ------------------------------------------------------------------------------------------------------------------------------
# case families

KLOOP = [Spec('nk%d_1tap' % nk, chunks=nk, B=b, T=t, N=n, k=1, bias=(nk % 2 == 1))
         for nk, b, t, n in ((1, 1, 70, 130), (2, 2, 129, 8), (3, 3, 50, 256), (4, 2, 64, 120), (5, 1, 200, 264), (6, 3, 33, 513),
                             (7, 2, 100, 249), (16, 1, 257, 128))] + \
        [Spec('nk7_7taps', chunks=1, k=7, B=2, T=90, N=200), Spec('nk6_2taps', chunks=3, k=2, B=3, T=45, N=136, mode='zero'),
         Spec('nk1_ldw_extra', chunks=1, k=1, B=3, T=43, N=72, ldw_extra=64), Spec('nk3_3taps_ldw_extra', chunks=1, k=3, B=2, T=77, N=264, ldw_extra=32),
         Spec('nk2_gather1', chunks=2, k=1, B=2, T=70, N=130, gather=1), Spec('nk1_gather1', chunks=1, k=1, B=1, T=130, N=40, gather=1)]

# (B, T, N): M = B * T.  P8 tiles (256 x 256): ntm in {1, 3, 4, 5, 9}, counts 1, 2, 3, 4, 5, 6, 9, 10, 27
GRID = [Spec('m%d_n%d' % (b * t, n), B=b, T=t, N=n, C=c, k=k, lda=lda)
        for b, t, n, c, k, lda in ((1, 1, 8, 40, 1, 'pad'), (1, 63, 120, 40, 3, 'ld32'), (2, 32, 128, 80, 1, 'ld32'), (1, 65, 130, 40, 3, 'pad'),
                                   (1, 127, 249, 24, 5, 'pad'), (4, 32, 256, 40, 1, 'pad'), (3, 43, 264, 40, 3, 'ld32'), (5, 51, 384, 40, 1, 'pad'),
                                   (1, 256, 512, 40, 3, 'pad'), (1, 257, 513, 40, 1, 'pad'), (1, 1283, 130, 40, 3, 'pad'), (9, 256, 8, 40, 1, 'pad'),
                                   (7, 100, 600, 24, 3, 'pad'), (8, 125, 64, 40, 1, 'pad'), (5, 256, 300, 40, 3, 'pad'), (1, 1200, 100, 40, 1, 'ld32'),
                                   (9, 256, 520, 24, 1, 'pad'), (6, 100, 20, 40, 3, 'pad'))]

EDGES = [Spec('t4_k7_pad_t_minus_1', B=40, T=4, k=7, N=48), Spec('t7_k6_zero', B=30, T=7, k=6, mode='zero', N=130),
         Spec('t9_k5_s2', B=33, T=9, k=5, stride=2, N=40), Spec('t50_k4', B=7, T=50, k=4, N=136), Spec('t127_k3_zero', B=3, T=127, k=3, mode='zero', N=72),
         Spec('t129_k2', B=3, T=129, k=2, N=264), Spec('t300_k1', B=2, T=300, k=1, N=48), Spec('t50_k5_s2_zero', B=6, T=50, k=5, stride=2, mode='zero', N=48),
         Spec('t7_k7_s2', B=41, T=7, k=7, stride=2, N=56), Spec('t129_k7_s2', B=3, T=129, k=7, stride=2, N=130), Spec('t9_k3', B=29, T=9, k=3, N=40, lda='ld32'),
         Spec('t300_k6_s2_zero', B=2, T=300, k=6, stride=2, mode='zero', N=40)]

DGRAD = [Spec('k1', gather=1, k=1, B=3, T=100, C=96, N=200), Spec('k3', gather=1, k=3, B=5, T=50, C=40, N=130),
         Spec('k5', gather=1, k=5, B=2, T=129, C=64, N=264, mode='zero'), Spec('k3_s2', gather=1, k=3, stride=2, B=3, T=45, C=40, N=72),
         Spec('k5_t4', gather=1, k=5, B=37, T=4, C=24, N=48)]

EPI = [
    Spec('bias_lrelu', B=3, T=50, N=100, k=3, bias=True, act=True, regs=True),
    Spec('bias_second_half', B=2, T=70, N=250, k=1, bias=True, out_cols='n', regs=False),
    Spec('prevec_t16', B=19, T=16, N=136, k=3, bias=True, pre_vec=True, act=True, regs=True),
    Spec('prevec_t24', B=13, T=24, N=136, k=3, bias=True, pre_vec=True, act=True, regs=False),
    Spec('out2_rows_vec2_t16', B=18, T=16, N=72, k=1, bias=True, out2='rows', vec2=True, regs=True),
    Spec('out2_rows_vec2_t24', B=12, T=24, N=72, k=1, bias=True, out2='rows', vec2=True, regs=False),
    Spec('split2_both_vec2_t16', B=17, T=16, N=272, k=3, bias=True, act=True, out='split', out2='split', vec2=True, regs=True),
    Spec('split2_both_vec2_t24', B=11, T=24, N=272, k=3, bias=True, act=True, out='split', out2='split', vec2=True, regs=False),
    Spec('split2_half_not_8', B=5, T=30, N=140, k=1, bias=True, out='split', out2='split', regs=False),
    Spec('split2_out_only', B=3, T=90, N=160, k=3, out='split', regs=True),
    Spec('rows_out2_split', B=9, T=32, N=96, k=1, out2='split', vec2=True, pre_vec=True, regs=True),
    Spec('dact', gather=1, B=3, T=100, N=136, dact=True, regs=True),
    Spec('add_bf16', gather=1, B=5, T=60, N=264, add='t', regs=True),
    Spec('add_f32', gather=1, B=5, T=60, N=264, add='f32', regs=False),
    Spec('dact_add', gather=1, B=2, T=129, N=200, dact=True, add='t', regs=True),
    Spec('dact_add_f32_out_f32', gather=1, B=2, T=129, N=200, dact=True, add='f32', out_f32=True, regs=False),
    Spec('out_f32', B=3, T=70, N=130, k=3, bias=True, act=True, out_f32=True, regs=False),
    Spec('out_cols_8_not_32', B=3, T=90, N=100, k=1, out_cols='r8', regs=True),
    Spec('out_cols_is_n', B=3, T=90, N=130, k=3, out_cols='n', regs=False),
    Spec('unaligned_rows', B=3, T=90, N=96, k=1, bias=True, unaligned=True, regs=False),
    Spec('dact_unaligned_n', gather=1, B=3, T=90, N=130, dact=True, add='t', out_cols='n', regs=False),
    Spec('colsum_t1', gather=1, B=300, T=1, N=72, colsum=(0, 0, 0), regs=True),
    Spec('colsum_t16_col8', gather=1, B=20, T=16, N=136, colsum=(8, 0, 1), dact=True, regs=True),
    Spec('colsum_t64_col16_post', gather=1, B=5, T=64, N=264, colsum=(16, 1, 1), dact=True, add='t', regs=True),
    Spec('colsum_t128_post_f32add', gather=1, B=3, T=128, N=72, colsum=(0, 1, 0), dact=True, add='f32', regs=False),
    Spec('colsum_t128_col24', gather=1, B=3, T=128, N=130, colsum=(24, 0, 1), add='t', out_cols='r8', regs=True),
    Spec('colsum_t64_post_plain', gather=1, B=6, T=64, N=40, colsum=(0, 1, 1), regs=True),
]

RAGGED = [Spec('t65_k5', B=9, T=65, k=5, N=72, lengths=[65, 64, 63, 3, 65, 4, 33, 64, 5], bias=True),
          Spec('t65_k5_s2', B=9, T=65, k=5, stride=2, N=72, lengths=[65, 64, 63, 3, 65, 4, 33, 64, 5], bias=True, act=True),
          Spec('t128_k3', B=5, T=128, k=3, N=136, lengths=[128, 2, 127, 128, 77]),
          Spec('t50_k7_zero', B=7, T=50, k=7, mode='zero', N=40, lengths=[4, 50, 7, 25, 49, 50, 13]),
          Spec('t129_k2_s2', B=4, T=129, k=2, stride=2, N=130, lengths=[129, 2, 128, 65])]

IMG = [Spec('5x5_s2_reflect', B=3, img=(12, 17, 5, 5), stride=2, pl=2, pr=2, N=72, bias=True),
       Spec('5x5_s2_zero', B=2, img=(13, 16, 5, 5), stride=2, pl=2, pr=2, mode='zero', N=40),
       Spec('3x3_zero', B=5, img=(9, 11, 3, 3), pl=1, pr=1, mode='zero', N=136),
       Spec('3x3_reflect', B=7, img=(7, 6, 3, 3), pl=1, pr=1, N=48, act=True),
       Spec('3x3_gather1', B=3, img=(6, 7, 3, 3), gather=1, N=72),
       Spec('w_out_1', B=4, img=(40, 3, 3, 3), pl=0, pr=0, mode='zero', N=48),
       Spec('taps_h_1', B=3, img=(9, 21, 1, 3), pl=0, pr=0, mode='zero', N=72)]

DETERMINISM = Spec('twice', B=3, T=171, k=3, N=264, C=96, bias=True, act=True)

FAMILIES = (('kloop', KLOOP), ('grid', GRID), ('edges', EDGES), ('dgrad', DGRAD), ('epilogue', EPI), ('ragged', RAGGED), ('2d', IMG))


def params(specs):
    return [pytest.param(sp, id=sp.name) for sp in specs]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('sp', params(KLOOP))
def test_k_loop(zs, sp, path, dtype):
    """nk = taps * cin_pad / KC in {1 .. 7, 16}: the prologue branches, the drain and the stage rotation of every kernel; as one
    tap of many chunks, as 7 taps of one chunk (a tap change every K tile) and as 2 taps of 3 chunks; ldw > taps * cin_pad."""
    run_case(zs[0], 'kloop', sp, dtype, path)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('sp', params(GRID))
def test_tile_grid(zs, sp, path, dtype):
    """M and N at, one below and one above the tile sizes; the P8 tile order with a short last group of tile rows and xcd_remap
    with fewer than 8 tiles and with a remainder."""
    run_case(zs[0], 'grid', sp, dtype, path)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('sp', params(EDGES))
def test_sample_edges(zs, sp, path, dtype):
    """Reflect / zero padding falling inside tiles: T_out that does not divide the tile height, k = 1 .. 7, stride 2 with odd and
    even T, reflect padding of T - 1 rows."""
    run_case(zs[0], 'edges', sp, dtype, path)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('sp', params(DGRAD))
def test_data_gradient(zs, sp, path, dtype):
    """gather = 1: the transposed-convolution row rule, in the padded domain (no fold)."""
    run_case(zs[0], 'dgrad', sp, dtype, path)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('sp', params(EPI))
def test_epilogue(zs, sp, path, dtype):
    """Every epilogue operand, on both epilogues of the P8 kernel (Spec.regs: which one the case is built to reach) and on the
    staging epilogue of the others."""
    if sp.colsum is not None and path == 'DMA64' and 64 % sp.T != 0:
        assert planned(zs[0], sp, dtype, path)[0] == 'DMA128'         # samples do not fit 64-row tiles: the plan says so
        run_case(zs[0], 'epilogue', sp, dtype, path, want_path='DMA128')
        return
    run_case(zs[0], 'epilogue', sp, dtype, path)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('sp', params(RAGGED))
def test_ragged(zs, sp, path, dtype):
    """lengths: every sample against the fp64 reference of that sample alone (the padding is applied at its own end; rows past its
    length come from zero rows) and bit for bit against a batch-1 launch of the sample."""
    L = zs[0]
    g, d, dev, outs = run_case(L, 'ragged', sp, dtype, path)
    T_out = g['T_out']
    for b, ln in enumerate(sp.lengths):
        plan, one = launch(L, sp, dtype, g, d, dev, path, sub=(b, ln))
        assert plan[0] == path
        n = (ln + sp.pl + sp.pr - g['taps']) // sp.stride + 1
        assert all_nan(one['out'][:GUARD]) and all_nan(one['out'][GUARD + n:])
        a = one['out'][GUARD:GUARD + n, :g['out_cols']]
        w = outs['out'][GUARD + b * T_out:GUARD + b * T_out + n, :g['out_cols']]
        assert torch.equal(a, w), '%s sample %d (length %d): the batch differs from the sample alone' % (sp.name, b, ln)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('sp', params(IMG))
def test_conv2d(zs, sp, path, dtype):
    """w_in > 0: 5x5 stride 2 and 3x3 stride 1, reflect and zero, gather 1 at stride 1, w_out = 1 and taps_h = 1."""
    run_case(zs[0], '2d', sp, dtype, path)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('path', PATHS)
def test_two_launches_are_bit_identical(zs, path, dtype):
    L = zs[0]
    sp = DETERMINISM
    g, d, dev, outs = run_case(L, 'twice', sp, dtype, path)
    _, again = launch(L, sp, dtype, g, d, dev, path)
    own = slice(GUARD, GUARD + g['rows'])
    assert torch.equal(outs['out'][own, :g['out_cols']], again['out'][own, :g['out_cols']])


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('ring_min_tiles,want', [(256, 'DMA64'), (0, 'RING_PP')])
def test_n_pad_384_is_never_p8(zs, ring_min_tiles, want, dtype):
    """A packed weight of 384 rows under the knobs that force P8 everywhere else: the plan falls through (to the ring when its
    tile threshold allows, else to the LDS-DMA kernel), the launch takes what the plan says, and the result is compared."""
    L = zs[0]
    sp = Spec('n384', B=5, T=51, N=384, k=1)
    g = geometry(sp, dtype, 'RING_PP')
    assert g['n_pad'] == 384
    force = dict(FORCE['P8'], gemm_ring=1, gemm_pp=1, gemm_ring_min_tiles=ring_min_tiles, gemm_dma64=1, gemm_dma64_max_tiles=256)
    with knobs(L, **force):
        assert query(L, struct_kw(L, sp, dtype, g, lambda n: DUMMY[n]))[0] == want
    d = Data(sp, dtype, g)
    (path, regs), outs = launch(L, sp, dtype, g, d, Device(sp, dtype, d), 'P8', force=force)
    assert (path, regs) == (want, 0)
    check_outputs('n384/%s/%s' % (path, dtype), sp, g, outs, reference(sp, dtype, g, d, False), ('grid', path, dtype))


def test_reflect_padding_as_long_as_the_sample_is_refused(zs):
    L = zs[0]
    sp = Spec('t3_k7', B=2, T=3, k=7, N=48)
    g = geometry(sp, 'bf16', 'DMA128')
    d = Data(sp, 'bf16', g)
    with pytest.raises(L.ZsError, match='Padding size should be less than the corresponding input dimension'):
        launch(L, sp, 'bf16', g, d, Device(sp, 'bf16', d), 'DMA128')


# the bench size under the default knobs: B = 256, seg_len = 128, widths of hps/zerospeech_english.json
PRODUCTION = [
    (Spec('conv_bank_k7_513_128', B=256, T=128, C=513, N=128, k=7, bias=True, act=True), 'DMA128', 0),
    (Spec('final_linear_1024_513', B=256, T=128, C=1024, N=513, k=1, bias=True), 'RING_PP', 0),
    (Spec('conv_k3_1024_2048_split2_out2', B=256, T=128, C=1024, N=2048, k=3, bias=True, act=True, out='split', out2='split', vec2=True), 'P8', 1),
    (Spec('dgrad_k1_mask_colsum', B=256, T=128, C=1024, N=1024, k=1, gather=1, dact=True, colsum=(512, 0, 1)), 'P8', 1),
    (Spec('inference_b1_t129', B=1, T=129, C=1024, N=1024, k=3, bias=True, act=True), 'DMA64', 0),
]


@pytest.mark.parametrize('sp,want,regs', [pytest.param(s, w, r, id=s.name) for s, w, r in PRODUCTION])
def test_production_shapes_default_knobs(zs, sp, want, regs):
    """No knob set: one launch per kernel the default dispatch takes at the bench size (bf16)."""
    L = zs[0]
    defaults = dict(gemm_dma=1, gemm_ring=1, gemm_ring_min_tiles=256, gemm_pp=1, gemm_p8=1, gemm_p8_min_tiles=200, gemm_dma64=1,
                    gemm_dma64_max_tiles=256)
    for k, v in defaults.items():          # the documented defaults are what the process runs with
        assert L.set_option(k, v) == v, k
    g = geometry(sp, 'bf16', 'default')
    d = Data(sp, 'bf16', g)
    (path, r), outs = launch(L, sp, 'bf16', g, d, Device(sp, 'bf16', d), 'default')
    assert (path, r) == (want, regs)
    check_outputs('production/%s/%s' % (sp.name, path), sp, g, outs, reference(sp, 'bf16', g, d, bool(r)), ('production', path, 'bf16'))


# ------------------------------------------------------------------------------------------------------------------------------
# layer logic: the stride-2 parity split and the column window of ConvLayer.dgrad


def dgrad_reference(dy, w, stride, Tp):
    """Transposed convolution in the padded domain: gp[b, u, ci] = sum_{t, j: t * stride + j = u} dy[b, t, co] w[co, ci, j];
    returns (value, sum of absolute terms), fp64."""
    B, Ty, Cout = dy.shape
    Cin, k = w.shape[1], w.shape[2]
    gp = torch.zeros(B, Tp, Cin, dtype=torch.float64)
    ga = torch.zeros(B, Tp, Cin, dtype=torch.float64)
    for j in range(k):
        gp[:, j:j + (Ty - 1) * stride + 1:stride] += dy @ w[:, :, j]
        ga[:, j:j + (Ty - 1) * stride + 1:stride] += dy.abs() @ w[:, :, j].abs()
    return gp, ga


# Cin / the window are chosen so that the operand ConvLayer packs has a multiple of 256 rows: every forced path is the path taken
LAYER = [  # name, B, T_x, Cout, Cin, k, stride, n_off, n_cols
    ('s2_k5_odd_domain', 3, 45, 48, 200, 5, 2, 0, None), ('s2_k4_even_domain', 2, 64, 40, 130, 4, 2, 0, None),
    ('s2_k3', 5, 33, 64, 390, 3, 2, 0, None), ('window_896_of_1409', 2, 70, 128, 1409, 1, 1, 0, 896),
    ('window_off_256', 3, 50, 72, 700, 3, 1, 256, 300), ('window_off_128', 2, 90, 40, 520, 1, 1, 128, 130),
]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('path', PATHS)
@pytest.mark.parametrize('case', [pytest.param(c, id=c[0]) for c in LAYER])
def test_layer_dgrad(zs, case, path, dtype):
    """ConvLayer.dgrad: stride 2 as two parity launches (an odd padded domain gets one extra zero row) and the n_off / n_cols
    column window, compared in the padded domain, before any fold.  The ZsGemmConv of every launch the layer makes is captured
    and its path asserted with zs_gemm_conv_path under the knobs of the launch."""
    L, layers = zs
    name, B, Tx, Cout, Cin, k, stride, n_off, n_cols = case
    gen = torch.Generator().manual_seed(zlib.crc32(('%s/%s' % (name, dtype)).encode()))
    ctx = layers.Ctx('cuda:0', dtype)
    w = spread((Cout, Cin, k), gen, 1.0 / math.sqrt(Cout * k))
    wd = w.to('cuda').contiguous()
    lay = layers.ConvLayer(ctx, wd, None, torch.zeros_like(wd), None, stride=stride)
    lay.pack()
    Ty = lay.t_out(Tx)
    Tp = Tx + lay.pad_l + lay.pad_r
    Te = Tp + (Tp & 1) if stride == 2 else Tp
    dy = rnd(spread((B, Ty, Cout), gen), dtype)
    dY = ctx.act('dy', B, Ty, Cout, ld=max(rup(Cout, 32), lay.cout_pad))
    dY.t.zero_()
    dY.t[:B * Ty * dY.ld].view(B * Ty, dY.ld)[:, :Cout] = dy.reshape(B * Ty, Cout).to('cuda', dY.t.dtype)
    ncol = Cin if n_cols is None else n_cols
    out = ctx.act('gp', B, Te, ncol)
    out.t.fill_(float('nan'))
    plans, call = [], L.call

    def recording_call(fname, sname, stream, **kw):
        st = call(fname, sname, stream, **kw)
        if fname == 'zs_gemm_conv':
            plans.append(query(L, {f: getattr(st, f) for f, _ in st._fields_}))
        return st
    L.call = recording_call
    try:
        with knobs(L, **FORCE[path]):
            if n_cols is None:
                lay.dgrad(dY, Tx, out)
            else:
                lay.dgrad(dY, Tx, out, n_cols=n_cols, n_off=n_off)
    finally:
        L.call = call
    torch.cuda.synchronize()
    assert len(plans) == (2 if stride == 2 else 1), plans
    assert all(p == path for p, _ in plans), '%s: forced %s, the launches of the layer took %s' % (name, path, plans)
    gp, ga = dgrad_reference(dy.double(), rnd(w, dtype).double(), stride, Te)
    gp, ga = gp[:, :, n_off:n_off + ncol], ga[:, :, n_off:n_off + ncol]
    K = (k if stride == 1 else (k + 1) // 2) * lay.cout_pad
    e = c_acc(K, dtype) * U * ga
    bound = e + (BF * (gp.abs() + e) if dtype == 'bf16' else 0.0)
    full = out.t[:B * Te * out.ld].view(B, Te, out.ld).float().cpu()
    compare('layer/%s/%s/%s' % (name, path, dtype), full[:, :, :ncol].reshape(B * Te, ncol), gp.reshape(B * Te, ncol), bound.reshape(B * Te, ncol),
            ('layer', path, dtype))
    assert (full[:, :, ncol:min(out.ld, rup(ncol, 32))] == 0).all()
    if Te != Tp:
        assert (full[:, Tp:, :ncol] == 0).all(), 'the extra row of an odd padded domain must be zeros'


# ------------------------------------------------------------------------------------------------------------------------------


def test_cases_reach_every_path(zs):
    """(path, register epilogue, dtype, gather) over all cases, from the plan of each case under the knobs it runs with: every
    path in both dtypes with gather 0 and 1; P8 / bf16 with and without the register epilogue, each with gather 0 and 1; and
    every case of every family takes the path it is forced to.  The plans here come from dummy operand addresses with the
    alignment of the real ones; run_case asserts the same path on the struct of the real launch."""
    L = zs[0]
    seen = {}
    for fam, specs in FAMILIES:
        for sp in specs:
            for path in PATHS:
                for dt in DTYPES:
                    p, regs = planned(L, sp, dt, path)
                    seen.setdefault((p, regs, dt, sp.gather), []).append('%s/%s' % (fam, sp.name))
                    # (colsum launches whose samples do not fit 64-row tiles: DMA128, asserted where they run)
                    assert p == path or (path == 'DMA64' and sp.colsum is not None and 64 % sp.T != 0 and p == 'DMA128'), (fam, sp.name, path, dt, p)
    print('\n[gemm paths]')
    for k in sorted(seen, key=lambda k: (PATHS.index(k[0]),) + k[1:]):
        print('[gemm paths] %-8s regs %d %-5s gather %d: %d cases' % (k + (len(seen[k]),)))
    want = set()
    for p in PATHS:
        for dt in DTYPES:
            for ga in (0, 1):
                want.add((p, 0, dt, ga))
    want |= {('P8', 1, 'bf16', 0), ('P8', 1, 'bf16', 1)}
    assert not want - set(seen), 'no case reaches %s' % sorted(want - set(seen))
    assert set(seen) <= want, sorted(set(seen) - want)
