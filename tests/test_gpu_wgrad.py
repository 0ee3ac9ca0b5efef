"""zs_gemm_wgrad (csrc/zs_gemm.hip) against fp64, element by element, on every path its plan can choose: the three K-loop kernels
(P8: gemm_wgrad_p8_kernel, 256x256 ping-pong; DMA: gemm_wgrad_dma_kernel, 128x128 LDS-DMA; REG: gemm_wgrad_kernel, register-staged,
bf16 and fp32) each followed by either slab reduce (wgrad_reduce_taps_kernel / wgrad_reduce_kernel).  zs_gemm_wgrad_path reports
kernel, reduce, splits and rows per split from the launch's own plan function; every case asserts all four on the struct it
launches, and test_cases_reach_every_path asserts that the cases reach every (kernel, reduce, dtype).

The test lays every operand out itself and calls zs_gemm_wgrad directly (no wgrad_call, no layer):
  * dY [M + slack rows][ldy] and X [B][x_batch_stride] with their own ld.  Columns past y_cols / x_cols, the slack rows and the
    rows between samples (x_batch_stride > T_in * ldx) hold NaN: the header calls them unreadable.  Columns [Cout, y_cols) and
    [Cin, x_cols) hold +-2^100 in some cases and NaN in others (Spec.ypad / xpad): the three loaders test whole 16-byte segments
    against y_cols / x_cols, so they read these columns; the values reach slab rows >= Cout and slab columns >= Cin, from which
    neither reduce stores anything (the header states this contract).  Values are spread over 2^-6 .. 2^6 with signs, dY holds
    exact zeros, bf16 operands are rounded once on the host and the reference uses the rounded values;
  * the workspace is exactly zs_gemm_wgrad_workspace_bytes long, NaN-filled before EVERY launch, and followed by a NaN guard that
    must be bit-unchanged afterwards: a slab region the K loop does not write and a reduce reads shows as a NaN in dW / db;
  * dW and db live inside larger NaN-filled buffers; so / si / sj address a sub-block (guard rows before and after, a row pitch
    wider than the block and a column offset in some cases).  After a launch every element the launch does not own is still NaN
    and every owned element is finite; with accumulate the owned elements are prefilled with known fp32 values that the
    reference adds; without db the db buffer is not passed and must stay NaN;
  * every case is launched twice, the second time with fresh NaN-filled buffers: dW / db must be bit-equal.

Reference: the source row of every (output row, tap) from the gather rule of zs_amd.h in NumPy index arithmetic (reflect / zero,
stride, pad_left beyond taps / 2, 2-D with j = kw * taps_h + kh); the products summed in fp64 once for the value and once with
absolute values for S = sum|terms|.  Every element of every case is compared; nothing is sampled.

Bound per element: C U S, U = 2^-24, r = min(rows_per_split, M) the rows of the fullest split (rows past a split's end are zero
rows: exact zero products, no rounding):
  * dW: C = c_acc(r) + splits + accumulate.  bf16: c_acc = ceil(r / 16) + 8: all three kernels walk a split in k-steps of 16 rows,
    one v_mfma_f32_32x32x16_bf16 per k-step and accumulator, in ascending row order (WFrag<bf16_t>::chunk, ZS_WD_KS, ZS_WP_MMA):
    a chain of ceil(r / 16) MFMA accumulations per element; + 8 as in tests/test_gpu_gemm.py.  fp32: ceil(r / 2) + 8: WFrag<float>
    ::chunk makes 16 v_mfma_f32_32x32x2_f32 per 32-row chunk, a chain of r / 2 (the K / 2 of test_gpu_gemm.py).  The reduce adds
    the `splits` slabs in order (wgrad_sum_splits) and accumulate adds one more term;
  * db: C = min(c_bias, r) + splits + accumulate, fp32 additions only.  128x128 kernels: a thread adds its row of every 32-row
    chunk (ceil(r / 32) additions), wgrad_tile_store then adds the 32 partials in row order: c_bias = ceil(r / 32) + 32.  P8: a
    thread adds rows kr0, kr0 + 16, kr0 + 32, kr0 + 48 of every 64-row K tile (kr0 = 0 .. 15: 4 ceil(r / 64) additions); the table
    red[(wr * 16 + kr0) * 128 + channel] has 32 rows, but they are 16 row lanes for each of the two wave groups wr, which own
    different halves of the 256 channels, and the final loop adds the 16 partials of one group ((tid >> 7) * 16 + r, r < 16):
    c_bias = 4 ceil(r / 64) + 16.  A sum of r terms has at most r roundings whatever its order (the others add exact zeros),
    hence the min.
  Every C is asserted to stay at or below the textbook r + splits + 1.

Measured worst fractions of the bound on an MI355X, dW / db (all elements of all cases):
  P8 / bf16 0.46 / 0.05, DMA / bf16 0.46 / 0.03, REG / bf16 0.46 / 0.03, REG / fp32 0.36 / 0.17 (rows reduce) and 0.36 / 0.11
  (taps reduce); the two reduces give the same dW fractions (they are bit-identical) and the three bf16 kernels meet their worst
  element in the same case.  No fraction exceeds 1 and the dW fractions are not near 0: the bound is not loose.  The bf16 db
  fractions are small because sums of a few hundred 8-bit significands are mostly exact in fp32.  The module takes about 4 s.

Value-only single-line mutations of zs_gemm.hip (scratch builds, never committed), the new tests that fail on each, and what the
suite before this file did with them:
  Each of the twelve fails new tests; the weight-gradient tests of the suite before (test_gpu_wgrad_dma.py, test_gpu_wgrad_p8.py and
  test_conv_backward / test_wgrad_split2_and_shift / the conv2d tests of test_gpu_kernels.py, run until the first failure) caught
  every one of them as well, so the table records no escape; what the new module adds is listed in the issue (per-element bound,
  poisoned workspace, asserted plan, fp32, the edges).  Failing new tests are counted over all (kernel, dtype, reduce) parameters.
   1 kh and kw swapped in conv_src_row_g (2-D gather): 64, every img_* case of test_geometry on every path.  Before: caught
     (test_wgrad_dma_bitwise_vs_register_staged[conv2d_3x3]).
   2 zero padding: source row 0 treated as padding in conv_src_row: 88, the zero-padded cases of test_geometry and test_rows on
     every path.  Before: caught (gru_3HxH_split2_shift).
   3 gemm_wgrad_dma_kernel: bias partial sums from the second K stage on: 86, every db case on DMA, no other path.  Before: caught.
   4 wgrad_sum_splits stops at splits - 1: 459, every case on every path.  Before: caught.
   5 wgrad_co_perm: odd co permuted the wrong way round: 24, the four co_split2 cases on every path.  Before: caught.
   6 wgrad_reduce_taps_kernel: the last float4 of ci dropped when Cin % 4 != 0: 16, c72x13_k3_m32, c40x261_k2_m63,
     img_5x5_cin13 / cin50 with the taps reduce on every kernel, no case with the rows reduce.  Before: caught (bank, Cin 513).
   7 wgrad_reduce_bias ignores accumulate: 56, every db + accumulate case on every path.  Before: caught.
   8 wgrad_tile_store: the bias column sum skips partial 0: 258, every db case on DMA and REG (bf16 and fp32), none on P8 (its own
     bias sum).  Before: caught.
   9 gemm_wgrad_p8_kernel: quadrant (1,1) multiplies k-step 3 of dY with k-step 2 of X: 79 on P8 only.  Before: caught.
  10 gemm_wgrad_dma_kernel: k-step 2 issued twice instead of k-steps 2, 3: 89 on DMA only.  Before: caught.
  11 WFrag<float>::chunk: 15 of the 16 MFMA steps of a chunk: 118 on REG / fp32 only.  Before: caught (test_conv_backward fp32).
  12 wgrad_reduce_kernel: accumulate ignored for the fourth ci of each float4: 60, the accumulate cases that take the rows reduce.
     Before: caught.

No kernel bug was found: no unwritten slab region, no pad column reaching a reduced element, no bound exceeded, and the plan report
agrees with every launch.
"""
import ctypes
import math
import time
import zlib

import numpy as np
import pytest
import torch

import test_gpu_gemm as G
from test_gpu_gemm import U, knobs, rnd, rup, spread

pytestmark = pytest.mark.gpu

KERNELS = ('P8', 'DMA', 'REG')
VARIANTS = (('P8', 'bf16'), ('DMA', 'bf16'), ('REG', 'bf16'), ('REG', 'fp32'))
FORCE = {'P8': dict(wgrad_p8=2), 'DMA': dict(wgrad_p8=0, wgrad_dma=1), 'REG': dict(wgrad_p8=0, wgrad_dma=0)}
GUARD = 3              # NaN rows before and after the dW block, NaN elements around db
WS_GUARD = 4096        # NaN floats behind the workspace
SLACK_ROWS = 64        # NaN rows behind dY and behind the last sample of X
BIG = 2.0 ** 100
STATS = {}             # (kernel, reduce, dtype, 'dW' | 'db') -> worst fraction of the bound
REFS = {}              # (case, dtype) -> data and reference, computed once and never modified


def c_acc(r, dtype):
    """MFMA accumulations per element over r rows (module docstring)."""
    return math.ceil(r / (2.0 if dtype == 'fp32' else 16.0)) + 8.0


def c_bias(r, kernel):
    return min(4.0 * math.ceil(r / 64.0) + 16.0 if kernel == 'P8' else math.ceil(r / 32.0) + 32.0, float(r))


@pytest.fixture(scope='module')
def zs():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    from zs_amd import _lib
    _lib.lib()
    t0 = time.time()
    yield _lib
    print('\n[wgrad] wall time of this module %.1f s; worst fraction of the bound per (kernel, reduce, dtype), dW / db:' % (time.time() - t0))
    for k, r, d in sorted({key[:3] for key in STATS}):
        print('[wgrad]   %-4s %-6s %-5s %.3f / %.3f' % (k, 'taps' if r else 'rows', d, STATS.get((k, r, d, 'dW'), 0.0), STATS.get((k, r, d, 'db'), 0.0)))


# ------------------------------------------------------------------------------------------------------------------------------
# a case


class Spec(object):
    """One launch.  Geometry: B samples of T input rows (2-D: img = (h_in, w_in, taps_h, taps_w), T = h_in * w_in), k taps, stride,
    padding (pl, pr; default the pad_layer() rule k // 2, k - 1 - k // 2; t_out overrides the output length), mode.  layout: 'conv'
    (Conv1d weight [co][ci][tap]: si = taps, sj = 1), 'linear' (taps 1: si = 1, sj = 0) or 'tci' ([co][tap][ci]: si = 1, sj = Cin);
    pitch: elements the dW row pitch `so` exceeds the block's width by, col0: the block's first column in that row.
    ypad / xpad: 'nan' or 'big', what columns [Cout, y_cols) / [Cin, x_cols) hold (default: by the name's checksum);
    ycols / xcols: extra 16-byte segments of such columns; xbs: elements between the samples of X."""

    DEFAULTS = dict(B=2, T=16, k=1, stride=1, pl=None, pr=None, t_out=None, mode='reflect', img=None, Cout=72, Cin=40, layout='conv',
                    pitch=0, col0=0, db=False, acc=False, split2=False, splits=1, alone=0, ypad=None, xpad=None, ycols=0, xcols=0, xbs=0)

    def __init__(self, name, **kw):
        self.name = name
        bad = set(kw) - set(self.DEFAULTS)
        assert not bad, bad
        self.__dict__.update(self.DEFAULTS)
        self.__dict__.update(kw)
        if self.pl is None:
            self.pl = self.k // 2
        if self.pr is None:
            self.pr = self.k - 1 - self.k // 2
        crc = zlib.crc32(name.encode())
        if self.ypad is None:
            self.ypad = 'nan' if crc & 1 else 'big'
        if self.xpad is None:
            self.xpad = 'nan' if crc & 2 else 'big'
        assert self.layout != 'linear' or (self.k == 1 and self.img is None)

    def __repr__(self):
        return self.name


def geometry(sp, dtype):
    """All integer fields of the ZsGemmWgrad of a case and the layout of its buffers."""
    es = 4 if dtype == 'fp32' else 2
    seg = 16 // es
    g = dict(es=es)
    if sp.img is not None:
        h_in, w_in, th, tw = sp.img
        taps = th * tw
        h_out = (h_in + sp.pl + sp.pr - th) // sp.stride + 1
        w_out = (w_in + sp.pl + sp.pr - tw) // sp.stride + 1
        T_in, T_out = h_in * w_in, h_out * w_out
        g.update(w_in=w_in, w_out=w_out, taps_h=th, h_in=h_in, h_out=h_out)
    else:
        taps, T_in = sp.k, sp.T
        T_out = sp.t_out if sp.t_out is not None else (T_in + sp.pl + sp.pr - taps) // sp.stride + 1
        g.update(w_in=0, w_out=0, taps_h=0)
    y_cols = rup(sp.Cout, seg) + sp.ycols * seg
    x_cols = rup(sp.Cin, seg) + sp.xcols * seg
    ldy, ldx = rup(y_cols, 8) + 8, rup(x_cols, 8) + 16
    if sp.layout == 'conv':
        width, si, sj = sp.Cin * taps, taps, 1
    elif sp.layout == 'linear':
        width, si, sj = sp.Cin, 1, 0
    else:
        width, si, sj = sp.Cin * taps, 1, sp.Cin
    so = width + sp.pitch
    assert sp.col0 + width <= so
    g.update(taps=taps, T_in=T_in, T_out=T_out, M=sp.B * T_out, y_cols=y_cols, x_cols=x_cols, ldy=ldy, ldx=ldx, xbs=T_in * ldx + sp.xbs,
             so=so, si=si, sj=sj, dw0=GUARD * so + sp.col0, dw_len=(GUARD + sp.Cout + GUARD) * so)
    return g


def reduce_of(sp, g, knob):
    return int(bool(knob) and sp.layout == 'conv' and 1 < g['taps'] <= 256)


def plan_splits(L, sp, g, kernel):
    """The split-K rule of wgrad_plan restated (zs_gemm.hip), under the knobs as they are now."""
    if sp.splits > 0:
        return sp.splits
    M, alone = g['M'], L.get_option('wgrad_alone')
    tile = 256 if kernel == 'P8' else 128
    tiles = -(-sp.Cout // tile) * g['taps'] * -(-sp.Cin // tile)
    if kernel != 'P8':
        target = L.get_option('wgrad_wgs128_alone' if alone else 'wgrad_wgs128') or 448
        return max(1, min(-(-target // tiles), -(-M // 256), 1024))
    wgs = L.get_option('wgrad_wgs') or 256
    slab = L.get_option('wgrad_slab_cost_alone' if alone else 'wgrad_slab_cost')
    kt, best, bs = -(-M // 64), 1e30, 1
    for s in range(1, 65):
        if s * 4 > kt:
            break
        cost = -(-tiles * s // wgs) * (-(-kt // s) + slab)
        if cost < best - 1e-9:
            best, bs = cost, s
    return bs


def struct_kw(L, sp, dtype, g, ptr):
    kw = dict(dtype=L.ZS_F32 if dtype == 'fp32' else L.ZS_BF16, dY=ptr('dY'), ldy=g['ldy'], y_cols=g['y_cols'], X=ptr('X'), ldx=g['ldx'],
              x_batch_stride=g['xbs'], x_cols=g['x_cols'], B=sp.B, T_in=g['T_in'], T_out=g['T_out'], taps=g['taps'], stride=sp.stride,
              pad_left=sp.pl, pad_mode=L.ZS_PAD_REFLECT if sp.mode == 'reflect' else L.ZS_PAD_ZERO, Cout=sp.Cout, Cin=sp.Cin, dW=ptr('dW'),
              so=g['so'], si=g['si'], sj=g['sj'], db=ptr('db') if sp.db else None, co_split2=int(sp.split2), accumulate=int(sp.acc),
              splits=sp.splits, workspace=ptr('ws'), w_in=g['w_in'], w_out=g['w_out'], taps_h=g['taps_h'])
    return kw


DUMMY = {n: 0x100000 * (i + 1) for i, n in enumerate(('dY', 'X', 'dW', 'db', 'ws'))}


def planned(L, sp, dtype, kernel, knob):
    """(kernel, reduce, splits, rows_per_split) the plan gives this case under the knobs it runs with, from dummy addresses."""
    g = geometry(sp, dtype)
    with knobs(L, wgrad_reduce_taps=knob, wgrad_alone=sp.alone, **FORCE[kernel]):
        s = L.STRUCTS['ZsGemmWgrad'](**{k: v for k, v in struct_kw(L, sp, dtype, g, lambda n: DUMMY[n]).items() if v is not None})
        k, r, n, rps = L.wgrad_path(s)
    return KERNELS[k], r, n, rps


# ------------------------------------------------------------------------------------------------------------------------------
# data, reference, launch


def source_rows(sp, g):
    """[M, taps] source row of each (output row, tap) within its sample, [M, taps] validity, [M] sample."""
    B, T_out, taps = sp.B, g['T_out'], g['taps']
    reflect = sp.mode == 'reflect'
    b = np.repeat(np.arange(B), T_out)
    t = np.tile(np.arange(T_out), B)
    j = np.arange(taps)
    if sp.img is not None:
        ho, wo = t // g['w_out'], t % g['w_out']
        kw_, kh = j // g['taps_h'], j % g['taps_h']
        h, okh = G.axis_rows(0, reflect, sp.stride, sp.pl, g['h_in'], ho, kh)
        w, okw = G.axis_rows(0, reflect, sp.stride, sp.pl, g['w_in'], wo, kw_)
        return h * g['w_in'] + w, okh & okw, b
    row, ok = G.axis_rows(0, reflect, sp.stride, sp.pl, g['T_in'], t, j)
    return row, ok, b


class Ref(object):
    """Host operands of a case (exactly the values the kernel reads) and its fp64 reference, in dW's channel order."""

    def __init__(self, sp, dtype, g):
        gen = torch.Generator().manual_seed(zlib.crc32(('%s/%s' % (sp.name, dtype)).encode()))
        M, Cout, Cin, taps, T_in = g['M'], sp.Cout, sp.Cin, g['taps'], g['T_in']
        nan = float('nan')
        dy = rnd(spread((M, Cout), gen), dtype)
        dy[torch.rand(dy.shape, generator=gen) < 0.125] = 0.0
        x = rnd(spread((sp.B, T_in, Cin), gen), dtype)
        sign = torch.where(torch.arange(max(g['y_cols'], g['x_cols'])) % 2 == 0, 1.0, -1.0) * BIG
        dY = torch.full((M + SLACK_ROWS, g['ldy']), nan)
        dY[:M, :Cout] = dy
        dY[:M, Cout:g['y_cols']] = nan if sp.ypad == 'nan' else sign[Cout:g['y_cols']]
        X = torch.full((sp.B * g['xbs'] + SLACK_ROWS * g['ldx'],), nan)
        Xv = X[:sp.B * g['xbs']].view(sp.B, g['xbs'])[:, :T_in * g['ldx']].view(sp.B, T_in, g['ldx'])
        Xv[:, :, :Cin] = x
        Xv[:, :, Cin:g['x_cols']] = nan if sp.xpad == 'nan' else sign[Cin:g['x_cols']]
        self.dY, self.X = dY.reshape(-1), X
        self.w0 = spread((Cout, Cin, taps), gen)
        self.b0 = spread((Cout,), gen)
        # fp64: value and sum of absolute terms
        rows, ok, b = source_rows(sp, g)
        dyd, xd = dy.double(), x.double()
        bi = torch.from_numpy(b)
        w = torch.zeros(Cout, Cin, taps, dtype=torch.float64)
        S = torch.zeros(Cout, Cin, taps, dtype=torch.float64)
        for j in range(taps):
            xg = xd[bi, torch.from_numpy(rows[:, j])] * torch.from_numpy(ok[:, j])[:, None]
            w[:, :, j] = dyd.T @ xg
            S[:, :, j] = dyd.abs().T @ xg.abs()
        bsum, bS = dyd.sum(0), dyd.abs().sum(0)
        if sp.split2:      # dW row co comes from dY column (co & 1) * Cout / 2 + (co >> 1)
            perm = torch.tensor([(co & 1) * (Cout // 2) + (co >> 1) for co in range(Cout)])
            w, S, bsum, bS = w[perm], S[perm], bsum[perm], bS[perm]
        if sp.acc:
            w, S = w + self.w0.double(), S + self.w0.double().abs()
            bsum, bS = bsum + self.b0.double(), bS + self.b0.double().abs()
        self.w, self.S, self.b, self.bS = w, S, bsum, bS
        co, ci, jj = torch.meshgrid(torch.arange(Cout), torch.arange(Cin), torch.arange(taps), indexing='ij')
        self.idx = g['dw0'] + co * g['so'] + ci * g['si'] + jj * g['sj']          # flat index of dW[co, ci, j]; linear: taps == 1
        assert self.idx.unique().numel() == self.idx.numel() and GUARD * g['so'] <= int(self.idx.min()) and int(self.idx.max()) < (GUARD + Cout) * g['so']


def get_ref(sp, dtype, g):
    key = (sp.name, dtype)
    if key not in REFS:
        REFS[key] = Ref(sp, dtype, g)
    return REFS[key]


def launch(L, sp, dtype, g, ref, dev, kernel, knob):
    """One launch into fresh NaN-filled dW / db / workspace.  Returns (plan, dW buffer, db buffer) on the host."""
    dW = torch.full((g['dw_len'],), float('nan'))
    db = torch.full((GUARD + sp.Cout + GUARD,), float('nan'))
    if sp.acc:
        dW[ref.idx.reshape(-1)] = ref.w0.reshape(-1)
        db[GUARD:GUARD + sp.Cout] = ref.b0
    dW, db = dW.cuda(), db.cuda()
    with knobs(L, wgrad_reduce_taps=knob, wgrad_alone=sp.alone, **FORCE[kernel]):
        probe = L.STRUCTS['ZsGemmWgrad'](**{k: v for k, v in struct_kw(L, sp, dtype, g, lambda n: DUMMY[n]).items() if v is not None})
        need = L.lib().zs_gemm_wgrad_workspace_bytes(ctypes.byref(probe))
        assert need % 4 == 0 and need > 0
        ws = torch.full((need // 4 + WS_GUARD,), float('nan'), device='cuda')
        t = dict(dY=dev['dY'], X=dev['X'], dW=dW, db=db, ws=ws)
        off = dict(dW=g['dw0'], db=GUARD)
        kw = struct_kw(L, sp, dtype, g, lambda n: L.ptr(t[n], off.get(n, 0)))
        s = L.call('zs_gemm_wgrad', 'ZsGemmWgrad', torch.cuda.current_stream().cuda_stream, workspace_bytes=need, **kw)
        k, r, n, rps = L.wgrad_path(s)
        assert L.lib().zs_gemm_wgrad_workspace_bytes(ctypes.byref(s)) == need
    torch.cuda.synchronize()
    guard = ws[need // 4:].view(torch.int32).cpu()
    assert bool((guard == 0x7fc00000).all()), '%s: the guard behind the workspace was written' % sp.name
    return (KERNELS[k], r, n, rps), dW.cpu(), db.cpu()


def compare(name, got, ref, S, C, key):
    assert torch.isfinite(got).all(), '%s: %d non-finite values where the launch owns the element' % (name, int((~torch.isfinite(got)).sum()))
    err = (got.double() - ref).abs()
    bound = C * U * S
    frac = err / (bound + 1e-300)
    worst = frac.max().item()
    STATS[key] = max(STATS.get(key, 0.0), worst)
    print('[wgrad] %-58s %-12s C %6.1f  worst err / bound %.3f' % (name, 'x'.join(str(d) for d in got.shape), C, worst))
    if worst > 1.0:
        i = np.unravel_index(int(frac.argmax()), frac.shape)
        raise AssertionError('%s: err %.4g > bound %.4g at %s (got %.7g, ref %.7g; %d elements over)' %
                             (name, err[i].item(), bound[i].item(), tuple(int(k) for k in i), got[i].item(), ref[i].item(), int((frac > 1).sum())))


def run_case(L, sp, kernel, dtype, knob):
    g = geometry(sp, dtype)
    ref = get_ref(sp, dtype, g)
    tdt = torch.float32 if dtype == 'fp32' else torch.bfloat16
    dev = dict(dY=ref.dY.to('cuda', tdt), X=ref.X.to('cuda', tdt))
    plan, dW, db = launch(L, sp, dtype, g, ref, dev, kernel, knob)
    tag = '%s/%s/%s/%s' % (sp.name, kernel, 'taps' if plan[1] else 'rows', dtype)
    # the plan of the launched struct
    want_kernel = 'REG' if dtype == 'fp32' else kernel
    with knobs(L, wgrad_alone=sp.alone):
        splits = plan_splits(L, sp, g, want_kernel)
    gran = 64 if want_kernel == 'P8' else 32
    rps = rup(-(-g['M'] // splits), gran)
    assert plan == (want_kernel, reduce_of(sp, g, knob), splits, rps), '%s: the launch took %s' % (tag, plan)
    # values
    r = min(rps, g['M'])
    C = c_acc(r, dtype) + splits + int(sp.acc)
    Cb = c_bias(r, want_kernel) + splits + int(sp.acc)
    assert C <= r + splits + 1 and Cb <= r + splits + 1, (tag, C, Cb, r, splits)
    key = (want_kernel, plan[1], dtype)
    own = torch.zeros(g['dw_len'], dtype=torch.bool)
    own[ref.idx.reshape(-1)] = True
    assert bool(torch.isnan(dW[~own]).all()), '%s: dW written outside the block (so %d, si %d, sj %d)' % (tag, g['so'], g['si'], g['sj'])
    compare(tag + ' dW', dW[ref.idx], ref.w, ref.S, C, key + ('dW',))
    assert bool(torch.isnan(db[:GUARD]).all() and torch.isnan(db[GUARD + sp.Cout:]).all()), '%s: db written outside [0, Cout)' % tag
    if sp.db:
        compare(tag + ' db', db[GUARD:GUARD + sp.Cout], ref.b, ref.bS, Cb, key + ('db',))
    elif sp.acc:
        assert torch.equal(db[GUARD:GUARD + sp.Cout], ref.b0), '%s: db is null, the buffer changed' % tag
    else:
        assert bool(torch.isnan(db).all()), '%s: db is null, the buffer changed' % tag
    # a second launch, fresh NaN-filled workspace and outputs: bit-equal
    plan2, dW2, db2 = launch(L, sp, dtype, g, ref, dev, kernel, knob)
    assert plan2 == plan
    assert torch.equal(dW[ref.idx], dW2[ref.idx]), '%s: dW differs between two launches' % tag
    if sp.db:
        assert torch.equal(db[GUARD:GUARD + sp.Cout], db2[GUARD:GUARD + sp.Cout]), '%s: db differs between two launches' % tag
    return plan


# ------------------------------------------------------------------------------------------------------------------------------
# cases: the smallest shapes that reach each edge.  M = B * T_out in {21, 32, 63, 64, 65, 200, 416, 640}

TILES = [  # Cout x Cin at, below and one past the 128 / 256 tiles; Cin % 4 != 0: the (Cin + 3) / 4 reduce and its tail
    Spec('c8x8_m21_linear', B=3, T=7, Cout=8, Cin=8, layout='linear', db=True),
    Spec('c72x136_k3_m32', B=2, T=16, Cout=72, Cin=136, k=3, db=True, ycols=1, ypad='nan'),
    Spec('c128x128_k2_m64', B=4, T=16, Cout=128, Cin=128, k=2, splits=2),
    Spec('c136x72_k3_m63_acc', B=9, T=7, Cout=136, Cin=72, k=3, db=True, acc=True, xcols=1, xpad='nan'),
    Spec('c264x264_m65_linear', B=1, T=65, Cout=264, Cin=264, layout='linear', db=True, pitch=24, col0=8),
    Spec('c200x256_k3_m200', B=5, T=40, Cout=200, Cin=256, k=3, db=True, splits=2),
    Spec('c256x200_m416_linear', B=26, T=16, Cout=256, Cin=200, layout='linear', splits=3, acc=True),
    Spec('c264x520_k2_m64', B=4, T=16, Cout=264, Cin=520, k=2, db=True),
    Spec('c520x200_m640_linear', B=5, T=128, Cout=520, Cin=200, layout='linear', db=True, splits=2),
    Spec('c72x13_k3_m32', B=2, T=16, Cout=72, Cin=13, k=3, db=True, xpad='big'),
    Spec('c72x13_k3_tci', B=2, T=16, Cout=72, Cin=13, k=3, layout='tci', acc=True, xpad='nan'),
    Spec('c40x261_k2_m63', B=9, T=7, Cout=40, Cin=261, k=2, splits=2, xpad='nan'),
    Spec('c40x261_linear_acc', B=9, T=7, Cout=40, Cin=261, layout='linear', db=True, acc=True, xpad='big'),
    Spec('split2_c72_m200', B=5, T=40, Cout=72, Cin=40, layout='linear', split2=True, db=True, splits=2),          # Cout / 2 = 36
    Spec('split2_c264_k3_acc', B=2, T=16, Cout=264, Cin=72, k=3, split2=True, db=True, acc=True, pitch=16),        # Cout / 2 = 132
    Spec('split2_c138_nodb_acc', B=4, T=16, Cout=138, Cin=136, k=2, split2=True, acc=True, ypad='nan'),
]

ROWS = [  # samples straddling 32- and 64-row chunks; P8: carried pointers (1-D, stride 1, T_out | 128) and the general path
    Spec('t7_m21_k3', B=3, T=7, k=3, db=True),
    Spec('t7_m63_k5', B=9, T=7, k=5),
    Spec('t16_m32_k3', B=2, T=16, k=3, db=True, acc=True),
    Spec('t16_m416_k3_s3', B=26, T=16, k=3, splits=3, db=True),
    Spec('t40_m200_k3', B=5, T=40, k=3, db=True),
    Spec('t40_m640_k3_s3', B=16, T=40, k=3, splits=3),
    Spec('t48_m48_k4', B=1, T=48, k=4, db=True),
    Spec('t48_m240_k3_s2', B=5, T=48, k=3, splits=2, db=True),
    Spec('t128_m640_k3_s5', B=5, T=128, k=3, splits=5, db=True),
    Spec('t128_m640_k7_s2_acc', B=5, T=128, k=7, splits=2, acc=True, Cout=40, Cin=24),
    Spec('t65_m65_k3', B=1, T=65, k=3, db=True),
    Spec('t64_m64_k3', B=1, T=64, k=3, db=True),
    Spec('t16_m416_k3_zero', B=26, T=16, k=3, mode='zero', db=True),                  # P8: carried pointers with zero rows, 7 K tiles
    Spec('t128_m640_k5_zero_s2', B=5, T=128, k=5, mode='zero', splits=2),
]

SPLITS = [  # explicit 1, 2, 3, 5; a short last split; trailing splits with no rows at all; the plan's own choice
    Spec('m200_s1', B=5, T=40, k=3, splits=1, db=True),
    Spec('m200_s2', B=5, T=40, k=3, splits=2, db=True, acc=True),
    Spec('m200_s3_short_last', B=5, T=40, k=3, splits=3, db=True),                    # 96 + 96 + 8 rows (P8: 128 + 72)
    Spec('m200_s5_empty_last', B=5, T=40, k=3, splits=5, db=True),                    # 64 + 64 + 64 + 8 + 0
    Spec('m21_s5_four_empty', B=3, T=7, k=3, splits=5, db=True, acc=True),            # 21 + 0 + 0 + 0 + 0
    Spec('m640_s7_p8_two_empty', B=5, T=128, k=2, splits=7, db=True, Cout=40, Cin=24),   # P8: 5 x 128 + 0 + 0; else 6 x 96 + 64
    Spec('m640_s9_two_empty', B=5, T=128, k=2, splits=9, db=True, Cout=40, Cin=24),      # 6 x 96 + 64 + 0 + 0 (P8: 5 x 128 + 4 x 0)
    Spec('m416_s13_linear', B=26, T=16, layout='linear', splits=13, db=True),         # 13 x 32: more than 8 slabs in the reduce
    Spec('m640_plan', B=5, T=128, k=3, splits=0, db=True),
    Spec('m640_plan_alone', B=5, T=128, k=3, splits=0, db=True, alone=1),
    Spec('m416_plan_linear_c264', B=26, T=16, Cout=264, Cin=136, layout='linear', splits=0, alone=1),
    Spec('m200_plan', B=5, T=40, k=2, splits=0, acc=True),
]

GEOMETRY = [Spec('k%d_reflect' % k, B=b, T=t, k=k, db=(k % 2 == 1), splits=1 + (k % 2)) for k, b, t in
            ((1, 3, 7), (2, 2, 16), (3, 5, 40), (4, 1, 48), (5, 1, 128), (6, 9, 7), (7, 4, 16))] + [
    Spec('k3_s2_reflect', B=2, T=32, k=3, stride=2, db=True),
    Spec('k5_s2_zero', B=5, T=80, k=5, stride=2, mode='zero', splits=2, db=True),
    Spec('k4_s2_zero_t7', B=9, T=14, k=4, stride=2, mode='zero'),
    Spec('k3_zero', B=5, T=40, k=3, mode='zero', db=True),
    Spec('gru_shift_linear', B=5, T=40, t_out=40, layout='linear', pl=1, mode='zero', db=True, splits=2),
    Spec('gru_shift_split2_window', B=5, T=40, t_out=40, Cout=264, Cin=128, layout='linear', pl=1, mode='zero', split2=True, db=True, ycols=2,
         xcols=3, ypad='big', xpad='big', pitch=128, col0=128),
    Spec('k3_pl3_zero_shift', B=2, T=16, t_out=16, k=3, pl=3, mode='zero', db=True),
    Spec('k3_pl2_reflect_shift', B=2, T=16, t_out=16, k=3, pl=2),
    Spec('xbs_k3', B=5, T=40, k=3, xbs=24, db=True, splits=2),
    Spec('xbs_linear_nan_window', B=4, T=16, layout='linear', xbs=8, ycols=1, xcols=1, ypad='nan', xpad='nan', acc=True),
    Spec('pitch_conv_k3', B=2, T=16, k=3, pitch=21, col0=9, db=True),
    Spec('pitch_tci_k3', B=2, T=16, k=3, layout='tci', pitch=40, col0=40, Cin=40),
    Spec('tci_k5_acc', B=3, T=7, k=5, layout='tci', db=True, acc=True, Cin=13),
    Spec('img_3x3_6x10_reflect', B=2, img=(6, 10, 3, 3), pl=1, pr=1, db=True),
    Spec('img_3x3_6x10_zero', B=2, img=(6, 10, 3, 3), pl=1, pr=1, mode='zero', splits=2),
    Spec('img_3x3_6x10_s2_reflect', B=5, img=(6, 10, 3, 3), pl=1, pr=1, stride=2),
    Spec('img_3x3_6x10_s2_zero', B=5, img=(6, 10, 3, 3), pl=1, pr=1, stride=2, mode='zero', db=True, acc=True),
    Spec('img_5x5_cin13', B=4, img=(8, 8, 5, 5), pl=2, pr=2, stride=2, Cin=13, db=True),
    Spec('img_5x5_cin50_acc', B=4, img=(8, 8, 5, 5), pl=2, pr=2, stride=2, mode='zero', Cin=50, acc=True, splits=2),    # taps reduce: 40 + 10 ci
    Spec('img_3x5_reflect', B=1, img=(6, 10, 3, 5), pl=2, pr=2, Cout=40, Cin=24, db=True),
    Spec('img_5x3_zero', B=1, img=(6, 10, 5, 3), pl=1, pr=1, mode='zero', Cout=40, Cin=24),
]

FAMILIES = (('tiles', TILES), ('rows', ROWS), ('splits', SPLITS), ('geometry', GEOMETRY))


def params(specs):
    """(spec, kernel, dtype, wgrad_reduce_taps): every case under the knob's default; under 0 where that changes the reduce."""
    out = []
    for sp in specs:
        for kernel, dtype in VARIANTS:
            for knob in (1, 0):
                if knob == 1 or reduce_of(sp, geometry(sp, dtype), 1):
                    out.append(pytest.param(sp, kernel, dtype, knob, id='%s-%s-%s-%s' % (sp.name, kernel, dtype, 'taps' if knob else 'rows')))
    return out


@pytest.mark.parametrize('sp,kernel,dtype,knob', params(TILES))
def test_tiles(zs, sp, kernel, dtype, knob):
    """Cout and Cin below one tile, at a tile and one segment past it, for the 128- and the 256-wide kernels; Cin in {13, 261}
    with x_cols rounded up to 16 bytes; co_split2 with Cout / 2 not a multiple of 8."""
    run_case(zs, sp, kernel, dtype, knob)


@pytest.mark.parametrize('sp,kernel,dtype,knob', params(ROWS))
def test_rows(zs, sp, kernel, dtype, knob):
    """M below one K tile, at and around 32 / 64, not a multiple of either; samples of 7, 16, 40, 48, 128 rows."""
    run_case(zs, sp, kernel, dtype, knob)


@pytest.mark.parametrize('sp,kernel,dtype,knob', params(SPLITS))
def test_splits(zs, sp, kernel, dtype, knob):
    """Explicit split counts, a short last split, trailing splits without rows, and splits = 0 under wgrad_alone 0 and 1."""
    run_case(zs, sp, kernel, dtype, knob)


@pytest.mark.parametrize('sp,kernel,dtype,knob', params(GEOMETRY))
def test_geometry(zs, sp, kernel, dtype, knob):
    """taps 1 .. 7, stride 2, zero padding, pad_left beyond taps / 2, the GRU shift and column windows, x_batch_stride, dW as a
    sub-block in three layouts, 2-D 3x3 / 5x5 / 3x5 / 5x3 on non-square images."""
    run_case(zs, sp, kernel, dtype, knob)


def test_cases_reach_every_path(zs):
    """(kernel, reduce, dtype) over all cases from the plan of each case under the knobs it runs with; beyond that: trailing empty
    splits on each kernel, both address paths of the P8 K loop, every pair of db / accumulate / co_split2 on each kernel."""
    L = zs
    seen, empty, carried, pairs = {}, set(), set(), {}
    for fam, specs in FAMILIES:
        for p in params(specs):
            sp, kernel, dtype, knob = p.values
            g = geometry(sp, dtype)
            k, r, n, rps = planned(L, sp, dtype, kernel, knob)
            assert k == ('REG' if dtype == 'fp32' else kernel) and r == reduce_of(sp, g, knob), (sp.name, kernel, dtype, knob, k, r)
            seen.setdefault((k, r, dtype), []).append(sp.name)
            if (n - 1) * rps >= g['M']:
                empty.add((k, dtype))
            if k == 'P8':
                carried.add(sp.img is None and sp.stride == 1 and 128 % g['T_out'] == 0)
            flags = [f for f in ('db', 'acc', 'split2') if getattr(sp, f)]
            for a in flags:
                for b in flags:
                    if a < b:
                        pairs.setdefault((k, dtype), set()).add((a, b))
    print('\n[wgrad paths]')
    for key in sorted(seen):
        print('[wgrad paths] %-4s reduce %d %-5s: %d cases' % (key + (len(seen[key]),)))
    want = {(k, r, d) for k, d in VARIANTS for r in (0, 1)}
    assert set(seen) == want, sorted(want ^ set(seen))
    assert empty == set(VARIANTS), sorted(empty)
    assert carried == {True, False}
    for v in VARIANTS:
        assert pairs[v] == {('acc', 'db'), ('db', 'split2'), ('acc', 'split2')}, (v, pairs[v])
