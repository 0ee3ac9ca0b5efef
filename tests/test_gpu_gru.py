"""The bidirectional GRU (csrc/zs_gru.hip, driven through layers.GruLayer) against fp64, step by step, on every launch path the
plan can choose: WIDE, PERSIST with PER 1/2/4 (forward) and PERB 3/6/12 (BPTT), STEP_FUSED and STEP_GEMM, fp32 and bf16.
zs_gru_path reports the plan of a launch; every case asserts it for both passes, and test_cases_reach_every_plan_value prints
the table of (pass, path, PER, dtype) the cases reach and asserts that it holds every value the plan can return.

The references are fed the kernel's own operands, so every bound is per step and independent of T:
  * forward, step t of direction d: h_prev is the kernel's stored `out` at the previous step of that direction (bitwise the bf16
    operand of its recurrent product on every path: granules, LDS image and `out` carry the same rounding of h), zero at the
    first step; gi is the kernel's `gi` buffer; W_hh is read back from the packed buffer, b_hh is fp32.  r, z, n, hn are
    recomputed in fp64 with the formulas at the top of zs_gru.hip and compared with the saved gate tape, h with
    (1 - z) n + z h_prev.
  * BPTT: the tape (gates, out, dout) and the kernel's stored dgh of the previous BPTT step (bitwise the operand of its carried
    product); the direct carry dh z is carried in fp64.  dgi and dgh are compared at every step.
  * parameter and input gradients: fp64 sums over the kernel's stored dgh / dgi / out / X (dW_hh of direction 1 over the
    h_{t+1} rows the pad_left = -1 gather reads).  At the decoder's full size a random subset of rows is checked.
All products over all T are single fp64 matmuls; only the elementwise carries loop over t.

Bounds (U = 2^-24; every check prints its measured error as a fraction of the bound):
  * accumulation of K products in fp32 (MFMA chains, the cross-wave sums): C_ACC(K) = (K / 16 + 8) U sum|terms|.
  * a gate: its pre-activation error through sigma' <= 1/4 (r, z) or tanh' <= 1 (n), plus C_F = 8 U for expf / tanhf / the
    division; each fp32 add or multiply of the gate math: U of its magnitude (C_E = 8 U of the chain's magnitude in the BPTT).
  * h: |n - h_prev| e_z + (1 - z) e_n, plus, in bf16, z 2^-8 |h_prev|: the kernel carries h_prev in fp32 and stores it rounded.
  * BPTT: the fp32 dh carry gets z e(dh_prev) + C_ACC(3H) U sum|dgh W| + 3 U (|dout| + |carry| + |dgh W|) per step;
    each output is its derivative w.r.t. dh times that, plus C_E U of its magnitude.
  * every bf16 output: one round-to-nearest-even, 2^-8 of the value.
  * parameter gradients (fp32 out, sums over B*T rows): C_WG = 24 U sum|terms|; dX (K = 6H, output in the compute dtype) and
    the input projection gi (K = Cin): C_ACC(K) U sum|terms| + the output rounding.
Measured worst fractions of the bound on an MI355X, fp32 / bf16: forward gates and h 0.26 / 1.00, BPTT dgi and dgh 0.23 / 1.00,
gi 0.45 / 1.00, dX 0.20 / 0.99, parameter gradients 0.32 / 0.15 (at most 7.7 U sum|terms|).  The bf16 fractions are the output
rounding itself (2^-8 of the value is reached just above a power of two); the fp32 ones leave a margin of 2 to 7.  An error of
one step, one row block or one tile is many bounds wide: value-only mutations of a single line (a bias scaled in row blocks
>= 1 only, the last BPTT step's zero h_prev, b_n outside r * (...), the direct carry scaled by 0.95, the pad_left of the
direction-1 dW_hh gather) each fail a case here."""
import contextlib
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF = 2.0 ** -8
C_F, C_E, C_WG = 8.0, 8.0, 24.0
PATHS = ('WIDE', 'PERSIST', 'STEP_FUSED', 'STEP_GEMM')
FULL = dict(B=256, T=128, Cin=1024, H=512)      # the decoder / generator GRU at the bench size


def c_acc(K):
    return K / 16.0 + 8.0


@pytest.fixture(scope='module')
def zs():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    from zs_amd import _lib, layers
    _lib.lib()
    return _lib, layers


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


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def query(L, pas, dtype, B, T, H, inter, aligned):
    rc = L.lib().zs_gru_path(pas, L.ZS_F32 if dtype == 'fp32' else L.ZS_BF16, B, T, H, int(inter), int(aligned))
    assert rc >= 0, L.last_error()
    return PATHS[rc & 255], rc >> 8


class Case(object):
    """One GRU configuration.  B may be 'wide_max' / 'persist_max' (+ '+1'): the largest batch whose WIDE / PERSIST grid fits one
    workgroup per CU, or the next one.  fwd / bwd: the expected (path, PER) of each pass; for the boundary cases: (path, None),
    asserted as 'this path' at the largest B and 'not this path' at the next one."""

    def __init__(self, name, dtype, B, T, Cin, H, fwd, bwd, persist=1, wide=1, out_col=None, extra=0, dout_col=None,
                 bcast=False, ragged=False, spot=False):
        self.name, self.dtype, self.B, self.T, self.Cin, self.H = name, dtype, B, T, Cin, H
        self.fwd, self.bwd, self.persist, self.wide = fwd, bwd, persist, wide
        self.out_col = Cin if out_col is None else out_col
        self.extra, self.dout_col, self.bcast, self.ragged, self.spot = extra, dout_col, bcast, ragged, spot

    def batch(self):
        if isinstance(self.B, int):
            return self.B
        base, _, plus = self.B.partition('+')
        return min(grid_max(base, pas, self.H) for pas in (0, 1)) + (1 if plus else 0)

    def layout(self):
        """(out_col, ldo, dout_col, ldd, ld of gi / dgi / dgh) as the test lays the buffers out."""
        H = self.H
        width = self.out_col + 2 * H + (2 * H if self.bcast else 0) + self.extra
        dcol = self.out_col if self.dout_col is None else self.dout_col
        return self.out_col, rup(width, 32), dcol, rup(dcol + 2 * H, 32), rup(6 * H, 32)

    def aligned(self, pas):
        """The WIDE kernels' layout condition for this case's columns and leading dimensions (the device pointers are asserted
        16-byte aligned when the case runs)."""
        oc, ldo, dcol, ldd, ldg = self.layout()
        ok = oc % 8 == 0 and ldo % 8 == 0 and ldg % 8 == 0 and (not self.bcast or (oc + 2 * self.H) % 8 == 0)
        return ok and (pas == 0 or (dcol % 8 == 0 and ldd % 8 == 0))

    def plan(self, L):
        B = self.batch()
        with knobs(L, gru_persist=self.persist, gru_wide=self.wide):
            return [query(L, pas, self.dtype, B, self.T, self.H, self.H % 32 == 0, self.aligned(pas)) for pas in (0, 1)]


def grid_max(kind, pas, H):
    """The largest B whose WIDE ('wide_max') / PERSIST ('persist_max') grid of pass `pas` is at most one workgroup per CU: WIDE
    16 rows x 64 units per workgroup; PERSIST 32 rows x 32 units (forward) / 16 rows x 64 units (BPTT); both directions."""
    rows, units = (16, 64) if kind == 'wide_max' or pas == 1 else (32, 32)
    return rows * (cus() // (2 * (H // units)))


def rup(x, m):
    return (x + m - 1) // m * m


W_, P_, F_, G_ = PATHS
CASES = [
    # every path / PER / dtype, both passes
    Case('wide128', 'bf16', 33, 9, 48, 128, (W_, 0), (W_, 0)),
    Case('wide256', 'bf16', 17, 8, 64, 256, (W_, 0), (W_, 0)),
    Case('wide512_b1_plain_layout', 'bf16', 1, 7, 32, 512, (W_, 0), (W_, 0), out_col=0),
    Case('persist_bf16_h128', 'bf16', 33, 9, 40, 128, (P_, 1), (P_, 3), wide=0),
    Case('persist_bf16_h256_t2', 'bf16', 17, 2, 64, 256, (P_, 2), (P_, 6), wide=0),
    Case('persist_bf16_h512', 'bf16', 40, 11, 32, 512, (P_, 4), (P_, 12), wide=0, extra=40),
    Case('persist_fp32_h64', 'fp32', 17, 10, 24, 64, (P_, 1), (P_, 3)),
    Case('persist_fp32_h128_t2', 'fp32', 33, 2, 40, 128, (P_, 2), (P_, 6)),
    Case('persist_fp32_h256_b1', 'fp32', 1, 9, 16, 256, (P_, 4), (P_, 12)),
    Case('fused_bf16_h96', 'bf16', 33, 7, 40, 96, (F_, 0), (F_, 0)),
    Case('fused_bf16_h512_b17', 'bf16', 17, 6, 32, 512, (F_, 0), (F_, 0), persist=0),
    Case('fused_fp32_h32', 'fp32', 17, 5, 24, 32, (F_, 0), (F_, 0)),
    Case('fused_fp32_h128_b1', 'fp32', 1, 6, 16, 128, (F_, 0), (F_, 0), persist=0),
    Case('gemm_bf16_h72', 'bf16', 17, 6, 40, 72, (G_, 0), (G_, 0)),
    Case('gemm_fp32_h72', 'fp32', 33, 5, 24, 72, (G_, 0), (G_, 0)),
    Case('gemm_bf16_h40_b1', 'bf16', 1, 4, 16, 40, (G_, 0), (G_, 0)),
    # T = 1: no persistent path
    Case('t1_bf16_h128', 'bf16', 17, 1, 32, 128, (F_, 0), (F_, 0)),
    Case('t1_fp32_h64', 'fp32', 3, 1, 16, 64, (F_, 0), (F_, 0)),
    # the two passes on different paths: dout_col even but not a multiple of 8 fails only the BPTT's WIDE layout test
    Case('wide_fwd_persist_bwd', 'bf16', 20, 6, 32, 512, (W_, 0), (P_, 12), dout_col=2),
    # the model's own shapes: encoder GRU (Cin 512, H 128, T = seg_len / 8), decoder / generator GRU at the bench size, and that
    # GRU at the longest inference tail and an odd T
    Case('encoder', 'bf16', 256, 16, 512, 128, (W_, 0), (W_, 0)),
    Case('encoder_fp32', 'fp32', 64, 16, 512, 128, (P_, 2), (P_, 6)),
    Case('decoder_full', 'bf16', FULL['B'], FULL['T'], FULL['Cin'], FULL['H'], (W_, 0), (W_, 0), spot=True),
    Case('decoder_t254', 'bf16', 16, 254, 1024, 512, (W_, 0), (W_, 0)),
    Case('decoder_t255_persist', 'bf16', 33, 255, 1024, 512, (P_, 4), (P_, 12), wide=0),
    Case('decoder_t255_fused', 'bf16', 17, 255, 64, 512, (F_, 0), (F_, 0), persist=0),
    # the grid boundary: the largest B whose grid fits one workgroup per CU, and the next B
    Case('wide_grid_max', 'bf16', 'wide_max', 5, 32, 128, (W_, None), (W_, None)),
    Case('wide_grid_max_plus1', 'bf16', 'wide_max+1', 5, 32, 128, (W_, None), (W_, None)),
    Case('persist_grid_max', 'bf16', 'persist_max', 5, 32, 128, (P_, None), (P_, None), wide=0),
    Case('persist_grid_max_plus1', 'bf16', 'persist_max+1', 5, 32, 128, (P_, None), (P_, None), wide=0),
    # append_emb broadcast block riding on the recurrence: persistent (WIDE, PERSIST) and per-step launches
    Case('bcast_wide', 'bf16', 33, 6, 32, 256, (W_, 0), (W_, 0), bcast=True),
    Case('bcast_persist_fp32', 'fp32', 17, 6, 24, 128, (P_, 2), (P_, 6), bcast=True),
    Case('bcast_fused', 'bf16', 17, 6, 32, 128, (F_, 0), (F_, 0), persist=0, bcast=True),
    Case('bcast_gemm', 'fp32', 5, 4, 16, 40, (G_, 0), (G_, 0), bcast=True),
    # ragged inference batches (dir1_forward): lengths 1 .. T, forward only
    Case('ragged_wide', 'bf16', 19, 23, 32, 128, (W_, 0), None, ragged=True),
    Case('ragged_persist_fp32', 'fp32', 19, 23, 24, 64, (P_, 1), None, ragged=True),
    Case('ragged_fused', 'bf16', 19, 23, 32, 128, (F_, 0), None, persist=0, ragged=True),
    Case('ragged_gemm', 'bf16', 19, 23, 32, 72, (G_, 0), None, ragged=True),
]


def every_plan_value():
    """Each (pass, path, PER, dtype) zs_gru_path can return."""
    out = set()
    for dt in ('fp32', 'bf16'):
        for pas, pers in ((0, (1, 2, 4)), (1, (3, 6, 12))):
            out |= {(pas, P_, p, dt) for p in pers} | {(pas, F_, 0, dt), (pas, G_, 0, dt)}
    return out | {(0, W_, 0, 'bf16'), (1, W_, 0, 'bf16')}


def test_cases_reach_every_plan_value(zs):
    L, _ = zs
    seen = {}
    for c in CASES:
        for pas, (path, per) in enumerate(c.plan(L)):
            if pas == 1 and c.bwd is None:
                continue
            seen.setdefault((pas, path, per, c.dtype), []).append(c.name)
    print('\n[gru paths] %d CUs' % cus())
    print('%-5s %-11s %-4s %-5s %s' % ('pass', 'path', 'PER', 'dtype', 'cases'))
    for k in sorted(seen, key=lambda k: (k[0], PATHS.index(k[1]), k[2], k[3])):
        print('%-5s %-11s %-4d %-5s %s' % ('fwd' if k[0] == 0 else 'bwd', k[1], k[2], k[3], ' '.join(seen[k])))
    missing = every_plan_value() - set(seen)
    assert not missing, 'plan values no case reaches: %s' % sorted(missing)
    assert set(seen) <= every_plan_value(), sorted(set(seen) - every_plan_value())


# ------------------------------------------------------------------------------------------------------------------------------
# checks


def check(name, got, ref, bound, stats=None):
    """|got - ref| <= bound elementwise; prints the measured error as a fraction of the bound."""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), name + ': non-finite output'
    err = (got - ref).abs()
    frac = err / bound
    worst = frac.max().item() if frac.numel() else 0.0
    if stats is not None:
        stats[name] = max(stats.get(name, 0.0), worst)
    if worst > 1.0:
        i = np.unravel_index(int(frac.argmax()), frac.shape)
        raise AssertionError('%s: err %.4g > bound %.4g at %s (got %.7g, ref %.7g; %d elements over)' %
                             (name, err[i].item(), bound[i].item(), tuple(int(k) for k in i), got[i].item(), ref[i].item(),
                              int((frac > 1).sum())))


def out_round(dtype, ref, e):
    """Storage rounding of a kernel output whose fp32 value is within e of ref."""
    return e + (BF * (ref.abs() + e) if dtype == 'bf16' else 0.0)


def prev_rows(x, walk_fwd, lengths=None):
    """x at the previous step of a direction (zero at its first step): t - 1 walking forward, t + 1 walking backward (a ragged
    sample's backward walk starts at its own last row)."""
    p = torch.zeros_like(x)
    if walk_fwd:
        p[:, 1:] = x[:, :-1]
    else:
        p[:, :-1] = x[:, 1:]
        if lengths is not None:
            for b, n in enumerate(lengths):
                p[b, n - 1] = 0
    return p


def check_fwd(dtype, H, h, gi, W, bhh, gates, stats, lengths=None):
    """Per-step forward check of rows [B, T] (fp64 host tensors read back from the kernel's buffers).  h: [B, T, 2H];
    gi: [B, T, 6H]; W: [2, 3H, H]; bhh: [2, 3H]; gates: [B, T, 2, 4, H] or None."""
    mask = None
    if lengths is not None:
        mask = (torch.arange(h.shape[1])[None, :] < torch.tensor(lengths)[:, None])[:, :, None]
    for d in range(2):
        hd = h[:, :, d * H:(d + 1) * H]
        hp = prev_rows(hd, d == 0, lengths)
        gh = hp @ W[d].T
        ga = hp.abs() @ W[d].abs().T
        e_gh = c_acc(H) * U * ga
        g = gi[:, :, 3 * H * d:3 * H * (d + 1)]
        b = bhh[d]
        sl = [slice(k * H, (k + 1) * H) for k in range(3)]
        pre_r = g[..., sl[0]] + gh[..., sl[0]] + b[sl[0]]
        pre_z = g[..., sl[1]] + gh[..., sl[1]] + b[sl[1]]
        r, z = torch.sigmoid(pre_r), torch.sigmoid(pre_z)
        e_r = 0.25 * (e_gh[..., sl[0]] + 2 * U * (g[..., sl[0]].abs() + gh[..., sl[0]].abs() + b[sl[0]].abs())) + C_F * U
        e_z = 0.25 * (e_gh[..., sl[1]] + 2 * U * (g[..., sl[1]].abs() + gh[..., sl[1]].abs() + b[sl[1]].abs())) + C_F * U
        hn = gh[..., sl[2]] + b[sl[2]]
        e_hn = e_gh[..., sl[2]] + U * (gh[..., sl[2]].abs() + b[sl[2]].abs())
        arg = g[..., sl[2]] + r * hn
        e_arg = hn.abs() * e_r + r * e_hn + 2 * U * (g[..., sl[2]].abs() + (r * hn).abs())
        n = torch.tanh(arg)
        e_n = e_arg + C_F * U
        href = (1 - z) * n + z * hp
        e_h = (n - hp).abs() * e_z + (1 - z) * e_n + 3 * U * (n.abs() + hp.abs())
        if dtype == 'bf16':
            e_h = e_h + z * BF * hp.abs()
        pairs = [('h', hd, href, e_h)]
        if gates is not None:
            pairs += [('r', gates[:, :, d, 0], r, e_r), ('z', gates[:, :, d, 1], z, e_z), ('n', gates[:, :, d, 2], n, e_n),
                      ('hn', gates[:, :, d, 3], hn, e_hn)]
        for nm, got, ref, e in pairs:
            bound = out_round(dtype, ref, e) + 1e-30
            if mask is not None:                          # rows past a sample's length hold garbage
                got, ref = torch.where(mask, got, 0.0), torch.where(mask, ref, 0.0)
            check('fwd %s' % nm, got, ref, bound, stats)


def check_bwd(dtype, H, h, gates, dout, dgi, dgh, W, stats):
    """Per-step BPTT check: h [B, T, 2H], gates [B, T, 2, 4, H], dout [B, T, 2H], dgi / dgh [B, T, 6H], W [2, 3H, H].
    Returns nothing; dgi / dgh are the kernel's."""
    B, T = h.shape[:2]
    for d in range(2):
        hp = prev_rows(h[:, :, d * H:(d + 1) * H], d == 0)
        r, z, n, hn = (gates[:, :, d, k] for k in range(4))
        do = dout[:, :, d * H:(d + 1) * H]
        gh_k = dgh[:, :, 3 * H * d:3 * H * (d + 1)]
        gprev = prev_rows(gh_k, d == 1)           # dgh of the previous BPTT step: t + 1 for direction 0, t - 1 for direction 1
        dhg = gprev @ W[d]
        dhg_a = gprev.abs() @ W[d].abs()
        dh = torch.zeros(B, T, H, dtype=torch.float64)
        e_dh = torch.zeros_like(dh)
        carry = torch.zeros(B, H, dtype=torch.float64)
        e_c = torch.zeros_like(carry)
        for t in (range(T - 1, -1, -1) if d == 0 else range(T)):
            v = do[:, t] + carry + dhg[:, t]
            e = e_c + c_acc(3 * H) * U * dhg_a[:, t] + 3 * U * (do[:, t].abs() + carry.abs() + dhg[:, t].abs())
            dh[:, t], e_dh[:, t] = v, e
            carry, e_c = v * z[:, t], z[:, t] * e
        adh = dh.abs()
        k_n = (1 - z) * (1 - n * n)
        dn_pre = dh * k_n
        dr_pre = dn_pre * hn * r * (1 - r)
        dz_pre = dh * (hp - n) * z * (1 - z)
        dnr = dn_pre * r
        m_n = adh * (1 + z) * (1 + n * n)
        m_r = m_n * hn.abs() * r * (1 + r)
        m_z = adh * (hp.abs() + n.abs()) * z * (1 + z)
        outs = [('dr', dr_pre, k_n * hn.abs() * r * (1 - r), m_r), ('dz', dz_pre, (hp - n).abs() * z * (1 - z), m_z),
                ('dn', dn_pre, k_n, m_n), ('dnr', dnr, k_n * r, m_n * r)]
        bounds = {}
        for nm, ref, k, m in outs:
            bounds[nm] = out_round(dtype, ref, k * e_dh + C_E * U * m) + 1e-30
        gi_k = dgi[:, :, 3 * H * d:3 * H * (d + 1)]
        for j, nm in enumerate(('dr', 'dz', 'dn')):
            check('bwd dgi.' + nm, gi_k[..., j * H:(j + 1) * H], dict((o[0], o[1]) for o in outs)[nm], bounds[nm], stats)
        for j, nm in enumerate(('dr', 'dz', 'dnr')):
            check('bwd dgh.' + nm, gh_k[..., j * H:(j + 1) * H], dict((o[0], o[1]) for o in outs)[nm], bounds[nm], stats)


def check_grads(dtype, H, Cin, h, X, dgi, dgh, Wih, dX, grads, stats, rows=None, xrows=None):
    """dW_hh, db_hh, dW_ih, db_ih (fp32) and dX over the kernel's stored dgh / dgi / out / X.  rows: the gradient rows checked
    (of 3H); xrows: the (b, t) rows of dX checked."""
    B, T = h.shape[:2]
    N = B * T
    for d in range(2):
        hp = prev_rows(h[:, :, d * H:(d + 1) * H], d == 0).reshape(N, H)   # pad_left +1 (h_{t-1}) / -1 (h_{t+1}) of the gather
        gh = dgh[:, :, 3 * H * d:3 * H * (d + 1)].reshape(N, 3 * H)
        gi = dgi[:, :, 3 * H * d:3 * H * (d + 1)].reshape(N, 3 * H)
        xx = X.reshape(N, Cin)
        sel = slice(None) if rows is None else rows
        for nm, dy, x in (('weight_hh', gh, hp), ('weight_ih', gi, xx)):
            dyr = dy[:, sel]
            ref, a = dyr.T @ x, dyr.abs().T @ x.abs()
            got = grads['RNN.%s_l0%s' % (nm, '_reverse' if d else '')][sel]
            check('grad ' + nm, got, ref, C_WG * U * a + 1e-30, stats)
            bn = nm.replace('weight', 'bias')
            ref, a = dyr.sum(0), dyr.abs().sum(0)
            got = grads['RNN.%s_l0%s' % (bn, '_reverse' if d else '')][sel]
            check('grad ' + bn, got, ref, C_WG * U * a + 1e-30, stats)
    g6 = dgi.reshape(N, 6 * H)
    xr = slice(None) if xrows is None else xrows
    ref, a = g6[xr] @ Wih, g6[xr].abs() @ Wih.abs()
    check('dX', dX.reshape(N, Cin)[xr], ref, out_round(dtype, ref, c_acc(6 * H) * U * a) + 1e-30, stats)


# ------------------------------------------------------------------------------------------------------------------------------
# one case


def rows_of(act):
    return act.t[act.off:act.off + act.rows * act.ld].view(act.B, act.T, act.ld)


def host(x):
    return x.detach().double().cpu()


def seed_of(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003


def make_layer(layers, ctx, case):
    B, T, Cin, H = case.batch(), case.T, case.Cin, case.H
    g = torch.Generator().manual_seed(seed_of(case.name))
    P = {}
    for sfx in ('', '_reverse'):
        P['RNN.weight_ih_l0' + sfx] = torch.randn(3 * H, Cin, generator=g) / math.sqrt(Cin)
        P['RNN.weight_hh_l0' + sfx] = torch.randn(3 * H, H, generator=g) * (1.5 / math.sqrt(H))
        P['RNN.bias_ih_l0' + sfx] = torch.randn(3 * H, generator=g) * 0.2
        P['RNN.bias_hh_l0' + sfx] = torch.randn(3 * H, generator=g) * 0.3
    dev = ctx.device
    Pd = {k: v.to(dev).contiguous() for k, v in P.items()}
    Gd = {k: torch.full_like(v, float('nan')) for k, v in Pd.items()}
    gru = layers.GruLayer(ctx, Pd, Gd, 'RNN.', name=case.name)
    gru.pack()
    X = ctx.act('x', B, T, Cin)
    rows_of(X)[:, :, :Cin] = torch.randn(B, T, Cin, generator=g).to(dev, ctx.tdt)
    return gru, Gd, X, g


def packed_whh(gru):
    """W_hh [2, 3H, H] as the kernels read it (rounded as packed), rows un-permuted."""
    H = gru.H
    pk = gru.whh_f[:2 * gru.hh_npad * gru.hh_ldw].view(2, gru.hh_npad, gru.hh_ldw)[:, :3 * H, :H]
    W = torch.zeros(2, 3 * H, H, dtype=torch.float64)
    if gru.fast:
        W[:, gru.perm.long().cpu()] = host(pk)
    else:
        W[:] = host(pk)
    return W


def run(L, layers, case, stats):
    dtype, T, Cin, H = case.dtype, case.T, case.Cin, case.H
    B = case.batch()
    ctx = layers.Ctx('cuda:0', dtype)
    try:
        with knobs(L, gru_persist=case.persist, gru_wide=case.wide):
            _run(L, layers, ctx, case, B, stats)
    finally:
        ctx.release()
        torch.cuda.empty_cache()


def assert_plan(L, case, pas, B, aligned, want):
    got = query(L, pas, case.dtype, B, case.T, case.H, case.H % 32 == 0, aligned)
    path, per = want
    if per is None:                                       # grid boundary cases
        fits = B <= grid_max(case.B.partition('+')[0], pas, case.H)
        assert (got[0] == path) == fits, (case.name, pas, B, got)
    else:
        assert got == want, (case.name, 'fwd' if pas == 0 else 'bwd', got, want)
    return got


def _run(L, layers, ctx, case, B, stats):
    dtype, T, Cin, H = case.dtype, case.T, case.Cin, case.H
    dev = ctx.device
    gru, Gd, X, g = make_layer(layers, ctx, case)
    oc, ldo, dcol, ldd, ldg = case.layout()
    cat = ctx.act('cat', B, T, ldo, ld=ldo)
    gi = ctx.act('gi', B, T, 6 * H)
    assert gi.ld == ldg
    gates = None if case.ragged else ctx.raw('gates', B * T * 8 * H, ctx.tdt)
    bcast = None
    if case.bcast:
        vec = torch.randn(7, 2 * H + 3, generator=g)
        idx = torch.randint(0, 7, (B,), generator=g)
        bcast = (vec.to(dev), idx.to(dev), oc + 2 * H)
    lengths = None
    if case.ragged:
        lens = torch.randint(1, T + 1, (B,), generator=g)
        lens[0], lens[1], lens[-1] = 1, T, T - 1
        lengths = lens.tolist()
    for p in (cat.ptr(), gi.ptr()) + ((gates.data_ptr(),) if gates is not None else ()):
        assert p % 16 == 0
    assert_plan(L, case, 0, B, case.aligned(0), case.fwd)
    persistent = False

    def forward():
        gru.fwd(X, cat, oc, gi, gates, bcast=bcast,
                lengths=torch.tensor(lengths, dtype=torch.int32, device=dev) if lengths is not None else None)
        gru.check(B)
        torch.cuda.synchronize()

    forward()
    persistent |= query(L, 0, dtype, B, T, H, H % 32 == 0, case.aligned(0))[0] in (W_, P_)
    h = host(rows_of(cat)[:, :, oc:oc + 2 * H])
    gih = host(rows_of(gi)[:, :, :6 * H])
    if lengths is not None:                               # undo the per-sample reversal of the direction-1 gate inputs
        for b, n in enumerate(lengths):
            gih[b, :n, 3 * H:] = gih[b, :n, 3 * H:].flip(0)
    gh_ = host(gates[:B * T * 8 * H].view(B, T, 2, 4, H)) if gates is not None else None
    W = packed_whh(gru)
    bhh = host(gru.bhh.view(2, 3 * H))
    Wih = host(gru.wih_f[:gru.ih_npad * gru.ih_ldw].view(gru.ih_npad, gru.ih_ldw)[:6 * H, :Cin])
    Xh = host(rows_of(X)[:, :, :Cin])
    # the input projection feeding the recurrence (spot rows at the full size)
    sel = torch.randperm(B * T, generator=g)[:512] if case.spot else slice(None)
    x2, g2 = Xh.reshape(B * T, Cin)[sel], gih.reshape(B * T, 6 * H)[sel]
    ref = x2 @ Wih.T + host(gru.bih)
    check('gi', g2, ref, out_round(dtype, ref, c_acc(Cin) * U * (x2.abs() @ Wih.abs().T) + U * ref.abs()) + 1e-30, stats)
    for b0 in range(0, B, 64):                            # rows are independent given the stored h: bounded memory
        bs = slice(b0, min(B, b0 + 64))
        check_fwd(dtype, H, h[bs], gih[bs], W, bhh, gh_[bs] if gh_ is not None else None, stats,
                  lengths=lengths[bs] if lengths is not None else None)
    if bcast is not None:
        got = host(rows_of(cat)[:, :, oc + 2 * H:oc + 4 * H])
        want = host(bcast[0][:, :2 * H].to(ctx.tdt))[bcast[1].cpu()].unsqueeze(1).expand(B, T, 2 * H)
        assert torch.equal(got, want), case.name + ': broadcast block'
    if case.bwd is None:
        return
    dcat = ctx.act('dcat', B, T, ldd, ld=ldd)
    rows_of(dcat)[:, :, dcol:dcol + 2 * H] = (torch.randn(B, T, 2 * H, generator=g) * 0.5).to(dev, ctx.tdt)
    dgi, dgh = ctx.act('dgi', B, T, 6 * H), ctx.act('dgh', B, T, 6 * H)
    dX = ctx.act('dX', B, T, Cin)
    for p in (dcat.ptr(), dgi.ptr(), dgh.ptr()):
        assert p % 16 == 0
    assert_plan(L, case, 1, B, case.aligned(1), case.bwd)
    persistent |= query(L, 1, dtype, B, T, H, H % 32 == 0, case.aligned(1))[0] in (W_, P_)

    def backward():
        gru.bwd(dcat, dcol, cat, oc, gates, X, dgi, dgh, dX)
        gru.check(B)
        torch.cuda.synchronize()

    backward()
    dout = host(rows_of(dcat)[:, :, dcol:dcol + 2 * H])
    dgih, dghh = host(rows_of(dgi)[:, :, :6 * H]), host(rows_of(dgh)[:, :, :6 * H])
    for b0 in range(0, B, 64):
        bs = slice(b0, min(B, b0 + 64))
        check_bwd(dtype, H, h[bs], gh_[bs], dout[bs], dgih[bs], dghh[bs], W, stats)
    grads = {k: host(v) for k, v in Gd.items()}
    rows = torch.randperm(3 * H, generator=g)[:96] if case.spot else None
    xrows = torch.randperm(B * T, generator=g)[:256] if case.spot else None
    check_grads(dtype, H, Cin, h, Xh, dgih, dghh, Wih, host(rows_of(dX)[:, :, :Cin]), grads, stats, rows, xrows)
    if persistent:                                        # a persistent pass again: bitwise the same
        first = [rows_of(cat).clone(), gates.clone(), rows_of(dgi).clone(), rows_of(dgh).clone()]
        forward()
        backward()
        for nm, a, b in zip(('out', 'gates', 'dgi', 'dgh'), first, [rows_of(cat), gates, rows_of(dgi), rows_of(dgh)]):
            assert torch.equal(a, b), '%s: persistent GRU %s differs between two runs' % (case.name, nm)



@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_gru_per_step_fp64(zs, case):
    L, layers = zs
    stats = {}
    run(L, layers, case, stats)
    print('\n[err] %s (B=%d T=%d H=%d %s), fraction of the bound: %s' % (case.name, case.batch(), case.T, case.H, case.dtype,
                                                                        ', '.join('%s %.2f' % kv for kv in sorted(stats.items()))))
