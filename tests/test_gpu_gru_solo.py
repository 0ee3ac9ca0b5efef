"""The one-workgroup GRU kernels (gru_solo_fwd_kernel / gru_solo_bwd_kernel in csrc/zs_gru.hip; bf16, H = 128) through
zs_gru_fwd / zs_gru_bwd called with hand-packed operands.

  * bit-equality: the solo launch and the same launch with "gru_solo_max_h" = 0 (the hand-off kernels gru_wide_*<4>) leave
    byte-identical buffers -- forward: every byte of the output rows (h, the broadcast block, the columns around them) and the
    gate tape; BPTT: every byte of dgi and dgh -- and two solo launches are identical to each other.  The solo kernels keep every
    accumulator chain and every gate expression of the wide kernels, so equality is the contract, not a tolerance.
  * the work buffer: filled with a pattern before the solo launch (error word 0, so that zs_gru_check has nothing to report) and
    byte-identical after it; zs_gru_check returns ZS_OK.
  * fp64: one forward and one BPTT case against the per-step fp64 recurrences of tests/test_gpu_gru.py with that file's bounds
    for the wide bf16 path (check_fwd / check_bwd), so the kernels are pinned to the truth and not only to the older kernels.
  * zs_gru_solo: 1 for these launches; 0 for H = 256, wide_aligned = 0, fp32, T = 1, "gru_solo_max_h" = 0 and
    "gru_spin_limit" = 0, with zs_gru_path unchanged.

(B, T): (1, 2) one row of a partial block, two steps; (16, 3) one full block; (17, 5) two workgroups per direction, the second
with one row; (40, 16) three, the last partial, at the workload's own step count."""
import itertools
import math

import pytest
import torch

import test_gpu_gru as G

pytestmark = pytest.mark.gpu

H = 128
SHAPES = [(1, 2), (16, 3), (17, 5), (40, 16)]
PATTERN = 0x5A17C3A5                   # int32 fill of the work buffer
FILL = 0x7B7B                             # int16 fill of output buffers (a finite bf16)


@pytest.fixture(scope='module')
def L():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    from zs_amd import _lib
    _lib.lib()
    return _lib


def solo(L, pas, dtype, B, T, H_, inter=1, aligned=1):
    rc = L.lib().zs_gru_solo(pas, dtype, B, T, H_, inter, aligned)
    assert rc >= 0, L.last_error()
    return rc


def filled(n, dev):
    return torch.full((n,), FILL, dtype=torch.int16, device=dev).view(torch.bfloat16)


class Problem(object):
    """Operands of one bidirectional GRU (H = 128 unless given) as the kernels read them: gi [B*T][6H], W_hh packed gate-interleaved
    per 32 units (forward) and transposed (BPTT), b_hh fp32, a work buffer."""

    def __init__(self, L, B, T, seed, H=H):
        self.L, self.B, self.T, self.H = L, B, T, H
        dev = self.dev = torch.device('cuda:0')
        g = torch.Generator().manual_seed(seed)
        W = (torch.randn(2, 3 * H, H, generator=g) * (1.5 / math.sqrt(H))).to(torch.bfloat16)
        self.W = W.double()
        n = torch.arange(3 * H)
        perm = (n % 96 // 32) * H + n // 96 * 32 + n % 32       # packed row p holds W_hh row perm[p]
        self.whh = W[:, perm].contiguous().to(dev)               # [2][3H][H]
        self.whh_t = W.transpose(1, 2).contiguous().to(dev)      # [2][H][3H]
        self.bhh = (torch.randn(2, 3 * H, generator=g) * 0.3).to(dev)
        self.gi = torch.randn(B, T, 6 * H, generator=g).to(torch.bfloat16).to(dev)
        self.vec = torch.randn(7, 2 * H + 3, generator=g).to(dev)
        self.idx = torch.randint(0, 7, (B,), generator=g).to(dev)
        self.dout = (torch.randn(B, T, 2 * H, generator=g) * 0.5).to(torch.bfloat16)
        nw = (L.lib().zs_gru_work_bytes(B, H) + 3) // 4
        self.work = torch.zeros(nw, dtype=torch.int32, device=dev)
        self.stream = torch.cuda.current_stream().cuda_stream

    def fill_work(self):
        self.work.fill_(PATTERN)
        self.work[0] = 0                  # the error word zs_gru_check reads
        return self.work.clone()

    def check(self):
        L = self.L
        return L.lib().zs_gru_check(L.ptr(self.work), self.B, self.H, self.stream)

    def fwd(self, tape=True, bcast=False, dir1=0, out_col=0, extra=0):
        """One zs_gru_fwd into fresh pattern-filled buffers.  Returns (rows [B, T, ldo], gates or None)."""
        L, B, T, H = self.L, self.B, self.T, self.H
        ldo = out_col + 2 * H + (2 * H if bcast else 0) + extra
        out = filled(B * T * ldo, self.dev)
        gates = filled(B * T * 8 * H, self.dev) if tape else None
        L.call('zs_gru_fwd', 'ZsGruFwd', self.stream, dtype=L.ZS_BF16, B=B, T=T, H=H, gi=L.ptr(self.gi), ldgi=6 * H,
               whh=L.ptr(self.whh), ldw=H, n_pad=3 * H, w_gstride=3 * H * H, bhh=L.ptr(self.bhh), bhh_gstride=3 * H,
               out=L.ptr(out), ldo=ldo, out_col=out_col, gates=L.ptr(gates), work=L.ptr(self.work),
               work_bytes=self.work.numel() * 4, whh_interleaved=1,
               bcast_vec=L.ptr(self.vec) if bcast else None, bcast_ld=self.vec.shape[1] if bcast else 0,
               bcast_idx=L.ptr(self.idx) if bcast else None, bcast_col=out_col + 2 * H if bcast else 0, dir1_forward=dir1)
        torch.cuda.synchronize()
        return out.view(B, T, ldo), gates

    def bwd(self, rows, out_col, gates, dout_col=0, extra=0):
        """One zs_gru_bwd over the forward's rows and tape.  Returns (dgi, dgh) [B, T, 6H]."""
        L, B, T, H = self.L, self.B, self.T, self.H
        ldd = dout_col + 2 * H + extra
        dcat = filled(B * T * ldd, self.dev).view(B, T, ldd)
        dcat[:, :, dout_col:dout_col + 2 * H] = self.dout.to(self.dev)
        dgi, dgh = filled(B * T * 6 * H, self.dev), filled(B * T * 6 * H, self.dev)
        L.call('zs_gru_bwd', 'ZsGruBwd', self.stream, dtype=L.ZS_BF16, B=B, T=T, H=H, dout=L.ptr(dcat), ldd=ldd, dout_col=dout_col,
               out=L.ptr(rows), ldo=rows.shape[2], out_col=out_col, gates=L.ptr(gates), whh_t=L.ptr(self.whh_t), ldw=3 * H,
               n_pad=H, w_gstride=3 * H * H, dgi=L.ptr(dgi), ldgi=6 * H, dgh=L.ptr(dgh), ldgh=6 * H, work=L.ptr(self.work),
               work_bytes=self.work.numel() * 4)
        torch.cuda.synchronize()
        return dgi.view(B, T, 6 * H), dgh.view(B, T, 6 * H)


def same(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize('B,T', SHAPES)
def test_forward_bit_equal_to_the_wide_path_and_work_untouched(L, B, T):
    p = Problem(L, B, T, 100 * B + T)
    assert solo(L, 0, L.ZS_BF16, B, T, H) == 1
    assert G.query(L, 0, 'bf16', B, T, H, 1, 1) == ('WIDE', 0)
    for tape, bcast, dir1, (out_col, extra) in itertools.product((True, False), (False, True), (0, 1), ((0, 0), (40, 24))):
        kw = dict(tape=tape, bcast=bcast, dir1=dir1, out_col=out_col, extra=extra)
        before = p.fill_work()
        rows, gates = p.fwd(**kw)
        assert torch.equal(p.work, before), ('solo forward wrote the work buffer', kw)
        assert p.check() == L.ZS_OK, L.last_error()
        rows2, gates2 = p.fwd(**kw)
        with G.knobs(L, gru_solo_max_h=0):
            assert solo(L, 0, L.ZS_BF16, B, T, H) == 0 and G.query(L, 0, 'bf16', B, T, H, 1, 1) == ('WIDE', 0)
            rows_w, gates_w = p.fwd(**kw)
            assert p.check() == L.ZS_OK, L.last_error()
        assert same(rows, rows2), ('two solo forward runs differ', kw)
        assert same(rows, rows_w), ('solo forward out differs from the wide path', kw)
        if tape:
            assert same(gates, gates2) and same(gates, gates_w), ('gate tape', kw)
        # the launch wrote what it owns and nothing else
        raw = rows.view(torch.int16)
        h = rows[:, :, out_col:out_col + 2 * H].float()
        assert torch.isfinite(h).all() and (h.abs() <= 1).all()
        assert (raw[:, :, :out_col] == FILL).all() and (raw[:, :, rows.shape[2] - extra:] == FILL).all(), kw
        if bcast:
            want = p.vec[:, :2 * H].to(torch.bfloat16)[p.idx].unsqueeze(1).expand(B, T, 2 * H)
            assert torch.equal(rows[:, :, out_col + 2 * H:out_col + 4 * H], want), kw


@pytest.mark.parametrize('B,T', SHAPES)
def test_backward_bit_equal_to_the_wide_path_and_work_untouched(L, B, T):
    p = Problem(L, B, T, 100 * B + T + 7)
    assert solo(L, 1, L.ZS_BF16, B, T, H) == 1 and solo(L, 1, L.ZS_BF16, B, T, H, inter=0) == 1
    assert G.query(L, 1, 'bf16', B, T, H, 1, 1) == ('WIDE', 0)
    for (out_col, extra), (dout_col, dextra) in (((0, 0), (0, 0)), ((40, 24), (16, 8))):
        rows, gates = p.fwd(out_col=out_col, extra=extra)
        kw = dict(out_col=out_col, dout_col=dout_col, extra=dextra)
        before = p.fill_work()
        dgi, dgh = p.bwd(rows, gates=gates, **kw)
        assert torch.equal(p.work, before), ('solo BPTT wrote the work buffer', kw)
        assert p.check() == L.ZS_OK, L.last_error()
        dgi2, dgh2 = p.bwd(rows, gates=gates, **kw)
        with G.knobs(L, gru_solo_max_h=0):
            assert solo(L, 1, L.ZS_BF16, B, T, H) == 0 and G.query(L, 1, 'bf16', B, T, H, 1, 1) == ('WIDE', 0)
            dgi_w, dgh_w = p.bwd(rows, gates=gates, **kw)
            assert p.check() == L.ZS_OK, L.last_error()
        assert same(dgi, dgi2) and same(dgh, dgh2), ('two solo BPTT runs differ', kw)
        assert same(dgi, dgi_w), ('solo dgi differs from the wide path', kw)
        assert same(dgh, dgh_w), ('solo dgh differs from the wide path', kw)
        assert torch.isfinite(dgi.float()).all() and torch.isfinite(dgh.float()).all()


def test_fp64_forward_and_backward(L):
    """B = 40, T = 16 against the per-step fp64 recurrences and the wide bf16 bounds of tests/test_gpu_gru.py."""
    B, T = 40, 16
    p = Problem(L, B, T, 4016)
    assert solo(L, 0, L.ZS_BF16, B, T, H) == 1 and solo(L, 1, L.ZS_BF16, B, T, H) == 1
    rows, gates = p.fwd(out_col=40, extra=24)
    dgi, dgh = p.bwd(rows, 40, gates, dout_col=16, extra=8)
    stats = {}
    h = G.host(rows[:, :, 40:40 + 2 * H])
    gh = G.host(gates.view(B, T, 2, 4, H))
    G.check_fwd('bf16', H, h, G.host(p.gi), p.W, G.host(p.bhh), gh, stats)
    G.check_bwd('bf16', H, h, gh, p.dout.double(), G.host(dgi), G.host(dgh), p.W, stats)
    print('\n[err] solo B=%d T=%d, fraction of the bound: %s' % (B, T, ', '.join('%s %.2f' % kv for kv in sorted(stats.items()))))
    assert {'fwd h', 'fwd r', 'fwd z', 'fwd n', 'fwd hn', 'bwd dgi.dn', 'bwd dgh.dnr'} <= set(stats)


def test_plan_query(L):
    BF16, F32 = L.ZS_BF16, L.ZS_F32
    for pas in (0, 1):
        for B, T in SHAPES:
            assert solo(L, pas, BF16, B, T, H) == 1
            assert G.query(L, pas, 'bf16', B, T, H, 1, 1) == ('WIDE', 0)
        B, T = 40, 16
        assert solo(L, pas, BF16, B, T, 256) == 0 and G.query(L, pas, 'bf16', B, T, 256, 1, 1) == ('WIDE', 0)
        assert solo(L, pas, BF16, B, T, H, aligned=0) == 0
        assert G.query(L, pas, 'bf16', B, T, H, 1, 0) == ('PERSIST', 3 if pas else 1)
        assert solo(L, pas, F32, B, T, H) == 0 and G.query(L, pas, 'fp32', B, T, H, 1, 1) == ('PERSIST', 6 if pas else 2)
        assert solo(L, pas, BF16, B, 1, H) == 0 and G.query(L, pas, 'bf16', B, 1, H, 1, 1) == ('STEP_FUSED', 0)
        for knob in ('gru_solo_max_h', 'gru_spin_limit'):
            with G.knobs(L, **{knob: 0}):
                assert solo(L, pas, BF16, B, T, H) == 0, knob
                assert G.query(L, pas, 'bf16', B, T, H, 1, 1) == ('WIDE', 0), knob
        assert solo(L, pas, BF16, B, T, H) == 1


def test_same_xcd_group_placement_is_bit_equal(L):
    """"gru_xcd_groups": the hand-off kernels' grid with the group index fastest, taken when (row groups x 2) is a multiple of 8
    (B = 64: 4 row groups).  Placement only: forward and BPTT results are byte-identical to the unit-chunk-fastest grid's."""
    B, T, Hw = 64, 5, 256
    p = Problem(L, B, T, 6405, H=Hw)
    assert solo(L, 0, L.ZS_BF16, B, T, Hw) == 0 and G.query(L, 0, 'bf16', B, T, Hw, 1, 1) == ('WIDE', 0)
    res = {}
    for v in (0, 1):
        with G.knobs(L, gru_xcd_groups=v):
            rows, gates = p.fwd(bcast=True, out_col=40, extra=24)
            assert p.check() == L.ZS_OK, L.last_error()
            dgi, dgh = p.bwd(rows, 40, gates, dout_col=16, extra=8)
            assert p.check() == L.ZS_OK, L.last_error()
        res[v] = (rows, gates, dgi, dgh)
    for nm, a, b in zip(('out', 'gates', 'dgi', 'dgh'), res[0], res[1]):
        assert same(a, b), nm
    assert (res[1][0][:, :, 40:40 + 2 * Hw].float().abs() <= 1).all()

