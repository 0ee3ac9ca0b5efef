"""Restarting dead codewords on the device:

* zs_vq_restart alone against the numpy definition of tests/vq_restart_ref.py, bit for bit in code, m, N, cnorm and both counters: K = 1,
  fewer rows than dead codewords, an E above one round of the workgroup, K = 65536 (every word of the rank scan), the dead set empty,
  one codeword, every second codeword and all but one, with and without idx_acc and the device seed word, guards behind every array,
  a second launch after the seed word advanced, and every ZS_EINVAL case;
* a VqBottleneck with restart on over 8 steps on fixed rows against the definition, fed the device's idx, in fp32 and bf16;
* the AEStep with it, eager against captured, over 8 iterations; the step without it launching no zs_vq_restart; main.py --vq_restart
  end to end and a conversion with the codebook it wrote."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import vq_ref as R  # noqa: E402
import vq_restart_ref as S  # noqa: E402
import vq_train_ref as T  # noqa: E402

GUARD = 64
FILL_I = -0x55555556
THRESH = 0.1
F32 = np.float32
SHAPES = [(48, 8, 1), (37, 6, 5), (5, 20, 37), (300, 64, 300), (130, 1024, 129), (64, 8, 65536)]
DEAD_SETS = ('none', 'one', 'second', 'all_but_one')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _pitched(rows, ld, fill):
    n, E = rows.shape
    buf = np.full(n * ld + GUARD, fill, dtype=F32)
    buf[:n * ld].reshape(n, ld)[:, :E] = rows
    return buf


def _guarded(a, fill):
    a = np.ascontiguousarray(a)
    return np.concatenate([a.ravel(), np.full(GUARD, fill, dtype=a.dtype)])


def _signed(u):
    """An unsigned 64-bit value as the int64 that holds its bits."""
    u &= S.M64
    return u - (1 << 64) if u >= 1 << 63 else u


def _dead_state(K, which):
    """(cnt, N): the dead set asked for; the codewords outside it are kept alive in turn by a count beside a small N, by N equal to
    the threshold as fp32, by a NaN and by a large N."""
    ks = np.arange(K)
    dead = {'none': np.zeros(K, bool), 'one': ks == K // 2, 'second': ks % 2 == 1, 'all_but_one': ks != K // 3}[which]
    cnt = np.where(dead, 0, np.array([3, 0, 0, 1])[ks % 4]).astype(np.int32)
    N = np.where(dead, F32(0.01), np.array([0.001, F32(THRESH), np.nan, 1.0], dtype=F32)[ks % 4]).astype(F32)
    assert np.array_equal(S.dead(cnt, N, THRESH), dead)
    return cnt, N


class Launch(object):
    """zs_vq_restart on device copies of the arrays, a guard behind each; run() launches and checks the guards and the operands the
    kernel only reads."""

    def __init__(self, dev, x, ld_x, idx_acc, cnt, N, m, code, ld_code, cnorm, seed, seed_dev, stride):
        self.n, self.E = x.shape
        self.K, self.ld_code = len(N), ld_code
        self.xb, self.cb = _pitched(x, ld_x, np.nan), _pitched(code, ld_code, 0.125)
        self.x = torch.from_numpy(self.xb).to(dev)
        self.code = torch.from_numpy(self.cb).to(dev)
        self.ia_h = None if idx_acc is None else _guarded(np.asarray(idx_acc, np.int32), FILL_I)
        self.ia = None if idx_acc is None else torch.from_numpy(self.ia_h).to(dev)
        self.cnt_h = _guarded(np.asarray(cnt, np.int32), FILL_I)
        self.cnt = torch.from_numpy(self.cnt_h).to(dev)
        self.N = torch.from_numpy(_guarded(np.asarray(N, F32), -3.0)).to(dev)
        self.m = torch.from_numpy(_guarded(np.asarray(m, F32), -3.0)).to(dev)
        self.cnorm = torch.from_numpy(_guarded(np.asarray(cnorm, F32), -3.0)).to(dev)
        self.work = torch.full((self.K + 2 + GUARD,), FILL_I, dtype=torch.int32, device=dev)
        self.stat = torch.full((2 + GUARD,), 7, dtype=torch.int32, device=dev)
        self.seed_dev = None if seed_dev is None else torch.tensor([_signed(seed_dev), FILL_I], dtype=torch.int64, device=dev)
        from zs_amd import _lib as L
        self.kw = dict(thresh=THRESH, x=L.ptr(self.x), n=self.n, ld_x=ld_x, idx_acc=L.ptr(self.ia), cnt=L.ptr(self.cnt), K=self.K, E=self.E,
                       N=L.ptr(self.N), m=L.ptr(self.m), code=L.ptr(self.code), ld_code=ld_code, cnorm=L.ptr(self.cnorm), seed=seed,
                       seed_ptr=L.ptr(self.seed_dev), stride=stride, work=L.ptr(self.work), restarted=L.ptr(self.stat),
                       skipped=L.ptr(self.stat, 1))

    def run(self):
        from zs_amd import _lib as L
        K, E = self.K, self.E
        before = self.stat[:2].cpu().numpy().copy()
        L.call('zs_vq_restart', 'ZsVqRestart', _stream(), **self.kw)
        torch.cuda.synchronize()
        out = self.code.cpu().numpy()
        new = out[:K * self.ld_code].reshape(K, self.ld_code)[:, :E].copy()
        assert np.array_equal(out, _pitched(new, self.ld_code, 0.125))                  # the pad columns and the guard are not touched
        assert (self.N[K:] == -3.0).all() and (self.m[K * E:] == -3.0).all() and (self.cnorm[K:] == -3.0).all()
        assert (self.work[K + 2:] == FILL_I).all() and (self.stat[2:] == 7).all()
        assert np.array_equal(self.x.cpu().numpy(), self.xb, equal_nan=True) and np.array_equal(self.cnt.cpu().numpy(), self.cnt_h)
        assert self.ia is None or np.array_equal(self.ia.cpu().numpy(), self.ia_h)
        assert self.seed_dev is None or int(self.seed_dev[1]) == FILL_I
        d = self.stat[:2].cpu().numpy() - before
        return (self.N[:K].cpu().numpy(), self.m[:K * E].cpu().numpy().reshape(K, E), new, self.cnorm[:K].cpu().numpy()), int(d[0]), int(d[1])


def _same(got, want, what):
    for name, a, b in zip(('N', 'm', 'code', 'cnorm'), got, want):
        assert np.array_equal(_bits(a), _bits(b)), '%s: %s differs in %d places' % (what, name, (_bits(a) != _bits(b)).sum())


# ---- zs_vq_restart alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_seed_word', [False, True])
@pytest.mark.parametrize('with_idx_acc', [False, True])
@pytest.mark.parametrize('n,E,K', SHAPES)
def test_restart_equals_the_definition(dev, n, E, K, with_idx_acc, with_seed_word):
    """with_idx_acc: idx_acc is given, every fifth row left out; with_seed_word: the device seed word is given, and the rows and the
    codebook lie at pitches above E."""
    from zs_amd.vq_train import restart_stride
    x = R.planted(n, E, 8, 0.3, 1)
    code = R.planted(K, E, 8, 0.3, 101)
    m = (code * F32(0.5)).astype(F32)
    cn = R.cnorm(code)
    stride = restart_stride(n)
    ia = np.where(np.arange(n) % 5 == 2, -1, np.arange(n) % K).astype(np.int32) if with_idx_acc else None
    seed, seed_dev = 0x9E3779B97F4A7C15 + n, ((1 << 64) - 12345 if with_seed_word else None)      # (with it the sum wraps)
    ld_x, ld_code = (E + 3, E + 1) if with_seed_word else (E, E)
    counts = {}
    for which in DEAD_SETS:
        cnt, N = _dead_state(K, which)
        want, w_restarted, w_skipped, taken = S.restart(THRESH, x, ia, cnt, N, m, code, cn, seed, seed_dev or 0, stride)
        got, restarted, skipped = Launch(dev, x, ld_x, ia, cnt, N, m, code, ld_code, cn, seed, seed_dev, stride).run()
        _same(got, want, which)
        assert (restarted, skipped) == (w_restarted, w_skipped), which
        assert restarted + skipped == int(S.dead(cnt, N, THRESH).sum())
        counts[which] = (restarted, skipped)
        if which == 'none':
            _same(got, (N, m, code, cn), 'nothing dead')
    print('n %d E %d K %d idx_acc %d seed word %d: (restarted, skipped) %s' % (n, E, K, with_idx_acc, with_seed_word, counts))
    assert counts['none'] == (0, 0) and sum(counts['all_but_one']) == K - 1 and sum(counts['second']) == K // 2
    if with_idx_acc and K - 1 >= n:                                    # every row is asked for, a left-out one among them
        assert counts['all_but_one'][1] > 0
    if K - 1 > n:                                                 # more dead codewords than rows: a row is taken twice
        rs = [r for _, r in taken]
        assert len(set(rs)) < len(rs) and len(set(rs)) == len({r for r in range(n) if ia is None or ia[r] >= 0})


def test_a_second_launch_after_the_seed_word_advanced_takes_other_rows(dev):
    from zs_amd.vq_train import restart_stride
    n, E, K = 300, 64, 300
    x, code = R.planted(n, E, 8, 0.3, 1), R.planted(K, E, 8, 0.3, 101)
    cn, stride, seed = R.cnorm(code), restart_stride(n), 3
    cnt, N = _dead_state(K, 'second')
    step = next(d for d in range(1, 9) if S.start_row(seed, 10 + d, n) != S.start_row(seed, 10, n))       # (chosen on the CPU)
    run = Launch(dev, x, E, None, cnt, N, code, code, E, cn, seed, 10, stride)
    a, ra, _ = run.run()
    want_a, wa, _, taken_a = S.restart(THRESH, x, None, cnt, N, code, code, cn, seed, 10, stride)
    _same(a, want_a, 'first launch')
    # the same launch arguments; the device word moved, and the dead set is as it was
    run.seed_dev[0] += step
    run.N.copy_(torch.from_numpy(_guarded(N, -3.0)))
    b, rb, _ = run.run()
    want_b, wb, _, taken_b = S.restart(THRESH, x, None, cnt, N, want_a[1], want_a[2], want_a[3], seed, 10 + step, stride)
    _same(b, want_b, 'second launch')
    assert ra == wa == rb == wb == K // 2 and taken_a[0][1] != taken_b[0][1] and not np.array_equal(a[2], b[2])


def test_argument_errors_launch_nothing(dev):
    from zs_amd import _lib as L
    n, E, K = 50, 20, 7
    x = torch.full((n, E), 0.5, device=dev)
    ia = torch.zeros(n, dtype=torch.int32, device=dev)
    cnt = torch.zeros(K, dtype=torch.int32, device=dev)
    N, m, code, cn = (torch.full(s, v, device=dev) for s, v in (((K,), 0.125), ((K, E), 0.75), ((K, E), 0.25), ((K,), 1.25)))
    work = torch.full((K + 2,), FILL_I, dtype=torch.int32, device=dev)
    stat = torch.full((2,), 5, dtype=torch.int32, device=dev)
    sd = torch.zeros(2, dtype=torch.int64, device=dev)
    ok = dict(thresh=0.5, x=L.ptr(x), n=n, ld_x=E, idx_acc=L.ptr(ia), cnt=L.ptr(cnt), K=K, E=E, N=L.ptr(N), m=L.ptr(m), code=L.ptr(code),
              ld_code=E, cnorm=L.ptr(cn), seed=1, seed_ptr=L.ptr(sd), stride=31, work=L.ptr(work), restarted=L.ptr(stat), skipped=L.ptr(stat, 1))
    for change in (dict(K=0), dict(K=-1), dict(K=65537), dict(E=0), dict(E=1025), dict(n=-1), dict(n=2 ** 31), dict(ld_x=E - 1), dict(ld_code=E - 1),
                   dict(thresh=0.0), dict(thresh=1.0), dict(thresh=-0.5), dict(thresh=1.5), dict(thresh=float('nan')),
                   dict(stride=0), dict(stride=-1), dict(stride=n + 1),
                   dict(x=None), dict(cnt=None), dict(N=None), dict(m=None), dict(code=None), dict(cnorm=None), dict(work=None),
                   dict(restarted=None), dict(skipped=None),
                   dict(x=L.ptr(x) + 2), dict(idx_acc=L.ptr(ia) + 2), dict(cnt=L.ptr(cnt) + 2), dict(N=L.ptr(N) + 2), dict(m=L.ptr(m) + 2),
                   dict(code=L.ptr(code) + 1), dict(cnorm=L.ptr(cn) + 2), dict(seed_ptr=L.ptr(sd) + 4), dict(work=L.ptr(work) + 2),
                   dict(restarted=L.ptr(stat) + 2), dict(skipped=L.ptr(stat) + 6)):
        with pytest.raises(L.ZsError, match='zs_vq_restart'):
            L.call('zs_vq_restart', 'ZsVqRestart', _stream(), **dict(ok, **change))
    assert L.lib().zs_vq_restart(None, None) == L.ZS_EINVAL                 # a null struct
    # n == 0 succeeds and launches nothing, whatever the operands and the stride
    L.call('zs_vq_restart', 'ZsVqRestart', _stream(), **dict(ok, n=0, stride=0, x=None, cnt=None, N=None, m=None, code=None, cnorm=None, work=None,
                                                             restarted=None, skipped=None))
    torch.cuda.synchronize()
    assert (N == 0.125).all() and (m == 0.75).all() and (code == 0.25).all() and (cn == 1.25).all() and (work == FILL_I).all()
    assert (stat == 5).all() and (x == 0.5).all() and (ia == 0).all() and (cnt == 0).all() and (sd == 0).all()
    # the same operands are a valid launch: every codeword is dead
    L.call('zs_vq_restart', 'ZsVqRestart', _stream(), **ok)
    torch.cuda.synchronize()
    assert int(stat[0]) == 5 + K and int(stat[1]) == 5 and (N == 1.0).all() and (code == 0.5).all() and (m == 0.5).all() and (cn == 5.0).all()


# ---- the bottleneck over 8 steps -------------------------------------------------------------------------------------------------------
TB, TT, TE, TK, FAR = 4, 50, 8, 8, 6                              # 200 rows: the 1 % cap on near rows is 2 rows


def _trajectory_inputs(bf16):
    """Rows around two centres and a starting codebook (row 0, the row farthest from it, and 6 codewords at 1000) for which the fp64
    argmin alone keeps the near rows under the cap on every one of the 8 steps: the seed is searched on the CPU, before the device
    is asked anything.  (A codeword at 1000 has a squared norm of 8e6, whose fp32 spacing alone puts about 1 into vq_ref.bound: while
    one is there, a row is near unless its two live codewords differ by more than 2 in score, so the centres must lie well apart.)"""
    n = TB * TT
    shift, stride = R.vq_shift(n, T.MAX_ABS), S.stride(n)
    for seed in range(20):
        x = T.cast(R.planted(n, TE, 2, 0.3, seed), bf16)
        far_row = int(((x - x[0]) ** 2).sum(1).argmax())
        code = np.concatenate([x[[0, far_row]], np.full((FAR, TE), 1000.0, dtype=F32)])
        st, worst = T.State(code), 0
        for t in range(8):
            worst = max(worst, int(R.near_rows(x, st.code, st.cnorm).sum()))
            idx, _ = R.assign(x, st.code, st.cnorm)
            S.step(st, x, idx, shift, 0.5, THRESH, 5, t + 1, stride)
        if worst <= 0.01 * n:
            return x, code
    raise AssertionError('no seed below 20 keeps the near rows under the cap')


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_bottleneck_trajectory_equals_the_definition(dev, dtype):
    from zs_amd import _lib as L, layers
    from zs_amd.vq import VectorCodebook
    from zs_amd.vq_train import VqBottleneck
    bf16 = dtype == 'bf16'
    n = TB * TT
    x, code = _trajectory_inputs(bf16)
    ctx = layers.Ctx(dev, dtype)
    bn = VqBottleneck(VectorCodebook(code, {'enc_mode': 'continues'}), 0.25, 0.5, n, ctx, restart=THRESH)
    assert bn.stride == S.stride(n) and bn.restart == THRESH
    bits = ctx.act('traj_bits', TB, TT, TE)
    bits.view2d().zero_()
    bits.view2d()[:, :TE] = torch.from_numpy(x).to(dev).to(ctx.tdt)
    sd = torch.zeros(1, dtype=torch.int64, device=dev)
    st = T.State(code)
    total = 0
    for t in range(8):
        sd += 1
        code_before, cn_before = st.code.copy(), st.cnorm.copy()
        bn.forward(bits, seed=5, seed_ptr=L.ptr(sd))
        torch.cuda.synchronize()
        idx = bn.idx.cpu().numpy()
        near = R.near_rows(x, code_before, cn_before)
        want_idx, _ = R.assign(x, code_before, cn_before)
        assert near.sum() <= 0.01 * n and np.array_equal(idx[~near], want_idx[~near]), 'step %d' % (t + 1)
        assert np.array_equal(_bits(bn.code_live.cpu().numpy()), _bits(code_before))     # the step read the codebook of the step before
        cnt, used, restarted, skipped, taken = S.step(st, x, idx, bn.shift, 0.5, THRESH, 5, t + 1, bn.stride)
        total += restarted
        _same((bn.N.cpu().numpy(), bn.m.cpu().numpy(), bn.code.cpu().numpy(), bn.cnorm.cpu().numpy()), (st.N, st.m, st.code, st.cnorm),
              'step %d' % (t + 1))
        s = bn.stats()
        assert (s['restarts'], s['skipped'], s['used']) == (total, 0, used) and skipped == 0
        assert s['dead'] == int((st.N < F32(THRESH)).sum())
        print('%s step %d: used %d, restarted %d (rows %s), dead now %d' % (dtype, t + 1, used, restarted, [r for _, r in taken], s['dead']))
        if t < 3:                                                # N of the far codewords: 0.5, 0.25, 0.125: above the threshold
            assert total == 0 and (st.N[TK - FAR:] == F32(0.5) ** (t + 1)).all() and (st.code[TK - FAR:] == 1000.0).all()
        if t == 3:                                               # 0.0625: dead after the fourth step and not before
            assert restarted >= FAR and {k for k, _ in taken} >= set(range(TK - FAR, TK)) and (st.N[TK - FAR:] == 1.0).all()
            rows_taken = len({r for _, r in taken})
        if t == 4:                                               # a codeword that sits on a row wins that row
            assert used >= rows_taken
    assert total >= FAR


# ---- the step ------------------------------------------------------------------------------------------------------------------------
NS = 0.01
SIZES = dict(c_in=80, c_h1=16, c_h2=32, c_h3=16, E=8, c_h=32, n_spk=4, seg_len=128)          # tests/test_gpu_encmodes.py's small model


def _nets(dev, dtype='fp32', seed=0, dp=0.0):
    from zs_amd.model import Decoder, Encoder
    s = SIZES
    torch.manual_seed(seed)
    enc = Encoder(c_in=s['c_in'], c_h1=s['c_h1'], c_h2=s['c_h2'], c_h3=s['c_h3'], ns=NS, dp=dp, enc_size=s['E'], seg_len=s['seg_len'],
                  enc_mode='continues', dtype=dtype).to(dev)
    dec = Decoder(c_in=s['E'], c_out=s['c_in'], c_h=s['c_h'], c_a=s['n_spk'], ns=NS, seg_len=s['seg_len'], dtype=dtype).to(dev)
    return enc, dec


def _bottleneck(dev, vectors, rows, decay=0.5, dtype='fp32', restart=THRESH):
    from zs_amd import layers
    from zs_amd.vq import VectorCodebook
    from zs_amd.vq_train import VqBottleneck
    return VqBottleneck(VectorCodebook(np.ascontiguousarray(vectors, F32), {'enc_mode': 'continues'}), 0.25, decay, rows,
                        layers.Ctx(dev, dtype), restart=restart)


def _far_codebook():
    """7 codewords: 3 near the encoder's rows, 4 at 1000, which no row takes."""
    return np.concatenate([R.planted(3, SIZES['E'], 4, 0.3, 2) * F32(0.1), np.full((4, SIZES['E']), 1000.0, dtype=F32)])


def _run_eight(dev, graph_warmup, dtype):
    from zs_amd.trainer import AEStep
    enc, dec = _nets(dev, dtype=dtype, seed=0, dp=0.5)
    B, Tn = 4, 32
    bn = _bottleneck(dev, _far_codebook(), B * 4, dtype=dtype)
    ae = AEStep(enc, dec, lr=1e-3, max_grad_norm=5.0, use_graph=True, vq=bn)
    ae.graph_warmup = graph_warmup
    g = torch.Generator().manual_seed(1)
    losses, restarts = [], []
    for _ in range(8):
        x = torch.rand(B, Tn, SIZES['c_in'], generator=g).to(dev)
        c = torch.randint(0, SIZES['n_spk'], (B,), generator=g).to(dev)
        losses.append((ae.step(x, c).item(), bn.loss.item()))
        restarts.append(bn.stats()['restarts'])
    torch.cuda.synchronize()
    state = [enc.flat_params()[0], dec.flat_params()[0]] + [getattr(ae.opt[k], a) for k in ('enc', 'dec') for a in ('m', 'v')] + \
        [bn.code, bn.cnorm, bn.N, bn.m, bn.idx, bn.stat]
    return losses, restarts, [t.clone() for t in state], len(ae._graphs)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_captured_step_equals_eager_with_restarts(dev, dtype):
    la, ra, sa, na = _run_eight(dev, 2, dtype)
    lb, rb, sb, nb = _run_eight(dev, 10 ** 9, dtype)
    assert na == 1 and nb == 0
    assert la == lb, (la, lb)
    assert ra == rb and ra[2] == 0 and ra[3] >= 4 and ra[-1] > 0, ra        # the four far codewords die on the fourth step
    for a, b in zip(sa, sb):
        assert torch.equal(a, b)
    assert all(np.isfinite(v) and v > 0 for l in la for v in l)
    assert float(sa[6].abs().max()) < 100.0                                 # no codeword is left at 1000


def test_a_step_without_restart_never_calls_the_entry_point(dev, monkeypatch):
    from zs_amd import _lib as L
    from zs_amd.trainer import AEStep
    names = []
    real_call = L.call
    monkeypatch.setattr(L, 'call', lambda fname, *a, **k: (names.append(fname), real_call(fname, *a, **k))[1])
    enc, dec = _nets(dev, seed=0)
    bn = _bottleneck(dev, _far_codebook(), 12, restart=None)
    assert bn.restart is None and not hasattr(bn, 'rwork') and not hasattr(bn, 'stride') and bn.stat.numel() == 4
    ae = AEStep(enc, dec, lr=1e-4, max_grad_norm=5.0, use_graph=False, vq=bn)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(3, 32, SIZES['c_in'], generator=g).to(dev)
    c = torch.randint(0, SIZES['n_spk'], (3,), generator=g).to(dev)
    for _ in range(5):
        ae.step(x, c)
    ae._execute(ae.plan(x, c, False, True), counted=True)                              # the counted plan too
    torch.cuda.synchronize()
    vq_calls = [n for n in names if n.startswith('zs_vq')]
    assert len(vq_calls) == 30 and 'zs_vq_restart' not in vq_calls
    s = bn.stats()
    assert 'restarts' not in s and 'dead' not in s and float(bn.code.abs().max()) == 1000.0     # dead codewords stay where they are
    ae.vq = _bottleneck(dev, _far_codebook(), 12)
    del names[:]
    ae.step(x, c)
    torch.cuda.synchronize()
    assert [n for n in names if n.startswith('zs_vq')] == ['zs_vq_assign', 'zs_vq_commit', 'zs_vq_accum', 'zs_vq_ema', 'zs_vq_restart',
                                                           'zs_vq_st_bwd']


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_main_vq_restart_then_convert_with_the_trained_codebook(dev, tmp_path, monkeypatch, capsys):
    from scipy.io import wavfile
    sys.path.insert(0, ROOT)
    import main as M
    from zs_amd import convert as cv, layers, vq as V
    from zs_amd.hps import hp
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('ZS_CKPT_EVERY', '5')
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    h = json.load(open(os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')))
    h.update(n_speakers=4, n_target_speakers=2, batch_size=4, enc_pretrain_iters=5, max_to_keep=3, enc_size=8, emb_size=32, seg_len=32)
    hps_path = str(tmp_path / 'hps.json')
    json.dump(h, open(hps_path, 'w'))
    K = 6
    start = str(tmp_path / 'K6.vq.npz')
    vectors = np.concatenate([R.planted(K - 2, 8, 4, 0.3, 4) * F32(0.1), np.full((2, 8), 1000.0, dtype=F32)])      # two that no row takes
    V.VectorCodebook(vectors, {'enc_mode': 'continues', 'seed': 0}).save(start)
    ck = tmp_path / 'ck'
    M.main(['--train_ae', '--synthetic', '--enc_mode', 'continues', '--hps_path', hps_path, '--ckpt_dir', str(ck), '--dtype', 'fp32',
            '--vq_train', start, '--vq_decay', '0.5', '--vq_restart', '0.1'])
    out = capsys.readouterr().out
    assert 'pre_AE:[000005/000005]' in out and 'perplexity=' in out and ', restarts=' in out
    cb_path = str(ck / 'model.pth-ae-5.vq.npz')
    cb = V.load_codebook(cb_path, 'continues', E=8)
    assert (cb.K, cb.E) == (K, 8) and cb.meta['trained_iterations'] == 5 and cb.meta['decay'] == 0.5
    assert cb.meta['restart'] == 0.1 and cb.meta['restarts'] >= 2 and np.abs(cb.vectors).max() < 100.0
    d = tmp_path / 'in'
    d.mkdir()
    rng = np.random.RandomState(5)
    for i, n in enumerate((9000, 12000)):
        t = np.arange(n) / 16000.0
        y = 0.3 * np.sin(2 * np.pi * (200.0 + 150.0 * i + 400.0 * t) * t) + 0.05 * rng.randn(n)
        wavfile.write(str(d / ('w%d.wav' % i)), 16000, (y * 32767).astype(np.int16))
    s2id = str(tmp_path / 'speaker2id.json')
    json.dump({'S015': 0, 'S020': 1, 'V001': 2, 'V002': 3}, open(s2id, 'w'))
    monkeypatch.setattr(hp, 'n_iter', 4)
    res = tmp_path / 'result'
    M.main(['--convert_dir', str(d), '--t_speaker', 'V001', '--result_dir', str(res), '--codebook', cb_path, '--enc_only', '--hps_path', hps_path,
            '--speaker2id_path', s2id, '--ckpt_pth', str(ck / 'model.pth-ae-5'), '--enc_mode', 'continues', '--g_mode', 'targeted_residual'])
    conv = os.path.join(os.path.join(str(res), './english/'), 'convert')
    for s in ('w0', 'w1'):
        idx = cv.read_indices(os.path.join(conv, 'V001', s + '.idx.txt'), K)           # raises for an index outside [0, K)
        assert len(idx) >= 2 and idx.min() >= 0 and idx.max() < K
        assert os.path.getsize(os.path.join(conv, 'V001', s + '.wav')) > 44
    layers.check_status(dev)
