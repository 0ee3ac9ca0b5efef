"""Quantiser dropout on the device:

* zs_rvq_drop_draw, zs_rvq_commit_drop and zs_rvq_gather_frag against the numpy definition of tests/rvq_drop_ref.py, bit for bit (the
  loss through zs_rvq_loss within 1e-6 of fp64), on the smallest shapes that cross one row, a wave that holds rows of several samples
  with different counts, eight stages, one 64-lane team over several rounds and more samples than a workgroup has rows, in fp32 and bf16,
  at three pitches, with the counts all S, all 1 and mixed; counts outside [1, S], bad indices and rows at ZS_VQ_MAX_ABS at stages a
  sample uses and at stages it does not, every ZS_EINVAL case, all with guards around every output; with every count at S the kernels
  against zs_rvq_commit and zs_rvq_gather;
* RvqBottleneck(dropout=P).forward against the definition, one AEStep iteration against the oracle's torch modules under autograd,
  eager against captured over 5 iterations, and main.py --rvq_train --rvq_dropout end to end.
The helpers that have nothing to do with dropout are tests/test_gpu_rvq_train.py's."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import rvq_drop_ref as D  # noqa: E402
import rvq_train_ref as RT  # noqa: E402
import test_gpu_rvq_train as G  # noqa: E402
import vq_ref as R  # noqa: E402
import vq_train_ref as T  # noqa: E402

F32 = np.float32
GUARD, FILL_I = G.GUARD, G.FILL_I
SHAPES = [(3, 1, 1, 1, 1), (5, 7, 6, 5, 3), (4, 16, 20, 37, 8), (2, 65, 1024, 129, 2), (300, 1, 64, 300, 4)]     # (B, T', E, K, S)
LD = {1: 8, 6: 8, 20: 24, 64: 72, 1024: 1024}                     # the Decoder-side operand's pitch (a multiple of 8)
_same, _stream, _pitched, _unpitch = G._same, G._stream, G._pitched, G._unpitch


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


def _patterns(B, S):
    """all S, all 1, mixed: sample b uses 1 + (b + 1) mod S stages (neighbours differ wherever S > 1)."""
    return (('all', np.full(B, S, np.int32)), ('one', np.ones(B, np.int32)), ('mixed', (1 + (np.arange(B) + 1) % S).astype(np.int32)))


_CASES = {}


def _case(B, Tq, E, K, S, bf16):
    """(x, codes) and, per pattern, the chain of the definition under zs_vq_assign's own indices: computed once, shared, never changed."""
    key = (B, Tq, E, K, S, bf16)
    if key not in _CASES:
        _CASES[key] = dict(xc=G._case(B * Tq, E, K, S, bf16), chains={})
    return _CASES[key]


def _chain(dev, B, Tq, E, K, S, bf16, name, s_use):
    """[(stage input r, idx of zs_vq_assign on all rows, a before, the definition's commit)] per stage."""
    case = _case(B, Tq, E, K, S, bf16)
    if name not in case['chains']:
        x, codes = case['xc']
        r, a, out = x, None, []
        for s in range(S):
            idx = G._assign(dev, r, codes[s], bf16 and s == 0)
            want = D.commit(r, idx, codes[s], a, D.row_mask(s_use, Tq, len(x), s))
            out.append((r, idx, a, want))
            r, a = want['r'], want['a']
        case['chains'][name] = out
    return case['chains'][name]


def _commit(dev, x, src_bf16, idx, code, a_in, ld, s_use, Tq, stage, want_xf=True, partial=None, change=None, run_bf16=None, plain=False):
    """zs_rvq_commit_drop (plain: zs_rvq_commit on the same operands) on rows x with NaN behind every output; a_in None: the first
    stage.  Returns numpy results and asserts the guards and the read-only operands."""
    from zs_amd import _lib as L
    n, E = x.shape
    K = code.shape[0]
    ld_x, ld_code, ld_r, ld_a, ld_xf = ld
    xb, cb = _pitched(x, ld_x), _pitched(code, ld_code)
    x_d = torch.from_numpy(xb).to(dev).to(torch.bfloat16 if src_bf16 else torch.float32)
    c_d = torch.from_numpy(cb).to(dev)
    ib = np.concatenate([np.asarray(idx, np.int32), np.full(GUARD, FILL_I, np.int32)])
    i_d = torch.from_numpy(ib).to(dev)
    sb = np.concatenate([np.asarray(s_use, np.int32), np.full(GUARD, FILL_I, np.int32)])
    s_d = torch.from_numpy(sb).to(dev)
    r_d = torch.full((n * ld_r + GUARD,), np.nan, device=dev)
    f_d = torch.full((n * ld_xf + GUARD,), np.nan, device=dev)
    a_d = torch.from_numpy(_pitched(a_in if a_in is not None else np.full((n, E), np.nan, F32), ld_a)).to(dev)
    ia = torch.full((n + GUARD,), FILL_I, dtype=torch.int32, device=dev)
    part = partial if partial is not None else torch.full((L.ZS_VQ_COMMIT_PARTS + GUARD,), np.nan, dtype=torch.float64, device=dev)
    stat = torch.full((4,), 7, dtype=torch.int32, device=dev)
    run_bf16 = src_bf16 if run_bf16 is None else run_bf16
    kw = dict(dtype=(L.ZS_BF16 if run_bf16 else L.ZS_F32), src_f32=int(run_bf16 and not src_bf16), first=int(a_in is None), x=L.ptr(x_d), n=n,
              ld_x=ld_x, idx=L.ptr(i_d), code=L.ptr(c_d), ld_code=ld_code, K=K, E=E, r=L.ptr(r_d), ld_r=ld_r, x_f32=(L.ptr(f_d) if want_xf else None),
              ld_xf=(ld_xf if want_xf else 0), idx_acc=L.ptr(ia), a=L.ptr(a_d), ld_a=ld_a, partial=L.ptr(part), bad=L.ptr(stat), over=L.ptr(stat, 1))
    if plain:
        L.call('zs_rvq_commit', 'ZsRvqCommit', _stream(), **kw)
    else:
        kw.update(s_use=L.ptr(s_d), rows_per_frag=Tq, stage=stage)
        kw.update(change or {})
        L.call('zs_rvq_commit_drop', 'ZsRvqCommitDrop', _stream(), **kw)
    torch.cuda.synchronize()
    r, ok_r = _unpitch(r_d, n, ld_r, E)
    a, ok_a = _unpitch(a_d, n, ld_a, E)
    f, ok_f = _unpitch(f_d, n, ld_xf, E)
    assert ok_r and ok_a and ok_f and (ia[n:] == FILL_I).all() and (stat[2:] == 7).all()
    if partial is None:
        assert torch.isnan(part[L.ZS_VQ_COMMIT_PARTS:]).all() and not torch.isnan(part[:L.ZS_VQ_COMMIT_PARTS]).any()
    assert np.array_equal(c_d.cpu().numpy(), cb, equal_nan=True) and np.array_equal(i_d.cpu().numpy(), ib) and np.array_equal(s_d.cpu().numpy(), sb)
    assert np.array_equal(x_d.float().cpu().numpy(), xb, equal_nan=True)
    if not want_xf:
        assert np.isnan(f).all()
    parts = part[:L.ZS_VQ_COMMIT_PARTS].cpu().numpy().copy()
    return dict(r=r, a=a, x_f32=f, idx_acc=ia[:n].cpu().numpy(), sq=float(parts.sum()), parts=parts, bad=int(stat[0]) - 7, over=int(stat[1]) - 7)


# ---- zs_rvq_drop_draw ----------------------------------------------------------------------------------------------------------------
def _draw(dev, seed, word, B, S, thr, Tq, change=None):
    """(s_use, active) of zs_rvq_drop_draw; word: the uint64 at seed_ptr (None: no seed_ptr)."""
    from zs_amd import _lib as L
    s_d = torch.full((B + GUARD,), FILL_I, dtype=torch.int32, device=dev)
    a_d = torch.full((S + GUARD,), FILL_I, dtype=torch.int32, device=dev)
    w_d = None if word is None else torch.tensor([word - (1 << 64) if word >= 1 << 63 else word], dtype=torch.int64, device=dev)
    kw = dict(seed=seed, seed_ptr=L.ptr(w_d), thr=thr, S=S, n_frag=B, rows_per_frag=Tq, s_use=L.ptr(s_d), active=L.ptr(a_d))
    kw.update(change or {})
    L.call('zs_rvq_drop_draw', 'ZsRvqDropDraw', _stream(), **kw)
    torch.cuda.synchronize()
    assert (s_d[B:] == FILL_I).all() and (a_d[S:] == FILL_I).all()
    return s_d[:B].cpu().numpy(), a_d[:S].cpu().numpy()


@pytest.mark.parametrize('B,Tq,S', [(1, 1, 1), (3, 1, 1), (5, 7, 3), (4, 16, 8), (2, 65, 2), (300, 1, 4), (4096, 3, 4), (1000, 5, 7)])
def test_draw_equals_the_definition_with_and_without_seed_ptr(dev, B, Tq, S):
    """Every sample's count and every stage's active rows, at P = 0.5, 1, 0.3 and 2^-24; seeds whose sum wraps around 2^64; more
    samples than the workgroup has lanes."""
    seen = set()
    for P in (0.5, 1.0, 0.3, 2.0 ** -24):
        thr = D.threshold(P)
        for seed, word in ((0, None), (7, None), (0, 0), (3, 0x123456789ABCDEF0), (2 ** 64 - 1, 5), (2 ** 63 + 11, 2 ** 64 - 3)):
            s_use, active = _draw(dev, seed, word, B, S, thr, Tq)
            want = D.draw(seed, word or 0, B, S, thr)
            assert np.array_equal(s_use, want) and s_use.dtype == np.int32, (P, seed, word)
            assert np.array_equal(active, D.active(want, S, Tq)) and active[0] == B * Tq
            seen.update(s_use.tolist())
            if P == 2.0 ** -24 and B < 1000:
                assert (s_use == S).all()
    assert seen <= set(range(1, S + 1)) and (B < 100 or seen == set(range(1, S + 1)))
    if B == 4096:                                                               # tests/test_rvq_drop_host.py's written-down counts
        assert np.bincount(_draw(dev, 0, 0, B, S, D.threshold(0.5), Tq)[0], minlength=5).tolist() == [0, 498, 555, 549, 2494]


# ---- zs_rvq_commit_drop --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('B,Tq,E,K,S', SHAPES)
def test_commit_equals_the_definition_over_the_chain(dev, B, Tq, E, K, S, bf16):
    """Stage 0 reads the rows in the compute dtype, every later stage the fp32 residual the stage before wrote (an inactive row: the
    copy); each stage's index is zs_vq_assign's of its own input, on all rows.  r, a, idx_acc and the fp32 copy bit for bit at three
    pitches and three patterns of counts; the sum of squares within 1e-12."""
    n = B * Tq
    x, codes = _case(B, Tq, E, K, S, bf16)['xc']
    for name, s_use in _patterns(B, S):
        chain = _chain(dev, B, Tq, E, K, S, bf16, name, s_use)
        for ld in G._pitches(E, bf16):
            for s, (r, idx, a, want) in enumerate(chain):
                got = _commit(dev, r, bf16 and s == 0, idx, codes[s], a, ld, s_use, Tq, s, want_xf=(s == 0), run_bf16=bf16)
                where = '%s stage %d ld %s' % (name, s, ld)
                assert _same(got['r'], want['r']) and _same(got['a'], want['a']), where
                act = D.row_mask(s_use, Tq, n, s)
                assert np.array_equal(got['idx_acc'], np.where(act, idx, -1)) and np.array_equal(got['idx_acc'], want['idx_acc']), where
                assert got['bad'] == 0 and got['over'] == 0 and abs(got['sq'] - want['sq']) <= 1e-12 * want['sq'], where
                assert _same(got['r'][~act], r[~act]) and (s == 0 or _same(got['a'][~act], a[~act]))      # the copy; a untouched
                if not act.any():
                    assert (got['parts'] == 0).all()
                if s == 0:
                    assert _same(got['x_f32'], x) and act.all()
        if name == 'mixed' and S > 1:
            last = chain[-1][3]
            full = RT.cascade(x, codes, idxs=[c[1] for c in chain])
            assert not np.array_equal(last['a'], full['a']) or n == 1           # the mask shows in what the backward reads


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('B,Tq,E,K,S', SHAPES)
def test_loss_partials_through_zs_rvq_loss_are_within_1e_6_of_fp64(dev, B, Tq, E, K, S, bf16):
    """tests/test_gpu_rvq_train.py's bound for loss_vq: relative 1e-6 against the fp64 sum of the stored residuals squared of the rows
    that took part, total and per stage, scaled over all n rows."""
    from zs_amd import _lib as L
    n, beta = B * Tq, 0.25
    x, codes = _case(B, Tq, E, K, S, bf16)['xc']
    P = L.ZS_VQ_COMMIT_PARTS
    for name, s_use in _patterns(B, S)[1:]:
        part = torch.full((S * P + GUARD,), np.nan, dtype=torch.float64, device=dev)
        chain = _chain(dev, B, Tq, E, K, S, bf16, name, s_use)
        for s, (r, idx, a, want) in enumerate(chain):
            _commit(dev, r, bf16 and s == 0, idx, codes[s], a, G._pitches(E, bf16)[0], s_use, Tq, s, partial=part[s * P:], run_bf16=bf16)
        loss = torch.full((1 + S + 2,), np.nan, device=dev)
        L.call('zs_rvq_loss', 'ZsRvqLoss', _stream(), partial=L.ptr(part), S=S, scale=beta / (float(n) * E), loss=L.ptr(loss))
        torch.cuda.synchronize()
        assert torch.isnan(loss[1 + S:]).all() and torch.isnan(part[S * P:]).all()
        got = loss[:1 + S].cpu().numpy().astype(np.float64)
        total, per = RT.losses([c[3]['sq'] for c in chain], beta, n, E)
        worst = max(abs(g - w) / w if w > 0 else abs(g) for g, w in zip(got, [total] + per))
        print('%s B %d T %d E %d K %d S %d bf16 %d: loss_vq %.9g (fp64 %.9g), stages %s, worst relative error %.3g' %
              (name, B, Tq, E, K, S, bf16, got[0], total, got[1:], worst))
        assert total > 0 and per[0] > 0 and worst <= 1e-6
        for s in range(S):                                                      # a stage nobody used: an exact zero
            assert (per[s] == 0) == (not D.row_mask(s_use, Tq, n, s).any()) and (per[s] > 0 or got[1 + s] == 0)


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('B,Tq,E,K,S', SHAPES)
def test_with_every_count_at_s_commit_is_zs_rvq_commit(dev, B, Tq, E, K, S, bf16):
    """No dropout: r, a, idx_acc, the fp32 copy, every one of the 1024 partials and both counters, bit for bit, with bad indices and
    rows at the bound among them."""
    n = B * Tq
    x, codes = _case(B, Tq, E, K, S, bf16)['xc']
    s_use = np.full(B, S, np.int32)
    chain = _chain(dev, B, Tq, E, K, S, bf16, 'all', s_use)
    for s in sorted({0, S - 1}):
        r, idx, a, _ = chain[s]
        r, idx = r.copy(), idx.copy()
        idx[0], idx[n - 1] = K, -1
        r[n // 2, 0] = np.inf
        for ld in G._pitches(E, bf16)[::2]:
            args = (dev, r, bf16 and s == 0, idx, codes[s], a, ld, s_use, Tq, s)
            got, want = _commit(*args, want_xf=(s == 0), run_bf16=bf16), _commit(*args, want_xf=(s == 0), run_bf16=bf16, plain=True)
            for k in ('r', 'a', 'x_f32'):
                assert _same(got[k], want[k]), (k, s, ld)
            assert np.array_equal(got['idx_acc'], want['idx_acc']) and (got['bad'], got['over']) == (want['bad'], want['over'])
            assert np.array_equal(got['parts'].view(np.uint64), want['parts'].view(np.uint64)) and want['over'] == 1 and want['bad'] == 2


@pytest.mark.parametrize('bf16', [False, True])
def test_bad_input_moves_the_counters_only_where_the_row_takes_part(dev, bf16):
    """30 samples of 10 rows; the odd samples use stage 1, the even ones do not.  Indices outside [0, K) (2^30 would be far outside the
    codebook) and rows with 65536, -inf, -70000 and NaN in samples of either kind, at stage 1: the rows of the even samples are copied
    whatever they hold and nothing is counted; those of the odd ones behave as zs_rvq_commit's.  At stage 0 every row takes part."""
    B, Tq, E, K = 30, 10, 64, 300
    n = B * Tq
    x, codes = G._case(n, E, K, 2, bf16)
    s_use = (1 + np.arange(B) % 2).astype(np.int32)
    ld = G._pitches(E, bf16)[0]
    rows = x.copy()
    idx = G._assign(dev, rows, codes[1], False).copy()
    idx[3], idx[5], idx[130], idx[299] = K, -1, 2 ** 30, -2 ** 31              # samples 0, 0, 13, 29
    rows[9, 2], rows[11, 63], rows[200, 0], rows[130, 1], rows[150, 3] = 65536.0, -np.inf, np.nan, np.nan, -70000.0   # samples 0, 1, 20, 13, 15
    a_in = R.planted(n, E, 8, 0.3, 77)
    act = D.row_mask(s_use, Tq, n, 1)
    want = D.commit(rows, idx, codes[1], a_in, act)
    got = _commit(dev, rows, False, idx, codes[1], a_in, ld, s_use, Tq, 1, want_xf=False, run_bf16=bf16)
    assert want['bad'] == 2 and want['over'] == 3 and got['bad'] == 2 and got['over'] == 3
    assert _same(got['r'], want['r']) and _same(got['a'], want['a']) and np.array_equal(got['idx_acc'], want['idx_acc'])
    assert (got['idx_acc'][~act] == -1).all() and _same(got['r'][~act], rows[~act]) and _same(got['a'][~act], a_in[~act])
    assert (got['idx_acc'][[130, 299, 11, 150]] == -1).all() and _same(got['a'][[130, 299]], a_in[[130, 299]])
    assert got['sq'] == np.inf                                                  # (the infinite row of sample 1)
    rows[11, 63] = 0.0
    want = D.commit(rows, idx, codes[1], a_in, act)
    got = _commit(dev, rows, False, idx, codes[1], a_in, ld, s_use, Tq, 1, want_xf=False, run_bf16=bf16)
    assert abs(got['sq'] - want['sq']) <= 1e-12 * want['sq'] and got['over'] == 2 and got['bad'] == 2
    # stage 0: the same poison in the compute dtype, every row active -- zs_rvq_commit's definition
    rows0 = x.copy()
    rows0[9, 2], rows0[11, 63], rows0[200, 0], rows0[5, 1] = 65536.0, -np.inf, (-70144.0 if bf16 else -70000.0), np.nan
    idx0 = G._assign(dev, rows0, codes[0], bf16).copy()
    idx0[3], idx0[5], idx0[130], idx0[299] = K, -1, 2 ** 30, -2 ** 31
    want = RT.commit(rows0, idx0, codes[0], None)
    got = _commit(dev, rows0, bf16, idx0, codes[0], None, ld, s_use, Tq, 0, run_bf16=bf16)
    assert want['bad'] == 4 and want['over'] == 4 and got['bad'] == 4 and got['over'] == 4
    assert _same(got['r'], want['r']) and _same(got['a'], want['a']) and np.array_equal(got['idx_acc'], want['idx_acc']) and _same(got['x_f32'], rows0)


# ---- zs_rvq_gather_frag --------------------------------------------------------------------------------------------------------------
def _gather(dev, idx, codes, s_use, B, Tq, ld, bf16, change=None):
    """zs_rvq_gather_frag of B fragments of T' frames (s_use an array), or zs_rvq_gather (s_use an int): (q fp32 [n, ld], bad)."""
    from zs_amd import _lib as L
    S, n = idx.shape
    K, E = codes[0].shape
    dt = torch.bfloat16 if bf16 else torch.float32
    ib = np.concatenate([np.ascontiguousarray(idx, np.int32).reshape(-1), np.full(GUARD, FILL_I, np.int32)])
    i_d = torch.from_numpy(ib).to(dev)
    c_d = torch.from_numpy(np.stack(codes).astype(F32)).to(dev)
    start = torch.arange(B, dtype=torch.int64, device=dev) * Tq
    length = torch.full((B,), Tq, dtype=torch.int32, device=dev)
    dst = torch.full((n * ld + GUARD,), 9.0, dtype=dt, device=dev)
    bad = torch.full((3,), 7, dtype=torch.int32, device=dev)
    kw = dict(dtype=(L.ZS_BF16 if bf16 else L.ZS_F32), idx=L.ptr(i_d), n_idx=n, ld_idx=n, S=S, code=L.ptr(c_d), ld_code=E, plane_code=K * E, K=K, E=E,
              start=L.ptr(start), len=L.ptr(length), n_frag=B, T=Tq, dst=L.ptr(dst), ld_dst=ld, bad=L.ptr(bad))
    if isinstance(s_use, (int, np.integer)):
        L.call('zs_rvq_gather', 'ZsRvqGather', _stream(), s_use=int(s_use), **kw)
    else:
        sb = np.concatenate([np.asarray(s_use, np.int32), np.full(GUARD, FILL_I, np.int32)])
        s_d = torch.from_numpy(sb).to(dev)
        kw.update(s_use=L.ptr(s_d))
        kw.update(change or {})
        L.call('zs_rvq_gather_frag', 'ZsRvqGatherFrag', _stream(), **kw)
        torch.cuda.synchronize()
        assert np.array_equal(s_d.cpu().numpy(), sb)
    torch.cuda.synchronize()
    assert (dst[n * ld:] == 9.0).all() and (bad[1:] == 7).all() and np.array_equal(i_d.cpu().numpy(), ib)
    return dst[:n * ld].float().cpu().numpy().reshape(n, ld), int(bad[0]) - 7


def _planes(B, Tq, K, S, s_use, seed):
    """Random planes of indices; every plane a sample does not use holds 2^30 on its rows: read as an index it would be far outside."""
    idx = np.random.RandomState(seed).randint(0, K, (S, B * Tq)).astype(np.int32)
    for s in range(S):
        idx[s, ~D.row_mask(np.clip(s_use, 0, S), Tq, B * Tq, s)] = 2 ** 30
    return idx


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('B,Tq,E,K,S', SHAPES)
def test_gather_equals_the_definition_and_zs_rvq_gather(dev, B, Tq, E, K, S, bf16):
    """The operand bit for bit for the three patterns; the planes behind a sample's count are not read (they hold 2^30); with every
    count at s the operand and the bad count are zs_rvq_gather(s_use = s)'s, bad frames among them."""
    _, codes = _case(B, Tq, E, K, S, bf16)['xc']
    ld = LD[E]
    for name, s_use in _patterns(B, S):
        idx = _planes(B, Tq, K, S, s_use, B + S)
        want, wbad = D.operand(codes, idx, s_use, Tq, ld, bf16)
        got, bad = _gather(dev, idx, codes, s_use, B, Tq, ld, bf16)
        assert _same(got, want) and bad == wbad == 0, name
        assert (got[:, E:] == 0).all() and (E == 1 and K == 1 or np.abs(got[:, :E]).max() > 0)
    for s in sorted({1, S}):
        idx = np.random.RandomState(s).randint(0, K, (S, B * Tq)).astype(np.int32)
        idx[0, 0], idx[s - 1, B * Tq - 1] = K, -1
        want, wbad = _gather(dev, idx, codes, s, B, Tq, ld, bf16)
        got, bad = _gather(dev, idx, codes, np.full(B, s, np.int32), B, Tq, ld, bf16)
        assert _same(got, want) and bad == wbad == (1 if B * Tq == 1 else 2) and (got[0] == 0).all()


@pytest.mark.parametrize('bf16', [False, True])
def test_gather_a_count_outside_1_to_s_is_a_zero_fragment_counted_per_frame(dev, bf16):
    B, Tq, E, K, S = 5, 7, 6, 5, 3
    _, codes = _case(B, Tq, E, K, S, bf16)['xc']
    for s_use in ([0, 3, 4, 1, -5], [2 ** 30, 2, -2 ** 31, 3, S + 1]):
        s_use = np.array(s_use, np.int64).astype(np.int32)
        idx = np.random.RandomState(1).randint(0, K, (S, B * Tq)).astype(np.int32)
        out = ~((s_use >= 1) & (s_use <= S))
        idx[:, np.repeat(out, Tq)] = 2 ** 30                                    # no index of such a fragment is read
        want, wbad = D.operand(codes, idx, s_use, Tq, 8, bf16)
        got, bad = _gather(dev, idx, codes, s_use, B, Tq, 8, bf16)
        assert _same(got, want) and bad == wbad == 3 * Tq
        assert (got[np.repeat(out, Tq)] == 0).all() and np.abs(got[np.repeat(~out, Tq)][:, :E]).max() > 0


# ---- argument errors -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(dev):
    from zs_amd import _lib as L
    E, B, Tq, K, ld, S = 20, 5, 10, 7, 24, 2
    n = B * Tq
    x = torch.full((n, ld), 0.5, device=dev)
    code = torch.full((S, K, E), 0.25, device=dev)
    idx = torch.zeros(S, n, dtype=torch.int32, device=dev)
    r, zf, a = (torch.full((n, ld), v, device=dev) for v in (9.0, 8.0, 6.0))
    ia = torch.full((n,), -7, dtype=torch.int32, device=dev)
    part = torch.full((L.ZS_VQ_COMMIT_PARTS,), -1.0, dtype=torch.float64, device=dev)
    stat = torch.full((4,), 5, dtype=torch.int32, device=dev)
    s_use = torch.full((B + 1,), 2, dtype=torch.int32, device=dev)
    ok = dict(dtype=L.ZS_F32, src_f32=0, first=1, x=L.ptr(x), n=n, ld_x=ld, idx=L.ptr(idx), code=L.ptr(code), ld_code=E, K=K, E=E, r=L.ptr(r), ld_r=ld,
              x_f32=L.ptr(zf), ld_xf=ld, idx_acc=L.ptr(ia), a=L.ptr(a), ld_a=ld, partial=L.ptr(part), bad=L.ptr(stat), over=L.ptr(stat, 1),
              s_use=L.ptr(s_use), rows_per_frag=Tq, stage=0)
    for change in (dict(K=0), dict(K=-1), dict(K=65537), dict(E=0), dict(E=1025), dict(n=-1), dict(n=2 ** 31), dict(x=None), dict(idx=None),
                   dict(code=None), dict(r=None), dict(idx_acc=None), dict(a=None), dict(partial=None), dict(bad=None), dict(over=None),
                   dict(ld_x=E - 1), dict(ld_code=E - 1), dict(ld_r=E - 1), dict(ld_xf=E - 1), dict(ld_a=E - 1), dict(dtype=5),
                   dict(x=L.ptr(x) + 2), dict(dtype=L.ZS_BF16, x=L.ptr(x) + 1), dict(idx=L.ptr(idx) + 2), dict(code=L.ptr(code) + 1),
                   dict(r=L.ptr(r) + 2), dict(x_f32=L.ptr(zf) + 2), dict(a=L.ptr(a) + 1), dict(partial=L.ptr(part) + 4), dict(idx_acc=L.ptr(ia) + 1),
                   dict(r=L.ptr(x)), dict(a=L.ptr(x)), dict(x_f32=L.ptr(x)), dict(a=L.ptr(r)), dict(x_f32=L.ptr(r)), dict(x_f32=L.ptr(a)),
                   dict(idx_acc=L.ptr(idx)), dict(s_use=None), dict(s_use=L.ptr(s_use) + 2), dict(idx_acc=L.ptr(s_use)), dict(rows_per_frag=0),
                   dict(rows_per_frag=-1), dict(stage=-1), dict(stage=8), dict(stage=1), dict(first=0)):
        with pytest.raises(L.ZsError, match='zs_rvq_commit_drop'):
            L.call('zs_rvq_commit_drop', 'ZsRvqCommitDrop', _stream(), **dict(ok, **change))
    L.call('zs_rvq_commit_drop', 'ZsRvqCommitDrop', _stream(), **dict(ok, n=0, x=None, idx=None, code=None, r=None, a=None, idx_acc=None, partial=None,
                                                                      bad=None, over=None, s_use=None))        # n == 0 succeeds
    sw = torch.full((B,), -7, dtype=torch.int32, device=dev)
    act = torch.full((S,), -7, dtype=torch.int32, device=dev)
    word = torch.zeros(2, dtype=torch.int64, device=dev)
    okd = dict(seed=1, seed_ptr=L.ptr(word), thr=2 ** 23, S=S, n_frag=B, rows_per_frag=Tq, s_use=L.ptr(sw), active=L.ptr(act))
    for change in (dict(thr=0), dict(thr=-1), dict(thr=2 ** 24 + 1), dict(S=0), dict(S=9), dict(S=-1), dict(n_frag=0), dict(n_frag=-1),
                   dict(n_frag=2 ** 20 + 1), dict(rows_per_frag=0), dict(n_frag=2 ** 20, rows_per_frag=2 ** 11), dict(s_use=None), dict(active=None),
                   dict(s_use=L.ptr(sw) + 2), dict(active=L.ptr(act) + 1), dict(seed_ptr=L.ptr(word) + 4)):
        with pytest.raises(L.ZsError, match='zs_rvq_drop_draw'):
            L.call('zs_rvq_drop_draw', 'ZsRvqDropDraw', _stream(), **dict(okd, **change))
    dst = torch.full((B, Tq, ld), 9.0, device=dev)
    start = torch.arange(B, dtype=torch.int64, device=dev) * Tq
    length = torch.full((B,), Tq, dtype=torch.int32, device=dev)
    okg = dict(dtype=L.ZS_F32, idx=L.ptr(idx), n_idx=n, ld_idx=n, S=S, s_use=L.ptr(s_use), code=L.ptr(code), ld_code=E, plane_code=K * E, K=K, E=E,
               start=L.ptr(start), len=L.ptr(length), n_frag=B, T=Tq, dst=L.ptr(dst), ld_dst=ld, bad=L.ptr(stat, 2))
    for change in (dict(S=0), dict(S=9), dict(S=-1), dict(s_use=None), dict(s_use=L.ptr(s_use) + 1), dict(K=0), dict(K=65537), dict(E=0), dict(E=1025),
                   dict(n_idx=-1), dict(n_idx=2 ** 31, ld_idx=2 ** 31), dict(ld_idx=n - 1), dict(ld_dst=E - 4), dict(ld_dst=20), dict(ld_code=E - 1),
                   dict(plane_code=(K - 1) * E + E - 1), dict(dtype=5), dict(T=0), dict(n_frag=-1), dict(n_frag=2 ** 20 + 1), dict(dst=None),
                   dict(start=None), dict(len=None), dict(code=None), dict(bad=None), dict(idx=None), dict(dst=L.ptr(dst) + 8), dict(code=L.ptr(code) + 2),
                   dict(idx=L.ptr(idx) + 2), dict(start=L.ptr(start) + 4), dict(len=L.ptr(length) + 2), dict(bad=L.ptr(stat) + 2)):
        with pytest.raises(L.ZsError, match='zs_rvq_gather_frag'):
            L.call('zs_rvq_gather_frag', 'ZsRvqGatherFrag', _stream(), **dict(okg, **change))
    L.call('zs_rvq_gather_frag', 'ZsRvqGatherFrag', _stream(), **dict(okg, n_frag=0, dst=None, start=None, len=None, s_use=None, bad=None))
    for fn in L.DROP_FUNCTIONS:
        assert getattr(L.lib(), fn)(None, None) == L.ZS_EINVAL                 # a null struct
    torch.cuda.synchronize()
    assert (r == 9.0).all() and (zf == 8.0).all() and (a == 6.0).all() and (ia == -7).all() and (part == -1.0).all() and (stat == 5).all()
    assert (x == 0.5).all() and (code == 0.25).all() and (idx == 0).all() and (s_use == 2).all() and (sw == -7).all() and (act == -7).all()
    assert (dst == 9.0).all() and (word == 0).all()


# ---- the bottleneck ------------------------------------------------------------------------------------------------------------------
SIZES, NS = G.SIZES, G.NS


def _bottleneck(dev, vectors, rows, beta=0.25, decay=0.99, dtype='fp32', restart=None, dropout=None):
    from zs_amd import layers
    from zs_amd.rvq import ResidualCodebook
    from zs_amd.rvq_train import RvqBottleneck
    return RvqBottleneck(ResidualCodebook(np.ascontiguousarray(vectors, F32), {'enc_mode': 'continues'}), beta, decay, rows,
                         layers.Ctx(dev, dtype), restart=restart, dropout=dropout)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_forward_with_dropout_equals_the_definition(dev, dtype):
    """After one forward: s_use and active are the draw's of the step's seed pair, and idx_acc, a, q, the losses and the next codebooks
    are the definition's under those counts and the device's own indices.  stats() carries every stage's active rows and raises nothing
    for the rows a stage left out."""
    B, T4, E, K, S = 6, 4, SIZES['E'], 16, 3
    n = B * T4
    bf16 = dtype == 'bf16'
    rows = T.cast(R.planted(n, E, 4, 0.3, 3), bf16)
    vec = np.stack([(R.planted(K, E, 4, 0.3, 10 + s) * F32(0.4 ** s)).astype(F32) for s in range(S)])
    bn = _bottleneck(dev, vec, n, dtype=dtype, dropout=1.0, decay=0.5, restart=0.9)
    bits = G._rows_act(bn, rows, B, T4)
    word = torch.tensor([0x1234567], dtype=torch.int64, device=dev)
    from zs_amd import _lib as L
    q = bn.forward(bits, 5, L.ptr(word))
    torch.cuda.synchronize()
    s_use = bn.s_use.cpu().numpy()
    assert np.array_equal(s_use, D.draw(5, 0x1234567, B, S, D.threshold(1.0))) and len(set(s_use.tolist())) >= 2
    assert np.array_equal(bn.active.cpu().numpy(), D.active(s_use, S, T4))
    idx = bn.idx.cpu().numpy()
    state = RT.State(vec)
    want = D.iteration(state, rows, np.zeros((n, E), F32), 0.25, 0.5, bn.shift, q.ld, T4, s_use, bf16, idxs=idx, restart=0.9, seed=5,
                       seed_dev=0x1234567, stride=bn.stride)
    assert _same(bn.a.cpu().numpy(), want['a']) and np.array_equal(bn.idx_acc.cpu().numpy(), want['idx_acc'])
    assert _same(q.view2d().float().cpu().numpy(), want['q'])
    st = bn.stats()
    assert st['active'] == D.active(s_use, S, T4).tolist() == [s['active'] for s in st['stages']] and st['s_use_mean'] == float(s_use.mean())
    assert abs(st['loss_vq'] - want['loss_vq']) <= 1e-6 * want['loss_vq'] and st['restarts'] == want['restarted'] and st['skipped'] == want['skipped']
    for s in range(S):
        assert abs(st['stages'][s]['loss_vq'] - want['loss_stage'][s]) <= 1e-6 * want['loss_stage'][s]
        assert _same(bn.code[s].cpu().numpy(), state.stages[s].code), s
    assert bn.ckpt_meta(1, st)['dropout'] == 1.0


def _oracle_step(esd, dsd, x_bft, c, codes, idx, s_use, beta, dt):
    """tests/test_gpu_rvq_train.py's _oracle_step under the counts s_use [B]: the quantiser is z + (q_masked - z).detach(), q_masked
    the sum of the sample's first s_use codewords; stage s commits its input to its codeword on the samples that use it, the mean
    taken over all elements.  Also returns d (stage 1's commitment term) / dz."""
    import zs_oracle as O
    ep = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in esd.items()}
    dp = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in dsd.items()}
    z = G._oracle_z(ep, x_bft.to(dt))                                                   # [B, E, T']
    B, E, T4 = z.shape
    su = torch.from_numpy(np.asarray(s_use)).view(B, 1, 1)
    qs = [torch.from_numpy(code[i]).to(dt).view(B, T4, E).permute(0, 2, 1) * (su > s).to(dt) for s, (code, i) in enumerate(zip(codes, idx))]
    q = qs[0]
    for t in qs[1:]:
        q = q + t
    x_dec = O.decoder_forward(dp, z + (q - z).detach(), c, NS, SIZES['seg_len'])
    l_rec = O.l1_loss(x_dec, x_bft.to(dt))
    l_vq, r, terms = 0.0, z, []
    for s, t in enumerate(qs):
        r = r - t.detach()                                                              # (an unused stage: minus zero, the copy)
        terms.append(beta * ((r * (su > s).to(dt)) ** 2).mean())
        l_vq = l_vq + terms[-1]
    g1 = torch.autograd.grad(terms[1], z, retain_graph=True)[0]
    (l_rec + l_vq).backward()
    return l_rec.item(), l_vq.item(), {k: v.grad for k, v in ep.items()}, {k: v.grad for k, v in dp.items()}, g1


def test_one_iteration_against_the_oracle(dev):
    """tests/test_gpu_rvq_train.py test_one_iteration_against_the_oracle's sizes and bounds with dropout 1: |loss - reference| < 1e-5 on
    both losses and gradients within 2e-3 of the tensor's largest |reference|, the oracle fed the device's idx and s_use.  A sample
    with s_use = 1 has a stage-1 commitment gradient of exactly zero on its rows: in the oracle, and on the device, where its rows of
    a are r_1 alone."""
    from zs_amd.trainer import AEStep
    enc, dec = G._nets(dev, seed=0)
    esd = {k: v.detach().cpu() for k, v in enc.state_dict().items()}
    dsd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    B, T_, beta, S = 3, 32, 0.25, 2
    x = torch.rand(B, T_, SIZES['c_in'], generator=g) * 0.98 + 1e-3
    c = torch.randint(0, SIZES['n_spk'], (B,), generator=g)
    with torch.no_grad():
        z64 = G._oracle_z({k: v.double() for k, v in esd.items()}, x.permute(0, 2, 1).double())
    rows = z64.permute(0, 2, 1).reshape(-1, SIZES['E']).numpy()                         # [B T', E]: 12 rows
    rs = np.random.RandomState(3)
    code0 = (rows[[0, 3, 6, 9, 11]] * (1.0 + 0.2 * rs.standard_normal((5, SIZES['E'])))).astype(F32)
    left = rows - code0[R.assign(rows, code0)[0]]
    code1 = (left[[1, 4, 7, 10, 2]] * (1.0 + 0.2 * rs.standard_normal((5, SIZES['E'])))).astype(F32)
    codes = [code0, code1]
    thr = D.threshold(1.0)
    seed = next(s for s in range(1, 100) if set(D.draw(s, 0, B, S, thr).tolist()) == {1, 2})      # a step's seed with both counts
    bn = _bottleneck(dev, np.stack(codes), len(rows), beta=beta, dropout=1.0)
    ae = AEStep(enc, dec, lr=1e-4, max_grad_norm=5.0, use_graph=False, vq=bn)
    loss = ae.step(x.to(dev), c.to(dev), update=False, seed=seed)
    torch.cuda.synchronize()
    idx, s_use = bn.idx.cpu().numpy(), bn.s_use.cpu().numpy()
    assert np.array_equal(s_use, D.draw(seed, 0, B, S, thr)) and set(s_use.tolist()) == {1, 2}
    T4 = len(rows) // B
    xb = x.permute(0, 2, 1)
    r32, v32, ge32, gd32, _ = _oracle_step(esd, dsd, xb, c, codes, idx, s_use, beta, torch.float32)
    r64, v64, ge64, gd64, g1 = _oracle_step(esd, dsd, xb, c, codes, idx, s_use, beta, torch.float64)
    assert abs(r32 - r64) < 1e-6 and abs(v32 - v64) < 1e-6
    picks = (('enc', enc, ge32, ge64, 'linear.weight'), ('enc', enc, ge32, ge64, 'conv2.weight'), ('dec', dec, gd32, gd64, 'conv1.weight'))
    for name, net, g32, g64, k in picks:
        scale = g64[k].abs().max().item()
        assert scale > 1e-6 and (g32[k].double() - g64[k]).abs().max().item() <= 2e-4 * scale, 'the fp32 oracle is ill-conditioned here'
    lv = float(bn.loss[0].item())
    print('s_use %s  loss_rec %.7f (oracle %.7f, |d| %.3g)  loss_vq %.7f (oracle %.7f, |d| %.3g)' %
          (s_use.tolist(), loss.item(), r32, abs(loss.item() - r32), lv, v32, abs(lv - v32)))
    assert abs(loss.item() - r32) < 1e-5 and abs(lv - v32) < 1e-5
    for name, net, g32, g64, k in picks:
        ref = g32[k].double()
        scale = ref.abs().max().item()
        e = (net.grad_view(k).detach().cpu().double() - ref).abs().max().item() / scale
        print('grad %s.%s: relative error %.3g of scale %.3g' % (name, k, e, scale))
        assert e < 2e-3
    # the mask is in those figures: without it (every sample from both stages) the oracle's loss_vq has the dropped stages' terms too
    _, v_all, _, _, _ = _oracle_step(esd, dsd, xb, c, codes, idx, np.full(B, S), beta, torch.float64)
    print('loss_vq of the oracle with every sample at S: %.7f' % v_all)
    assert v_all > v64
    # a sample decoded from one stage: no stage-1 commitment gradient on its rows, exactly
    one = np.repeat(s_use == 1, T4)
    g1 = g1.permute(0, 2, 1).reshape(-1, SIZES['E']).numpy()                            # d (stage 1's term) / d z, [B T', E]
    assert (g1[one] == 0).all() and np.abs(g1[~one]).max() > 0
    a, ia = bn.a.cpu().numpy(), bn.idx_acc.cpu().numpy()
    r1, r2 = bn.res[1].cpu().numpy(), bn.res[0].cpu().numpy()                           # S = 2: what stage 0 and stage 1 wrote
    assert (ia[1][one] == -1).all() and (ia[1][~one] >= 0).all() and (ia[0] >= 0).all()
    assert _same(a[one], r1[one]) and _same(r2[one], r1[one])                           # a is r_1 alone; r_2 is its copy
    assert _same(a[~one], (r1[~one] + r2[~one]).astype(F32)) and np.abs(r2[~one]).max() > 0 and not np.array_equal(a[~one], r1[~one])
    st = bn.stats()
    assert st['active'] == D.active(s_use, S, T4).tolist() and abs(st['loss_vq'] - v64) < 1e-5


def _run_five(dev, graph_warmup, dtype):
    from zs_amd.trainer import AEStep
    enc, dec = G._nets(dev, dtype=dtype, seed=0, dp=0.5)
    B, T_ = 4, 32
    vec = np.stack([R.planted(7, SIZES['E'], 4, 0.3, 2) * F32(0.1), R.planted(7, SIZES['E'], 4, 0.3, 3) * F32(0.02),
                    R.planted(7, SIZES['E'], 4, 0.3, 4) * F32(0.004)])
    bn = _bottleneck(dev, vec, B * 4, decay=0.5, dtype=dtype, restart=0.9, dropout=0.75)
    ae = AEStep(enc, dec, lr=1e-3, max_grad_norm=5.0, use_graph=True, vq=bn)
    ae.graph_warmup = graph_warmup
    g = torch.Generator().manual_seed(1)
    losses, counts = [], []
    for _ in range(5):
        x = torch.rand(B, T_, SIZES['c_in'], generator=g).to(dev)
        c = torch.randint(0, SIZES['n_spk'], (B,), generator=g).to(dev)
        losses.append((ae.step(x, c).item(),) + tuple(bn.loss.cpu().tolist()))
        counts.append(tuple(bn.s_use.cpu().tolist()) + tuple(bn.active.cpu().tolist()))
    torch.cuda.synchronize()
    state = [enc.flat_params()[0], dec.flat_params()[0]] + [getattr(ae.opt[k], a) for k in ('enc', 'dec') for a in ('m', 'v')] + \
        [bn.code, bn.cnorm, bn.N, bn.m, bn.idx, bn.idx_acc, bn.stat, bn.a]
    bn.stats()
    assert bn.steps == (5 if graph_warmup > 5 else 3)                                   # (a replay does not pass through forward())
    return losses, [t.clone() for t in state], len(ae._graphs), counts


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_captured_equals_eager_and_a_rerun(dev, dtype):
    """Weights, Adam moments, every stage's state, the losses and each iteration's s_use, bitwise; the captured step draws anew on
    every replay."""
    la, sa, na, ca = _run_five(dev, 2, dtype)
    lb, sb, nb, cb = _run_five(dev, 10 ** 9, dtype)
    lc, sc, nc, cc = _run_five(dev, 2, dtype)
    assert na == nc == 1 and nb == 0
    assert la == lb == lc, (la, lb, lc)
    assert ca == cb == cc, (ca, cb, cc)
    for a, b, c in zip(sa, sb, sc):
        assert torch.equal(a, b) and torch.equal(a, c)
    print('s_use | active per iteration: %s' % (ca,))
    assert len({c[:4] for c in ca}) >= 2 and len({c[:4] for c in ca[2:]}) >= 2          # between iterations, and between replays
    assert all(1 <= v <= 3 for c in ca for v in c[:4]) and all(c[4] == 16 for c in ca)
    assert len({l[0] for l in la}) == 5 and all(np.isfinite(v) and v >= 0 for l in la for v in l)


def test_without_dropout_the_step_calls_none_of_the_new_entry_points(dev, monkeypatch):
    from zs_amd import _lib as L
    from zs_amd.trainer import AEStep
    names = []
    real_call = L.call
    monkeypatch.setattr(L, 'call', lambda fname, *a, **k: (names.append(fname), real_call(fname, *a, **k))[1])
    enc, dec = G._nets(dev, seed=0)
    vec = np.stack([R.planted(5, SIZES['E'], 4, 0.3, 2) * F32(0.1), R.planted(5, SIZES['E'], 4, 0.3, 3) * F32(0.01)])
    g = torch.Generator().manual_seed(1)
    x = torch.rand(3, 32, SIZES['c_in'], generator=g).to(dev)
    c = torch.randint(0, SIZES['n_spk'], (3,), generator=g).to(dev)
    ae = AEStep(enc, dec, lr=1e-4, max_grad_norm=5.0, use_graph=False, vq=_bottleneck(dev, vec, 12))
    ae.step(x, c)
    torch.cuda.synchronize()
    stage = ['zs_vq_assign', 'zs_rvq_commit', 'zs_vq_accum', 'zs_vq_ema']
    assert [n for n in names if n.startswith('zs_vq') or n.startswith('zs_rvq')] == stage * 2 + ['zs_rvq_loss', 'zs_rvq_gather', 'zs_rvq_st_bwd']
    del names[:]
    ae.vq = _bottleneck(dev, vec, 12, dropout=0.5)
    ae.step(x, c)
    torch.cuda.synchronize()
    stage[1] = 'zs_rvq_commit_drop'
    assert [n for n in names if n.startswith('zs_vq') or n.startswith('zs_rvq')] == \
        ['zs_rvq_drop_draw'] + stage * 2 + ['zs_rvq_loss', 'zs_rvq_gather_frag', 'zs_rvq_st_bwd']


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_main_rvq_dropout_then_convert_from_one_stage(dev, tmp_path, monkeypatch, capsys):
    from scipy.io import wavfile
    sys.path.insert(0, ROOT)
    import main as M
    from zs_amd import convert as cv, layers, rvq as V, vq as V1
    from zs_amd.hps import hp
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('ZS_CKPT_EVERY', '4')
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    h = json.load(open(os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')))
    h.update(n_speakers=4, n_target_speakers=2, batch_size=4, enc_pretrain_iters=4, max_to_keep=3, enc_size=8, emb_size=32, seg_len=32)
    hps_path = str(tmp_path / 'hps.json')
    json.dump(h, open(hps_path, 'w'))
    K, S = 6, 3
    start = str(tmp_path / 'K6x3.rvq.npz')
    vec = np.stack([R.planted(K, 8, 4, 0.3, 4 + s) * F32(0.1 * 0.3 ** s) for s in range(S)]).astype(F32)
    V.ResidualCodebook(vec, {'enc_mode': 'continues', 'seed': 0}).save(start)
    ck = tmp_path / 'ck'
    M.main(['--train_ae', '--synthetic', '--enc_mode', 'continues', '--hps_path', hps_path, '--ckpt_dir', str(ck), '--dtype', 'fp32',
            '--rvq_train', start, '--vq_decay', '0.9', '--vq_restart', '0.5', '--rvq_dropout', '0.5'])
    out = capsys.readouterr().out
    assert 'pre_AE:[000004/000004]' in out and 'loss_vq=' in out and 'used2=' in out and 'restarts=' in out
    assert 'active0=1.000' in out and 'active1=' in out and 'active2=' in out
    cb_path = str(ck / 'model.pth-ae-4.rvq.npz')
    cb = V1.load_codebook(cb_path, 'continues', E=8)
    assert isinstance(cb, V.ResidualCodebook) and (cb.S, cb.K, cb.E) == (S, K, 8) and not np.array_equal(cb.vectors, vec)
    assert cb.meta['trained_iterations'] == 4 and cb.meta['dropout'] == 0.5 and cb.meta['restart'] == 0.5 and len(cb.meta['used']) == S
    d = tmp_path / 'in'
    d.mkdir()
    rng = np.random.RandomState(5)
    t = np.arange(9000) / 16000.0
    y = 0.3 * np.sin(2 * np.pi * (200.0 + 400.0 * t) * t) + 0.05 * rng.randn(9000)
    wavfile.write(str(d / 'w0.wav'), 16000, (y * 32767).astype(np.int16))
    s2id = str(tmp_path / 'speaker2id.json')
    json.dump({'S015': 0, 'S020': 1, 'V001': 2, 'V002': 3}, open(s2id, 'w'))
    monkeypatch.setattr(hp, 'n_iter', 4)
    res = tmp_path / 'result1'
    M.main(['--convert_dir', str(d), '--t_speaker', 'V001', '--result_dir', str(res), '--codebook', cb_path, '--rvq_stages', '1', '--enc_only',
            '--hps_path', hps_path, '--speaker2id_path', s2id, '--ckpt_pth', str(ck / 'model.pth-ae-4'), '--enc_mode', 'continues',
            '--g_mode', 'targeted_residual'])
    conv = os.path.join(os.path.join(str(res), './english/'), 'convert')
    idx = cv.read_index_rows(os.path.join(conv, 'V001', 'w0.idx.txt'), K, S)
    assert idx.shape[1] == 1 and len(idx) >= 2 and idx.min() >= 0 and idx.max() < K
    assert os.path.getsize(os.path.join(conv, 'V001', 'w0.wav')) > 44
    layers.check_status(dev)
