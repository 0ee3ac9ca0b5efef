"""--segment on the device:

* zs_seg_viterbi against the fp32 definition of tests/segment_ref.py with array_equal (idx, n_seg, cost), and on integer scores
  against the fp64 optimum exactly;
* zs_vq_scores against zs_vq_assign (the lowest argmin of every row, on both decompositions) and the fp64 scores under vq_ref.bound;
* zs_code_scores against numpy popcount exactly, and against zs_code_assign."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import segment_ref as R  # noqa: E402
import vq_ref as VR  # noqa: E402

GUARD = 64
FILL_I = -0x55555556
LAMS = (0.0, 0.37, 1.0, 5.0, 1e30)
KS = (1, 2, 63, 64, 65, 255, 256, 257, 1024, 4096)
MIXED = (0, 1, 2, 3, 64, 0, 65, 300, 7, 0)                          # empty utterances first, in the middle and last


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _scores(rs, n, K, kind):
    if kind == 'int':
        return rs.randint(0, 17, size=(n, K)).astype(np.float32)         # ties everywhere
    return rs.standard_normal((n, K)).astype(np.float32)


def _viterbi(dev, s, lens, lam, ld=None, row=None, raw=None):
    """zs_seg_viterbi over utterances of `lens` units whose scores are the rows of s [sum lens, K] in utterance order.  The rows lie at
    pitch ld with NaN in the columns >= K; row: None, or the score row of every unit (the rows of s are moved there; n_rows = max + 1
    unless raw gives the table as it is passed).  Guards behind every output.  Returns dict(idx, n_seg, cost, bad)."""
    from zs_amd import _lib as L, segment as S
    n, K = s.shape
    ld = ld or K
    uoffs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert uoffs[-1] == n
    n_rows = n if row is None else int(max(row.max() + 1, 1)) if len(row) else 1
    buf = np.full((max(n_rows, 1), ld), np.nan, dtype=np.float32)
    buf[(np.arange(n) if row is None else row), :K] = s
    s_d = torch.from_numpy(buf).to(dev)
    idx = torch.full((n + GUARD,), FILL_I, dtype=torch.int32, device=dev)
    n_seg = torch.full((len(lens) + GUARD,), FILL_I, dtype=torch.int32, device=dev)
    cost = torch.full((len(lens) + GUARD,), float('nan'), dtype=torch.float64, device=dev)
    bad = torch.zeros(1 + GUARD, dtype=torch.int32, device=dev)
    wb = S.work_bytes(n, K)
    work = torch.full(((wb + 7) // 8 + GUARD,), 0x5555555555555555, dtype=torch.int64, device=dev)
    row_pass = row if raw is None else raw
    row_d = None if row_pass is None else torch.from_numpy(np.ascontiguousarray(row_pass, dtype=np.int64)).to(dev)
    L.call('zs_seg_viterbi', 'ZsSegViterbi', _stream(), scores=L.ptr(s_d), n_rows=n_rows, ld_s=ld, uoffs=L.ptr(torch.from_numpy(uoffs).to(dev)),
           n_utt=len(lens), row=L.ptr(row_d), n_units=n, lam=float(lam), K=K, work=L.ptr(work), work_bytes=wb, idx=L.ptr(idx),
           n_seg=L.ptr(n_seg), cost=L.ptr(cost), bad=L.ptr(bad))
    torch.cuda.synchronize()
    assert (idx[n:] == FILL_I).all() and (n_seg[len(lens):] == FILL_I).all() and torch.isnan(cost[len(lens):]).all()
    assert (bad[1:] == 0).all() and (work[(wb + 7) // 8:] == 0x5555555555555555).all()
    assert np.array_equal(s_d.cpu().numpy(), buf, equal_nan=True)         # read only
    return dict(idx=idx[:n].cpu().numpy(), n_seg=n_seg[:len(lens)].cpu().numpy(), cost=cost[:len(lens)].cpu().numpy(), bad=int(bad[0]),
                uoffs=uoffs)


def _check(got, s, lens, lam, exact_int=False):
    """Every utterance against the fp32 definition with array_equal; on integer scores with an integer lambda the path's objective,
    in Python integers, is the fp64 optimum."""
    o = got['uoffs']
    for u, T in enumerate(lens):
        su = s[o[u]:o[u + 1]]
        idx, n_seg, cost = R.viterbi32(su, np.float32(lam))
        assert np.array_equal(got['idx'][o[u]:o[u + 1]], idx), (u, T)
        assert got['n_seg'][u] == n_seg and got['cost'][u] == cost, (u, T)
        if exact_int and T:
            si = su.astype(np.int64)
            assert R.objective(si, int(lam), got['idx'][o[u]:o[u + 1]]) == R.viterbi64(si, float(lam))[0]
    assert got['bad'] == 0


@pytest.mark.parametrize('K', KS)
def test_viterbi_is_the_fp32_definition(dev, K):
    """Mixed utterance lengths in one launch, both kinds of scores, every lambda; the pitch and the row table alternate."""
    rs = np.random.RandomState(K)
    lens = list(MIXED)
    n = sum(lens)
    case = 0
    for kind in ('gauss', 'int'):
        s = _scores(rs, n, K, kind)
        for lam in LAMS:
            ld = K + 3 * (case % 2)
            row = rs.permutation(n + 5)[:n] if case % 3 == 1 else None
            got = _viterbi(dev, s, lens, lam, ld=ld, row=row)
            _check(got, s, lens, lam, exact_int=(kind == 'int' and lam in (0.0, 1.0, 5.0)))
            if lam == 0.0:
                assert np.array_equal(got['idx'], s.argmin(1))            # the assign kernels' answer
            if lam == 1e30:
                assert (got['n_seg'] == (np.asarray(lens) > 0)).all()
            case += 1


@pytest.mark.parametrize('T', [0, 1, 2, 3, 64, 65, 300])
def test_viterbi_one_utterance_of_every_length(dev, T):
    rs = np.random.RandomState(T)
    for K, lam, kind in ((5, 1.0, 'int'), (70, 0.37, 'gauss'), (300, 5.0, 'int')):
        s = _scores(rs, T, K, kind)
        got = _viterbi(dev, s, [T], lam, ld=K + 3)
        _check(got, s, [T], lam, exact_int=(kind == 'int'))


@pytest.mark.parametrize('n_utt', [1, 3, 70])
def test_viterbi_batches(dev, n_utt):
    """More utterances than one launch has lengths for: every workgroup takes its own, empty ones among them."""
    rs = np.random.RandomState(n_utt)
    lens = [int(x) for x in rs.randint(0, 40, size=n_utt)]
    lens[0] = 0 if n_utt > 1 else 33
    lens[-1] = 0 if n_utt > 1 else 33
    n = sum(lens)
    for K, lam, kind in ((64, 1.0, 'int'), (129, 0.37, 'gauss')):
        s = _scores(rs, n, K, kind)
        row = rs.permutation(n)
        got = _viterbi(dev, s, lens, lam, row=row)
        _check(got, s, lens, lam, exact_int=(kind == 'int'))
        again = _viterbi(dev, s, lens, lam, row=row)
        for k in ('idx', 'n_seg', 'cost'):
            assert got[k].tobytes() == again[k].tobytes()                 # two runs are bitwise equal


@pytest.mark.parametrize('where', ['negative', 'beyond'])
def test_viterbi_row_out_of_range_costs_one_utterance(dev, where):
    rs = np.random.RandomState(5)
    lens, K, lam = [9, 12, 0, 6], 70, 1.0
    n = sum(lens)
    s = _scores(rs, n, K, 'int')
    row = rs.permutation(n)
    raw = row.copy()
    raw[9 + 4] = -1 if where == 'negative' else n                         # a unit of utterance 1
    got = _viterbi(dev, s, lens, lam, row=row, raw=raw)
    assert got['bad'] == 1
    assert (got['idx'][9:21] == -1).all() and got['n_seg'][1] == 0
    for u in (0, 2, 3):
        o = got['uoffs']
        idx, n_seg, cost = R.viterbi32(s[o[u]:o[u + 1]], np.float32(lam))
        assert np.array_equal(got['idx'][o[u]:o[u + 1]], idx) and got['n_seg'][u] == n_seg and got['cost'][u] == cost


def test_viterbi_scores_that_are_not_finite_stay_in_range(dev):
    rs = np.random.RandomState(6)
    for K in (3, 300):
        s = _scores(rs, 40, K, 'gauss')
        s[7] = np.inf
        s[20] = np.nan
        s[30, ::2] = -np.inf
        got = _viterbi(dev, s, [25, 15], 0.5)
        assert got['idx'].min() >= 0 and got['idx'].max() < K and got['bad'] == 0
        assert (got['n_seg'] >= 1).all()


def test_viterbi_argument_errors_launch_nothing(dev):
    from zs_amd import _lib as L, segment as S
    n, K = 20, 70
    s = torch.zeros(n, K, device=dev)
    uoffs = torch.tensor([0, 8, 20], dtype=torch.int64, device=dev)
    row = torch.arange(n, dtype=torch.int64, device=dev)
    idx = torch.full((n,), FILL_I, dtype=torch.int32, device=dev)
    n_seg = torch.full((2,), FILL_I, dtype=torch.int32, device=dev)
    cost = torch.full((2,), float('nan'), dtype=torch.float64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    work = torch.zeros(S.work_bytes(n, K) // 8 + 2, dtype=torch.int64, device=dev)
    good = dict(scores=L.ptr(s), n_rows=n, ld_s=K, uoffs=L.ptr(uoffs), n_utt=2, row=L.ptr(row), n_units=n, lam=1.0, K=K, work=L.ptr(work),
                work_bytes=S.work_bytes(n, K), idx=L.ptr(idx), n_seg=L.ptr(n_seg), cost=L.ptr(cost), bad=L.ptr(bad))
    assert L.lib().zs_seg_viterbi(None, _stream()) == L.ZS_EINVAL
    for change in (dict(K=0), dict(K=S.MAX_K + 1), dict(ld_s=K - 1), dict(lam=-1.0), dict(lam=float('nan')), dict(lam=float('inf')),
                   dict(n_units=-1), dict(n_utt=-1), dict(n_rows=-1), dict(scores=None), dict(idx=None), dict(work=None), dict(uoffs=None),
                   dict(bad=None), dict(work_bytes=S.work_bytes(n, K) - 1), dict(work=L.ptr(work) + 4), dict(scores=L.ptr(s) + 2),
                   dict(idx=L.ptr(idx) + 2), dict(cost=L.ptr(cost) + 4), dict(uoffs=L.ptr(uoffs) + 4), dict(row=None, n_rows=n - 1)):
        kw = dict(good)
        kw.update(change)
        st = L.SEGMENT_STRUCTS['ZsSegViterbi'](**{k: v for k, v in kw.items() if v is not None})
        assert L.lib().zs_seg_viterbi(ctypes.addressof(st), _stream()) == L.ZS_EINVAL, change
    torch.cuda.synchronize()
    assert (idx == FILL_I).all() and (n_seg == FILL_I).all() and torch.isnan(cost).all() and int(bad[0]) == 0 and (work == 0).all()
    st = L.SEGMENT_STRUCTS['ZsSegViterbi'](**dict(good, n_utt=0))                 # nothing to do succeeds
    assert L.lib().zs_seg_viterbi(ctypes.addressof(st), _stream()) == 0
    torch.cuda.synchronize()
    assert (idx == FILL_I).all()


def test_segment_viterbi_wrapper(dev):
    """zs_amd.segment.viterbi: the launch above behind its checks, uoffs from the host."""
    from zs_amd import segment as S
    rs = np.random.RandomState(8)
    lens = [5, 0, 31]
    s = _scores(rs, 36, 10, 'int')
    buf = torch.from_numpy(np.concatenate([s, np.full((36, 2), np.nan, dtype=np.float32)], axis=1)).to(dev)
    idx, n_seg, cost = S.viterbi(buf, np.asarray([0, 5, 5, 36]), 2.0, K=10)
    got = dict(idx=idx.cpu().numpy(), n_seg=n_seg.cpu().numpy(), cost=cost.cpu().numpy(), bad=0, uoffs=np.asarray([0, 5, 5, 36]))
    _check(got, s, lens, 2.0, exact_int=True)
    r = S.runs(got['idx'], got['uoffs'])
    assert [len(x) for x in r] == got['n_seg'].tolist()
    with pytest.raises(ValueError):
        S.viterbi(buf, np.asarray([0, 36]), -1.0)


# ---- zs_vq_scores ---------------------------------------------------------------------------------------------------------------------
def _vq_case(rs, n, E, K):
    code = rs.standard_normal((K, E)).astype(np.float32)
    if K > 9:                                                             # planted ties: identical codewords, identical cnorm
        code[9] = code[5]
        code[K - 1] = code[min(20, K - 2)]
    x = (code[rs.randint(K, size=n)] + 0.05 * rs.standard_normal((n, E))).astype(np.float32)
    if K > 9:
        x[0] = code[9]
    return x, code


def _vq_scores(dev, x, code, cn, bf16, ld_s, misalign=False):
    from zs_amd import _lib as L, vq as V
    n, E = x.shape
    K = code.shape[0]
    xt = torch.from_numpy(x)
    xt = xt.to(torch.bfloat16) if bf16 else xt
    if misalign:                                                          # rows one element behind a 16-byte boundary: scalar loads
        flat = torch.zeros(n * E + 1, dtype=xt.dtype)
        flat[1:] = xt.reshape(-1)
        x_d = flat.to(dev)[1:].view(n, E)
    else:
        x_d = xt.to(dev)
    code_d, cn_d = torch.from_numpy(code).to(dev), torch.from_numpy(cn).to(dev)
    out = torch.full((n * ld_s + GUARD,), float('nan'), dtype=torch.float32, device=dev)
    V.launch_scores(_stream(), (L.ZS_BF16 if bf16 else L.ZS_F32), L.ptr(x_d), n, E, code_d, cn_d, L.ptr(out), ld_s)
    idx = {}
    for name, work in (('rows', None), ('split', V.workspace(dev))):
        idx[name] = torch.full((n,), FILL_I, dtype=torch.int32, device=dev)
        V.assign(x_d, code_d, cn_d, idx=idx[name], work=work)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.isnan(o[n * ld_s:]).all()
    o = o[:n * ld_s].reshape(n, ld_s)
    assert np.isnan(o[:, K:]).all()                                       # the columns >= K are untouched
    return o[:, :K], {k: v.cpu().numpy() for k, v in idx.items()}, x_d.float().cpu().numpy()


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('E', [1, 3, 33, 1024])
def test_vq_scores_are_the_scores_of_assign(dev, E, bf16):
    rs = np.random.RandomState(E + 7 * bf16)
    case = 0
    for n in (1, 127, 129):
        for K in (1, 127, 129, 1024):
            x, code = _vq_case(rs, n, E, K)
            cn = VR.cnorm(code)
            ld_s = K + (3 if case % 2 else 0)
            got, idx, xr = _vq_scores(dev, x, code, cn, bf16, ld_s, misalign=(case % 3 == 2))
            assert not np.signbit(got[got == 0]).any()                    # -0 is written as +0
            low = got.argmin(1)                                           # numpy: the first least entry
            assert np.array_equal(low, idx['rows']) and np.array_equal(low, idx['split']), (n, K)
            err = np.abs(got.astype(np.float64) - VR.scores(xr, code, cn))
            assert (err <= VR.bound(xr, code, cn)[:, None]).all(), (n, K, err.max())
            if K > 9:
                assert np.array_equal(got[:, 9], got[:, 5]) and not (low == 9).any()
            case += 1


def test_vq_scores_argument_errors_launch_nothing(dev):
    from zs_amd import _lib as L, segment as S
    n, E, K = 10, 8, 20
    x = torch.zeros(n, E, device=dev)
    code, cn = torch.zeros(K, E, device=dev), torch.zeros(K, device=dev)
    out = torch.full((n, K), float('nan'), device=dev)
    good = dict(dtype=L.ZS_F32, src_f32=0, x=L.ptr(x), n=n, ld_x=E, code=L.ptr(code), ld_code=E, cnorm=L.ptr(cn), K=K, E=E, scores=L.ptr(out),
                ld_s=K)
    assert L.lib().zs_vq_scores(None, _stream()) == L.ZS_EINVAL
    for change in (dict(K=0), dict(K=S.MAX_K + 1), dict(E=0), dict(ld_s=K - 1), dict(ld_x=E - 1), dict(ld_code=E - 1), dict(n=-1), dict(x=None),
                   dict(scores=None), dict(cnorm=None), dict(scores=L.ptr(out) + 2), dict(x=L.ptr(x) + 2), dict(dtype=77)):
        kw = dict(good)
        kw.update(change)
        st = L.SEGMENT_STRUCTS['ZsVqScores'](**{k: v for k, v in kw.items() if v is not None})
        assert L.lib().zs_vq_scores(ctypes.addressof(st), _stream()) == L.ZS_EINVAL, change
    st = L.SEGMENT_STRUCTS['ZsVqScores'](**dict(good, n=0))
    assert L.lib().zs_vq_scores(ctypes.addressof(st), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---- zs_code_scores -------------------------------------------------------------------------------------------------------------------
def _bits(rows, E):
    return np.unpackbits(rows, axis=1, bitorder='little')[:, :E].astype(np.float64)


@pytest.mark.parametrize('E', [1, 7, 8, 9, 33, 1024])
def test_code_scores_are_popcounts(dev, E):
    from zs_amd import _lib as L, codebook as C
    rs = np.random.RandomState(E)
    nb = (E + 7) // 8
    n = 300                                                               # two workgroups, the second ragged
    for K, ld_s in ((1, 1), (5, 8), (5, 5), (1024, 1024), (1024, 1027)):
        units = rs.randint(0, 256, size=(n, nb)).astype(np.uint8)         # garbage bits at the columns >= E of the last byte
        code = rs.randint(0, 256, size=(K, nb)).astype(np.uint8)
        if K > 4:
            code[4] = code[1]                                             # a tie for every unit
            units[3] = code[4]
        u_d, c_d = torch.from_numpy(units).to(dev), torch.from_numpy(code).to(dev)
        out = torch.full((n * ld_s + GUARD,), float('nan'), dtype=torch.float32, device=dev)
        L.call('zs_code_scores', 'ZsCodeScores', _stream(), units=L.ptr(u_d), n=n, row_bytes=nb, code=L.ptr(c_d), K=K, code_bytes=nb, E=E,
               scores=L.ptr(out), ld_s=ld_s)
        idx = torch.full((n,), FILL_I, dtype=torch.int32, device=dev)
        dist = torch.full((n,), FILL_I, dtype=torch.int32, device=dev)
        C.assign(u_d, c_d, E, idx=idx, dist=dist)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.isnan(o[n * ld_s:]).all()
        o = o[:n * ld_s].reshape(n, ld_s)
        assert np.isnan(o[:, K:]).all()
        ub, cb = _bits(units, E), _bits(code, E)
        want = ub @ (1.0 - cb).T + (1.0 - ub) @ cb.T                      # exact in double
        assert np.array_equal(o[:, :K].astype(np.float64), want), (E, K)
        assert np.array_equal(o[:, :K].min(1), dist.cpu().numpy()) and np.array_equal(o[:, :K].argmin(1), idx.cpu().numpy())
        assert np.array_equal(u_d.cpu().numpy(), units) and np.array_equal(c_d.cpu().numpy(), code)


def test_codebook_scores_methods(dev):
    """The codebooks' scores_ are those launches."""
    from zs_amd.codebook import Codebook
    from zs_amd.vq import VectorCodebook
    rs = np.random.RandomState(1)
    E, K, n = 12, 6, 70
    packed = rs.randint(0, 256, size=(K, 2)).astype(np.uint8)
    packed[:, 1] &= 0x0f
    cb = Codebook(packed, E)
    units = rs.randint(0, 256, size=(n, 2)).astype(np.uint8)
    out = torch.full((n, K + 2), float('nan'), device=dev)
    cb.scores_(torch.from_numpy(units).to(dev), out)
    ub, cbits = _bits(units, E), _bits(packed, E)
    assert np.array_equal(out[:, :K].cpu().numpy().astype(np.float64), ub @ (1.0 - cbits).T + (1.0 - ub) @ cbits.T)
    assert torch.isnan(out[:, K:]).all()
    vec = VectorCodebook(rs.standard_normal((K, E)).astype(np.float32))
    x = torch.from_numpy(rs.standard_normal((n, E)).astype(np.float32)).to(dev)
    out = torch.full((n, K), float('nan'), device=dev)
    vec.scores_(x, out)
    idx, _ = vec.snap(x)
    assert np.array_equal(out.cpu().numpy().argmin(1), idx.cpu().numpy())


# ---- the drivers, in fp32 -------------------------------------------------------------------------------------------------------------
SEG, LU = 32, 4
UNIT_COUNTS = (1, 2, LU, 2 * LU + 1, 5 * LU)


def _trainer(path, enc_mode):
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    torch.manual_seed(3)
    hps = make_hps(enc_size=8, emb_size=32, n_speakers=4, n_target_speakers=2, seg_len=SEG)
    return Trainer(hps, None, 'targeted_residual', enc_mode, log_dir=os.path.join(str(path), 'log'), dtype='fp32', device=torch.device('cuda:0'))


def _field_noise(E, seed=1234, T=64):
    U = torch.rand(T, E, 2, generator=torch.Generator().manual_seed(seed))
    base = (-torch.log(-torch.log(U + 1e-20) + 1e-20)).cuda()
    return lambda n, t, e: base[:t].unsqueeze(0).expand(n, t, E, 2).contiguous()


def _specs_of_units(counts, seed=7):
    """Spectrograms whose utterances return exactly `counts` units (the frame counts are found by the encoder's own rule)."""
    from zs_amd import convert as cv
    rng = np.random.RandomState(seed)
    frames = []
    for c in counts:
        n = next(n for n in range(1, 60 * 8) if cv._unit_counts([np.zeros((n, 513), np.float32)], SEG)[0] == c)
        frames.append(n)
    return [(rng.rand(n, 513) * 0.98 + 1e-3).astype(np.float32) for n in frames]


@pytest.fixture(scope='module')
def kinds(dev, tmp_path_factory):
    """(trainer, codebook, noise_fn, lambda) under a bit and under a vector codebook."""
    from zs_amd import codebook as C, convert as cv, vq
    out = {}
    tr = _trainer(tmp_path_factory.mktemp('bits'), 'multilabel_binary')
    noise = _field_noise(8)
    e, _ = cv.encode_batch(_specs_of_units(UNIT_COUNTS), tr, SEG, noise_fn=noise)
    cb = C.fit(torch.from_numpy(np.concatenate([cv.pack_units(a) for a in e])).to(dev), 6, E=8)
    out['bit'] = (tr, cb, noise, 1.0)
    tr = _trainer(tmp_path_factory.mktemp('cont'), 'continues')
    rows = torch.cat(cv.encode_rows_on_device(_specs_of_units(UNIT_COUNTS), tr, SEG)).cpu().numpy()
    rs = np.random.RandomState(4)
    code = (rows[rs.permutation(len(rows))[:12]] + 0.01 * rs.standard_normal((12, 8))).astype(np.float32)
    out['vector'] = (tr, vq.VectorCodebook(code), None, float(np.float32(0.37 * np.median(((rows[:, None] - code[None]) ** 2).sum(-1)))))
    return out


def _count_calls(monkeypatch):
    from zs_amd import _lib as L
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda *a, **k: (calls.append(a[0]), real(*a, **k))[1])
    return calls


NEW = ('zs_vq_scores', 'zs_code_scores', 'zs_seg_viterbi')


@pytest.mark.parametrize('max_batch', [256, 3])
@pytest.mark.parametrize('kind', ['bit', 'vector'])
def test_encode_batch_segment_is_the_definition_on_the_device_scores(dev, kinds, kind, max_batch, monkeypatch):
    from zs_amd import convert as cv, layers
    tr, cb, noise, lam = kinds[kind]
    specs = _specs_of_units(UNIT_COUNTS)
    q = cv._enqueue_encode(specs, tr, SEG, None, noise, max_batch, dec_to_host=False, codebook=cb, segment=lam)
    torch.cuda.synchronize()
    assert np.diff(q.uoffs).tolist() == list(UNIT_COUNTS)
    scores = q.seg_scores.cpu().numpy()
    row = np.arange(int(q.uoffs[-1])) if q.seg_row is None else q.seg_row.cpu().numpy()
    assert scores.shape[1] == cb.K and (kind == 'bit') == (q.seg_row is None)
    want = [R.viterbi32(scores[row[q.uoffs[u]:q.uoffs[u + 1]]], np.float32(lam))[0] for u in range(len(specs))]
    calls = _count_calls(monkeypatch)
    enc, _, idx = cv.encode_batch(specs, tr, SEG, noise_fn=noise, max_batch=max_batch, codebook=cb, want_idx=True, segment=lam)
    assert all(np.array_equal(a, b) for a, b in zip(idx, want))
    assert calls.count('zs_seg_viterbi') == 1 and 'zs_vq_assign' not in calls and 'zs_code_assign' not in calls
    assert calls.count('zs_vq_scores' if kind == 'vector' else 'zs_code_scores') == (len(q.chunks) if kind == 'vector' else 1)
    assert sum(len(S_) for S_ in want) > sum(1 + int((np.diff(w) != 0).sum()) for w in want)          # lambda joins something
    for e, i in zip(enc, idx):                                            # the units returned are the codewords of the path
        assert np.array_equal(e, cb.vectors[i] if kind == 'vector' else cv.unpack_units(cb.packed[i], 8))
    # lambda = 0: the indices without segment; and without segment none of the new entry points is entered, launch for launch
    del calls[:]
    e0, _, i0 = cv.encode_batch(specs, tr, SEG, noise_fn=noise, max_batch=max_batch, codebook=cb, want_idx=True)
    plain = list(calls)
    del calls[:]
    e1, _, i1 = cv.encode_batch(specs, tr, SEG, noise_fn=noise, max_batch=max_batch, codebook=cb, want_idx=True, segment=None)
    assert calls == plain and not set(NEW) & set(plain)
    ez, _, iz = cv.encode_batch(specs, tr, SEG, noise_fn=noise, max_batch=max_batch, codebook=cb, want_idx=True, segment=0.0)
    assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(i0, i1, iz))
    assert all(np.array_equal(a, b) for a, b in zip(e0, ez))
    layers.check_status(dev)


@pytest.mark.parametrize('max_batch', [256, 3])
@pytest.mark.parametrize('kind', ['bit', 'vector'])
def test_resynth_batch_segment_speaks_the_path(dev, kinds, kind, max_batch):
    from zs_amd import convert as cv, layers
    tr, cb, noise, lam = kinds[kind]
    specs = _specs_of_units(UNIT_COUNTS[1:])                              # the Decoder needs two units
    spk = [2, 3, 2, 3]
    _, _, idx = cv.encode_batch(specs, tr, SEG, noise_fn=noise, max_batch=max_batch, codebook=cb, want_idx=True, segment=lam)
    for overlap in (0, 16):
        kw = {'overlap': overlap} if overlap else {}
        if kind == 'vector':
            _, w = cv.synth_index_batch(idx, tr, SEG, spk, cb, n_iter=4, max_batch=max_batch, **kw)
        else:
            _, w = cv.synth_units_batch([cb.packed[i] for i in idx], tr, SEG, spk, n_iter=4, packed=True, max_batch=max_batch, **kw)
        e1, w1, idx1, total = cv.resynth_batch(specs, tr, SEG, spk, n_iter=4, noise_fn=noise, max_batch=max_batch, codebook=cb, want_idx=True,
                                               segment=lam, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(idx, idx1))
        assert all(np.array_equal(a, b) and len(a) > 0 for a, b in zip(w, w1)), overlap
        assert total >= 0
    # the summed distance is the path's: at lambda = 0 the nearest codewords', as without segment
    t0 = cv.resynth_batch(specs, tr, SEG, spk, n_iter=4, noise_fn=noise, codebook=cb, want_idx=True)[3]
    tz = cv.resynth_batch(specs, tr, SEG, spk, n_iter=4, noise_fn=noise, codebook=cb, want_idx=True, segment=0.0)[3]
    assert tz == t0 if kind == 'bit' else abs(tz - t0) <= 1e-5 * abs(t0)
    assert total >= tz
    layers.check_status(dev)


def test_segment_refusals_come_before_any_launch(dev, kinds, monkeypatch):
    from zs_amd import convert as cv, rvq, vq
    tr = kinds['vector'][0]
    specs = _specs_of_units((2, LU))
    rs = np.random.RandomState(0)
    res = rvq.ResidualCodebook((rs.randn(2, 16, 8) * 0.5).astype(np.float32))
    big = vq.VectorCodebook(rs.randn(4097, 8).astype(np.float32))
    calls = _count_calls(monkeypatch)
    for cb, match in ((res, 'residual codebook'), (big, '4096'), (None, 'needs a codebook')):
        with pytest.raises(ValueError, match=match):
            cv.encode_batch(specs, tr, SEG, codebook=cb, segment=1.0)
        with pytest.raises(ValueError, match=match):
            cv.resynth_batch(specs, tr, SEG, [2, 3], n_iter=4, codebook=cb, segment=1.0)
        with pytest.raises(ValueError, match=match):
            cv.convert_wavs([np.zeros(8000, np.float32)] * 2, None, tr, SEG, [2, 3], n_iter=4, codebook=cb, segment=1.0)
    for bad in (-1.0, float('nan'), float('inf'), 'x'):
        with pytest.raises(ValueError, match='lambda'):
            cv.encode_batch(specs, tr, SEG, codebook=kinds['vector'][1], segment=bad)
    with pytest.raises(ValueError, match='segment'):
        cv.encode_batch(specs, tr, SEG, decode_speakers=[2, 3], codebook=kinds['vector'][1], segment=1.0)
    assert calls == []


# ---- main.py -----------------------------------------------------------------------------------------------------------------------
def _tone(n, f0, seed):
    rng = np.random.RandomState(seed)
    t = np.arange(n) / 16000.0
    return (0.3 * np.sin(2 * np.pi * f0 * t) + 0.1 * np.sin(2 * np.pi * 2.7 * f0 * t) + 0.02 * rng.randn(n)).astype(np.float32)


def test_main_segment_on_a_folder(dev, tmp_path, monkeypatch, capsys):
    import json
    sys.path.insert(0, ROOT)
    import main as M
    from zs_amd import convert as cv, segment as S
    from zs_amd.hps import hp
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(hp, 'n_iter', 4)
    monkeypatch.setenv('ZS_CKPT_EVERY', '4')
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    h = json.load(open(os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')))
    h.update(n_speakers=4, n_target_speakers=2, batch_size=4, enc_pretrain_iters=4, max_to_keep=3, enc_size=8, emb_size=32, seg_len=SEG,
             load_model_list='encoder, decoder')
    hps_path = str(tmp_path / 'hps.json')
    json.dump(h, open(hps_path, 'w'))
    M.main(['--train_ae', '--synthetic', '--hps_path', hps_path, '--ckpt_dir', str(tmp_path / 'ck'), '--dtype', 'fp32'])
    ckpt = str(tmp_path / 'ck' / 'model.pth-ae-4')
    s2id = str(tmp_path / 'speaker2id.json')
    json.dump({'S015': 0, 'S020': 1, 'V001': 2, 'V002': 3}, open(s2id, 'w'))
    d = tmp_path / 'wavs'
    d.mkdir()
    lengths = {'long_a': 24000, 'long_b': 30100, 'short': 8000}
    for i, (name, n) in enumerate(sorted(lengths.items())):
        cv.write_wav(str(d / (name + '.wav')), _tone(n, 220.0 + 60.0 * i, i), 16000)
    common = ['--t_speaker', 'V001', '--enc_only', '--hps_path', hps_path, '--speaker2id_path', s2id, '--ckpt_pth', ckpt]
    book = str(tmp_path / 'K6.codebook.npz')
    torch.manual_seed(5)
    M.main(['--fit_codebook', '6', '--fit_dir', str(d), '--codebook_out', book, '--hps_path', hps_path, '--ckpt_pth', ckpt])
    outs = {}
    for tag, extra in (('plain', []), ('seg', ['--segment', '2'])):
        torch.manual_seed(11)                                             # the encoder's own noise: the same draws in both runs
        M.main(['--convert_dir', str(d), '--result_dir', str(tmp_path / tag), '--codebook', book] + extra + common)
        outs[tag] = os.path.join(str(tmp_path / tag), './english/', 'convert')
    m_plain = json.load(open(os.path.join(outs['plain'], 'convert_dir.json')))
    m_seg = json.load(open(os.path.join(outs['seg'], 'convert_dir.json')))
    assert set(m_seg) - set(m_plain) == {'segment'} and 'segment' not in m_plain          # the key is present in that run only
    assert not [f for f in os.listdir(os.path.join(outs['plain'], 'V001')) if f.endswith('.seg.txt')]
    seg = m_seg['segment']
    assert seg['lambda'] == 2.0 and len(m_seg['items']) == 3
    n_units = n_runs = 0
    for name in lengths:
        base = os.path.join(outs['seg'], 'V001', name)
        idx = cv.read_indices(base + '.idx.txt', 6)
        runs = S.read_segments(base + '.seg.txt', 6)
        assert np.array_equal(S.expand(runs), idx)                        # the .seg.txt expands to the .idx.txt
        assert len(open(base + '.txt').read().splitlines()) == len(idx)   # the per-frame files stay per frame
        n_units, n_runs = n_units + len(idx), n_runs + len(runs)
    assert seg['units'] == n_units and seg['segments'] == n_runs and abs(seg['mean_run_units'] - n_units / n_runs) < 1e-12
    assert 'Hamming bits' in capsys.readouterr().out
    # the run files just written, spoken: the wavs of the segmented conversion, byte for byte
    res = tmp_path / 'synth'
    M.main(['--synth_dir', os.path.join(outs['seg'], 'V001'), '--result_dir', str(res), '--codebook', book, '--segments'] + common)
    out = os.path.join(str(res), './english/', 'synth')
    m = json.load(open(os.path.join(out, 'synth_dir.json')))
    assert len(m['items']) == 3 and m['segment']['segments'] == n_runs and m['segment']['lambda'] is None
    for name in lengths:
        a = open(os.path.join(out, 'V001', name + '.wav'), 'rb').read()
        assert a == open(os.path.join(outs['seg'], 'V001', name + '.wav'), 'rb').read(), name
        assert open(os.path.join(out, 'V001', name + '.seg.txt')).read() == open(os.path.join(outs['seg'], 'V001', name + '.seg.txt')).read()
    res0 = tmp_path / 'synth0'
    M.main(['--synth_dir', os.path.join(outs['plain'], 'V001'), '--result_dir', str(res0), '--codebook', book] + common)
    assert 'segment' not in json.load(open(os.path.join(str(res0), './english/', 'synth', 'synth_dir.json')))
    capsys.readouterr()
