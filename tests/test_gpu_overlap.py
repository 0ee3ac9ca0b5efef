"""Overlapped decode windows on the device (--overlap):

* zs_xfade_gather against the numpy statement (tests/xfade_ref.py), bit for bit, over the alignments a row of 513 floats can have,
  de-normalised against zs_gen_scatter's own expression, and what it refuses;
* synth_units_batch / synth_index_batch(overlap=V) against the reference's blend of every window spoken alone through the existing
  path, bit for bit in fp32, with and without the generator, at two chunk sizes; in bf16 within the ragged bound;
* nothing changes without the option; resynth_batch(overlap=V) is encode_batch followed by synth_units_batch(overlap=V);
* main.py --convert_dir / --synth_dir --overlap on a temporary folder."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import xfade_ref as X  # noqa: E402

SEG, LU = 32, 4
UNITS = [2 * LU, 2 * LU + 1, 3 * LU + 2, 9 * LU]        # one window; the shortest with two; a tail of every length class; many joins
SPK_AE, SPK_GEN = [0, 1, 2, 3], [2, 3, 3, 2]            # distinct speakers; the generator converts to 2 and 3 only
NAN = float('nan')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


def _rup(x, m):
    return (x + m - 1) // m * m


# ---- the kernel --------------------------------------------------------------------------------------------------------------------
def _tables(rows, src_rows, seed):
    """Tables that hold every kind of row: blended, no source, a bad i0 (src_rows), a bad i1 (2^30), -2^31 in either, one source.
    The weights of rows that are not blended are NaN: they are not read."""
    rng = np.random.RandomState(seed)
    i0 = rng.randint(0, src_rows, rows).astype(np.int64)
    i1 = np.full(rows, -1, dtype=np.int64)
    w0 = np.full(rows, np.nan, dtype=np.float32)
    w1 = np.full(rows, np.nan, dtype=np.float32)
    for r in range(rows):
        kind = (r + 1) % 7
        if kind == 1:
            i1[r] = rng.randint(0, src_rows)
            w0[r], w1[r] = np.float32(rng.rand()), np.float32(rng.rand())
        elif kind == 2:
            i0[r] = -1
        elif kind == 3:
            i0[r] = src_rows
        elif kind == 4:
            i1[r], w0[r], w1[r] = 2 ** 30, 0.5, 0.5
        elif kind == 5:
            i0[r] = -2 ** 31
        elif kind == 6:
            i1[r], w0[r], w1[r] = -2 ** 31, 0.5, 0.5
    return i0.astype(np.int32), i1.astype(np.int32), w0, w1


def _launch(dev, src, src_rows, ld_src, tabs, rows, cols, out_ld, denorm, off, change=None):
    """zs_xfade_gather into a NaN buffer that starts `off` floats behind a 16-byte boundary, with a guard of 64 floats behind it.
    src: a flat device tensor that starts at the same offset.  Returns the whole output buffer."""
    from zs_amd import _lib as L
    out = torch.full((off + rows * out_ld + 64,), NAN, dtype=torch.float32, device=dev)
    assert out.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
    t = [torch.from_numpy(a).to(dev) for a in tabs]
    kw = dict(src=L.ptr(src, off), src_rows=src_rows, ld_src=ld_src, i0=L.ptr(t[0]), i1=L.ptr(t[1]), w0=L.ptr(t[2]), w1=L.ptr(t[3]),
              out=L.ptr(out, off), rows=rows, out_ld=out_ld, cols=cols, denorm=denorm)
    kw.update(change or {})
    L.call('zs_xfade_gather', 'ZsXfadeGather', torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    return out


def _lds(cols):
    return [cols, cols + 3, _rup(cols + 1, 4)]                       # the row itself, an odd pitch, a multiple of 4 above it


@pytest.mark.parametrize('cols', [1, 3, 4, 5, 513])
def test_xfade_gather_equals_the_reference(dev, cols):
    src_rows = 7
    rng = np.random.RandomState(cols)
    for ld_src in _lds(cols):
        for off in (0, 1):
            host = rng.randn(off + src_rows * ld_src + 4).astype(np.float32)
            src = torch.from_numpy(host).to(dev)
            table = host[off:off + src_rows * ld_src].reshape(src_rows, ld_src)
            for out_ld in _lds(cols):
                for rows in (1, 2, 257):
                    tabs = _tables(rows, src_rows, rows + out_ld)
                    out = _launch(dev, src, src_rows, ld_src, tabs, rows, cols, out_ld, 0, off).cpu().numpy()
                    body = out[off:off + rows * out_ld].reshape(rows, out_ld)
                    want = X.gather(table, *tabs, cols)
                    where = (cols, ld_src, out_ld, rows, off)
                    assert np.array_equal(body[:, :cols].view(np.int32), want.view(np.int32)), where
                    assert np.isnan(body[:, cols:]).all() and np.isnan(out[:off]).all() and np.isnan(out[off + rows * out_ld:]).all(), where
    # every kind of row was there, and the rows without a source are zeros
    i0, i1, w0, w1 = _tables(257, src_rows, 0)
    assert ((i1 >= 0) & (i1 < src_rows)).any() and (i0 == -1).any() and (i0 == src_rows).any() and (i1 == 2 ** 30).any()
    assert (i0 == -2 ** 31).any() and (i1 == -2 ** 31).any() and ((i1 == -1) & (i0 >= 0) & (i0 < src_rows)).any()
    assert not X.gather(np.ones((src_rows, 2), np.float32), i0, i1, w0, w1, 2)[(i0 < 0) | (i0 >= src_rows) | (i1 < -1) | (i1 >= src_rows)].any()


def test_xfade_gather_denormalised_is_gen_scatters_expression(dev):
    from zs_amd import _lib as L
    src_rows, rows, cols, off = 9, 257, 513, 1
    rng = np.random.RandomState(5)
    host = (rng.rand(off + src_rows * cols + 4) * 1.4 - 0.2).astype(np.float32)          # below 0 and above 1 too: the clip is part of it
    src = torch.from_numpy(host).to(dev)
    tabs = _tables(rows, src_rows, 11)
    plain = _launch(dev, src, src_rows, cols, tabs, rows, cols, cols, 0, off)
    amp = _launch(dev, src, src_rows, cols, tabs, rows, cols, cols, 1, off)
    want = torch.full_like(plain, NAN)
    dst = torch.arange(rows, dtype=torch.int32, device=dev)
    L.call('zs_gen_scatter', 'ZsGenScatter', torch.cuda.current_stream().cuda_stream, xd=L.ptr(plain, off), ld_xd=cols, dst=L.ptr(dst),
           rows=rows, amp=L.ptr(want, off), amp_ld=cols, amp_rows=rows, mode=0, denorm=1)
    torch.cuda.synchronize()
    a, b = amp[off:off + rows * cols], want[off:off + rows * cols]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.isnan(amp[:off]).all() and torch.isnan(amp[off + rows * cols:]).all()
    ref = X.denorm(plain[off:off + rows * cols].cpu().numpy())
    assert np.abs(a.cpu().numpy() - ref).max() <= 1e-4 * ref.max()                      # and it is the expression of convert.py:56-58


def test_xfade_gather_refusals_launch_nothing(dev):
    from zs_amd import _lib as L
    src_rows, rows, cols = 5, 6, 513
    src = torch.ones(src_rows * cols + 4, device=dev)
    tabs = (np.zeros(rows, np.int32), np.full(rows, -1, np.int32), np.ones(rows, np.float32), np.ones(rows, np.float32))
    out = torch.full((rows * cols + 64,), NAN, device=dev)
    t = [torch.from_numpy(a).to(dev) for a in tabs]
    ok = dict(src=L.ptr(src), src_rows=src_rows, ld_src=cols, i0=L.ptr(t[0]), i1=L.ptr(t[1]), w0=L.ptr(t[2]), w1=L.ptr(t[3]), out=L.ptr(out),
              rows=rows, out_ld=cols, cols=cols, denorm=0)
    for change in (dict(src=None), dict(i0=None), dict(i1=None), dict(w0=None), dict(w1=None), dict(out=None), dict(rows=-1),
                   dict(src_rows=-1), dict(ld_src=-1), dict(out_ld=-1), dict(cols=-1), dict(ld_src=cols - 1), dict(out_ld=cols - 1),
                   dict(cols=cols + 1), dict(rows=2 ** 31), dict(rows=2 ** 40), dict(rows=2 ** 31, denorm=1)):
        with pytest.raises(L.ZsError, match='zs_xfade_gather'):
            L.call('zs_xfade_gather', 'ZsXfadeGather', torch.cuda.current_stream().cuda_stream, **dict(ok, **change))
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    L.call('zs_xfade_gather', 'ZsXfadeGather', torch.cuda.current_stream().cuda_stream, rows=0, cols=cols, ld_src=cols, out_ld=cols)   # nothing to do
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    good = _launch(dev, src, src_rows, cols, tabs, rows, cols, cols, 0, 0)               # and the valid call writes
    assert (good[:rows * cols] == 1).all() and torch.isnan(good[rows * cols:]).all()


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def _trainer(path, dtype='fp32', enc_mode='multilabel_binary', seed=3):
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    torch.manual_seed(seed)
    hps = make_hps(enc_size=8, emb_size=32, n_speakers=4, n_target_speakers=2, seg_len=SEG)
    return Trainer(hps, None, 'targeted_residual', enc_mode, log_dir=os.path.join(str(path), 'log'), dtype=dtype,
                   device=torch.device('cuda:0')), hps


def _field_noise(E, seed=1234, T=64):
    U = torch.rand(T, E, 2, generator=torch.Generator().manual_seed(seed))
    base = (-torch.log(-torch.log(U + 1e-20) + 1e-20)).cuda()

    def noise_fn(n, t, e):
        assert e == E and t <= base.shape[0]
        return base[:t].unsqueeze(0).expand(n, t, E, 2).contiguous()
    return noise_fn


def _specs(frames, seed=7):
    rng = np.random.RandomState(seed)
    return [(rng.rand(n, 513) * 0.98 + 1e-3).astype(np.float32) for n in frames]


@pytest.fixture(scope='module')
def bits(dev, tmp_path_factory):
    tr, hps = _trainer(tmp_path_factory.mktemp('bits'))
    rng = np.random.RandomState(21)
    return {'tr': tr, 'hps': hps, 'units': [(rng.rand(n, 8) < 0.5).astype(np.float32) for n in UNITS]}


@pytest.fixture(scope='module')
def cont(dev, tmp_path_factory):
    """The 'continues' trainer, a vector codebook (K = 16) and a residual one (K = 16, S = 3), and index sequences of UNITS."""
    from zs_amd import rvq, vq
    tr, _ = _trainer(tmp_path_factory.mktemp('cont'), enc_mode='continues')
    rng = np.random.RandomState(22)
    vec = vq.VectorCodebook((rng.randn(16, 8) * 0.5).astype(np.float32))
    res = rvq.ResidualCodebook((rng.randn(3, 16, 8) * np.array([0.5, 0.2, 0.1])[:, None, None]).astype(np.float32))
    return {'tr': tr, 'vec': vec, 'res': res, 'idx': [rng.randint(0, 16, (n, 3)).astype(np.int32) for n in UNITS]}


def _check_definition(speak, seqs, spk, V, enc_only):
    """speak(seqs, speakers, **kw) -> synth_*_batch's result.  The overlapped spectrograms against the blend of every window spoken
    alone, as an utterance of its own, through the path without overlap; the wavs against the vocoder on those spectrograms."""
    from zs_amd import convert as cv
    wins = [X.windows(len(s), SEG, V) for s in seqs]
    alone = [s[a:b] for s, ws in zip(seqs, wins) for a, b in ws]
    alone_spk = [c for c, ws in zip(spk, wins) for _ in ws]
    dec, _ = speak(alone, alone_spk, enc_only=enc_only, n_iter=4, want_specs=True)
    want, at = [], 0
    for ws in wins:
        want.append(X.blend_windows(ws, dec[at:at + len(ws)]))
        at += len(ws)
    assert [len(ws) for ws in wins] == [1, 2] + [len(ws) for ws in wins[2:]] and len(wins[3]) > 8
    for max_batch in (256, 3):
        got, wavs = speak(seqs, spk, enc_only=enc_only, n_iter=4, want_specs=True, overlap=V, max_batch=max_batch)
        for u, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape == (8 * len(seqs[u]), 513) and np.array_equal(a.view(np.int32), b.view(np.int32)), (u, max_batch)
    assert not np.array_equal(got[1], np.concatenate(dec[1:3])[:len(got[1])])            # a join was blended, not cut
    ref_wavs = cv.spectrogram2wav_batch(got, n_iter=4)
    none, wavs2 = speak(seqs, spk, enc_only=enc_only, n_iter=4, overlap=V)               # the gather de-normalises: the same wavs
    assert none is None
    for a, b, c in zip(wavs, ref_wavs, wavs2):
        assert a.dtype == np.float32 and len(a) > 0 and np.array_equal(a, b) and np.array_equal(a, c)


@pytest.mark.parametrize('V', [8, 16])
@pytest.mark.parametrize('enc_only', [True, False])
def test_synth_units_overlap_is_the_blend_of_the_windows(dev, bits, enc_only, V):
    from zs_amd import convert as cv, layers
    tr = bits['tr']
    _check_definition(lambda u, c, **kw: cv.synth_units_batch(u, tr, SEG, c, **kw), bits['units'], SPK_AE if enc_only else SPK_GEN, V, enc_only)
    layers.check_status(dev)


@pytest.mark.parametrize('V', [8, 16])
@pytest.mark.parametrize('enc_only', [True, False])
@pytest.mark.parametrize('book', ['vector', 'residual1', 'residual3'])
def test_synth_index_overlap_is_the_blend_of_the_windows(dev, cont, book, enc_only, V):
    from zs_amd import convert as cv, layers
    tr = cont['tr']
    if book == 'vector':
        cb, seqs = cont['vec'], [i[:, 0].copy() for i in cont['idx']]
    else:
        cb, seqs = cont['res'], [np.ascontiguousarray(i[:, :int(book[-1])]) for i in cont['idx']]
    _check_definition(lambda u, c, **kw: cv.synth_index_batch(u, tr, SEG, c, cb, **kw), seqs, SPK_AE if enc_only else SPK_GEN, V, enc_only)
    layers.check_status(dev)


def _count_calls(monkeypatch):
    from zs_amd import _lib as L
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda *a, **k: (calls.append(a[0]), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize('enc_only', [True, False])
def test_nothing_changes_without_overlap(dev, bits, enc_only, monkeypatch):
    from zs_amd import convert as cv
    tr, units = bits['tr'], bits['units']
    spk = SPK_AE if enc_only else SPK_GEN
    calls = _count_calls(monkeypatch)
    s0, w0 = cv.synth_units_batch(units, tr, SEG, spk, enc_only=enc_only, n_iter=4, want_specs=True)
    plain = list(calls)
    del calls[:]
    s1, w1 = cv.synth_units_batch(units, tr, SEG, spk, enc_only=enc_only, n_iter=4, want_specs=True, overlap=0)
    assert calls == plain and 'zs_xfade_gather' not in calls                             # launch for launch, none of them the new one
    assert all(np.array_equal(a, b) for a, b in zip(s0, s1)) and all(np.array_equal(a, b) for a, b in zip(w0, w1))
    del calls[:]
    # utterances of at most 2 Lu units are one window each: the same wavs with and without the overlap
    short = [units[3][:n] for n in (2, LU, LU + 1, 2 * LU)]
    _, wa = cv.synth_units_batch(short, tr, SEG, spk, enc_only=enc_only, n_iter=4, overlap=16)
    assert calls.count('zs_xfade_gather') == 1
    _, wb = cv.synth_units_batch(short, tr, SEG, spk, enc_only=enc_only, n_iter=4, overlap=0)
    _, wc = cv.synth_units_batch(short, tr, SEG, spk, enc_only=enc_only, n_iter=4)
    assert all(np.array_equal(a, b) and np.array_equal(a, c) and len(a) > 0 for a, b, c in zip(wa, wb, wc))
    # a refused value is refused before any launch
    del calls[:]
    for bad in (4, 12, 24):
        with pytest.raises(ValueError, match='overlap must be'):
            cv.synth_units_batch(units, tr, SEG, spk, enc_only=enc_only, n_iter=4, overlap=bad)
    assert calls == []


# ---- conversion --------------------------------------------------------------------------------------------------------------------
FRAMES = [200, 75, 45, 33, 20, 90, 300]
SPK = [2, 3, 2, 3, 2, 3, 2]


@pytest.mark.parametrize('enc_only', [True, False])
def test_resynth_overlap_is_encode_then_synth(dev, bits, enc_only, monkeypatch):
    from zs_amd import codebook as C, convert as cv, layers
    tr = bits['tr']
    specs, noise_fn = _specs(FRAMES), _field_noise(8)
    e, _ = cv.encode_batch(specs, tr, SEG, noise_fn=noise_fn)
    assert max(len(a) for a in e) > 2 * LU and min(len(a) for a in e) <= 2 * LU
    _, w = cv.synth_units_batch(e, tr, SEG, SPK, enc_only=enc_only, n_iter=4, overlap=16)
    calls = _count_calls(monkeypatch)
    e1, w1 = cv.resynth_batch(specs, tr, SEG, SPK, n_iter=4, noise_fn=noise_fn, enc_only=enc_only, overlap=16)
    assert calls.count('zs_xfade_gather') == 1
    assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(e, e1))
    assert all(np.array_equal(a, b) and len(a) > 0 for a, b in zip(w, w1))
    _, w_cut = cv.resynth_batch(specs, tr, SEG, SPK, n_iter=4, noise_fn=noise_fn, enc_only=enc_only)
    assert not np.array_equal(w_cut[0], w1[0])                                           # the long utterance is joined differently
    # deferred, two batches in flight, small chunks
    fa = cv.resynth_batch(specs, tr, SEG, SPK, n_iter=4, noise_fn=noise_fn, enc_only=enc_only, overlap=16, defer=True, max_batch=3)
    fb = cv.resynth_batch(specs[:2], tr, SEG, SPK[:2], n_iter=4, noise_fn=noise_fn, enc_only=enc_only, overlap=16, defer=True)
    ea, wa = fa()
    eb, wb = fb()
    ref3, _ = cv.encode_batch(specs, tr, SEG, noise_fn=noise_fn, max_batch=3)
    _, w3 = cv.synth_units_batch(ref3, tr, SEG, SPK, enc_only=enc_only, n_iter=4, overlap=16, max_batch=3)
    assert all(np.array_equal(a, b) for a, b in zip(ea, ref3)) and all(np.array_equal(a, b) for a, b in zip(wa, w3))
    assert all(np.array_equal(a, b) for a, b in zip(eb, e[:2])) and all(np.array_equal(a, b) for a, b in zip(wb, w[:2]))
    # a bit codebook with want_idx: the snapped units, their indices, and the speech of the snapped units
    cb = C.fit(torch.from_numpy(np.concatenate([cv.pack_units(a) for a in e])).to(dev), 8, E=8)
    es, _, idx = cv.encode_batch(specs, tr, SEG, noise_fn=noise_fn, codebook=cb, want_idx=True)
    _, ws = cv.synth_units_batch(es, tr, SEG, SPK, enc_only=enc_only, n_iter=4, overlap=16)
    e2, w2, idx2, total = cv.resynth_batch(specs, tr, SEG, SPK, n_iter=4, noise_fn=noise_fn, enc_only=enc_only, overlap=16, codebook=cb,
                                           want_idx=True)
    assert all(np.array_equal(a, b) for a, b in zip(es, e2)) and all(np.array_equal(a, b) for a, b in zip(idx, idx2)) and total >= 0
    assert all(np.array_equal(a, b) for a, b in zip(ws, w2))
    layers.check_status(dev)


def test_resynth_overlap_under_vector_and_residual_codebooks(dev, cont):
    from zs_amd import convert as cv, layers
    tr = cont['tr']
    specs = _specs(FRAMES)
    for cb in (cont['vec'], cont['res'], cont['res'].with_stages(2)):
        e, _, idx = cv.encode_batch(specs, tr, SEG, codebook=cb, want_idx=True)
        _, w = cv.synth_index_batch(idx, tr, SEG, SPK, cb, n_iter=4, overlap=8)
        res = cv.resynth_batch(specs, tr, SEG, SPK, n_iter=4, overlap=8, codebook=cb, want_idx=True)
        assert all(np.array_equal(a, b) for a, b in zip(e, res[0])) and all(np.array_equal(a, b) for a, b in zip(idx, res[2]))
        assert all(np.array_equal(a, b) and len(a) > 0 for a, b in zip(w, res[1]))
    layers.check_status(dev)


def test_resynth_overlap_refusals_come_before_any_launch(dev, bits, cont, monkeypatch):
    from zs_amd import convert as cv
    calls = _count_calls(monkeypatch)
    specs = _specs([200, 75])
    with pytest.raises(ValueError, match=r"overlap = 16 .*'continues'"):
        cv.resynth_batch(specs, cont['tr'], SEG, [2, 3], n_iter=4, overlap=16)
    with pytest.raises(ValueError, match=r"overlap = 16 .*'continues'"):
        cv.convert_wavs([np.zeros(8000, np.float32)], None, cont['tr'], SEG, [2], n_iter=4, overlap=16)
    with pytest.raises(ValueError, match='overlap must be'):
        cv.resynth_batch(specs, bits['tr'], SEG, [2, 3], n_iter=4, overlap=12)
    with pytest.raises(ValueError, match='overlap = 16 .*utterance 1 returns 1'):
        cv.resynth_batch(_specs([200, 5]), bits['tr'], SEG, [2, 3], n_iter=4, overlap=16)
    with pytest.raises(RuntimeError, match='can only convert to target speakers'):
        cv.resynth_batch(specs, bits['tr'], SEG, [2, 0], n_iter=4, overlap=16, enc_only=False)
    assert calls == []


def test_overlap_bf16_within_the_ragged_bound(dev, tmp_path):
    """The overlapped spectrogram against the same blend of the per-window bf16 decodes, within the bound
    test_synth_units_bf16_within_the_ragged_bound uses between two batchings of the same fragments: 2e-2 of the maximum."""
    from zs_amd import convert as cv, layers
    tr, _ = _trainer(tmp_path, dtype='bf16')
    rng = np.random.RandomState(23)
    units = [(rng.rand(n, 8) < 0.5).astype(np.float32) for n in UNITS]
    wins = [X.windows(len(s), SEG, 16) for s in units]
    alone = [s[a:b] for s, ws in zip(units, wins) for a, b in ws]
    dec, _ = cv.synth_units_batch(alone, tr, SEG, [c for c, ws in zip(SPK_AE, wins) for _ in ws], n_iter=4, want_specs=True)
    got, w = cv.synth_units_batch(units, tr, SEG, SPK_AE, n_iter=4, want_specs=True, overlap=16)
    worst, same, at = 0.0, True, 0
    for ws, g in zip(wins, got):
        want = X.blend_windows(ws, dec[at:at + len(ws)])
        at += len(ws)
        assert g.shape == want.shape
        worst = max(worst, float(np.abs(g - want).max() / max(1e-6, np.abs(want).max())))
        same = same and np.array_equal(g, want)
    print('bf16: overlapped spectrograms vs the blend of the windows alone: bitwise equal %s, worst rel diff %.3g' % (same, worst))
    assert worst < 2e-2
    assert all(np.isfinite(x).all() and len(x) > 0 for x in w)
    layers.check_status(dev)


# ---- main.py -----------------------------------------------------------------------------------------------------------------------
def _tone(n, f0, seed):
    rng = np.random.RandomState(seed)
    t = np.arange(n) / 16000.0
    return (0.3 * np.sin(2 * np.pi * f0 * t) + 0.1 * np.sin(2 * np.pi * 2.7 * f0 * t) + 0.02 * rng.randn(n)).astype(np.float32)


def test_main_overlap_on_a_folder(dev, tmp_path, monkeypatch, capsys):
    sys.path.insert(0, ROOT)
    import main as M
    from zs_amd import convert as cv
    from zs_amd.hps import hp
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(hp, 'n_iter', 4)                             # (--gl_iters would leave hp changed behind this test)
    monkeypatch.setenv('ZS_CKPT_EVERY', '4')
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    h = json.load(open(os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')))
    h.update(n_speakers=4, n_target_speakers=2, batch_size=4, enc_pretrain_iters=4, max_to_keep=3, enc_size=8, emb_size=32, seg_len=SEG,
             load_model_list='encoder, decoder')
    hps_path = str(tmp_path / 'hps.json')
    json.dump(h, open(hps_path, 'w'))
    M.main(['--train_ae', '--synthetic', '--hps_path', hps_path, '--ckpt_dir', str(tmp_path / 'ck'), '--dtype', 'fp32'])
    ckpt = str(tmp_path / 'ck' / 'model.pth-ae-4')
    assert os.path.exists(ckpt)
    s2id = str(tmp_path / 'speaker2id.json')
    json.dump({'S015': 0, 'S020': 1, 'V001': 2, 'V002': 3}, open(s2id, 'w'))
    d = tmp_path / 'wavs'
    d.mkdir()
    lengths = {'long_a': 24000, 'long_b': 30100, 'short': 8000}       # 121 and 151 frames (more than 2 seg_len), 41 frames
    for i, (name, n) in enumerate(sorted(lengths.items())):
        cv.write_wav(str(d / (name + '.wav')), _tone(n, 220.0 + 60.0 * i, i), 16000)
    common = ['--t_speaker', 'V001', '--enc_only', '--hps_path', hps_path, '--speaker2id_path', s2id, '--ckpt_pth', ckpt]
    outs = {}
    for tag, extra in (('cut', []), ('over', ['--overlap', '16'])):
        torch.manual_seed(11)                                        # the encoder's own noise: the same draws in both runs
        res = tmp_path / tag
        M.main(['--convert_dir', str(d), '--result_dir', str(res)] + extra + common)
        outs[tag] = os.path.join(str(res), './english/', 'convert')
    m_cut = json.load(open(os.path.join(outs['cut'], 'convert_dir.json')))
    m_over = json.load(open(os.path.join(outs['over'], 'convert_dir.json')))
    assert 'overlap' not in m_cut and m_over['overlap'] == 16 and len(m_cut['items']) == len(m_over['items']) == 3
    assert set(m_over) - set(m_cut) == {'overlap'}

    def blob(root, name):
        return open(os.path.join(root, 'V001', name), 'rb').read()
    units = {}
    for name in lengths:
        assert blob(outs['cut'], name + '.txt') == blob(outs['over'], name + '.txt')      # the units do not change
        units[name] = len(blob(outs['cut'], name + '.txt').splitlines())
        same = blob(outs['cut'], name + '.wav') == blob(outs['over'], name + '.wav')
        assert same == (name == 'short'), name
    assert units['short'] <= 2 * LU < min(units['long_a'], units['long_b'])
    # the unit files just written, spoken with the overlap: the wavs of the overlapped conversion
    res = tmp_path / 'synth'
    M.main(['--synth_dir', os.path.join(outs['over'], 'V001'), '--result_dir', str(res), '--overlap', '16'] + common)
    out = os.path.join(str(res), './english/', 'synth')
    m = json.load(open(os.path.join(out, 'synth_dir.json')))
    assert m['overlap'] == 16 and len(m['items']) == 3
    for it in m['items']:
        name = os.path.basename(it['input'])[:-4]
        assert it['units'] == units[name] and it['fragments'] == [b - a for a, b in X.windows(it['units'], SEG, 16)]
        assert blob(out, name + '.wav') == blob(outs['over'], name + '.wav')
    res0 = tmp_path / 'synth0'
    M.main(['--synth_dir', os.path.join(outs['over'], 'V001'), '--result_dir', str(res0)] + common)
    m0 = json.load(open(os.path.join(str(res0), './english/', 'synth', 'synth_dir.json')))
    assert 'overlap' not in m0 and all(it['fragments'] == cv.unit_fragments(it['units'], SEG) for it in m0['items'])
    capsys.readouterr()
