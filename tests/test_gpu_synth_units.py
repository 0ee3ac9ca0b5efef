"""Speech from unit files on the device (--synth_dir):

* zs_units_unpack against convert.unpack_units and zs_units_pack against convert.pack_units, the definitions, bit for bit;
* synth_units_batch against resynth_batch on the same utterances, bit for bit in fp32, with and without the generator, from plain and
  from packed units, deferred too; in bf16 within the bound two batchings of the same fragments are allowed;
* an utterance where the fragment rule on units differs from the rule on frames, against the Decoder module on the fragments named;
* what is refused before any launch;
* synth_dir / main.py --synth_dir on a temporary folder."""
import json
import os
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEG = 32
FRAMES = [200, 75, 45, 33, 20, 90]          # none = 0 or 1 (mod 32) above 64, none below MIN_LEN: pieces + tail, tail only, short ones
SPK = [2, 3, 2, 3, 2, 3]                    # target speakers: the generator converts to these only
STARTS, LENS, T_CHUNK, N_ROWS = [7, 30, 0, 12, 21], [5, 2, 3, 0, 5], 5, 40


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


def _rup(x, m):
    return (x + m - 1) // m * m


def _tdt(dtype):
    from zs_amd import _lib as L
    return (L.ZS_F32, torch.float32) if dtype == 'fp32' else (L.ZS_BF16, torch.bfloat16)


def _bits(t):
    """The raw bits of a float32 / bfloat16 tensor (so that -0 and NaN payloads count)."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _tables(dev, starts=STARTS, lens=LENS):
    return (torch.tensor(starts, dtype=torch.int64, device=dev), torch.tensor(lens, dtype=torch.int32, device=dev))


def _unpack(dev, dtype, packed, E, starts, lens, T, ld, n_room=None):
    """zs_units_unpack into a NaN buffer with room for n_room fragments and a guard of 64 elements behind them."""
    from zs_amd import _lib as L
    zdt, tdt = _tdt(dtype)
    n_room = n_room or len(starts)
    buf = torch.full((n_room * T * ld + 64,), float('nan'), dtype=tdt, device=dev)
    st, ln = _tables(dev, starts, lens)
    L.call('zs_units_unpack', 'ZsUnitsUnpack', torch.cuda.current_stream().cuda_stream, dtype=zdt, packed=L.ptr(packed),
           n_units=packed.shape[0], row_bytes=packed.shape[1], E=E, start=L.ptr(st), len=L.ptr(ln), n_frag=len(starts), T=T,
           dst=L.ptr(buf), ld_dst=ld)
    torch.cuda.synchronize()
    return buf


def _expected(units, E, starts, lens, T, ld, n_units):
    out = np.zeros((len(starts), T, ld), dtype=np.float32)
    for f, (s, n) in enumerate(zip(starts, lens)):
        if 0 <= n <= T and s >= 0 and s + n <= n_units:
            out[f, :n, :E] = units[s:s + n]
    return out


# ---- the two kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('E', [6, 20, 64, 1024])
def test_units_unpack_equals_unpack_units(dev, E, dtype):
    from zs_amd import convert as cv
    rng = np.random.RandomState(E)
    units = (rng.rand(N_ROWS, E) < 0.5).astype(np.float32)
    host = cv.pack_units(units)
    assert np.array_equal(cv.unpack_units(host, E), units)
    packed = torch.from_numpy(host).to(dev)
    _, tdt = _tdt(dtype)
    ld, n = _rup(E, 32), len(STARTS)
    buf = _unpack(dev, dtype, packed, E, STARTS, LENS, T_CHUNK, ld, n_room=n + 1)
    want = torch.from_numpy(_expected(units, E, STARTS, LENS, T_CHUNK, ld, N_ROWS)).to(dev, tdt)
    got = buf[:n * T_CHUNK * ld].view(n, T_CHUNK, ld)
    assert torch.equal(_bits(got), _bits(want))                      # the units, zero rows behind them, zero columns [E, ld)
    assert torch.isnan(buf[n * T_CHUNK * ld:]).all()                 # nothing past the chunk: the next fragment's room and the guard
    again = _unpack(dev, dtype, packed, E, STARTS, LENS, T_CHUNK, ld, n_room=n + 1)
    assert torch.equal(_bits(again[:n * T_CHUNK * ld]), _bits(buf[:n * T_CHUNK * ld]))
    # entries out of range give zero fragments and read nothing; the others are not disturbed
    for f, (s, ln_) in ((1, (N_ROWS - 1, 2)), (0, (-1, 5)), (4, (21, T_CHUNK + 1)), (2, (0, -3)), (1, (2 ** 40, 2))):
        starts, lens = list(STARTS), list(LENS)
        starts[f], lens[f] = s, ln_
        got = _unpack(dev, dtype, packed, E, starts, lens, T_CHUNK, ld)
        want = torch.from_numpy(_expected(units, E, starts, lens, T_CHUNK, ld, N_ROWS)).to(dev, tdt)
        assert (want[f] == 0).all()
        assert torch.equal(_bits(got[:n * T_CHUNK * ld].view(n, T_CHUNK, ld)), _bits(want)) and torch.isnan(got[n * T_CHUNK * ld:]).all()
    # bits above column E in a row's last byte (not what pack_units writes) do not reach the operand
    if E % 8:
        dirty = packed.clone()
        dirty[:, -1] |= (0xff << (E % 8)) & 0xff
        got = _unpack(dev, dtype, dirty, E, STARTS, LENS, T_CHUNK, ld)
        assert torch.equal(_bits(got[:n * T_CHUNK * ld]), _bits(buf[:n * T_CHUNK * ld]))


def _pack(dev, dtype, src, src_f32, ld_src, E, row_bytes, starts=STARTS, lens=LENS, T=T_CHUNK):
    from zs_amd import _lib as L
    zdt, _ = _tdt(dtype)
    out = torch.full((N_ROWS, row_bytes), 0xAA, dtype=torch.uint8, device=dev)
    st, ln = _tables(dev, starts, lens)
    L.call('zs_units_pack', 'ZsUnitsPack', torch.cuda.current_stream().cuda_stream, dtype=zdt, src_f32=int(src_f32), src=L.ptr(src),
           ld_src=ld_src, n_frag=len(starts), T=T, E=E, start=L.ptr(st), len=L.ptr(ln), packed=L.ptr(out), n_units=N_ROWS,
           row_bytes=row_bytes)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('E', [6, 20, 64, 1024])
def test_units_pack_equals_pack_units(dev, E, dtype):
    from zs_amd import convert as cv
    rng = np.random.RandomState(100 + E)
    n, T = len(STARTS), T_CHUNK
    x = (rng.rand(n, T, E) < 0.5).astype(np.float32)
    _, tdt = _tdt(dtype)
    nb = (E + 7) // 8
    want = np.full((N_ROWS, nb), 0xAA, dtype=np.uint8)
    for f, (s, ln_) in enumerate(zip(STARTS, LENS)):
        want[s:s + ln_] = cv.pack_units(x[f, :ln_])
    changed = np.zeros(N_ROWS, dtype=bool)
    for s, ln_ in zip(STARTS, LENS):
        changed[s:s + ln_] = True
    ld = _rup(E, 32)
    wide = np.ones((n, T, ld), dtype=np.float32)                     # ones in the columns [E, ld): they are not units
    wide[:, :, :E] = x
    for f, ln_ in enumerate(LENS):
        wide[f, ln_:] = 1.0                                          # rows t >= len: not read, nothing written for them
    layouts = [(torch.from_numpy(wide).to(dev, tdt), False, ld),     # the engine's own bits buffer: engine dtype, ld = rup(E, 32)
               (torch.from_numpy(wide).to(dev), True, ld),           # fp32 at the same pitch
               (torch.from_numpy(np.where(np.arange(T)[None, :, None] < np.array(LENS)[:, None, None], x, 1.0).astype(np.float32)).to(dev),
                True, E)]                                            # fp32 rows of E values back to back (E = 6, 20: no 16-byte loads)
    for src, f32, ld_src in layouts:
        got = _pack(dev, dtype, src, f32, ld_src, E, nb)
        assert np.array_equal(got.cpu().numpy(), want), (f32, ld_src)
        assert (got.cpu().numpy()[~changed] == 0xAA).all() and (~changed).any()
        # and back: zs_units_unpack of what zs_units_pack wrote gives the source's units
        back = _unpack(dev, dtype, got, E, STARTS, LENS, T, ld)[:n * T * ld].view(n, T, ld)
        for f, ln_ in enumerate(LENS):
            assert torch.equal(back[f, :ln_, :E].float().cpu(), torch.from_numpy(x[f, :ln_])) and (back[f, ln_:] == 0).all()
    # a wider packed row: the bytes behind the columns are written as zeros; an entry out of range writes nothing
    got = _pack(dev, dtype, layouts[0][0], False, ld, E, nb + 1)
    assert np.array_equal(got.cpu().numpy()[changed][:, :nb], want[changed]) and (got.cpu().numpy()[changed][:, nb] == 0).all()
    assert (got.cpu().numpy()[~changed] == 0xAA).all()
    for f, (s, ln_) in ((0, (N_ROWS - 2, 5)), (4, (-1, 5)), (1, (30, T + 1))):
        starts, lens = list(STARTS), list(LENS)
        starts[f], lens[f] = s, ln_
        got = _pack(dev, dtype, layouts[0][0], False, ld, E, nb, starts, lens).cpu().numpy()
        rows = np.arange(STARTS[f], STARTS[f] + LENS[f])
        assert (got[rows] == 0xAA).all()
        others = changed.copy()
        others[rows] = False
        assert np.array_equal(got[others], want[others]) and (got[~changed] == 0xAA).all()


def test_units_argument_errors_launch_nothing(dev):
    from zs_amd import _lib as L
    E, T, ld, n = 20, T_CHUNK, 32, len(STARTS)
    st_ = torch.cuda.current_stream().cuda_stream
    packed = torch.full((N_ROWS, 3), 0x55, dtype=torch.uint8, device=dev)
    start, length = _tables(dev)
    dst = torch.full((n * T * ld,), 7.0, device=dev)
    ok = dict(dtype=L.ZS_F32, packed=L.ptr(packed), n_units=N_ROWS, row_bytes=3, E=E, start=L.ptr(start), len=L.ptr(length), n_frag=n, T=T,
              dst=L.ptr(dst), ld_dst=ld)
    big = L.ENUMS['ZS_UNITS_MAX_FRAG'] + 1
    for change in (dict(packed=None), dict(start=None), dict(len=None), dict(dst=None), dict(E=0), dict(E=-4), dict(ld_dst=16), dict(ld_dst=E),
                   dict(n_frag=-1), dict(n_frag=big), dict(row_bytes=2), dict(T=0), dict(n_units=-1), dict(dtype=7),
                   dict(dst=L.ptr(dst) + 4)):
        with pytest.raises(L.ZsError, match='zs_units_unpack'):
            L.call('zs_units_unpack', 'ZsUnitsUnpack', st_, **dict(ok, **change))
    torch.cuda.synchronize()
    assert (dst == 7.0).all()
    L.call('zs_units_unpack', 'ZsUnitsUnpack', st_, **dict(ok, n_frag=0, dst=None, packed=None))     # an empty chunk succeeds
    torch.cuda.synchronize()
    assert (dst == 7.0).all()
    src = torch.ones(n * T * ld, device=dev)
    out = torch.full((N_ROWS, 3), 0xAA, dtype=torch.uint8, device=dev)
    ok = dict(dtype=L.ZS_F32, src_f32=1, src=L.ptr(src), ld_src=ld, n_frag=n, T=T, E=E, start=L.ptr(start), len=L.ptr(length),
              packed=L.ptr(out), n_units=N_ROWS, row_bytes=3)
    for change in (dict(src=None), dict(start=None), dict(len=None), dict(packed=None), dict(E=0), dict(ld_src=E - 1), dict(n_frag=-1),
                   dict(n_frag=big), dict(row_bytes=2), dict(T=-1), dict(n_units=-1), dict(dtype=7), dict(src=L.ptr(src) + 2)):
        with pytest.raises(L.ZsError, match='zs_units_pack'):
            L.call('zs_units_pack', 'ZsUnitsPack', st_, **dict(ok, **change))
    torch.cuda.synchronize()
    assert (out == 0xAA).all()
    L.call('zs_units_pack', 'ZsUnitsPack', st_, **dict(ok, n_frag=0, src=None, packed=None))
    torch.cuda.synchronize()
    assert (out == 0xAA).all()
    L.call('zs_units_pack', 'ZsUnitsPack', st_, **ok)                 # and the valid call writes: ones -> every column's bit
    torch.cuda.synchronize()
    assert out[7:12].cpu().tolist() == [[0xff, 0xff, 0x0f]] * 5 and (out[3:7] == 0xAA).all()


# ---- synthesis from units ------------------------------------------------------------------------------------------------------------
def _trainer(path, dtype='fp32', enc_mode='multilabel_binary', seed=3):
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    torch.manual_seed(seed)
    hps = make_hps(enc_size=8, emb_size=32, n_speakers=4, n_target_speakers=2, seg_len=SEG)
    return Trainer(hps, None, 'targeted_residual', enc_mode, log_dir=os.path.join(str(path), 'log'), dtype=dtype,
                   device=torch.device('cuda:0')), hps


def _field_noise(E, seed=1234, T=64):
    """noise_fn whose every batch position reads the same field: a fragment's noise does not depend on where it is batched."""
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
def fp32(dev, tmp_path_factory):
    """The small fp32 trainer and, computed once, the units of FRAMES: plain (encode_batch) and packed (encode_batch(packed=True))."""
    from zs_amd import convert as cv
    tr, hps = _trainer(tmp_path_factory.mktemp('fp32'))
    specs = _specs(FRAMES)
    noise_fn = _field_noise(8)
    e, _ = cv.encode_batch(specs, tr, SEG, noise_fn=noise_fn)
    ep, _ = cv.encode_batch(specs, tr, SEG, noise_fn=noise_fn, packed=True)
    return {'tr': tr, 'hps': hps, 'specs': specs, 'noise_fn': noise_fn, 'e': e, 'ep': ep}


def test_encode_batch_packed_equals_pack_units(dev, fp32):
    from zs_amd import convert as cv, layers
    for n, a, p in zip(FRAMES, fp32['e'], fp32['ep']):
        assert p.dtype == np.uint8 and p.shape == (len(a), 1) and len(a) == sum(cv.unit_fragments(len(a), SEG))
        assert np.array_equal(cv.unpack_units(p, 8), a) and np.array_equal(p, cv.pack_units(a))
    # the MIN_LEN truncation goes through len: an input shorter than MIN_LEN frames gives one unit, and the decoded rows come along
    short = _specs([5, 40], seed=9)
    e, d = cv.encode_batch(short, fp32['tr'], SEG, decode_speakers=[2, 3], noise_fn=fp32['noise_fn'])
    ep, dp = cv.encode_batch(short, fp32['tr'], SEG, decode_speakers=[2, 3], noise_fn=fp32['noise_fn'], packed=True)
    assert [len(p) for p in ep] == [1, 5] and all(np.array_equal(cv.unpack_units(p, 8), a) for p, a in zip(ep, e))
    assert all(np.array_equal(a, b) for a, b in zip(d, dp))
    layers.check_status(dev)


@pytest.mark.parametrize('enc_only', [True, False])
def test_synth_units_equals_resynth(dev, fp32, enc_only):
    from zs_amd import convert as cv, layers
    tr, specs, noise_fn = fp32['tr'], fp32['specs'], fp32['noise_fn']
    for n in FRAMES:
        assert n >= cv.MIN_LEN and not (n % SEG in (0, 1) and n > 2 * SEG)
    e, w = cv.resynth_batch(specs, tr, SEG, SPK, n_iter=4, noise_fn=noise_fn, enc_only=enc_only)
    assert all(np.array_equal(a, b) for a, b in zip(e, fp32['e']))
    assert [cv.unit_fragments(len(a), SEG) for a in e[:3]] == [[4, 4, 4, 4, 4, 5], [4, 6], [6]]
    none, w1 = cv.synth_units_batch(e, tr, SEG, SPK, enc_only=enc_only, n_iter=4)
    assert none is None and len(w1) == len(w)
    for a, b in zip(w, w1):
        assert b.dtype == np.float32 and len(b) > 0 and np.array_equal(a, b)
    _, w2 = cv.synth_units_batch(fp32['ep'], tr, SEG, SPK, enc_only=enc_only, n_iter=4, packed=True)
    assert all(np.array_equal(a, b) for a, b in zip(w, w2))
    # the spectrograms the vocoder was given, when asked for, change nothing
    s3, w3 = cv.synth_units_batch(e, tr, SEG, SPK, enc_only=enc_only, n_iter=4, want_specs=True)
    assert all(np.array_equal(a, b) for a, b in zip(w, w3)) and [s.shape for s in s3] == [(8 * len(a), 513) for a in e]
    if enc_only:
        _, d = cv.encode_batch(specs, tr, SEG, decode_speakers=SPK, noise_fn=noise_fn)
        assert all(np.array_equal(a, b) for a, b in zip(d, s3))
    # small chunks (several plain and ragged batches), and enqueued twice before the first wait
    fa = cv.synth_units_batch(e, tr, SEG, SPK, enc_only=enc_only, n_iter=4, defer=True, max_batch=3)
    fb = cv.synth_units_batch(fp32['ep'][:2], tr, SEG, SPK[:2], enc_only=enc_only, n_iter=4, defer=True, packed=True)
    _, wa = fa()
    _, wb = fb()
    assert all(np.array_equal(a, b) for a, b in zip(w, wa)) and all(np.array_equal(a, b) for a, b in zip(w[:2], wb))
    layers.check_status(dev)


def test_synth_units_bf16_within_the_ragged_bound(dev, tmp_path):
    """The decoded spectrograms of synth_units_batch against encode_batch's in bf16: the bound tests/test_gpu_ragged.py allows between
    two batchings of the same fragments, relative difference below 2e-2 of the maximum.  Here the batchings are the same, and on the
    MI355X the two were in fact bit-equal (the test prints which)."""
    from zs_amd import convert as cv, layers
    tr, _ = _trainer(tmp_path, dtype='bf16')
    specs, noise_fn = _specs(FRAMES), _field_noise(8)
    e, d = cv.encode_batch(specs, tr, SEG, decode_speakers=SPK, noise_fn=noise_fn)
    s, w = cv.synth_units_batch(e, tr, SEG, SPK, n_iter=4, want_specs=True)
    ep, _ = cv.encode_batch(specs, tr, SEG, noise_fn=noise_fn, packed=True)
    assert all(np.array_equal(cv.unpack_units(p, 8), a) for p, a in zip(ep, e))
    worst, same = 0.0, True
    for a, b in zip(d, s):
        assert a.shape == b.shape
        worst = max(worst, float(np.abs(a - b).max() / max(1e-6, np.abs(a).max())))
        same = same and np.array_equal(a, b)
    print('bf16: synth_units_batch vs encode_batch decoded spectrograms: bitwise equal %s, worst rel diff %.3g' % (same, worst))
    assert worst < 2e-2
    assert all(np.isfinite(x).all() and len(x) > 0 for x in w)
    layers.check_status(dev)


def test_synth_units_off_the_frame_rule(dev, fp32):
    """97 frames = 1 (mod 32): the frame rule cuts [4, 4, 4] units, unit_fragments [4, 8].  The synthesis is the Decoder on the
    fragments unit_fragments names."""
    from zs_amd import convert as cv, layers
    tr = fp32['tr']
    spec = _specs([97], seed=11)
    e, _ = cv.encode_batch(spec, tr, SEG, noise_fn=fp32['noise_fn'])
    assert [cv._t8(b - a) for a, b in cv.fragments(97, SEG)] == [4, 4, 4] and cv.unit_fragments(len(e[0]), SEG) == [4, 8]
    s, w = cv.synth_units_batch(e, tr, SEG, [3], n_iter=4, want_specs=True)
    assert s[0].shape == (96, 513) and len(w[0]) > 0 and np.isfinite(w[0]).all()
    at = 0
    for n in cv.unit_fragments(len(e[0]), SEG):
        bits = torch.from_numpy(e[0][at:at + n].T[None].copy()).to(dev)
        xd = tr.Decoder(bits, torch.tensor([3], device=dev))[0].T.cpu().numpy()
        assert np.abs(xd - s[0][8 * at:8 * (at + n)]).max() < 1e-6, (at, n)
        at += n
    layers.check_status(dev)


def test_synth_units_refusals_come_before_any_launch(dev, fp32, tmp_path, monkeypatch):
    from zs_amd import _lib as L, convert as cv
    tr, e = fp32['tr'], fp32['e']
    cont, _ = _trainer(tmp_path, enc_mode='continues')
    calls = []
    real = L.call
    monkeypatch.setattr(L, 'call', lambda *a, **k: (calls.append(a[0]), real(*a, **k))[1])
    with pytest.raises(ValueError, match='fewer than 2 units'):
        cv.synth_units_batch([e[0], e[1][:1]], tr, SEG, [2, 3], n_iter=4)
    with pytest.raises(ValueError, match='fewer than 2 units'):
        cv.synth_units_batch([cv.pack_units(e[1][:1])], tr, SEG, [2], n_iter=4, packed=True)
    with pytest.raises(ValueError, match='width'):
        cv.synth_units_batch([np.zeros((6, 9), np.float32)], tr, SEG, [2], n_iter=4)
    with pytest.raises(ValueError, match='packed units'):
        cv.synth_units_batch([np.zeros((6, 2), np.uint8)], tr, SEG, [2], n_iter=4, packed=True)
    with pytest.raises(ValueError, match='0 or 1'):
        cv.synth_units_batch([np.full((6, 8), 0.5, np.float32)], tr, SEG, [2], n_iter=4)
    with pytest.raises(RuntimeError, match='can only convert to target speakers'):
        cv.synth_units_batch(e[:2], tr, SEG, [2, 0], enc_only=False, n_iter=4)
    with pytest.raises(ValueError, match='outside'):
        cv.synth_units_batch(e[:2], tr, SEG, [2, 4], n_iter=4)
    with pytest.raises(ValueError, match='target speakers for'):
        cv.synth_units_batch(e[:2], tr, SEG, [2], n_iter=4)
    with pytest.raises(ValueError, match='continues'):
        cv.synth_units_batch(e[:2], cont, SEG, [2, 3], n_iter=4)
    with pytest.raises(ValueError, match='continues'):
        cv.encode_batch(fp32['specs'][:2], cont, SEG, packed=True)
    assert calls == []


# ---- synth_dir -------------------------------------------------------------------------------------------------------------------------
def test_synth_dir_on_a_folder(dev, fp32, tmp_path, monkeypatch, capsys):
    sys.path.insert(0, ROOT)
    import main as M
    from zs_amd import convert as cv, layers
    from zs_amd.hps import hp
    tr, hps, e = fp32['tr'], fp32['hps'], fp32['e']
    d = tmp_path / 'units'
    d.mkdir()
    names = ['u200', 'u075', 'u045', 'u033', 'u020', 'u090']
    for name, a in zip(names, e):                                     # the files a --test_encode / --convert_dir run writes
        cv.write_encodings(str(d / (name + '.txt')), a)
    (d / 'bad.txt').write_text('0 1 0 1 0 1 0 1\n0 1 2 1 0 1 0 1\n')
    cv.write_encodings(str(d / 'one.txt'), e[1][:1])
    (d / 'notes.md').write_text('ignored: not a *.txt')
    s2id = str(tmp_path / 'speaker2id.json')
    json.dump({'S015': 0, 'S020': 1, 'V001': 2, 'V002': 3}, open(s2id, 'w'))
    hps_path = str(tmp_path / 'hps.json')
    json.dump(hps._asdict(), open(hps_path, 'w'))
    tr.save_model(str(tmp_path / 'model.pth'), 's2', 1)
    monkeypatch.setattr(hp, 'n_iter', 4)

    def check(out, manifest, targets, rate):
        for t in targets:
            assert sorted(os.listdir(os.path.join(out, t))) == sorted(n + '.wav' for n in names)
            for n in names:
                with wave.open(os.path.join(out, t, n + '.wav'), 'rb') as f:
                    assert (f.getframerate(), f.getsampwidth(), f.getnchannels()) == (rate, 2, 1) and f.getnframes() > 0
        assert sorted(os.listdir(out)) == sorted(list(targets) + ['synth_dir.json'])
        assert json.load(open(os.path.join(out, 'synth_dir.json'))) == manifest
        assert sorted((os.path.basename(i['input']), i['target']) for i in manifest['items']) == sorted((n + '.txt', t) for n in names
                                                                                                        for t in targets)
        units = {n + '.txt': len(a) for n, a in zip(names, e)}
        for i in manifest['items']:
            assert i['wav'] == os.path.join(out, i['target'], os.path.basename(i['input'])[:-4] + '.wav') and os.path.exists(i['wav'])
            assert i['units'] == units[os.path.basename(i['input'])] and i['fragments'] == cv.unit_fragments(i['units'], SEG)
        skipped = {os.path.basename(s['input']): s['reason'] for s in manifest['skipped']}
        assert sorted(skipped) == ['bad.txt', 'one.txt']
        assert 'line 2' in skipped['bad.txt'] and 'cannot be read' in skipped['bad.txt'] and 'fewer than 2 units' in skipped['one.txt']

    with pytest.raises(RuntimeError, match='can only convert to target speakers'):
        cv.synth_dir(tr, SEG, str(d), s2id, str(tmp_path / 'refused'), ['V001', 'S015'], False)
    assert not (tmp_path / 'refused').exists()
    res = tmp_path / 'result'
    M.main(['--synth_dir', str(d), '--t_speaker', 'V001,V002', '--hps_path', hps_path, '--speaker2id_path', s2id,
            '--ckpt_pth', str(tmp_path / 'model.pth-s2-1'), '--result_dir', str(res), '--g_mode', 'targeted_residual'])
    out = os.path.join(os.path.join(str(res), './english/'), 'synth')           # {result_dir}/{sub_result_dir}/synth, as main.py joins them
    manifest = json.load(open(os.path.join(out, 'synth_dir.json')))
    check(out, manifest, ['V001', 'V002'], 16000)
    assert manifest['enc_only'] is False
    printed = capsys.readouterr().out
    assert 'skipped' in printed and 'bad.txt' in printed and 'one.txt' in printed
    # --out_sr; several groups (batch=2) with one group in flight while the previous one is written; autoencoder only
    monkeypatch.setattr(hp, 'out_sr', 22050)
    out2 = str(tmp_path / 'out2')
    m2 = cv.synth_dir(tr, SEG, str(d), s2id, out2, ['V002'], True, batch=2, n_iter=4)
    check(out2, m2, ['V002'], 22050)
    layers.check_status(dev)
