"""Batched voice conversion through the stage-2 generator (convert.py:151-168 with enc_only=False, trainer.py:198-213) and
--cross_test (convert.py:268-300).

* zs_gen_scatter against the unfused sequence it replaces (combine, padded gather, zs_gl_denormalize), bit for bit;
* encode_batch(enc_only=False) against Trainer.test_step fragment by fragment with the same Gumbel noise, bit for bit, for every
  generator mode that is built, in fp32 and bf16; and against the oracle's gen_step;
* resynth_batch(enc_only=False) against encode_batch + spectrogram2wav_batch of the converted spectrograms;
* the host-side target check, and main.py --cross_test end to end on a store written by zs_amd.preprocess."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G_MODES = ['naive', 'targeted', 'targeted_residual', 'spectrogram']


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


def _t8(n):
    return ((((n + 1) // 2 + 1) // 2) + 1) // 2


def _trainer(g_mode, dtype, tmp_path, seed=0):
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    torch.manual_seed(seed)
    hps = make_hps(enc_size=16, emb_size=32, n_speakers=4, n_target_speakers=2)
    return Trainer(hps, None, g_mode, 'multilabel_binary', log_dir=str(tmp_path / 'log'), dtype=dtype, device=torch.device('cuda:0'))


def _gumbel(U):
    return -torch.log(-torch.log(U + 1e-20) + 1e-20)


def _field_noise(E, seed=1234, T=128):
    """noise_fn whose every batch position reads the same field: a fragment's noise is base[:T'] wherever it is batched."""
    base = _gumbel(torch.rand(T, E, 2, generator=torch.Generator().manual_seed(seed))).cuda()

    def noise_fn(n, t, e):
        assert e == E and t <= base.shape[0]
        return base[:t].unsqueeze(0).expand(n, t, E, 2).contiguous()
    return base, noise_fn


def _specs(rng, lens):
    return [np.clip(rng.rand(n, 513).astype(np.float32), 1e-8, 1) for n in lens]


def _per_fragment(tr, spec, c, base, seg_len=128):
    """convert() fragment by fragment through Trainer.test_step(enc_only=False) -> (converted [T_out, 513], encodings)."""
    from zs_amd import convert as cv
    spec, padded = cv._pad_min(spec)
    frags = [(0, len(spec))] if len(spec) <= seg_len else cv.fragments(len(spec), seg_len)
    outs, encs = [], []
    for a, b in frags:
        x = torch.from_numpy(np.ascontiguousarray(spec[a:b])[None]).float()
        G = base[:_t8(b - a)].unsqueeze(0).contiguous()
        xd, enc = tr.test_step(x, torch.tensor([c]), enc_only=False, verbose=False, G=G)
        outs.append(xd[0].T)
        encs.append(enc[0].T)
    enc = np.concatenate(encs, axis=0)
    if padded:
        enc = enc[:cv.MIN_LEN // 8]
    return np.concatenate(outs, axis=0), enc


# ---- kernel ----------------------------------------------------------------------------------------------------------------------
def _scatter(cv, L, xd, m, ld_xd, ld_m, dst, conv, mode, denorm):
    st = torch.cuda.current_stream().cuda_stream
    L.call('zs_gen_scatter', 'ZsGenScatter', st, xd=L.ptr(xd), ld_xd=ld_xd, m=L.ptr(m), ld_m=ld_m, dst=L.ptr(dst), rows=dst.numel(),
           amp=L.ptr(conv), amp_ld=conv.shape[2], amp_rows=conv.shape[0] * conv.shape[1], mode=mode, denorm=denorm)


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_gen_scatter_equals_combine_gather_denormalise(dev, mode):
    """Two ragged chunks (ld 544 and 600) scattered into a padded [n_utt, T_max, 513] buffer: bitwise equal to the unfused
    sequence -- combine (xd; zs_gen_combine_fwd add mode; torch xd + xd*m), padded gather, zs_gl_denormalize."""
    from zs_amd import _lib as L, convert as cv
    g = torch.Generator().manual_seed(10 + mode)
    # utterance u's frames, in order: (chunk, sample, rows) pieces; utterance 2 is shorter (padding rows)
    chunk_shapes = [(3, 48, 544), (2, 40, 600)]                       # (B, T, ld)
    pieces = {0: [(0, 0, 48), (1, 1, 40)], 1: [(0, 2, 48), (1, 0, 24)], 2: [(0, 1, 16)]}
    ulens = [sum(n for _, _, n in p) for u, p in sorted(pieces.items())]
    n_utt, Tm = len(ulens), max(ulens)
    xds, ms = [], []
    for B, T, ld in chunk_shapes:
        xd = torch.rand(B * T, ld, generator=g)
        m = torch.rand(B * T, ld, generator=g) * 2 - 1 if mode != 1 else torch.rand(B * T, ld, generator=g) * 0.5 - 0.25
        xds.append(xd.to(dev)); ms.append(m.to(dev))
    dsts = [np.full(B * T, -1, dtype=np.int32) for B, T, _ in chunk_shapes]
    for u, p in pieces.items():
        at = 0
        for ci, b, n in p:
            T = chunk_shapes[ci][1]
            dsts[ci][b * T:b * T + n] = np.arange(u * Tm + at, u * Tm + at + n)
            at += n
    for denorm in (1, 0):
        conv = torch.full((n_utt, Tm, 513), float('nan'), device=dev)
        for ci, (B, T, ld) in enumerate(chunk_shapes):
            _scatter(cv, L, xds[ci], ms[ci], ld, ld, torch.from_numpy(dsts[ci]).to(dev), conv, mode, denorm)
        pad = np.concatenate([np.arange(u * Tm + ulens[u], (u + 1) * Tm, dtype=np.int32) for u in range(n_utt)])
        zero = torch.zeros(513, device=dev)
        _scatter(cv, L, zero, None, 0, 0, torch.from_numpy(pad).to(dev), conv, 0, denorm)
        # the unfused chain
        comb = []
        for ci, (B, T, ld) in enumerate(chunk_shapes):
            xd, m = xds[ci], ms[ci]
            if mode == 0:
                c = xd[:, :513].clone()
            elif mode == 1:
                c = torch.empty(B * T, 513, device=dev)
                L.check(L.lib().zs_gen_combine_fwd(L.ptr(xd), L.ptr(m), ld, L.ptr(c), B * T, 513, 0, torch.cuda.current_stream().cuda_stream),
                        'zs_gen_combine_fwd')
            else:
                c = xd[:, :513] + xd[:, :513] * m[:, :513]
            comb.append(c)
        t = torch.zeros(n_utt, Tm, 513, device=dev)
        for u, p in pieces.items():
            at = 0
            for ci, b, n in p:
                T = chunk_shapes[ci][1]
                t[u, at:at + n] = comb[ci][b * T:b * T + n]
                at += n
        if denorm:
            ref = torch.empty_like(t)
            L.check(L.lib().zs_gl_denormalize(L.ptr(t), L.ptr(ref), t.numel(), torch.cuda.current_stream().cuda_stream), 'zs_gl_denormalize')
        else:
            ref = t
        assert torch.equal(conv, ref), (mode, denorm, (conv - ref).abs().max().item())
    if mode == 2:              # the product is rounded before the add: an FMA would differ in the last bit somewhere
        x = xds[0][:, :513].cpu().numpy().astype(np.float64)
        mm = ms[0][:, :513].cpu().numpy().astype(np.float64)
        fused = (x + x * mm).astype(np.float32)                      # one rounding of the exact x + x*m (fma)
        unfused = (comb[0].cpu().numpy())
        assert (fused != unfused).sum() > 0
        assert np.array_equal(unfused, (xds[0][:, :513] + xds[0][:, :513] * ms[0][:, :513]).cpu().numpy())


def test_gen_scatter_rejects_bad_arguments(dev):
    from zs_amd import _lib as L
    st = torch.cuda.current_stream().cuda_stream
    xd = torch.zeros(4, 544, device=dev)
    conv = torch.zeros(1, 4, 513, device=dev)
    dst = torch.arange(4, dtype=torch.int32, device=dev)
    ok = dict(xd=L.ptr(xd), ld_xd=544, m=L.ptr(xd), ld_m=544, dst=L.ptr(dst), rows=4, amp=L.ptr(conv), amp_ld=513, amp_rows=4, mode=1,
              denorm=1)
    L.call('zs_gen_scatter', 'ZsGenScatter', st, **ok)
    for bad in (dict(ld_xd=512), dict(ld_m=100), dict(mode=3), dict(mode=-1), dict(m=None), dict(amp_ld=500), dict(rows=0),
                dict(dst=None)):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(L.ZsError):
            L.call('zs_gen_scatter', 'ZsGenScatter', st, **kw)
    kw = dict(ok, m=None, mode=0)                                    # mode 0 reads no m
    L.call('zs_gen_scatter', 'ZsGenScatter', st, **kw)
    torch.cuda.synchronize()


# ---- driver: per-fragment equality ------------------------------------------------------------------------------------------------
LENS = [5, 128, 300, 700, 129, 9, 385, 640, 256, 200]       # < MIN_LEN, = seg_len, tails, many fragments


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('g_mode', G_MODES)
def test_encode_batch_generator_equals_test_step(dev, tmp_path, g_mode, dtype):
    from zs_amd import convert as cv, layers
    tr = _trainer(g_mode, dtype, tmp_path, seed=3)
    rng = np.random.RandomState(4)
    specs = _specs(rng, LENS)
    spk = [int(s) for s in rng.randint(0 if g_mode == 'naive' else 2, 4, size=len(specs))]
    base, noise_fn = _field_noise(16)
    n_frag = sum(1 if n <= 128 else len(cv.fragments(n, 128)) for n in LENS)
    encs, convs = cv.encode_batch(specs, tr, 128, decode_speakers=spk, noise_fn=noise_fn, max_batch=4, enc_only=False)
    assert n_frag > 2 * 4
    for u, spec in enumerate(specs):
        ref, ref_enc = _per_fragment(tr, spec, spk[u], base)
        assert convs[u].shape == ref.shape, (u, convs[u].shape, ref.shape)
        assert np.array_equal(encs[u], ref_enc), (g_mode, dtype, u)
        assert np.array_equal(convs[u], ref), (g_mode, dtype, u, float(np.abs(convs[u] - ref).max()))
    # the generator changed something (the path is not the autoencoder's)
    _, decs = cv.encode_batch(specs[:3], tr, 128, decode_speakers=spk[:3], noise_fn=noise_fn, max_batch=4)
    assert any(not np.array_equal(a, b) for a, b in zip(decs, convs[:3]))
    # device hand-over: the same values
    _, convs_d = cv.encode_batch(specs, tr, 128, decode_speakers=spk, noise_fn=noise_fn, max_batch=4, enc_only=False, to_host=False)
    assert all(torch.is_tensor(d) and d.is_cuda and np.array_equal(d.cpu().numpy(), c) for d, c in zip(convs_d, convs))
    layers.check_status(dev)


@pytest.mark.parametrize('g_mode', ['naive', 'targeted', 'targeted_residual'])
def test_encode_batch_generator_vs_oracle_gen_step(dev, tmp_path, g_mode):
    import zs_oracle as O
    from zs_amd import convert as cv
    tr = _trainer(g_mode, 'fp32', tmp_path, seed=5)
    rng = np.random.RandomState(6)
    lens = [300, 128, 200, 9]
    specs = _specs(rng, lens)
    spk = [3, 2, 3, 2]
    encs, convs = cv.encode_batch(specs, tr, 128, decode_speakers=spk, enc_only=False)
    dsd = {k: v.detach().cpu() for k, v in tr.Decoder.state_dict().items()}
    gsd = {k: v.detach().cpu() for k, v in tr.Generator.state_dict().items()}
    shift = torch.tensor([2])
    worst = 0.0
    for u, n in enumerate(lens):
        frags = O.fragment_plan(n, 128)[1]
        o8 = o = 0
        for a, b in frags:
            tp = _t8(b - a)
            if len(encs[u]) < o8 + tp:                       # a padded short utterance: encodings truncated to MIN_LEN // 8
                break
            bits = torch.from_numpy(encs[u][o8:o8 + tp].T[None].copy())
            with torch.no_grad():
                ref = O.gen_step(dsd, gsd, bits, torch.tensor([spk[u]]), shift, tr.hps.ns, 128, g_mode=g_mode)[0].T.numpy()
            worst = max(worst, float(np.abs(ref - convs[u][o:o + 8 * tp]).max()))
            o8 += tp
            o += 8 * tp
    assert worst < 1e-3, worst


# ---- vocoder -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('g_mode', ['targeted_residual', 'spectrogram'])
def test_resynth_batch_generator_equals_encode_then_vocoder(dev, tmp_path, g_mode):
    from zs_amd import _lib as L, convert as cv
    tr = _trainer(g_mode, 'fp32', tmp_path, seed=7)
    rng = np.random.RandomState(8)
    lens = [int(n) for n in rng.randint(600, 701, size=40)]
    specs = _specs(rng, lens)
    spk = [2 + (i % 2) for i in range(len(specs))]
    _, noise_fn = _field_noise(16, seed=99)
    e0, c0 = cv.encode_batch(specs, tr, 128, decode_speakers=spk, noise_fn=noise_fn, enc_only=False)
    for do_trim in (False, True):
        w0 = cv.spectrogram2wav_batch(c0, n_iter=4, do_trim=do_trim)
        e1, w1 = cv.resynth_batch(specs, tr, 128, spk, n_iter=4, do_trim=do_trim, noise_fn=noise_fn, enc_only=False)
        print('gl chains used: %d' % L.lib().zs_gl_chains_used())
        assert len(e1) == len(w1) == len(specs)
        for a, b, w, w2, c in zip(e0, e1, w0, w1, c0):
            assert np.array_equal(a, b) and w2.dtype == np.float32 and np.array_equal(w, w2)
            assert len(w2) <= 200 * (c.shape[0] - 1) and (do_trim or len(w2) == 200 * (c.shape[0] - 1))
    # two batches in flight (defer=True) give what they give one at a time
    sa, sb = specs[:3], specs[3:8]
    ra = cv.resynth_batch(sa, tr, 128, spk[:3], n_iter=4, noise_fn=noise_fn, enc_only=False)
    rb = cv.resynth_batch(sb, tr, 128, spk[3:8], n_iter=4, noise_fn=noise_fn, enc_only=False)
    fa = cv.resynth_batch(sa, tr, 128, spk[:3], n_iter=4, noise_fn=noise_fn, enc_only=False, defer=True)
    fb = cv.resynth_batch(sb, tr, 128, spk[3:8], n_iter=4, noise_fn=noise_fn, enc_only=False, defer=True)
    for (e_ref, w_ref), (e_got, w_got) in ((ra, fa()), (rb, fb())):
        assert all(np.array_equal(a, b) for a, b in zip(e_ref, e_got)) and all(np.array_equal(a, b) for a, b in zip(w_ref, w_got))


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_source_range_target_raises_before_anything_is_enqueued(dev, tmp_path):
    from zs_amd import convert as cv, layers
    tr = _trainer('targeted_residual', 'fp32', tmp_path)
    rng = np.random.RandomState(1)
    specs = _specs(rng, [300, 200])
    cv.encode_batch(specs, tr, 128, decode_speakers=[2, 3], enc_only=False)          # warm: every buffer exists
    status = layers.device_status(dev).clone()
    torch.cuda.synchronize()
    for fn in (lambda: cv.encode_batch(specs, tr, 128, decode_speakers=[2, 1], enc_only=False),
               lambda: cv.resynth_batch(specs, tr, 128, [0, 3], n_iter=4, enc_only=False)):
        with pytest.raises(RuntimeError, match='can only convert to target speakers'):
            fn()
        assert torch.cuda.current_stream().query()
    assert torch.equal(layers.device_status(dev), status)
    # enc_only keeps accepting any speaker, as before
    cv.encode_batch(specs, tr, 128, decode_speakers=[0, 1])


def test_naive_generator_accepts_every_speaker(dev, tmp_path):
    from zs_amd import convert as cv
    tr = _trainer('naive', 'fp32', tmp_path)
    rng = np.random.RandomState(2)
    specs = _specs(rng, [150, 300, 90, 129])
    encs, convs = cv.encode_batch(specs, tr, 128, decode_speakers=[0, 1, 2, 3], enc_only=False)
    assert all(np.isfinite(c).all() for c in convs)
    with pytest.raises(ValueError):
        cv.encode_batch(specs, tr, 128, decode_speakers=[0, 1, 2, 4], enc_only=False)


# ---- --cross_test -----------------------------------------------------------------------------------------------------------------
def _tone(rng, n):
    t = np.arange(n) / 16000.0
    y = 0.3 * np.sin(2 * np.pi * rng.uniform(100, 3000) * t) + 0.1 * np.sin(2 * np.pi * rng.uniform(3000, 7000) * t) + 0.02 * rng.randn(n)
    return (np.clip(y, -1, 1) * 32767).astype(np.int16)


def test_main_cross_test(dev, tmp_path, monkeypatch, capsys):
    from scipy.io import wavfile
    import main as M
    from zs_amd import convert as cv, dataloader as D, preprocess as P
    from zs_amd.hps import hp, make_hps
    rng = np.random.RandomState(12)
    dirs = {k: tmp_path / k for k in ('source', 'target', 'test')}
    for d in dirs.values():
        d.mkdir()
    for spk in ('S015', 'S020'):
        wavfile.write(str(dirs['source'] / ('%s_0001.wav' % spk)), 16000, _tone(rng, 30000))
    for spk in ('V001', 'V002'):
        wavfile.write(str(dirs['target'] / ('%s_0001.wav' % spk)), 16000, _tone(rng, 30000))
    test_utts = {'S130': {'0001': 70000, '0002': 12000}, 'S089': {'0003': 30000, '0004': 1200}}
    for spk, utts in test_utts.items():
        for utt, n in utts.items():
            wavfile.write(str(dirs['test'] / ('%s_%s.wav' % (spk, utt))), 16000, _tone(rng, n))
    ds = str(tmp_path / 'dataset_english.npz')
    idx = [str(tmp_path / n) for n in ('index.json', 'index_source.json', 'index_target.json')]
    s2id = str(tmp_path / 'speaker2id.json')
    P.preprocess(str(dirs['source']), str(dirs['target']), str(dirs['test']), ds, idx[0], idx[1], idx[2], s2id, seg_len=128,
                 n_samples=4, dset='train', remake=True)
    speaker2id = json.load(open(s2id))
    assert sorted(speaker2id) == ['S015', 'S020', 'V001', 'V002'] and speaker2id['V001'] >= 2 and speaker2id['V002'] >= 2
    # a stage-2 checkpoint of small nets and the hps file that describes them
    hps = make_hps(enc_size=16, emb_size=32, n_speakers=4, n_target_speakers=2)
    hps_path = str(tmp_path / 'hps.json')
    json.dump(hps._asdict(), open(hps_path, 'w'))
    tr = _trainer('targeted_residual', 'fp32', tmp_path, seed=9)
    tr.save_model(str(tmp_path / 'model.pth'), 's2', 1)
    ckpt = str(tmp_path / 'model.pth-s2-1')
    monkeypatch.setattr(hp, 'n_iter', 4)
    store = D.NpzStore(ds, 'r')
    frames = {(s, u): store['test/%s/%s/lin' % (s, u)].shape[0] for s, utts in test_utts.items() for u in utts}
    assert len(set(frames.values())) == len(frames) and max(frames.values()) > 256
    for extra in ([], ['--enc_only']):
        res = tmp_path / ('result%d' % len(extra))
        M.main(['--cross_test', '--hps_path', hps_path, '--dataset_path', ds, '--speaker2id_path', s2id, '--ckpt_pth', ckpt,
                '--result_dir', str(res), '--g_mode', 'targeted_residual'] + extra)
        got = {d: sorted(os.listdir(str(res / d))) for d in os.listdir(str(res)) if '_to_' in d}
        want = {}
        for src, utts in test_utts.items():
            for tar in ('V001', 'V002'):
                want['%s_to_%s' % (src, tar)] = sorted(['%s_%s.wav' % (tar, u) for u in utts] + ['%s_%s.txt' % (src, u) for u in utts])
        assert got == want
        import wave
        for (src, utt), T in frames.items():
            spec, padded = cv._pad_min(np.zeros((T, 513), np.float32))
            T_in = len(spec)
            frags = [(0, T_in)] if T_in <= 128 else cv.fragments(T_in, 128)
            t_out = sum(8 * _t8(b - a) for a, b in frags)
            for tar in ('V001', 'V002'):
                with wave.open(str(res / ('%s_to_%s' % (src, tar)) / ('%s_%s.wav' % (tar, utt))), 'rb') as f:
                    assert f.getframerate() == hp.sr and f.getsampwidth() == 2
                    assert 0 < f.getnframes() <= 200 * (t_out - 1)
                rows = open(str(res / ('%s_to_%s' % (src, tar)) / ('%s_%s.txt' % (src, utt)))).read().split('\n')
                assert rows[-1] == ''
                rows = rows[:-1]
                assert len(rows) == (cv.MIN_LEN // 8 if padded else t_out // 8)
                assert all(len(r.split(' ')) == 16 and set(r.split(' ')) <= {'0', '1'} for r in rows)
    capsys.readouterr()
