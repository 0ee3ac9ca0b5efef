"""GPU: fast Griffin-Lim (ZsGlIter::momentum, the `momentum` keyword of the vocoder drivers) against the numpy restatement in
tests/fgla_ref.py, its bit-for-bit invariances (tiles, prefetch, launch chains, zs_gl_iter against zs_griffin_lim), the default
path unchanged, and its quality on real speech (the reference's demo outputs in tests/golden/fgla_speech.npz).
Tolerances: one iteration 2e-4 of the scale (as the plain fused iteration); audio after 1..8 iterations 1e-3 of the waveform scale
(the vocoder's audio tolerance)."""
import ctypes

import numpy as np
import pytest
import torch

import fgla_ref as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cv():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    from zs_amd import convert
    return convert


def _to_dev(Xc, Tm):
    """complex [513, T] -> complex64 as fp32 [1, Tm, 513, 2] on the device (rows >= T zero)."""
    T = Xc.shape[1]
    t = torch.zeros(1, Tm, 513, 2, device='cuda:0')
    t[0, :T, :, 0] = torch.from_numpy(np.ascontiguousarray(Xc.real.T.astype(np.float32))).cuda()
    t[0, :T, :, 1] = torch.from_numpy(np.ascontiguousarray(Xc.imag.T.astype(np.float32))).cuda()
    return t


def _from_dev(t, T):
    a = t[0, :T].cpu().numpy()
    return (a[..., 0] + 1j * a[..., 1]).T


@pytest.mark.parametrize('alpha', [0.5, 0.99])
@pytest.mark.parametrize('T,tile', [(4, 0), (5, 4), (17, 4), (40, 10), (53, 26), (131, 0), (131, 42)])
def test_fgla_iteration_vs_restatement(cv, T, tile, alpha):
    """One zs_gl_iter with momentum on a random complex spectrogram and a random state E_prev: spec_out = mag * A / max(1e-8, |A|)
    with A = E - beta E_prev, and the state then holds E.  With mag = |A_ref| the projection reproduces A itself.  Rows past the
    length of spec_out and of the state stay untouched, and the final pass (spec_out = NULL) leaves the state alone."""
    import zs_oracle as O
    from zs_amd import _lib as L
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.RandomState(100 + T)
    X = (rng.randn(513, T) + 1j * rng.randn(513, T)).astype(np.complex64)
    P = (rng.randn(513, T) + 1j * rng.randn(513, T)).astype(np.complex64)
    x_ref = O.istft(X)
    E = O.stft(x_ref)
    A = E - F.beta_of(alpha) * P
    Tm = T + 3
    spec_in = _to_dev(X, Tm)
    prev = _to_dev(P, Tm)
    prev[0, T:] = 5.0
    spec_out = torch.full((1, Tm, 513, 2), 7.0, device='cuda:0')
    mag = torch.zeros(1, Tm, 513, device='cuda:0')
    mag[0, :T] = torch.from_numpy(np.ascontiguousarray(np.abs(A).T.astype(np.float32))).cuda()
    lengths = torch.tensor([T], dtype=torch.int32, device='cuda:0')
    wav = torch.full((1, 200 * (Tm - 1)), 3.0, device='cuda:0')
    args = dict(mag=L.ptr(mag), lengths=L.ptr(lengths), n_utt=1, T_max=Tm, wav=L.ptr(wav), wav_ld=wav.shape[1], tile_frames=tile,
                momentum=alpha, spec_prev=L.ptr(prev))
    L.call('zs_gl_iter', 'ZsGlIter', st, spec_in=L.ptr(spec_in), spec_out=L.ptr(spec_out), **args)
    prev_after = prev.clone()
    L.call('zs_gl_iter', 'ZsGlIter', st, spec_in=L.ptr(spec_in), spec_out=None, **args)
    torch.cuda.synchronize()
    got = _from_dev(spec_out, T)
    err = np.abs(got - A).max() / np.abs(A).max()
    assert err < 2e-4, err
    e_got = _from_dev(prev_after, T)
    assert np.abs(e_got - E).max() < 2e-4 * np.abs(E).max(), np.abs(e_got - E).max() / np.abs(E).max()
    assert (spec_out[0, T:] == 7.0).all() and (prev_after[0, T:] == 5.0).all()
    assert torch.equal(prev, prev_after)
    w = wav[0].cpu().numpy()
    assert np.abs(w[:200 * (T - 1)] - x_ref).max() < 2e-4 * np.abs(x_ref).max()
    assert (w[200 * (T - 1):] == 3.0).all()


def test_zs_gl_iter_rejects_bad_momentum_and_state(cv):
    """Momentum outside [0, 1) or not finite, momentum > 0 without a state, or a state that overlaps a spectrogram buffer: a negative
    return code and no launch, from zs_gl_iter and from zs_griffin_lim.  (Every buffer lies inside one allocation.)"""
    from zs_amd import _lib as L
    dev = torch.device('cuda:0')
    T = 8
    pool = torch.zeros(4, T, 513, 2, device=dev)
    spec_in, spec_out, prev = pool[0:1], pool[1:2], pool[2:3]
    spec_in.fill_(9.0)
    mag = torch.ones(1, T, 513, device=dev)
    lengths = torch.tensor([T], dtype=torch.int32, device=dev)
    wav = torch.zeros(1, 200 * (T - 1), device=dev)
    S = L.STRUCTS['ZsGlIter']
    base = dict(mag=L.ptr(mag), lengths=L.ptr(lengths), n_utt=1, T_max=T, wav=L.ptr(wav), wav_ld=wav.shape[1])
    st = torch.cuda.current_stream().cuda_stream
    bad = [dict(momentum=1.0, spec_prev=L.ptr(prev)), dict(momentum=-0.25, spec_prev=L.ptr(prev)),
           dict(momentum=float('nan'), spec_prev=L.ptr(prev)), dict(momentum=float('inf'), spec_prev=L.ptr(prev)),
           dict(momentum=0.5, spec_prev=None), dict(momentum=0.5, spec_prev=L.ptr(spec_in)),
           dict(momentum=0.5, spec_prev=L.ptr(spec_out)), dict(momentum=0.5, spec_prev=L.ptr(spec_in, 513 * 2 * (T - 1)))]
    for kw in bad:
        with pytest.raises(L.ZsError, match='momentum|spec_prev'):
            L.call('zs_gl_iter', 'ZsGlIter', st, spec_in=L.ptr(spec_in), spec_out=L.ptr(spec_out), **dict(base, **kw))
        p = S(**dict(base, **kw))
        assert L.lib().zs_griffin_lim(ctypes.addressof(p), L.ptr(spec_in), L.ptr(spec_out), 2, st) < 0, kw
    torch.cuda.synchronize()
    assert (spec_in == 9.0).all() and (pool[1:] == 0).all() and (wav == 0).all()          # nothing was launched


def _ragged_mags(lens, seed):
    import zs_oracle as O
    return [np.abs(O.stft(F.speechlike(T, seed + i))).astype(np.float32) for i, T in enumerate(lens)]


@pytest.mark.parametrize('alpha', [0.5, 0.99])
@pytest.mark.parametrize('n_iter', [1, 2, 8])
def test_fgla_loop_vs_restatement_ragged(cv, n_iter, alpha):
    """zs_griffin_lim with momentum on a ragged batch (4, 5, 31, 257, 700 frames): every utterance's waveform within 1e-3 of the
    scale of the numpy restatement, the padding samples untouched (zero)."""
    lens = [4, 5, 31, 257, 700]
    mags = _ragged_mags(lens, 30)
    wav, _, got_lens = cv.griffin_lim_batch(mags, n_iter=n_iter, momentum=alpha)
    w = wav.cpu().numpy()
    assert got_lens == lens
    for i, T in enumerate(lens):
        ref = F.fgla(mags[i], n_iter, alpha)
        err = np.abs(w[i, :200 * (T - 1)] - ref).max() / np.abs(ref).max()
        assert err < 1e-3, (T, err)
        assert (w[i, 200 * (T - 1):] == 0).all()


def test_fgla_audio_700_frames_60_iterations(cv):
    """A 700-frame utterance, 60 FGLA iterations (alpha = 0.99): the error against the restatement is reported as for the plain loop
    (test_griffin_lim_audio_700_frames_vs_oracle).  With momentum the iteration amplifies rounding: the fp32 restatement itself
    differs from an fp64 one by ~1e-2 of the scale here, so the assertion is on the spectral convergence both reach."""
    import zs_oracle as O
    S = np.abs(O.stft(F.speechlike(700, 2))).astype(np.float32)
    w_gpu = cv.griffin_lim(S, n_iter=60, momentum=0.99)
    w_ref = F.fgla(S, 60, 0.99)
    assert w_gpu.shape == w_ref.shape == (200 * 699,)
    err = np.abs(w_gpu - w_ref).max() / np.abs(w_ref).max()
    rms = np.sqrt(np.mean((w_gpu - w_ref) ** 2)) / np.sqrt(np.mean(w_ref ** 2))
    sc_gpu, sc_ref = F.spectral_convergence(w_gpu, S), F.spectral_convergence(w_ref, S)
    print('FGLA 60 iterations, 700 frames: max err %.3g of scale, rms err %.3g; SC gpu %.4g restatement %.4g' % (err, rms, sc_gpu, sc_ref))
    assert np.isfinite(w_gpu).all() and sc_gpu < 1.05 * sc_ref + 1e-3


def test_fgla_is_tile_prefetch_and_driver_invariant(cv):
    """alpha = 0.99, bit for bit: tile_frames 0 / 10 / 42 and gl_prefetch 0 / 1 give the same waveforms, and three chained zs_gl_iter
    calls (X0 = S in spec_in, a zero-filled state) give what zs_griffin_lim gives for n_iter = 2."""
    from zs_amd import _lib as L
    lens = [16, 61, 300, 97]
    mags = _ragged_mags(lens, 50)
    outs = [cv.griffin_lim_batch(mags, n_iter=5, momentum=0.99, tile_frames=f)[0] for f in (0, 10, 42)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    old = L.set_option('gl_prefetch', 0)
    try:
        off = cv.griffin_lim_batch(mags, n_iter=5, momentum=0.99)[0]
    finally:
        L.set_option('gl_prefetch', old)
    assert torch.equal(outs[0], off)
    # the loop driven by hand
    wav2, lengths, _ = cv.griffin_lim_batch(mags, n_iter=2, momentum=0.99)
    dev = torch.device('cuda:0')
    n, Tm = len(lens), max(lens)
    mag = torch.zeros(n, Tm, 513, device=dev)
    for i, m in enumerate(mags):
        mag[i, :lens[i]] = torch.from_numpy(np.ascontiguousarray(m.T)).to(dev)
    a = torch.zeros(n, Tm, 513, 2, device=dev)
    a[..., 0] = mag
    b = torch.empty_like(a)
    prev = torch.zeros_like(a)
    wav = torch.zeros(n, 200 * (Tm - 1), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    args = dict(mag=L.ptr(mag), lengths=L.ptr(lengths), n_utt=n, T_max=Tm, wav=L.ptr(wav), wav_ld=wav.shape[1], momentum=0.99,
                spec_prev=L.ptr(prev))
    L.call('zs_gl_iter', 'ZsGlIter', st, spec_in=L.ptr(a), spec_out=L.ptr(b), **args)
    L.call('zs_gl_iter', 'ZsGlIter', st, spec_in=L.ptr(b), spec_out=L.ptr(a), **args)
    L.call('zs_gl_iter', 'ZsGlIter', st, spec_in=L.ptr(a), spec_out=None, **args)
    torch.cuda.synchronize()
    assert torch.equal(wav, wav2)


@pytest.mark.parametrize('alpha', [0.0, 0.99])
def test_fgla_launch_chains_equal_one_chain(cv, alpha):
    """32 utterances of 600..700 frames (unequal, host lengths given): zs_griffin_lim's launch chains offset the state exactly as the
    spectrogram buffers -- the default (several chains) and gl_chains = 1 give the same waveforms bit for bit."""
    from zs_amd import _lib as L
    rng = np.random.RandomState(11)
    lens = [int(t) for t in rng.randint(600, 701, size=32)]
    assert len(set(lens)) > 1
    mags = [np.abs(rng.randn(513, T)).astype(np.float32) * np.linspace(1, 0.01, 513, dtype=np.float32)[:, None] for T in lens]
    many = cv.griffin_lim_batch(mags, n_iter=6, momentum=alpha)[0]
    torch.cuda.synchronize()
    used = int(L.lib().zs_gl_chains_used())
    old = L.set_option('gl_chains', 1)
    try:
        one = cv.griffin_lim_batch(mags, n_iter=6, momentum=alpha)[0]
        torch.cuda.synchronize()
        assert int(L.lib().zs_gl_chains_used()) == 1
    finally:
        L.set_option('gl_chains', old)
    print('alpha %.2f: %d chains' % (alpha, used))
    assert used > 1
    assert torch.equal(many, one)


def test_default_path_unchanged(cv, monkeypatch):
    """momentum = 0.0, no keyword, and hp.gl_momentum = 0 give the same bits, for griffin_lim_batch and spectrogram2wav_batch."""
    from zs_amd.hps import hp
    mags = _ragged_mags([40, 129, 300], 70)
    a = cv.griffin_lim_batch(mags, n_iter=7, momentum=0.0)[0]
    b = cv.griffin_lim_batch(mags, n_iter=7)[0]
    monkeypatch.setattr(hp, 'gl_momentum', 0)
    c = cv.griffin_lim_batch(mags, n_iter=7)[0]
    assert torch.equal(a, b) and torch.equal(a, c)
    monkeypatch.undo()
    rng = np.random.RandomState(5)
    norm = [np.clip(rng.rand(T, 513).astype(np.float32), 1e-8, 1) for T in (40, 129, 300)]
    x = cv.spectrogram2wav_batch(norm, n_iter=7, momentum=0.0)
    y = cv.spectrogram2wav_batch(norm, n_iter=7)
    monkeypatch.setattr(hp, 'gl_momentum', 0)
    z = cv.spectrogram2wav_batch(norm, n_iter=7)
    assert all(np.array_equal(p, q) and np.array_equal(p, r) for p, q, r in zip(x, y, z))
    fg = cv.griffin_lim_batch(mags, n_iter=7, momentum=0.99)[0]
    assert not torch.equal(a, fg)


def test_fgla_quality_on_real_speech(cv):
    """The fixture's three utterances (the reference's demo outputs, de-normalised as the vocoder sees them), SC on the host from the
    GPU waveforms: FGLA 100 iterations beats the plain 300, and FGLA 50 beats the plain 50, on every utterance."""
    S = F.fixture_amplitudes()
    _, names = F.fixture_waves()
    runs = {(100, 0.99): None, (300, 0.0): None, (50, 0.99): None, (50, 0.0): None}
    for n_iter, alpha in runs:
        wav, _, lens = cv.griffin_lim_batch(S, n_iter=n_iter, momentum=alpha)
        w = wav.cpu().numpy()
        runs[(n_iter, alpha)] = [F.spectral_convergence(w[i, :200 * (T - 1)], S[i]) for i, T in enumerate(lens)]
    for i, name in enumerate(names):
        print('%s (%d frames): SC plain 50 %.4f, plain 300 %.4f, fgla 50 %.4f, fgla 100 %.4f' % (
            name, S[i].shape[1], runs[(50, 0.0)][i], runs[(300, 0.0)][i], runs[(50, 0.99)][i], runs[(100, 0.99)][i]))
        assert runs[(100, 0.99)][i] < runs[(300, 0.0)][i]
        assert runs[(50, 0.99)][i] < runs[(50, 0.0)][i]


def _gumbel_fn(seed):
    def noise_fn(n, Tp, E):
        g = torch.Generator().manual_seed(seed + Tp)
        return -torch.log(-torch.log(torch.rand(n, Tp, E, 2, generator=g) + 1e-20) + 1e-20)
    return noise_fn


def test_drivers_take_momentum(cv, tmp_path, monkeypatch):
    """resynth_batch(momentum=0.99) = encode_batch + spectrogram2wav_batch(momentum=0.99) with the same noise (enc_only=True); the
    generator path (enc_only=False) runs with momentum and differs from alpha = 0; spectrogram2wav reads hp.gl_momentum."""
    from zs_amd.hps import hp, make_hps
    from zs_amd.trainer import Trainer
    torch.manual_seed(3)
    hps = make_hps(enc_size=16, emb_size=32, n_speakers=4, n_target_speakers=2)
    tr = Trainer(hps, None, 'targeted_residual', 'multilabel_binary', log_dir=str(tmp_path / 'log'), dtype='fp32')
    rng = np.random.RandomState(12)
    specs = [np.clip(rng.rand(n, 513).astype(np.float32), 1e-8, 1) for n in (300, 140, 90)]
    spk = [2, 3, 2]
    noise_fn = _gumbel_fn(500)
    e0, d0 = cv.encode_batch(specs, tr, 128, decode_speakers=spk, noise_fn=noise_fn)
    w0 = cv.spectrogram2wav_batch(d0, n_iter=20, do_trim=False, momentum=0.99)
    e1, w1 = cv.resynth_batch(specs, tr, 128, spk, n_iter=20, do_trim=False, noise_fn=noise_fn, momentum=0.99)
    for a, b, w, w2 in zip(e0, e1, w0, w1):
        assert np.array_equal(a, b) and np.array_equal(w, w2) and np.isfinite(w2).all()
    _, wp = cv.resynth_batch(specs, tr, 128, spk, n_iter=20, do_trim=False, noise_fn=noise_fn)
    assert any(not np.array_equal(p, q) for p, q in zip(wp, w1))
    _, g_fg = cv.resynth_batch(specs, tr, 128, spk, n_iter=20, do_trim=False, noise_fn=noise_fn, enc_only=False, momentum=0.99)
    _, g_pl = cv.resynth_batch(specs, tr, 128, spk, n_iter=20, do_trim=False, noise_fn=noise_fn, enc_only=False, momentum=0.0)
    assert len(g_fg) == len(specs) and all(np.isfinite(w).all() and w.shape == p.shape for w, p in zip(g_fg, g_pl))
    assert any(not np.array_equal(p, q) for p, q in zip(g_fg, g_pl))
    m = np.clip(rng.rand(150, 513).astype(np.float32), 1e-8, 1)
    explicit = cv.spectrogram2wav(m, n_iter=20, momentum=0.99)
    monkeypatch.setattr(hp, 'gl_momentum', 0.99)
    assert np.array_equal(cv.spectrogram2wav(m, n_iter=20), explicit)
