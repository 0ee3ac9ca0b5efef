"""GPU: the STFT, Griffin-Lim and feature kernels against the fp64 reference of tests/audio_ref.py, per frame.

Measure (audio_ref.frame_err / wav_err): the L2 error of every output frame (every block of 200 waveform samples) over s_t, the largest
L2 norm among the input and the fp64 output frames of its dependency range.  Bound: 16 x the same measure of the fp32 twin against
fp64, computed here on the same input, and never above 1e-5.  Every test prints its figures; with ZS_AUDIO_ERRORS_OUT set to a path
the table is written there as well (profiles/audio_fp64_errors.txt is one such run).
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import audio_ref as R

pytestmark = pytest.mark.gpu

NB, HOP = R.NB, R.HOP
_ROWS = []


@pytest.fixture(scope='module')
def L():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    from zs_amd import _lib
    yield _lib
    path = os.environ.get('ZS_AUDIO_ERRORS_OUT')
    if path and _ROWS:
        with open(path, 'w') as f:
            f.write('%-58s %-6s %11s %11s %8s %11s\n' % ('case', 'output', 'fp32 twin', 'GPU', 'factor', 'bound'))
            for r in _ROWS:
                f.write('%-58s %-6s %11.3e %11.3e %8.2f %11.3e\n' % r)


def _dev():
    return torch.device('cuda:0')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def check(case, what, gpu, twin, factor=R.FACTOR):
    """Record and assert one figure: gpu <= factor x twin <= 1e-5."""
    bound = factor * twin
    _ROWS.append((case, what, twin, gpu, gpu / twin if twin > 0 else 0.0, bound))
    print('%s %s: fp32 twin %.3e  GPU %.3e  factor %.2f  bound %.3e' % (case, what, twin, gpu, gpu / twin if twin > 0 else 0.0, bound))
    assert bound <= R.CAP, (case, what, bound)
    assert gpu <= bound, (case, what, gpu, bound)


def spec_tensor(Z, rows, fill):
    """complex [513, T] -> fp32 [rows, 513, 2] on the host, rows past T filled."""
    out = np.full((rows, NB, 2), fill, dtype=np.float32)
    T = Z.shape[1]
    out[:T, :, 0] = Z.real.T
    out[:T, :, 1] = Z.imag.T
    return out


def real_tensor(M, rows, fill):
    out = np.full((rows, NB), fill, dtype=np.float32)
    out[:M.shape[1]] = M.T
    return out


def spec_of(t, T):
    a = t[:T].cpu().numpy()
    return (a[..., 0] + 1j * a[..., 1]).T


@functools.lru_cache(maxsize=None)
def gl_ref(T, F, alpha):
    X, mag, prev, lv = R.gl_case(T, F)
    return X, mag, prev, lv, R.gl_reference(X, mag, prev, alpha)


def assert_iteration(case, ref, X, mag, alpha, lv, out, state, wav):
    """One utterance's outputs of one iteration against its fp64 reference."""
    T = X.shape[1]
    assert np.isfinite(out).all()
    keep = ref['keep']
    check(case, 'spec', R.frame_err(out, ref['out'], ref['sO'], keep).max(), ref['twin_O'])
    ill = ~keep
    assert (np.abs(out)[ill] <= mag[ill].astype(np.float64) * (1 + 1e-6)).all()
    for t in R.zero_dependency_frames(lv):
        assert (out[:, t] == 0).all(), t
    assert (out[mag == 0] == 0).all()
    if alpha > 0:
        check(case, 'state', R.frame_err(state, ref['E'], ref['sE']).max(), ref['twin_E'])
    check(case, 'wav', R.wav_err(wav[:HOP * (T - 1)], ref['wav'], ref['sW']).max(), ref['twin_W'])


class Batch(object):
    """The device buffers of a ragged batch for zs_gl_iter: everything past an utterance's frames, and every row of an utterance
    under 4 frames, holds fill values (NaN where the kernel must not read, numbers where it must not write)."""

    def __init__(self, lengths, F, T_max, alpha):
        dev = _dev()
        n = len(lengths)
        self.lengths, self.T_max = lengths, T_max
        si = np.full((n, T_max, NB, 2), np.nan, dtype=np.float32)
        mg = np.full((n, T_max, NB), np.nan, dtype=np.float32)
        pv = np.full((n, T_max, NB, 2), 9.0, dtype=np.float32)
        for u, T in enumerate(lengths):
            if T < 4:
                continue
            X, mag, prev, lv = R.gl_case(T, F)
            si[u], mg[u], pv[u] = spec_tensor(X, T_max, np.nan), real_tensor(mag, T_max, np.nan), spec_tensor(prev, T_max, 9.0)
        self.spec_in, self.mag = torch.from_numpy(si).to(dev), torch.from_numpy(mg).to(dev)
        self.prev0 = pv
        self.prev = torch.from_numpy(pv).to(dev)
        self.spec_out = torch.full((n, T_max, NB, 2), 7.0, device=dev)
        self.wav = torch.full((n, HOP * (T_max - 1) + 5), 3.0, device=dev)
        self.len_t = torch.tensor(lengths, dtype=torch.int32, device=dev)

    def run(self, L, F, alpha):
        kw = dict(spec_in=L.ptr(self.spec_in), mag=L.ptr(self.mag), lengths=L.ptr(self.len_t), n_utt=len(self.lengths), T_max=self.T_max,
                  wav=L.ptr(self.wav), wav_ld=self.wav.shape[1], tile_frames=F)
        if alpha > 0:
            kw.update(momentum=alpha, spec_prev=L.ptr(self.prev))
        L.call('zs_gl_iter', 'ZsGlIter', _stream(), spec_out=L.ptr(self.spec_out), **kw)
        L.call('zs_gl_iter', 'ZsGlIter', _stream(), spec_out=None, **kw)
        torch.cuda.synchronize()

    def assert_untouched(self, alpha):
        for u, T in enumerate(self.lengths):
            T = T if T >= 4 else 0
            assert (self.spec_out[u, T:] == 7.0).all(), u
            assert np.array_equal(self.prev[u, T:].cpu().numpy(), self.prev0[u, T:]), u
            assert (self.wav[u, HOP * max(T - 1, 0):] == 3.0).all(), u
        if alpha == 0:
            assert np.array_equal(self.prev.cpu().numpy(), self.prev0)


GL_CASES = [(T, F, a, 1) for (T, F) in R.GL_SHAPES for a in (0.0, 0.5)] + [(T, F, a, 0) for (T, F) in R.GL_NO_PREFETCH for a in (0.0, 0.5)]


@pytest.mark.parametrize('T,F,alpha,prefetch', GL_CASES)
def test_gl_iter_vs_fp64(L, T, F, alpha, prefetch):
    """zs_gl_iter, plain (alpha = 0) and with momentum (alpha = 0.5, random spec_prev), on every tile class: one tile with every frame
    reflected (4, 0); halos from both neighbours and balanced tiles of uneven length (5, 4), (17, 4); 4 waves (40, 10); 8 waves and
    large LDS (53, 26), (131, 42); (17, 4) and (53, 26) also without prefetch.  The input has a stretch at 1e-3 that starts one frame
    after a tile boundary and 8 all-zero frames; the magnitudes are independent of E, with exact zeros, and nonzero on the zero
    frames.  spec_out, the state E and the final-pass wav are within 16 x the fp32 twin's error; ill-conditioned bins (audio_ref.ILL)
    are only bounded in magnitude; the frames whose whole dependency range is zero come out exactly 0; nothing past T is written."""
    X, mag, prev, lv, ref = gl_ref(T, F, alpha)
    b = Batch([T], F, T + 3, alpha)
    old = L.set_option('gl_prefetch', prefetch)
    try:
        b.run(L, F, alpha)
    finally:
        L.set_option('gl_prefetch', old)
    case = 'gl_iter T=%d tile=%d alpha=%g prefetch=%d' % (T, F, alpha, prefetch)
    assert_iteration(case, ref, X, mag, alpha, lv, spec_of(b.spec_out[0], T), spec_of(b.prev[0], T), b.wav[0].cpu().numpy())
    b.assert_untouched(alpha)


RAGGED = [0, 3, 4, 23, 9]


@pytest.mark.parametrize('F', [4, 26])
@pytest.mark.parametrize('alpha', [0.0, 0.5])
def test_gl_iter_ragged_batch_vs_fp64(L, F, alpha):
    """lengths 0, 3, 4, 23, 9 in one launch (T_max 26): tiles past an utterance's last return early, utterances under 4 frames are
    skipped (their rows of spec_out, the state and wav keep their fill), every other row is within the bound of its own
    single-utterance fp64 reference."""
    b = Batch(RAGGED, F, 26, alpha)
    b.run(L, F, alpha)
    for u, T in enumerate(RAGGED):
        if T < 4:
            continue
        X, mag, prev, lv, ref = gl_ref(T, F, alpha)
        case = 'gl_iter ragged u=%d T=%d tile=%d alpha=%g' % (u, T, F, alpha)
        assert_iteration(case, ref, X, mag, alpha, lv, spec_of(b.spec_out[u], T), spec_of(b.prev[u], T), b.wav[u].cpu().numpy())
    b.assert_untouched(alpha)


@pytest.mark.parametrize('T,F', [(17, 4), (53, 26)])
@pytest.mark.parametrize('n_iter', [0, 1])
def test_griffin_lim_from_magnitudes_vs_fp64(L, T, F, n_iter):
    """zs_griffin_lim with n_iter = 0 and 1, the FROM_MAG instantiations (the final pass on the magnitudes themselves; one iteration
    from zero phase), momentum 0.99, spec_a / spec_b / spec_prev pre-filled with garbage.  n_iter = 0: wav = istft(S).  n_iter = 1:
    the state equals E_1 = stft(istft(S)), and the waveform is istft(S E / |E|) of the very fp32 E the kernel left in the state (the
    phase of a small |E_1| bin decides a full magnitude, so the waveform is compared from the projected state on; its bound is the
    twin's error on the fp64 E_1, which the kernel has no part in)."""
    dev = _dev()
    S = np.abs(R.gl_case(T, F)[0]).astype(np.float32)
    Tm = T + 2
    mag = torch.from_numpy(real_tensor(S, Tm, np.nan)).to(dev).unsqueeze(0).contiguous()
    sa, sb, sp = (torch.full((1, Tm, NB, 2), v, device=dev) for v in (np.nan, -5.0, np.nan))
    wav = torch.full((1, HOP * (Tm - 1)), 3.0, device=dev)
    lens = torch.tensor([T], dtype=torch.int32, device=dev)
    p = L.STRUCTS['ZsGlIter'](mag=L.ptr(mag), lengths=L.ptr(lens), n_utt=1, T_max=Tm, wav=L.ptr(wav), wav_ld=wav.shape[1], tile_frames=F,
                              momentum=0.99, spec_prev=L.ptr(sp))
    L.check(L.lib().zs_griffin_lim(ctypes.addressof(p), L.ptr(sa), L.ptr(sb), n_iter, _stream()), 'zs_griffin_lim')
    torch.cuda.synchronize()
    w = wav[0].cpu().numpy()
    assert (w[HOP * (T - 1):] == 3.0).all() and np.isfinite(w[:HOP * (T - 1)]).all()
    case = 'griffin_lim n_iter=%d T=%d tile=%d' % (n_iter, T, F)
    sW = R.wav_scale(S, T)
    if n_iter == 0:
        w64, w32 = R.istft(S, np.float64), R.istft(S, np.float32)
        check(case, 'wav', R.wav_err(w[:len(w64)], w64, sW).max(), R.wav_err(w32, w64, sW).max())
        return
    E64, E32 = R.stft(R.istft(S, np.float64), np.float64), R.stft(R.istft(S, np.float32), np.float32)
    sE = R.spec_scale(S, E64)
    E_gpu = spec_of(sp[0], T)
    check(case, 'state', R.frame_err(E_gpu, E64, sE).max(), R.frame_err(E32, E64, sE).max())
    assert torch.isnan(sp[0, T:]).all()
    X64 = R.project(E64, S, np.float64)
    twin = R.wav_err(R.istft(R.project(E64.astype(np.complex64), S, np.float32), np.float32), R.istft(X64, np.float64), sW).max()
    w64 = R.istft(R.project(E_gpu, S, np.float64), np.float64)
    check(case, 'wav', R.wav_err(w[:len(w64)], w64, sW).max(), twin)


@pytest.mark.parametrize('F', [4])
def test_split_kernels_ragged_vs_fp64(L, F):
    """zs_gl_istft and zs_gl_stft_project on the ragged batch 0, 3, 4, 23, 9: the same measure and bound as the fused kernel, rows
    past T and the rows of utterances under 4 frames untouched (both kernels skip them, as zs_gl_iter does)."""
    dev = _dev()
    Tm = 26
    b = Batch(RAGGED, F, Tm, 0.0)
    n = len(RAGGED)
    frames = torch.zeros(n, Tm, 1024, device=dev)
    L.call('zs_gl_istft', 'ZsGlIstft', _stream(), spec=L.ptr(b.spec_in), mag=L.ptr(b.mag), lengths=L.ptr(b.len_t), n_utt=n, T_max=Tm,
           wav=L.ptr(b.wav), wav_ld=b.wav.shape[1], frames_ws=L.ptr(frames))
    torch.cuda.synchronize()
    wav_in = np.full((n, b.wav.shape[1]), np.nan, dtype=np.float32)
    for u, T in enumerate(RAGGED):
        w = b.wav[u].cpu().numpy()
        if T < 4:
            assert (w == 3.0).all(), u
            continue
        X, mag, prev, lv, ref = gl_ref(T, F, 0.0)
        check('gl_istft ragged u=%d T=%d' % (u, T), 'wav', R.wav_err(w[:HOP * (T - 1)], ref['wav'], ref['sW']).max(), ref['twin_W'])
        assert (w[HOP * (T - 1):] == 3.0).all(), u
        wav_in[u, :HOP * (T - 1)] = ref['wav'].astype(np.float32)
    # forward: an fp32 waveform (the fp64 istft, rounded) is the exact input of both precisions
    wv = torch.from_numpy(wav_in).to(dev)
    spec = torch.full((n, Tm, NB, 2), 7.0, device=dev)
    L.call('zs_gl_stft_project', 'ZsGlStft', _stream(), wav=L.ptr(wv), wav_ld=wv.shape[1], mag=L.ptr(b.mag), lengths=L.ptr(b.len_t), n_utt=n,
           T_max=Tm, spec=L.ptr(spec))
    torch.cuda.synchronize()
    for u, T in enumerate(RAGGED):
        if T < 4:
            assert (spec[u] == 7.0).all(), u
            continue
        X, mag, prev, lv, _ = gl_ref(T, F, 0.0)
        y = wav_in[u, :HOP * (T - 1)]
        E64, E32 = R.stft(y, np.float64), R.stft(y, np.float32)
        o64, o32 = R.project(E64, mag, np.float64), R.project(E32, mag, np.float32)
        inp = np.sqrt(512.0) * np.sqrt((R.frames_of(y, np.float64) ** 2).sum(axis=1))      # Parseval: the frame's norm as a half spectrum
        sE = np.maximum(inp, R.frame_norms(E64))
        sO = np.maximum(sE, R.frame_norms(o64))
        twin_E = R.frame_err(E32, E64, sE).max()
        keep = np.abs(E64) >= R.ILL * R.FACTOR * twin_E * sE[None, :]
        out = spec_of(spec[u], T)
        assert np.isfinite(out).all()
        check('gl_stft_project ragged u=%d T=%d' % (u, T), 'spec', R.frame_err(out, o64, sO, keep).max(), R.frame_err(o32, o64, sO, keep).max())
        assert (np.abs(out)[~keep] <= mag[~keep].astype(np.float64) * (1 + 1e-6)).all()
        assert (out[mag == 0] == 0).all()
        assert (spec[u, T:] == 7.0).all(), u


def deemph_tol(ref):
    """One fp32 rounding of an fp64 recursion; the carry reassociation of the scan is negligible beside it."""
    return 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * np.abs(ref).max()


@pytest.mark.parametrize('coef', [0.97, 0.0])
def test_deemphasis_short_rows_vs_fp64(L, coef):
    """zs_gl_deemphasis on rows of 1, 2, 3, 8, 9 and 701 frames (L = 200 (T - 1) samples, 256 chunks of C = ceil(L / 256)): no samples;
    L = 200 (C = 1) and 400 (C = 2) with empty chunks; L = 1400 (C = 6, a last chunk of 2: the pow(a, n) branch); L = 1600 (C = 7, a
    last chunk of 4); a long row.  coef = 0 returns the input bit for bit.  Samples past L are untouched."""
    dev = _dev()
    Ts = [1, 2, 3, 8, 9, 701]
    ld = HOP * 700 + 7
    rng = np.random.RandomState(11)
    x = (rng.randn(len(Ts), ld) * 0.1).astype(np.float32)
    w = torch.from_numpy(x).to(dev)
    lens = torch.tensor(Ts, dtype=torch.int32, device=dev)
    L.check(L.lib().zs_gl_deemphasis(L.ptr(w), ld, L.ptr(lens), len(Ts), coef, _stream()), 'zs_gl_deemphasis')
    got = w.cpu().numpy()
    for u, T in enumerate(Ts):
        n = HOP * (T - 1)
        assert np.array_equal(got[u, n:], x[u, n:]), T
        if coef == 0.0:
            assert np.array_equal(got[u, :n], x[u, :n]), T
        elif n:
            ref = R.deemphasis(x[u, :n], coef)
            d = np.abs(got[u, :n] - ref)
            print('deemphasis T=%d: max |d| / tol %.3f' % (T, (d / deemph_tol(ref)).max()))
            assert (d <= deemph_tol(ref)).all(), T


def test_frame_mse_values_vs_fp64(L):
    """zs_gl_frame_mse (frame 2048, hop 512) on rows of 8, 40 and 123 frames with a head and a tail at 1e-5: every value within 1e-12
    (relative) of fp64, a 2048-term fp64 sum in another order.  Rows with L <= frame_length / 2 (6 frames and 1 frame) and the frames
    past L / hop are untouched."""
    dev = _dev()
    Ts = [8, 6, 40, 1, 123]
    ld = HOP * 122
    rng = np.random.RandomState(12)
    x = (rng.randn(len(Ts), ld) * 0.1).astype(np.float32)
    for u, T in enumerate(Ts):
        n = HOP * (T - 1)
        x[u, :int(0.13 * n)] *= 1e-5
        x[u, int(0.81 * n):n] *= 1e-5
    nf = 1 + ld // 512
    mse = torch.full((len(Ts), nf + 2), -1.0, dtype=torch.float64, device=dev)
    lens = torch.tensor(Ts, dtype=torch.int32, device=dev)
    L.check(L.lib().zs_gl_frame_mse(L.ptr(torch.from_numpy(x).to(dev)), ld, L.ptr(lens), len(Ts), 2048, 512, L.ptr(mse), nf + 2, _stream()),
            'zs_gl_frame_mse')
    m = mse.cpu().numpy()
    for u, T in enumerate(Ts):
        n = HOP * (T - 1)
        if n <= 1024:
            assert (m[u] == -1.0).all(), T
            continue
        ref = R.frame_mse(x[u, :n])
        k = 1 + n // 512
        rel = np.abs(m[u, :k] - ref) / ref
        print('frame_mse T=%d: max rel err %.3g' % (T, rel.max()))
        assert (rel <= 1e-12).all(), T
        assert (m[u, k:] == -1.0).all(), T


@pytest.mark.parametrize('n', [1, 255, 257, 4096 * 256 + 1])
def test_denormalize_vs_fp64(L, n):
    """zs_gl_denormalize at the clip edges and on random values; n = 4096 * 256 + 1 reaches the grid-stride loop.  Relative error
    <= 2e-6: powf is good to a few ulp, and the rounding of the exponent m * 0.05 in [-4, 1] is multiplied by ln 10 * |y|."""
    dev = _dev()
    edge = np.array([-0.5, 0, 1e-8, 0.25, 0.5, 1 - 2.0 ** -24, 1, 1.5], dtype=np.float32)
    x = np.random.RandomState(n % 1000).uniform(-0.1, 1.1, size=n).astype(np.float32)
    x[:min(n, len(edge))] = edge[:n]
    if n > 4096 * 256:
        x[-1] = 0.75                                              # the one element of the second grid-stride round
    xi = torch.from_numpy(x).to(dev)
    out = torch.full((n + 3,), 7.0, device=dev)
    L.check(L.lib().zs_gl_denormalize(L.ptr(xi), L.ptr(out), n, _stream()), 'zs_gl_denormalize')
    got = out.cpu().numpy()
    ref = R.denormalize(x)
    rel = np.abs(got[:n] - ref) / ref
    print('denormalize n=%d: max rel err %.3g' % (n, rel.max()))
    assert (rel <= 2e-6).all() and (got[n:] == 7.0).all()


PRE_N = [2, 199, 200, 256, 257, 400, 401, 512, 513, 801, 4999]
PREEMPH, REF_DB, MAX_DB = 0.97, 20.0, 100.0


@functools.lru_cache(maxsize=None)
def pre_inputs():
    rng = np.random.RandomState(21)
    ys = []
    for n in PRE_N:
        y = (rng.randn(n) * 0.1).astype(np.float32)
        y[n // 2:] *= 1e-3                                         # loud, then 60 dB down
        ys.append(y)
    refs = []
    for y in ys:
        mag64, amp64 = R.pre_spectrogram(y, PREEMPH, REF_DB, MAX_DB, np.float64)
        _, amp32 = R.pre_spectrogram(y, PREEMPH, REF_DB, MAX_DB, np.float32)
        inp = np.sqrt(512.0) * np.sqrt((R.frames_of(y, np.float64) ** 2).sum(axis=1))   # the windowed input frame as a half spectrum
        s = np.maximum(inp, R.frame_norms(amp64.T))
        refs.append((amp64, s, R.frame_err(amp32.T, amp64.T, s).max()))
    return ys, refs


@pytest.mark.parametrize('mag_ld', [513, 520])
@pytest.mark.parametrize('with_start', [False, True])
def test_pre_spectrogram_vs_fp64(L, mag_ld, with_start):
    """zs_pre_spectrogram on windows of 2 .. 4999 samples in one batch: at 400 samples and below the reflect padding of 512 folds more
    than once (the triangle wave of np.pad), 401 is the first length a single reflection serves, 513 the first with a frame that needs
    none on one side.  With `start` the windows sit at offsets inside NaN-filled rows: nothing outside a window may be read.  amp is
    within 16 x the fp32 twin per frame; mag lies in the fp64 image of [amp_ref - delta, amp_ref + delta] (delta: the frame's absolute
    amp bound), widened by 4 fp32 ulp (audio_ref.norm_db_interval), the 1e-5 floor included.  Padding columns of mag, rows past each
    utterance's frames and T_max > every frame count: untouched."""
    dev = _dev()
    ys, refs = pre_inputs()
    n_utt = len(ys)
    ld = max(PRE_N) + 64
    T_max = 1 + max(PRE_N) // HOP + 2
    wav = np.full((n_utt, ld), np.nan if with_start else 0.0, dtype=np.float32)
    starts = [(7 * u + 1) % 60 if with_start else 0 for u in range(n_utt)]
    for u, y in enumerate(ys):
        wav[u, starts[u]:starts[u] + len(y)] = y
    mag = torch.full((n_utt, T_max, mag_ld), 7.0, device=dev)
    amp = torch.full((n_utt, T_max, NB), 9.0, device=dev)
    wv = torch.from_numpy(wav).to(dev)
    ns = torch.tensor(PRE_N, dtype=torch.int32, device=dev)
    st = torch.tensor(starts, dtype=torch.int32, device=dev)
    L.call('zs_pre_spectrogram', 'ZsPreSpec', _stream(), wav=L.ptr(wv), wav_ld=ld, n_samples=L.ptr(ns), n_utt=n_utt, T_max=T_max,
           preemph=PREEMPH, ref_db=REF_DB, max_db=MAX_DB, mag=L.ptr(mag), mag_ld=mag_ld, amp=L.ptr(amp), start=L.ptr(st) if with_start else None)
    torch.cuda.synchronize()
    g_mag, g_amp = mag.cpu().numpy(), amp.cpu().numpy()
    assert (g_mag[:, :, NB:] == 7.0).all()
    for u, n in enumerate(PRE_N):
        T = 1 + n // HOP
        amp64, s, twin = refs[u]
        assert (g_mag[u, T:] == 7.0).all() and (g_amp[u, T:] == 9.0).all(), n
        case = 'pre_spectrogram n=%d mag_ld=%d start=%d' % (n, mag_ld, starts[u])
        check(case, 'amp', R.frame_err(g_amp[u, :T].T, amp64.T, s).max(), twin)
        delta = (R.FACTOR * twin * s)[:, None]
        lo, hi = R.norm_db_interval(np.maximum(amp64 - delta, 0.0), amp64 + delta, REF_DB, MAX_DB)
        got = g_mag[u, :T, :NB].astype(np.float64)
        assert ((got >= lo) & (got <= hi)).all(), (n, np.abs(got - R.norm_db(amp64, REF_DB, MAX_DB)).max())


@pytest.mark.parametrize('n_mels', [1, 80, 130])
@pytest.mark.parametrize('rows', [1, 3])
def test_pre_mel_vs_fp64(L, n_mels, rows):
    """zs_pre_mel with 1, 80 and 130 mel bands (130 exceeds the 128-thread block: the strided loop) on 1 and 3 rows, one all-zero row
    (the 1e-5 floor).  The fp64 reference starts from the very fp32 amp on the device; the result lies in the fp64 image of
    [s - delta, s + delta], delta = 513 * 2^-24 * sum_k |b_k a_k| (a 513-term fp32 sum in any order), widened by 4 fp32 ulp."""
    dev = _dev()
    rng = np.random.RandomState(100 * n_mels + rows)
    a = (np.abs(rng.randn(rows, NB)) * 10.0 ** rng.uniform(-6, 1, size=(rows, 1))).astype(np.float32)
    if rows > 1:
        a[rows // 2] = 0.0
    basis = (rng.rand(n_mels, NB) * (rng.rand(n_mels, NB) < 0.2)).astype(np.float32)
    if rows == 1 and n_mels == 1:
        a[:] = 0.0                                                 # the floor on the smallest launch as well
    ad, bd = torch.from_numpy(a).to(dev), torch.from_numpy(basis).to(dev)
    mel = torch.full((rows * n_mels + 5,), 7.0, device=dev)
    L.check(L.lib().zs_pre_mel(L.ptr(ad), L.ptr(bd), L.ptr(mel), rows, n_mels, REF_DB, MAX_DB, _stream()), 'zs_pre_mel')
    got = mel.cpu().numpy()
    assert (got[rows * n_mels:] == 7.0).all()
    got = got[:rows * n_mels].reshape(rows, n_mels).astype(np.float64)
    a64, b64 = ad.cpu().numpy().astype(np.float64), basis.astype(np.float64)
    s = a64 @ b64.T
    delta = NB * 2.0 ** -24 * (np.abs(a64) @ np.abs(b64).T)
    lo, hi = R.norm_db_interval(np.maximum(s - delta, 0.0), s + delta, REF_DB, MAX_DB)
    print('pre_mel n_mels=%d rows=%d: max |d| %.3g' % (n_mels, rows, np.abs(got - R.norm_db(s, REF_DB, MAX_DB)).max()))
    assert ((got >= lo) & (got <= hi)).all()
    if not a[rows // 2].any():
        assert (got[rows // 2] == float(np.float32(1e-8))).all()
