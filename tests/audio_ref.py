"""Plain NumPy / SciPy restatement of the audio path at both ends of the model, in two precisions, and the per-frame error
measure the audio tests share.

Every operation takes `dtype`.  np.float64 is the reference.  np.float32 is its fp32 twin: every array and every transform stays
single precision (scipy.fft computes in single precision for single-precision input; np.fft does not, so it is not used here).
The twin's distance from the reference is what fp32 arithmetic costs on a given input, and the GPU tests bound the kernels by a
multiple of it, on the same input, with the same measure.

Inputs that are exact in fp32 are the same numbers in both precisions: the window (the oracle's fp32 hann), beta (fgla_ref.beta_of),
the pre-emphasis coefficient, the mel basis.

Layouts follow the oracle: spectrograms of the vocoder are complex [513, T]; pre_spectrogram / pre_mel give [T, 513] / [T, n_mels].
"""
import numpy as np
import scipy.fft

import zs_oracle as O
from fgla_ref import beta_of

N_FFT, HOP, WIN, NB = 1024, 200, 800, 513
TINY32 = float(np.finfo(np.float32).tiny)


def _cdtype(dtype):
    return np.complex64 if np.dtype(dtype) == np.float32 else np.complex128


def window(dtype):
    """hann(800) centred in 1024: the oracle's fp32 values, in `dtype`."""
    return O.hann_padded().astype(dtype)


def reflect_index(j, n):
    """np.pad(mode='reflect') as an index map for ANY pad width: a triangle wave of period 2 (n - 1); n == 1 maps everything to 0."""
    j = np.asarray(j, dtype=np.int64)
    if n == 1:
        return np.zeros_like(j)
    P = 2 * (n - 1)
    m = np.mod(j, P)
    return np.where(m < n, m, P - m)


def old_pre_reflect_index(j, n):
    """What pre_spectrogram_kernel computed before the triangle-wave rule: reflect once, then clamp.  Kept to state, on the CPU,
    for which window lengths the two rules differ (test_audio_ref_host.py)."""
    j = np.asarray(j, dtype=np.int64)
    j = np.where(j < 0, -j, j)
    j = np.where(j >= n, 2 * (n - 1) - j, j)
    return np.clip(j, 0, n - 1)


def padded(y, pad):
    y = np.asarray(y)
    return y[reflect_index(np.arange(-pad, len(y) + pad), len(y))]


def frames_of(y, dtype):
    """The windowed, reflect-padded frames [T, 1024] of y, T = 1 + len(y) // 200."""
    yp = padded(np.asarray(y, dtype=dtype), N_FFT // 2)
    T = 1 + len(y) // HOP
    idx = np.arange(N_FFT)[None, :] + HOP * np.arange(T)[:, None]
    return yp[idx] * window(dtype)[None, :]


def stft(y, dtype=np.float64):
    """librosa.stft(y, 1024, 200, win_length=800), center=True with reflect padding: complex [513, 1 + len(y) // 200]."""
    out = scipy.fft.rfft(frames_of(y, dtype), axis=1).T
    assert out.dtype == _cdtype(dtype)
    return out


def istft(S, dtype=np.float64):
    """librosa.istft(S, 200, win_length=800) (<= 0.7): irfft that ignores the imaginary parts of DC and Nyquist, window, overlap-add,
    division by the window-sum-square where it exceeds tiny(fp32), centre trim: 200 (T - 1) samples."""
    S = np.array(S, dtype=_cdtype(dtype))
    S[0] = S[0].real
    S[N_FFT // 2] = S[N_FFT // 2].real
    w = window(dtype)
    T = S.shape[1]
    ytmp = scipy.fft.irfft(S.T, n=N_FFT, axis=1)
    assert ytmp.dtype == np.dtype(dtype)
    ytmp = ytmp * w[None, :]
    n = N_FFT + HOP * (T - 1)
    y = np.zeros(n, dtype=dtype)
    wss = np.zeros(n, dtype=dtype)
    wsq = w * w
    for i in range(T):
        y[i * HOP:i * HOP + N_FFT] += ytmp[i]
        wss[i * HOP:i * HOP + N_FFT] += wsq
    nz = wss > TINY32
    y[nz] /= wss[nz]
    return y[N_FFT // 2:n - N_FFT // 2]


def project(A, mag, dtype):
    A = np.asarray(A, dtype=_cdtype(dtype))
    return (np.asarray(mag, dtype=dtype) * (A / np.maximum(dtype(1e-8), np.abs(A)))).astype(_cdtype(dtype))


def gl_iter(X, mag, prev=None, beta=0, dtype=np.float64):
    """One Griffin-Lim iteration: wav = istft(X), E = stft(wav), A = E - beta prev (A = E without prev), spec_out = mag A / max(1e-8, |A|).
    Returns (spec_out, E, wav)."""
    wav = istft(X, dtype)
    E = stft(wav, dtype)
    A = E if prev is None else E - dtype(beta) * np.asarray(prev, dtype=_cdtype(dtype))
    return project(A, mag, dtype), E, wav


def griffin_lim(S, n_iter, alpha=0.0, dtype=np.float64, states=False):
    """n_iter (fast) Griffin-Lim iterations from zero phase, then the inverse transform.  states: also the last E."""
    S = np.asarray(S, dtype=dtype)
    beta = beta_of(alpha)
    X = S.astype(_cdtype(dtype))
    prev = None
    for _ in range(n_iter):
        X, prev, _ = gl_iter(X, S, prev if alpha > 0 else None, beta, dtype)
    wav = istft(X, dtype)
    return (wav, prev) if states else wav


def deemphasis(x, coef, dtype=np.float64):
    """scipy.signal.lfilter([1], [1, -coef], x): y[n] = x[n] + coef y[n-1], with coef the fp32 number the C entry point receives."""
    c = dtype(np.float32(coef))
    y = np.empty(len(x), dtype=dtype)
    acc = dtype(0)
    for i, v in enumerate(np.asarray(x, dtype=dtype)):
        acc = v + c * acc
        y[i] = acc
    return y


def frame_mse(x, frame_length=2048, hop=512, dtype=np.float64):
    """Mean square of the centred, reflect-padded frames of librosa.effects.trim: 1 + len(x) // hop values."""
    yp = padded(np.asarray(x, dtype=dtype), frame_length // 2)
    nf = 1 + len(x) // hop
    idx = np.arange(frame_length)[None, :] + hop * np.arange(nf)[:, None]
    return np.mean(yp[idx] ** 2, axis=1, dtype=dtype)


def denormalize(x, dtype=np.float64):
    """convert.py:56-58, element by element (no transpose): 10 ** ((clip(x, 0, 1) * 100 - 100 + 20) * 0.05)."""
    m = np.clip(np.asarray(x, dtype=dtype), 0, 1) * dtype(O.MAX_DB) - dtype(O.MAX_DB) + dtype(O.REF_DB)
    return np.power(dtype(10.0), m * dtype(0.05))


def norm_db(a, ref_db, max_db, dtype=np.float64):
    """clip((20 log10(max(1e-5, a)) - ref_db + max_db) / max_db, 1e-8, 1): monotone in a."""
    a = np.asarray(a, dtype=dtype)
    db = dtype(20) * np.log10(np.maximum(dtype(1e-5), a))
    return np.clip((db - dtype(ref_db) + dtype(max_db)) / dtype(max_db), dtype(1e-8), dtype(1))


def preemphasis(y, preemph, dtype):
    y = np.asarray(y, dtype=dtype)
    return np.append(y[:1], y[1:] - dtype(np.float32(preemph)) * y[:-1]).astype(dtype)


def pre_spectrogram(y, preemph=O.PREEMPH, ref_db=O.REF_DB, max_db=O.MAX_DB, dtype=np.float64):
    """preprocess.py:239-258 after the trim: (mag [T, 513] normalised, amp [T, 513] linear)."""
    amp = np.abs(stft(preemphasis(y, preemph, dtype), dtype)).T
    return norm_db(amp, ref_db, max_db, dtype), amp


def pre_mel(amp, basis, ref_db=O.REF_DB, max_db=O.MAX_DB, dtype=np.float64):
    """amp [rows, 513], basis [n_mels, 513] -> normalised mel [rows, n_mels]."""
    s = np.asarray(amp, dtype=dtype) @ np.asarray(basis, dtype=dtype).T
    return norm_db(s, ref_db, max_db, dtype)


def norm_db_interval(lo, hi, ref_db, max_db):
    """The fp64 image of [lo, hi] under norm_db, widened by 4 fp32 ulp.  norm_db in fp32 rounds 20 log10(a), the two dB offsets and
    the division: its intermediates are as large as M = max(|dB|, ref_db, max_db), so an ulp of the expression is ulp32(M) / max_db
    next to the ulp of the result itself -- near the floor the result is far smaller than the dB values it is the difference of."""
    f_lo, f_hi = norm_db(lo, ref_db, max_db), norm_db(hi, ref_db, max_db)
    db = np.abs(20.0 * np.log10(np.maximum(1e-5, np.maximum(np.abs(lo), np.abs(hi)))))
    M = np.maximum(db, max(abs(ref_db), abs(max_db))).astype(np.float32)
    w = 4.0 * (np.spacing(M).astype(np.float64) / max_db + np.spacing(f_hi.astype(np.float32)).astype(np.float64))
    return f_lo - w, f_hi + w


# ---- the error measure -------------------------------------------------------------------------------------------------------------

def frame_norms(Z):
    """L2 norm of every frame (column) of a [bins, T] array."""
    return np.sqrt((np.abs(np.asarray(Z)).astype(np.float64) ** 2).sum(axis=0))


def window_max(v, lo, hi):
    """out[t] = max(v[t + lo .. t + hi]) with the range cut at the ends."""
    v = np.asarray(v, dtype=np.float64)
    n = len(v)
    return np.array([v[max(0, t + lo):min(n, t + hi + 1)].max() if min(n, t + hi + 1) > max(0, t + lo) else 0.0 for t in range(n)])


def spec_scale(inp, out64):
    """s_t: the largest L2 norm among the input frames and the fp64 output frames t-3 .. t+3, the dependency range of one
    Griffin-Lim iteration (a sample is touched by 4 frames, a frame touches 800 samples)."""
    return window_max(np.maximum(frame_norms(inp), frame_norms(out64)), -3, 3)


def frame_err(got, ref64, scale, keep=None):
    """||got_t - ref64_t||_2 / s_t per frame (over the bins of `keep` only).  A frame of scale 0 has error 0 if it is reproduced
    exactly and inf if not."""
    d = np.abs(np.asarray(got).astype(np.complex128) - ref64)
    if keep is not None:
        d = d * keep
    e = np.sqrt((d ** 2).sum(axis=0))
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(scale > 0, e / scale, np.where(e > 0, np.inf, 0.0))


def wav_scale(inp, T):
    """Per block of 200 samples b (T - 1 of them): the largest time-domain norm ||X_i|| sqrt(2 / 1024) (Parseval for a half
    spectrum) of the input frames i = b-1 .. b+2, the four whose 800-sample windows overlap the block."""
    return window_max(frame_norms(inp) * np.sqrt(2.0 / N_FFT), -1, 2)[:T - 1]


def wav_err(got, ref64, scale):
    """||got_b - ref64_b||_2 / s_b per block of 200 samples."""
    nb = len(ref64) // HOP
    d = (np.asarray(got, dtype=np.float64)[:nb * HOP] - ref64[:nb * HOP]).reshape(nb, HOP)
    e = np.sqrt((d ** 2).sum(axis=1))
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(scale > 0, e / scale, np.where(e > 0, np.inf, 0.0))


FACTOR = 16.0          # GPU bound = FACTOR x the fp32 twin's error in the same measure, on the same input
CAP = 1e-5             # and never above the worst-case bound of an fp32 radix-2 1024-point transform, log2(N) * ~10 eps + window rounding
# |A_ref| below ILL x the frame's absolute error bound B s_t (an L2 bound, so it bounds every bin): the phase of that bin is
# ill-conditioned.  Measured on the CPU (test_audio_ref_host.py): ~0.4 % of the bins of an interior frame at full level; ~6 % of the
# first and the last frame (reflection makes their spectrum real up to a phase ramp: a one-dimensional Gaussian, not a Rayleigh
# amplitude); and every bin of a quiet or zero frame two or three frames from a loud one, whose scale is the loud neighbour's.
# Comparing a bin with its share B s_t / sqrt(513) instead would keep those, but lets 1 / |A| amplify single bins until the twin's
# own error reaches 3e-6 (16 x that is past the 1e-5 cap), so the L2 bound it is.
ILL = 1000.0


# ---- inputs of the Griffin-Lim iteration tests ----------------------------------------------------------------------------------

GL_SHAPES = [(4, 0), (5, 4), (17, 4), (40, 10), (53, 26), (131, 42)]          # (T, tile_frames)
GL_NO_PREFETCH = [(17, 4), (53, 26)]
# T: (first quiet frame, quiet frames, first of the 8 zero frames).  The quiet stretch starts one frame after a tile boundary of the
# tile sizes T is run with (tile_starts; checked in test_audio_ref_host.py).
GL_STRETCH = {5: (3, 1, None), 9: (4, 2, None), 17: (4, 2, 8), 23: (4, 3, 12), 40: (11, 6, 24), 53: (18, 8, 38), 131: (33, 13, 70)}


def tile_starts(T, F):
    F = F if F > 0 else 10
    nt = (T + F - 1) // F
    return [tile * T // nt for tile in range(nt + 1)]


def gl_levels(T, F):
    """Per-frame level of the test spectrogram: 1, a stretch at 1e-3 that starts one frame after a tile boundary, and 8 all-zero
    frames (level 0).  Short utterances get what fits: T = 5 one quiet frame behind its only tile boundary, T = 4 none."""
    lv = np.ones(T)
    if T in GL_STRETCH:
        b, q, z = GL_STRETCH[T]
        lv[b:b + q] = 1e-3
        if z is not None:
            lv[z:z + 8] = 0.0
    return lv


def gl_case(T, F, seed=None):
    """(X complex64 [513, T], mag fp32 [513, T], prev complex64 [513, T], levels): a random spectrogram with nonzero imaginary parts
    at DC and Nyquist, magnitudes independent of it with ~5 % exact zeros and nonzero on the zero frames, a random state."""
    rng = np.random.RandomState(1000 * T + F if seed is None else seed)
    lv = gl_levels(T, F)
    X = ((rng.randn(NB, T) + 1j * rng.randn(NB, T)) * lv[None, :]).astype(np.complex64)
    mag = (np.abs(rng.randn(NB, T)) * np.where(lv > 0, lv, 1.0)[None, :]).astype(np.float32)
    mag[rng.rand(NB, T) < 0.05] = 0.0
    prev = ((rng.randn(NB, T) + 1j * rng.randn(NB, T)) * lv[None, :]).astype(np.complex64)     # zero where X is: A = E - beta prev
    return X, mag, prev, lv


def zero_dependency_frames(lv):
    """Frames whose whole dependency range t-3 .. t+3 has level 0."""
    T = len(lv)
    return [t for t in range(T) if t - 3 >= 0 and t + 3 < T and not lv[t - 3:t + 4].any()]


def gl_reference(X, mag, prev, alpha):
    """fp64 reference and fp32 twin of one iteration, the measure's scales, the twin's errors and the bounds they give.
    Returns a dict; 'keep' marks the bins whose phase is well conditioned (|A_ref| >= ILL x the frame's absolute bound on E)."""
    beta = beta_of(alpha)
    pv = prev if alpha > 0 else None
    o64, E64, w64 = gl_iter(X, mag, pv, beta, np.float64)
    o32, E32, w32 = gl_iter(X, mag, pv, beta, np.float32)
    T = X.shape[1]
    sE = spec_scale(X, E64)
    twin_E = frame_err(E32, E64, sE)
    bound_E = FACTOR * twin_E.max()
    A64 = E64 if pv is None else E64 - np.float64(beta) * pv.astype(np.complex128)
    keep = np.abs(A64) >= ILL * bound_E * sE[None, :]
    inp_o = np.maximum(frame_norms(X), frame_norms(pv) if pv is not None else 0.0)
    sO = window_max(np.maximum(inp_o, frame_norms(o64)), -3, 3)
    twin_O = frame_err(o32, o64, sO, keep)
    sW = wav_scale(X, T)
    twin_W = wav_err(w32, w64, sW)
    return dict(out=o64, E=E64, wav=w64, A=A64, sE=sE, sO=sO, sW=sW, keep=keep,
                twin_E=twin_E.max(), twin_O=twin_O.max(), twin_W=twin_W.max(),
                bound_E=bound_E, bound_O=FACTOR * twin_O.max(), bound_W=FACTOR * twin_W.max())
