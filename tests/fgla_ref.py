"""Numpy restatement of fast Griffin-Lim (Perraudin et al. 2013, the `momentum` of librosa / torchaudio) on the oracle's stft /
istft, and the helpers the FGLA tests share.  With alpha = 0 it is zs_oracle.griffin_lim, operation for operation:
    E_n = stft(istft(X_{n-1}))         X_0 = S (zero phase)
    A_n = E_n - beta E_{n-1}           beta = alpha / (1 + alpha), A_1 = E_1
    X_n = S * A_n / max(1e-8, |A_n|)
    x   = istft(X_N)
"""
import os

import numpy as np

import zs_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURE = 'fgla_speech.npz'
FIXTURE_NAMES = ['128-m-1024/2.wav', '128-c-1024/4.wav', 's2-128-m-1024/1.wav']
FIXTURE_SAMPLES = [86200, 67000, 51712]


def beta_of(alpha):
    """beta as the kernels use it: fp32 alpha / (1 + alpha)."""
    a = np.float32(alpha)
    return np.float32(a / (np.float32(1) + a))


def fgla(spectrogram, n_iter, alpha):
    """Waveform of n_iter FGLA iterations on real [513, T] magnitudes (fp32, the oracle's transforms)."""
    S = np.asarray(spectrogram, dtype=np.float32)
    beta = beta_of(alpha)
    X = S.astype(np.complex64)
    prev = None
    for _ in range(n_iter):
        E = O.stft(O.istft(X))
        A = E if prev is None else E - beta * prev
        phase = A / np.maximum(1e-8, np.abs(A))
        X = S * phase
        prev = E
    return np.real(O.istft(X))


def spectral_convergence(wav, S):
    """SC = ||S - |STFT(x)||| / ||S||."""
    S = np.asarray(S, dtype=np.float64)
    return float(np.linalg.norm(np.abs(O.stft(wav)).astype(np.float64) - S) / np.linalg.norm(S))


def fixture_waves():
    """The fixture's utterances as float32 waveforms in [-1, 1) (int16 / 32768), with their names."""
    z = np.load(os.path.join(GOLD, FIXTURE), allow_pickle=False)
    names = [str(n) for n in z['names']]
    return [z['wav.%d' % i].astype(np.float32) / 32768.0 for i in range(len(names))], names


def fixture_amplitudes():
    """Amplitude spectrograms [513, T] (fp32) of the fixture's utterances, through the product's normalise / de-normalise path:
    zs_oracle.get_spectrograms(y, do_trim=False), then denormalize -- what the vocoder of a resynthesis sees."""
    waves, _ = fixture_waves()
    out = []
    for y in waves:
        _, mag = O.get_spectrograms(y, do_trim=False)
        out.append(np.asarray(O.denormalize(mag), dtype=np.float32))
    return out


def speechlike(n_frames, seed):
    """A harmonic + noise signal with a moving pitch and formant-like envelope: 200*(n_frames-1) samples at 16 kHz."""
    rng = np.random.RandomState(seed)
    n = 200 * (n_frames - 1)
    t = np.arange(n) / 16000.0
    f0 = 120 + 40 * np.sin(2 * np.pi * 0.7 * t)
    ph = 2 * np.pi * np.cumsum(f0) / 16000.0
    y = sum((0.5 / k) * np.sin(k * ph + rng.rand() * 6.28) * (1 + 0.5 * np.sin(2 * np.pi * (0.3 + 0.1 * k) * t)) for k in range(1, 24))
    y = y * (0.2 + 0.8 * (np.sin(2 * np.pi * 1.3 * t) > -0.3)) + 0.02 * rng.randn(n)
    return (0.2 * y / np.abs(y).max()).astype(np.float32)
