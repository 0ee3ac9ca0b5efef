"""Independent NumPy restatement of the resampler's definition (zs_amd/resample.py), by the DIRECT sum over the input samples in
fp64 -- no polyphase bank, no phase arithmetic -- and the helpers the resampling tests share.

    tab[i] = rolloff * sinc(rolloff * i / 512) * K[i],  i = 0..32768,  K = right half of numpy.kaiser(2 * 32768 + 1, beta)
    h(u):  a = |u| * 512, i = floor(a);  tab[i] + (a - i) * (tab[i + 1] - tab[i]) if i < 32768 else 0
    s = min(1, sr_out / sr_in),  n_out = ceil(n_in * sr_out / sr_in)
    y[t] = s * sum_{m = 0}^{n_in - 1} x[m] * h(s * (t * sr_in / sr_out - m))
    A[t] = s * sum_m |x[m] * h(...)|                    (the scale of the rounding bound of an fp32 evaluation)

t * sr_in / sr_out - m is formed as the exact integer t * sr_in - m * sr_out over sr_out (one rounding), so the argument of h
carries no cancellation error at large t.  The sum runs over every m at which h can be non-zero (|t * sr_in / sr_out - m| * s <
64, a window of at most 2 * 64 / s + 1 samples): the terms left out are exact zeros.
"""
import numpy as np

NZ, STEPS = 64, 512
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492

_TAB = []


def table():
    if not _TAB:
        n = NZ * STEPS
        i = np.arange(n + 1, dtype=np.float64)
        x = ROLLOFF * i / STEPS
        with np.errstate(invalid='ignore', divide='ignore'):
            sinc = np.where(x == 0, 1.0, np.sin(np.pi * x) / (np.pi * x))
        _TAB.append(ROLLOFF * sinc * np.kaiser(2 * n + 1, BETA)[n:])
    return _TAB[0]


def h(u):
    tab = table()
    a = np.abs(u) * STEPS
    i = np.floor(a).astype(np.int64)
    ok = i < NZ * STEPS
    i = np.minimum(i, NZ * STEPS - 1)
    return np.where(ok, tab[i] + (a - i) * (tab[i + 1] - tab[i]), 0.0)


def n_out(n_in, sr_in, sr_out):
    return (int(n_in) * int(sr_out) + int(sr_in) - 1) // int(sr_in)


def resample_ref(x, sr_in, sr_out):
    """(y fp64 [n_out], A fp64 [n_out]) of the definition above for a 1-D signal x."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    no = n_out(n, sr_in, sr_out)
    s = min(1.0, sr_out / sr_in)
    half = int(np.ceil(NZ / s)) + 1                                     # h is zero beyond |m - centre| >= 64 / s
    t = np.arange(no, dtype=np.int64)
    m = (t * sr_in // sr_out)[:, None] + np.arange(-half, half + 1, dtype=np.int64)[None, :]
    inside = (m >= 0) & (m < n)
    num = t[:, None] * sr_in - m * sr_out                               # exact
    w = h(s * (num / float(sr_out)))
    terms = np.where(inside, x[np.clip(m, 0, n - 1)] * w, 0.0)
    return s * terms.sum(axis=1), s * np.abs(terms).sum(axis=1)


def bound(n_tap, A):
    """|fp32 evaluation - exact| for a sum of n_tap products of fp32-rounded taps, accumulated in fp32 in any order: each of the
    n_tap terms carries the tap's rounding (2^-24 relative), the product's (absorbed by an FMA) and at most n_tap - 1 additions'
    (2^-24 of a partial sum each, partial sums bounded by A); (n_tap + 4) * 2^-24 * A covers them to first order, the 1e-12 the
    fp64 reference's own error."""
    return (n_tap + 4) * 2.0 ** -24 * A + 1e-12


def tone_wav(rng, n, sr, silence=0):
    """The signal of tests/test_preprocess.py::_tone_wav generated at the rate `sr`."""
    t = np.arange(n) / float(sr)
    y = 0.3 * np.sin(2 * np.pi * rng.uniform(100, 3000) * t) + 0.1 * np.sin(2 * np.pi * rng.uniform(3000, 7000) * t)
    y = y + 0.02 * rng.randn(n)
    if silence:
        y[:silence] *= 1e-5
        y[-silence:] *= 1e-5
    return y.astype(np.float32)
