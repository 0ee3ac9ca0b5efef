"""Host: the two-precision reference of tests/audio_ref.py against the oracle, numpy's reflect padding and fgla_ref; the reflect rule
of pre_spectrogram_kernel before and after the triangle wave, as indices; and the share of bins the Griffin-Lim iteration tests
treat as ill-conditioned.  No GPU."""
import numpy as np

import audio_ref as R
import fgla_ref
import zs_oracle as O

EPS32 = 2.0 ** -24


def _wave(n, seed):
    rng = np.random.RandomState(seed)
    y = (rng.randn(n) * 0.1).astype(np.float32)
    y[n // 3:n // 2] *= 1e-3
    return y


def _close32(a, b, k=64):
    """a agrees with the oracle's fp32 result b to the oracle's own rounding: k fp32 epsilons of the largest value."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b).max()
    assert err <= k * EPS32 * np.abs(b).max(), (err, np.abs(b).max())


def test_fp64_reference_agrees_with_the_oracle():
    """stft, istft, griffin_lim (2 iterations), get_spectrograms(do_trim=False), denormalize, de_preemphasis and trim's frame means, on
    inputs of 513 samples or more (numpy's reflect padding of 512 and the triangle wave are the same map there)."""
    for n in (513, 801, 4999):
        y = _wave(n, n)
        S = R.stft(y)
        _close32(S, O.stft(y))
        _close32(R.istft(S.astype(np.complex64)), O.istft(S.astype(np.complex64)))
        mel, mag = O.get_spectrograms(y, do_trim=False)
        m64, a64 = R.pre_spectrogram(y)
        # the oracle's amplitudes carry its fp32 transform's rounding, 64 eps of the largest; the log maps that interval
        d = 64 * EPS32 * a64.max()
        lo, hi = R.norm_db_interval(np.maximum(a64 - d, 0), a64 + d, O.REF_DB, O.MAX_DB)
        assert ((mag >= lo) & (mag <= hi)).all() and ((m64 >= lo) & (m64 <= hi)).all()
        s64 = a64 @ O.mel_basis().astype(np.float64).T
        d = 64 * EPS32 * a64.max() * O.mel_basis().sum(axis=1)[None, :]
        lo, hi = R.norm_db_interval(np.maximum(s64 - d, 0), s64 + d, O.REF_DB, O.MAX_DB)
        m = R.pre_mel(a64, O.mel_basis())
        assert ((mel >= lo) & (mel <= hi)).all() and ((m >= lo) & (m <= hi)).all()
    mags = np.abs(R.stft(_wave(200 * 16, 5))).astype(np.float32)
    # two iterations pass through a projection: fp32 rounding of E moves the phase of small bins, 1e-4 of the scale covers it
    _close32(R.griffin_lim(mags, 2), O.griffin_lim(mags, n_iter=2), k=1e-4 / EPS32)
    x = np.random.RandomState(1).rand(7, 513).astype(np.float32) * 1.2 - 0.1
    # the oracle evaluates in fp32 for fp32 input: the rounding of the exponent m * 0.05 in [-4, 1] times ln 10 * |y|, as on the GPU
    assert np.allclose(R.denormalize(x).T, O.denormalize(x), rtol=2e-6, atol=0)
    assert np.allclose(R.denormalize(x).T, O.denormalize(x.astype(np.float64)), rtol=1e-13, atol=0)
    w = _wave(3000, 2)
    # the oracle filters with the Python float 0.97, the kernels with the fp32 number: (0.97 - fp32(0.97)) * gain 33 apart
    assert np.allclose(R.deemphasis(w, 0.97), O.de_preemphasis(w, float(np.float32(0.97))), rtol=1e-13, atol=1e-16)
    yp = np.pad(w.astype(np.float64), 1024, mode='reflect')
    idx = np.arange(2048)[None, :] + 512 * np.arange(1 + len(w) // 512)[:, None]
    assert np.allclose(R.frame_mse(w), np.mean(yp[idx] ** 2, axis=1), rtol=1e-13, atol=0)
    _, (a, b) = O.trim(w)
    db = 10 * np.log10(np.maximum(1e-10, R.frame_mse(w)))
    keep = np.flatnonzero(db - db.max() > -60)
    assert (a, b) == (int(keep[0]) * 512, min(len(w), (int(keep[-1]) + 1) * 512))


def test_reflect_rule_is_numpys_for_every_length():
    """reflect_index equals np.pad(mode='reflect') with a pad of 512 for every length 2 .. 700."""
    for n in range(2, 701):
        ref = np.pad(np.arange(n), 512, mode='reflect')
        assert np.array_equal(R.reflect_index(np.arange(-512, n + 512), n), ref), n
    assert (R.reflect_index(np.arange(-5, 6), 1) == 0).all()


def test_reflect_once_then_clamp_differs_below_401_samples():
    """The rule pre_spectrogram_kernel used before (reflect once, clamp) against the triangle wave, over the window's support
    (n in [112, 912) of the frame) of every frame: different indices for 300 of the lengths 2 .. 400, the same for every length from
    401 on -- the short-window cases of test_gpu_audio_fp64.py fail with the old rule, and longer windows keep their bits."""
    differ = []
    for n in range(2, 1201):
        t = np.arange(1 + n // 200)[:, None]
        j = 200 * t + np.arange(112, 912)[None, :] - 512
        if not np.array_equal(R.old_pre_reflect_index(j, n), R.reflect_index(j, n)):
            differ.append(n)
    assert len(differ) == 300 and max(differ) == 400, (len(differ), max(differ))


def test_fp32_twin_is_single_precision_and_equals_fgla_ref():
    """Every transform of the twin stays fp32 (asserted inside stft / istft), and fgla_ref.fgla (the oracle's fp32 transforms) equals
    griffin_lim(dtype=float32) to fp32 rounding through two projections."""
    y = _wave(200 * 16, 9)
    S = np.abs(R.stft(y)).astype(np.float32)
    for alpha in (0.0, 0.99):
        a = R.griffin_lim(S, 2, alpha, np.float32)
        assert a.dtype == np.float32
        _close32(a, fgla_ref.fgla(S, 2, alpha), k=1e-4 / EPS32)


def test_quiet_stretch_starts_one_frame_after_a_tile_boundary():
    for T, F in R.GL_SHAPES + [(23, 4), (9, 4)]:
        lv = R.gl_levels(T, F)
        if T in R.GL_STRETCH:
            b = R.GL_STRETCH[T][0]
            assert b - 1 in R.tile_starts(T, F)[1:-1] and lv[b] == 1e-3 and lv[b - 1] == 1.0, (T, F)
        if T >= 17:
            assert (lv == 0).sum() == 8 and len(R.zero_dependency_frames(lv)) == 2


def test_ill_conditioned_share_of_the_iteration_inputs():
    """The bins whose phase the GPU tests do not compare (|A_ref| < 1000 x the frame's absolute bound), counted with the fp32 twin:
    at most 1 % of the bins of the interior frames at full level whose neighbours within 3 frames are at full level too; at most 10 %
    of the first and the last frame (reflection makes their spectrum real up to a phase ramp).  Frames within 3 of a level change are
    ill-conditioned by the measure itself: their scale is the loud neighbour's.  The twin's error stays under 1e-5 / 16 everywhere."""
    for T, F in R.GL_SHAPES + [(23, 4), (9, 4)]:
        for alpha in (0.0, 0.5):
            X, mag, prev, lv = R.gl_case(T, F)
            r = R.gl_reference(X, mag, prev, alpha)
            for k in ('bound_E', 'bound_O', 'bound_W'):
                assert 0 < r[k] <= R.CAP, (T, F, alpha, k, r[k])
            ill = (~r['keep']).mean(axis=0)
            full = np.array([lv[max(0, t - 3):t + 4].min() == 1.0 for t in range(T)])
            inner = full.copy()
            inner[[0, T - 1]] = False
            if inner.any():
                assert ill[inner].mean() <= 0.01, (T, F, alpha, ill[inner].mean())
            assert ill[[0, T - 1]].max() <= 0.10, (T, F, alpha, ill[[0, T - 1]])
            for t in R.zero_dependency_frames(lv):
                assert not r['E'][:, t].any() and not r['out'][:, t].any()
