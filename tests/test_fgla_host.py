"""Fast Griffin-Lim (momentum) without a GPU: the numpy restatement the GPU tests compare with, the keyword validation that runs
before any device work, the --gl_iters / --gl_momentum command line, and the real-speech fixture."""
import math
import os
import sys

import numpy as np
import pytest

import fgla_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HPS = os.path.join(ROOT, 'hps', 'zerospeech_english.json')


def test_restatement_at_zero_momentum_is_the_oracle_loop():
    import zs_oracle as O
    S = np.abs(O.stft(F.speechlike(60, 1))).astype(np.float32)
    for n in (0, 1, 7):
        assert np.array_equal(F.fgla(S, n, 0.0), O.griffin_lim(S, n_iter=n))


def test_restatement_fgla_100_beats_plain_300_on_speech():
    """The fixture's 259-frame utterance through the product's normalise / de-normalise path: FGLA (alpha = 0.99) reaches a lower
    spectral convergence in 100 iterations than the plain loop in 300."""
    import zs_oracle as O
    S = F.fixture_amplitudes()[2]
    assert S.shape == (513, 259)
    sc_fgla = F.spectral_convergence(F.fgla(S, 100, 0.99), S)
    sc_plain = F.spectral_convergence(O.griffin_lim(S, n_iter=300), S)
    print('SC fgla(0.99, 100) %.4f  plain(300) %.4f' % (sc_fgla, sc_plain))
    assert sc_fgla < sc_plain


@pytest.mark.parametrize('m', [-0.1, 1.0, float('nan'), float('inf'), 'x'])
def test_momentum_out_of_range_raises_before_device_work(m):
    import zs_amd  # noqa: F401
    from zs_amd import convert as cv
    mags = [np.ones((513, 8), dtype=np.float32)]
    with pytest.raises(ValueError):
        cv.griffin_lim_batch(mags, n_iter=1, momentum=m)
    with pytest.raises(ValueError):
        cv.griffin_lim(mags[0], n_iter=1, momentum=m)
    with pytest.raises(ValueError):
        cv.spectrogram2wav_batch([np.full((8, 513), 0.5, dtype=np.float32)], n_iter=1, momentum=m)
    with pytest.raises(ValueError):
        cv.resynth_batch([np.full((8, 513), 0.5, dtype=np.float32)], None, 128, [0], n_iter=1, momentum=m)
    with pytest.raises(ValueError):
        cv.cross_test(None, 128, 'no-such-dataset', 'no-such-speaker2id.json', 'no-result-dir', True, momentum=m)


def test_split_impl_has_no_momentum():
    import zs_amd  # noqa: F401
    from zs_amd import convert as cv
    with pytest.raises(ValueError):
        cv.griffin_lim_batch([np.ones((513, 8), dtype=np.float32)], n_iter=1, impl='split', momentum=0.5)


def test_default_momentum_comes_from_hp(monkeypatch):
    import zs_amd  # noqa: F401
    from zs_amd import convert as cv
    from zs_amd.hps import hp
    assert hp.gl_momentum == 0.0 and hp.n_iter == 300
    assert cv.gl_momentum(None) == 0.0 and cv.gl_momentum(0.99) == pytest.approx(0.99)
    monkeypatch.setattr(hp, 'gl_momentum', 0.5)
    assert cv.gl_momentum(None) == 0.5
    monkeypatch.setattr(hp, 'gl_momentum', 1.5)              # a bad process default is caught by every entry point that reads it
    with pytest.raises(ValueError):
        cv.spectrogram2wav_batch([np.full((8, 513), 0.5, dtype=np.float32)], n_iter=1)
    with pytest.raises(ValueError):
        cv.griffin_lim_batch([np.ones((513, 8), dtype=np.float32)], n_iter=1)


def _main():
    sys.path.insert(0, ROOT)
    import main
    return main


def test_cli_gl_flags_land_in_hp(monkeypatch):
    main = _main()
    from zs_amd.hps import hp
    monkeypatch.setattr(hp, 'n_iter', hp.n_iter)             # restored after the test
    monkeypatch.setattr(hp, 'gl_momentum', hp.gl_momentum)
    main.argument_runner(['--test', '--hps_path', HPS])
    assert hp.n_iter == 300 and hp.gl_momentum == 0.0
    args, _ = main.argument_runner(['--test', '--gl_iters', '100', '--gl_momentum', '0.99', '--hps_path', HPS])
    assert args.gl_iters == 100 and args.gl_momentum == 0.99
    assert hp.n_iter == 100 and hp.gl_momentum == 0.99
    main.argument_runner(['--test', '--gl_iters', '0', '--hps_path', HPS])
    assert hp.n_iter == 0 and hp.gl_momentum == 0.99        # a flag that is not given leaves hp as it is
    for bad in (['--gl_momentum', '1'], ['--gl_momentum', '1.5'], ['--gl_momentum', '-0.1'], ['--gl_momentum', 'nan'],
                ['--gl_momentum', 'x'], ['--gl_iters', '-1'], ['--gl_iters', '2.5']):
        with pytest.raises(SystemExit):
            main.build_parser().parse_args(bad)


def test_cli_gl_flags_reach_the_vocoder_of_every_test_mode(monkeypatch, tmp_path):
    """main.py --test --cross_test --test_single --gl_iters 100 --gl_momentum 0.99: each driver runs with hp set (the drivers' vocoder
    reads hp.n_iter / hp.gl_momentum when no keyword is given; the GPU tests check that it does)."""
    main = _main()
    import zs_amd.convert as cv
    from zs_amd.hps import hp
    monkeypatch.setattr(hp, 'n_iter', hp.n_iter)
    monkeypatch.setattr(hp, 'gl_momentum', hp.gl_momentum)
    seen = {}

    def record(name):
        def fn(*a, **kw):
            assert 'n_iter' not in kw and 'momentum' not in kw
            seen[name] = (hp.n_iter, hp.gl_momentum, cv.gl_momentum(None))
        return fn
    monkeypatch.setattr(cv, 'get_trainer', lambda *a, **kw: object())
    for name in ('test_from_list', 'cross_test', 'test_single'):
        monkeypatch.setattr(cv, name, record(name))
    main.main(['--test', '--cross_test', '--test_single', '--gl_iters', '100', '--gl_momentum', '0.99', '--hps_path', HPS,
               '--result_dir', str(tmp_path / 'result'), '--ckpt_pth', str(tmp_path / 'model.pth')])
    assert seen == {k: (100, 0.99, 0.99) for k in ('test_from_list', 'cross_test', 'test_single')}


def test_fixture_contents():
    z = np.load(os.path.join(F.GOLD, F.FIXTURE), allow_pickle=False)
    assert sorted(z.files) == ['names', 'wav.0', 'wav.1', 'wav.2']
    assert [str(n) for n in z['names']] == F.FIXTURE_NAMES
    for i, n in enumerate(F.FIXTURE_SAMPLES):
        w = z['wav.%d' % i]
        assert w.dtype == np.int16 and w.shape == (n,) and np.abs(w.astype(np.int32)).max() > 1000
    frames = [1 + n // 200 for n in F.FIXTURE_SAMPLES]
    assert frames == [432, 336, 259]
    assert math.isclose(sum(F.FIXTURE_SAMPLES) * 2 / 1e3, 409.8, rel_tol=1e-3)
