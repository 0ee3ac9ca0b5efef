"""The weight averages through checkpoints, loading and resume: the `<net>_ema` entries of a checkpoint, Trainer.load_model /
convert.get_trainer with use_ema, and Trainer.train(resume=True) with averages, against an uninterrupted run bit for bit.

The runs are six pretrain_AE iterations on small nets with a checkpoint every three (the pattern of test_gpu_resume.py, its
helpers re-stated here).  decay 0.5: after a few steps at lr 1e-4 the average is far enough from the weights to differ in most
elements, and close enough that nothing else about the nets changes."""
import io
import json
import os
import shutil
from contextlib import redirect_stdout

import pytest
import torch

pytestmark = pytest.mark.gpu

ITERS, EVERY, DECAY = 6, 3, 0.5
NETS = ('encoder', 'decoder', 'generator', 'classifier', 'patch_discriminator', 'target_classifier')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _cadence(monkeypatch):
    monkeypatch.setenv('ZS_CKPT_EVERY', str(EVERY))
    monkeypatch.setenv('ZS_LOG_EVERY', '1')


def _hps(iters=ITERS, **kw):
    from zs_amd.hps import make_hps
    d = dict(enc_size=8, emb_size=32, n_speakers=102, n_target_speakers=2, batch_size=4, enc_pretrain_iters=iters,
             dis_pretrain_iters=iters, iters=iters, patch_iters=iters, tclf_iters=iters, n_latent_steps=1, lat_sched_iters=4,
             n_patch_steps=2, max_to_keep=10)
    d.update(kw)
    return make_hps(**d)


_SETS = {}


def _data():
    from zs_amd.dataloader import SyntheticDataset
    if not _SETS:
        _SETS['data'] = SyntheticDataset(96, seg_len=128, n_speakers=102, seed=0)
    return _SETS['data']


def _trainer(dev, log_dir, seed, ema, iters=ITERS):
    """A fresh Trainer on a fresh loader at position 0, torch seeded with `seed` first."""
    from zs_amd.dataloader import DataLoader
    from zs_amd.trainer import Trainer
    hps = _hps(iters)
    torch.manual_seed(seed)
    return Trainer(hps, DataLoader(_data(), hps.batch_size), hps.g_mode, hps.enc_mode, log_dir=log_dir, dtype='bf16', device=dev, ema=ema)


def _train(tr, model_path, **kw):
    buf = io.StringIO()
    with redirect_stdout(buf):
        tr.train(model_path, 'train', mode='pretrain_AE', **kw)
    torch.cuda.synchronize()
    return buf.getvalue().replace('\r', '\n')


def _final(tr):
    out = {}
    for name, net in zip(NETS, tr.nets()):
        out['w.' + name] = net.flat_params()[0].clone()
    for name, o in (('enc', tr.ae.opt['enc']), ('dec', tr.ae.opt['dec']), ('clf', tr.clf.opt)):
        out['m.' + name], out['v.' + name], out['t.' + name] = o.m.clone(), o.v.clone(), o.t
        if o.ema is not None:
            out['ema.' + name] = o.ema.clone()
    out.update({'adam_step': tr.ae.adam_step, 'seed_dev': tr.ae._seed_dev.clone(), 'step_dev': tr.ae._step_dev.clone(),
                'loss.ae': tr.ae._loss.clone(), 'consumed': dict(tr._consumed)})
    return out


def _assert_same_final(fa, fb):
    assert set(fa) == set(fb)
    for k, a in fa.items():
        if isinstance(a, torch.Tensor):
            assert torch.equal(a, fb[k]), k
        else:
            assert a == fb[k], (k, a, fb[k])


def _assert_same_file(a, b):
    assert list(a) == list(b)
    for key in a:
        assert list(a[key]) == list(b[key]), key
        for k, v in a[key].items():
            assert v.dtype == b[key][k].dtype and torch.equal(v, b[key][k]), (key, k)


_A = {}


def _run_a(dev, tmp_path_factory):
    """The uninterrupted run with averages, once per session: resume=True from an empty directory (the asynchronous writer)."""
    if not _A:
        d = tmp_path_factory.mktemp('ema_A')
        tr = _trainer(dev, str(d / 'log'), 0, DECAY)
        out = _train(tr, str(d / 'ck' / 'model.pth'), resume=True)
        assert 'starting from iteration 0' in out
        _A.update(dir=d / 'ck', tr=tr, final=_final(tr))
    return _A


def test_checkpoint_carries_the_averages(dev, tmp_path_factory):
    from zs_amd import resume
    A = _run_a(dev, tmp_path_factory)
    tr = A['tr']
    ck = torch.load(str(A['dir'] / ('model.pth-ae-%d' % ITERS)), weights_only=True)
    assert list(ck) == list(NETS) + ['encoder_ema', 'decoder_ema', 'classifier_ema']           # the nets that have an optimizer now
    for key, opt in (('encoder', tr.ae.opt['enc']), ('decoder', tr.ae.opt['dec']), ('classifier', tr.clf.opt)):
        raw, avg = ck[key], ck[key + '_ema']
        assert list(raw) == list(avg), key
        offs, differs = opt.net._zs['offsets'], 0
        for k, v in raw.items():
            assert avg[k].dtype == v.dtype and avg[k].shape == v.shape, (key, k)
            assert avg[k].untyped_storage().nbytes() == v.numel() * v.element_size()               # a tensor of its own, not a view
            if k in offs:
                assert torch.equal(avg[k], opt.ema[offs[k]:offs[k] + v.numel()].view(v.shape).cpu()), (key, k)
                differs += int(not torch.equal(avg[k], v))
            else:                                                                                  # a buffer outside the flat storage
                assert torch.equal(avg[k], v), (key, k)
        if key == 'classifier':                                                                    # never stepped: the average is the weights
            assert differs == 0 and torch.equal(opt.ema, opt.net.flat_params()[0])
        else:
            assert differs > 0, key
    st = torch.load(resume.state_path(str(A['dir'] / ('model.pth-ae-%d' % ITERS))), weights_only=True)
    assert st['ema'] == DECAY
    for name in ('enc', 'dec'):
        assert set(st['steps']['ae'][name]) == {'m', 'v', 't', 'ema'}
        assert torch.equal(st['steps']['ae'][name]['ema'], tr.ae.opt[name].ema.cpu())
    # the synchronous writer gives the same file
    tr.save_model(str(A['dir'].parent / 'sync.pth'), 'ae', ITERS)
    tr.model_kept.pop()
    _assert_same_file(ck, torch.load(str(A['dir'].parent / ('sync.pth-ae-%d' % ITERS)), weights_only=True))


def test_without_the_average_the_files_are_as_ever(dev, tmp_path):
    from zs_amd import resume
    tr = _trainer(dev, str(tmp_path / 'log'), 0, None, iters=EVERY)
    _train(tr, str(tmp_path / 'r' / 'model.pth'), resume=True)
    os.makedirs(str(tmp_path / 'd'))
    tr2 = _trainer(dev, str(tmp_path / 'log2'), 0, None, iters=EVERY)
    _train(tr2, str(tmp_path / 'd' / 'model.pth'))
    for path in (str(tmp_path / 'r' / 'model.pth-ae-3'), str(tmp_path / 'd' / 'model.pth-ae-3')):
        assert list(torch.load(path, weights_only=True)) == list(NETS)
    st = torch.load(resume.state_path(str(tmp_path / 'r' / 'model.pth-ae-3')), weights_only=True)
    assert {'version', 'tag', 'iteration', 'target_guided', 'autolocker', 'world', 'batch_size', 'dtype', 'g_mode', 'enc_mode',
            'use_graph', 'flat_len', 'steps', 'consumed', 'rng', 'model_kept'} == set(st)
    assert all(set(st['steps']['ae'][n]) == {'m', 'v', 't'} for n in ('enc', 'dec'))
    # the averages change nothing the run computes: the weights of the run with them are these (three iterations of it)
    tr3 = _trainer(dev, str(tmp_path / 'log3'), 0, DECAY, iters=EVERY)
    os.makedirs(str(tmp_path / 'e'))
    _train(tr3, str(tmp_path / 'e' / 'model.pth'))
    A_ck = torch.load(str(tmp_path / 'e' / 'model.pth-ae-3'), weights_only=True)
    off = torch.load(str(tmp_path / 'd' / 'model.pth-ae-3'), weights_only=True)
    _assert_same_file({k: A_ck[k] for k in NETS}, off)
    # and use_ema on a file without averages is refused, naming the file
    from zs_amd.convert import get_trainer
    hp = str(tmp_path / 'hps.json')
    json.dump(_hps()._asdict(), open(hp, 'w'))
    path = str(tmp_path / 'd' / 'model.pth-ae-3')
    with pytest.raises(ValueError, match='model.pth-ae-3'):
        with redirect_stdout(io.StringIO()):
            get_trainer(hp, path, _hps().g_mode, _hps().enc_mode, use_ema=True)


def test_use_ema_loads_the_averages(dev, tmp_path, tmp_path_factory):
    from zs_amd.convert import get_trainer
    from zs_amd.trainer import Trainer
    A = _run_a(dev, tmp_path_factory)
    path = str(A['dir'] / ('model.pth-ae-%d' % ITERS))
    ck = torch.load(path, weights_only=True)
    hps = _hps()
    hp = str(tmp_path / 'hps.json')
    json.dump(hps._asdict(), open(hp, 'w'))
    said = {}
    trs = {}
    for use in (True, False):
        buf = io.StringIO()
        with redirect_stdout(buf):
            trs[use] = get_trainer(hp, path, hps.g_mode, hps.enc_mode, use_ema=use)
        said[use] = buf.getvalue()
    # the line of tags alone: the paths printed above it name temporary directories (which may hold any text)
    tags = {use: [l for l in said[use].split('\n') if l.startswith('[Trainer] - [')] for use in said}
    assert tags[True] == ['[Trainer] - [encoder_ema], [decoder_ema], [generator], Loaded!']      # the generator has no average in the file
    assert tags[False] == ['[Trainer] - [encoder], [decoder], [generator], Loaded!']
    for key, net in (('encoder', 'Encoder'), ('decoder', 'Decoder')):
        for k, v in getattr(trs[True], net).state_dict().items():
            assert torch.equal(v.cpu(), ck[key + '_ema'][k]), (key, k)
        for k, v in getattr(trs[False], net).state_dict().items():
            assert torch.equal(v.cpu(), ck[key][k]), (key, k)
    ref = Trainer(hps, None, hps.g_mode, hps.enc_mode, log_dir=str(tmp_path / 'log'), device=dev)
    ref.Encoder.load_state_dict(ck['encoder_ema'])
    ref.Decoder.load_state_dict(ck['decoder_ema'])
    g = torch.Generator().manual_seed(3)
    x, c = torch.rand(1, 128, 513, generator=g) * 0.98 + 1e-3, torch.tensor([1])        # [B, T, F]; T / 8 = 16 units
    U = torch.rand(1, 16, 8, 2, generator=g)
    outs = {k: t.test_step(x, c, enc_only=True, verbose=False, U=U) for k, t in (('ema', trs[True]), ('raw', trs[False]), ('ref', ref))}
    assert (outs['ema'][0] == outs['ref'][0]).all() and (outs['ema'][1] == outs['ref'][1]).all()
    assert (outs['ema'][0] != outs['raw'][0]).any()
    # a training run that starts from the averaged autoencoder: its own averages restart from the loaded weights
    tr = _trainer(dev, str(tmp_path / 'log2'), 7, 0.9)
    with redirect_stdout(io.StringIO()):
        tr.load_model(path, 'encoder, decoder', use_ema=True)
    for key, opt in (('encoder', tr.ae.opt['enc']), ('decoder', tr.ae.opt['dec'])):
        w = opt.net.flat_params()[0]
        assert torch.equal(opt.ema, w) and opt.ema.data_ptr() != w.data_ptr()
        assert all(torch.equal(v.cpu(), ck[key + '_ema'][k]) for k, v in opt.net.state_dict().items())


@pytest.mark.parametrize('writer', ['async', 'sync'])
def test_resumed_run_with_averages_equals_the_uninterrupted_run(dev, tmp_path, tmp_path_factory, writer):
    """Run A trains six iterations.  Run B is a fresh Trainer (other seed) on A's directory as it stood after iteration 3 ('async':
    written by the loop's writer thread) or on a directory a three-iteration run left through save_model + save_state ('sync'),
    and goes to six: weights, moments, averages, counters and the final `<net>_ema` entries are byte-equal."""
    from zs_amd import resume
    A = _run_a(dev, tmp_path_factory)
    names = ['model.pth-ae-%d' % it for it in (EVERY, ITERS)]
    dir_b = tmp_path / 'B'
    if writer == 'async':
        shutil.copytree(str(A['dir']), str(dir_b))
        os.remove(str(dir_b / names[1]))
        os.remove(str(dir_b / 'train_state' / (names[1] + '.pt')))
    else:
        dir_b.mkdir()
        tr3 = _trainer(dev, str(tmp_path / 'log3'), 0, DECAY, iters=EVERY)
        _train(tr3, str(dir_b / 'model.pth'))                                                  # save_model at iteration 3
        tr3.save_state(resume.state_path(str(dir_b / names[0])), tag='ae', iteration=EVERY)
        _assert_same_file(torch.load(str(dir_b / names[0]), weights_only=True), torch.load(str(A['dir'] / names[0]), weights_only=True))
        del tr3
    tr_b = _trainer(dev, str(tmp_path / 'logB'), 1234, DECAY)
    assert not torch.equal(tr_b.Encoder.flat_params()[0], A['tr'].Encoder.flat_params()[0])
    out_b = _train(tr_b, str(dir_b / 'model.pth'), resume=True)
    assert 'continuing at iteration 3 of 6' in out_b
    _assert_same_final(A['final'], _final(tr_b))
    assert not torch.equal(A['final']['ema.enc'], A['final']['w.encoder'])
    ck_a, ck_b = (torch.load(str(d / names[1]), weights_only=True) for d in (A['dir'], dir_b))
    assert 'encoder_ema' in ck_b and 'decoder_ema' in ck_b
    _assert_same_file(ck_a, ck_b)


def test_a_state_with_another_average_is_refused(dev, tmp_path, tmp_path_factory):
    A = _run_a(dev, tmp_path_factory)
    for ema, said in ((0.9, r'ema is 0\.5 in the file, 0\.9 in this run'), (None, r'ema is 0\.5 in the file, None in this run')):
        tr = _trainer(dev, str(tmp_path / ('log_%s' % ema)), 0, ema)
        w0 = tr.Encoder.flat_params()[0].clone()
        with pytest.raises(ValueError, match=said):
            _train(tr, str(A['dir'] / 'model.pth'), resume=True)
        assert torch.equal(w0, tr.Encoder.flat_params()[0]) and tr.ae.adam_step == 0               # refused before anything was loaded
    tr = _trainer(dev, str(tmp_path / 'log_off'), 0, None)
    with pytest.raises(ValueError, match='ema'):                                                   # the optimizer itself refuses too
        tr.ae.opt['enc'].load_state_dict(A['tr'].ae.opt['enc'].state_dict())
    with pytest.raises(ValueError, match='ema'):
        A['tr'].ae.opt['enc'].load_state_dict(tr.ae.opt['enc'].state_dict())


def test_stage_two_checkpoint_is_the_same_from_both_writers(dev, tmp_path):
    """A patchGAN run with averages to its first checkpoint, resume=True (test_gpu_resume.py's patchgan_tg case): a prefixed net
    has an average, and the averages of three nets lie outside this mode's state tree.  save_model writes the same file."""
    from zs_amd.dataloader import DataLoader, SyntheticDataset
    from zs_amd.trainer import Trainer
    hps = _hps(EVERY)
    torch.manual_seed(0)
    tr = Trainer(hps, None, hps.g_mode, hps.enc_mode, log_dir=str(tmp_path / 'log'), dtype='bf16', device=dev, ema=DECAY)
    tr.ae.use_graph = True
    tr.add_duo_loader(DataLoader(SyntheticDataset(96, seg_len=128, n_speakers=100, seed=1), hps.batch_size),
                      DataLoader(SyntheticDataset(96, seg_len=128, n_speakers=2, seed=2, speaker_offset=100), hps.batch_size))
    with redirect_stdout(io.StringIO()):
        tr.train(str(tmp_path / 'r' / 'model.pth'), 'train', mode='patchGAN', target_guided=True, resume=True)
    torch.cuda.synchronize()
    ck = torch.load(str(tmp_path / 'r' / ('model.pth-s2-%d' % EVERY)), weights_only=True)
    assert list(ck) == list(NETS) + ['encoder_ema', 'decoder_ema', 'generator_ema', 'classifier_ema', 'patch_discriminator_ema']
    assert ck['patch_discriminator_ema'] and all(k.startswith('module.') for k in ck['patch_discriminator_ema'])
    assert not any(k.startswith('module.') for k in ck['generator_ema'])
    tr.save_model(str(tmp_path / 'sync.pth'), 's2', EVERY)
    _assert_same_file(ck, torch.load(str(tmp_path / ('sync.pth-s2-%d' % EVERY)), weights_only=True))
