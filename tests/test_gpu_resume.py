"""Resumable training on the GPU: Trainer.train(resume=True), the train-state files and main.py --resume.

Every case is a six-iteration run on small nets with a checkpoint every three iterations.  Run A trains through; run B is a fresh
Trainer (other seed, so other initial weights and RNG) on a copy of A's directory as it stood after iteration 3.  B must run
iterations 4-6 only and end bit-equal to A: every flat parameter buffer, every Adam moment, every counter and the last loss.  A's
steps 4-6 are graph replays where the case captures; B's steps 4-5 are the eager warm-up steps and step 6 the first replay.

Bound for a case whose two fresh runs differ (test_fresh_runs_repeat prints the difference of every case): per tensor
max|a - b| / max|b| <= 4 x the largest such difference between two fresh runs, for at most two of the eight cases."""
import io
import json
import os
import shutil
import sys
from contextlib import redirect_stdout

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS, EVERY = 6, 3
# case -> (mode, target_guided, graphs, pooled)
CASES = {'ae_host_fed': ('pretrain_AE', False, True, False), 'ae_eager': ('pretrain_AE', False, False, False),
         'ae_pool_fed': ('pretrain_AE', False, True, True), 'patchgan_tg': ('patchGAN', True, True, False),
         'autolocker': ('autolocker', True, True, False), 't_classify': ('t_classify', False, True, False),
         'train_s1': ('train', False, True, False), 'pretrain_c': ('pretrain_C', False, True, False)}
TAG = {'pretrain_AE': 'ae', 'pretrain_C': 'c', 'train': 's1', 'patchGAN': 's2', 'autolocker': 's2', 't_classify': 'tclf'}


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


def _sets():
    """96 items per set: 23 positions per pass, more than any case takes in six iterations (18 at most)."""
    from zs_amd.dataloader import SyntheticDataset
    if not _SETS:
        _SETS.update(data=SyntheticDataset(96, seg_len=128, n_speakers=102, seed=0),
                     source=SyntheticDataset(96, seg_len=128, n_speakers=100, seed=1),
                     target=SyntheticDataset(96, seg_len=128, n_speakers=2, seed=2, speaker_offset=100))
    return _SETS


def _trainer(case, dev, log_dir, seed, iters=ITERS, **hps_kw):
    """A fresh Trainer for `case` on fresh loaders at position 0, torch seeded with `seed` first."""
    from zs_amd.dataloader import DataLoader
    from zs_amd.pool import DevicePool, PoolLoader
    from zs_amd.trainer import Trainer
    mode, _, graphs, pooled = CASES[case]
    hps, sets = _hps(iters, **hps_kw), _sets()
    duo = mode in ('patchGAN', 'autolocker')
    if pooled:
        pool = DevicePool([sets['data']], dev)
        mk = lambda s: PoolLoader(pool, s, hps.batch_size)
    else:
        mk = lambda s: DataLoader(s, hps.batch_size)
    torch.manual_seed(seed)
    tr = Trainer(hps, None if duo else mk(sets['data']), hps.g_mode, hps.enc_mode, log_dir=log_dir, dtype='bf16', device=dev)
    tr.ae.use_graph = graphs
    if duo:
        tr.add_duo_loader(mk(sets['source']), mk(sets['target']))
    return tr


def _train(tr, case, model_path, **kw):
    """tr.train for the case; returns what it printed."""
    mode, tg, _, _ = CASES[case]
    buf = io.StringIO()
    with redirect_stdout(buf):
        tr.train(model_path, 'train', mode=mode, target_guided=tg, **kw)
    torch.cuda.synchronize()
    return buf.getvalue().replace('\r', '\n')


def _opts(tr):
    o = {'ae.enc': tr.ae.opt['enc'], 'ae.dec': tr.ae.opt['dec'], 'clf': tr.clf.opt}
    if tr.s2 is not None:
        o.update({'s2.gen': tr.s2.gen_opt, 's2.patch': tr.s2.patch_opt})
    if tr.tclf is not None:
        o['tclf'] = tr.tclf.opt
    return o


def _final(tr):
    """Everything a run ends with, by name: tensors (cloned) and counters.  Uses no API newer than the training loop itself."""
    out = {}
    for name, net in zip(('enc', 'dec', 'gen', 'clf', 'D', 'tclf'), tr.nets()):
        out['w.' + name] = net.flat_params()[0].clone()
    for name, o in _opts(tr).items():
        out['m.' + name], out['v.' + name], out['t.' + name] = o.m.clone(), o.v.clone(), o.t
    out.update({'adam_step': tr.ae.adam_step, 'seed_dev': tr.ae._seed_dev.clone(), 'step_dev': tr.ae._step_dev.clone(),
                'loss.ae': tr.ae._loss.clone(), 'loss.clf': tr.clf.loss.clone(), 'correct.clf': tr.clf.correct.clone()})
    if tr.s2 is not None:
        out.update({'step_no': tr.s2.step_no, 'loss.s2_clf': tr.s2.loss_clf.clone(), 'loss.s2_rec': tr.s2.loss_rec.clone()})
        if hasattr(tr.s2, 'loss_reenc'):
            out['loss.reenc'] = tr.s2.loss_reenc.clone()
    if tr.tclf is not None:
        out.update({'loss.tclf': tr.tclf.loss.clone(), 'correct.tclf': tr.tclf.correct.clone()})
    out['consumed'] = dict(getattr(tr, '_consumed', {}))
    return out


def _rel_diff(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _spread(fa, fb):
    """Largest per-tensor max|a - b| / max|b| between two finals; 0.0 means bit-equal tensors and equal counters."""
    worst = 0.0
    for k, a in fa.items():
        b = fb[k]
        if isinstance(a, torch.Tensor):
            if not torch.equal(a, b):
                worst = max(worst, _rel_diff(a, b), 5e-324)
        else:
            assert a == b, (k, a, b)
    return worst


_PLAIN = {}


def _plain_runs(case, dev, tmp_path_factory):
    """Two fresh six-iteration runs of the case without resume (the code path of the parent commit), once per session."""
    if case not in _PLAIN:
        runs = []
        for i in range(2):
            d = tmp_path_factory.mktemp('plain_%s_%d' % (case, i))
            tr = _trainer(case, dev, str(d / 'log'), seed=0)
            _train(tr, case, str(d / 'model.pth'))
            runs.append(_final(tr))
            del tr
        _PLAIN[case] = runs
    return _PLAIN[case]


@pytest.mark.parametrize('case', list(CASES))
def test_fresh_runs_repeat(dev, tmp_path_factory, case):
    """The precondition of bit-exact resumption, on code the parent commit already has: two fresh runs are bit-equal."""
    a, b = _plain_runs(case, dev, tmp_path_factory)
    s = _spread(a, b)
    print('%s: largest relative difference between two fresh runs: %.3g' % (case, s))
    assert s == 0.0, (case, s)


_BOUNDED = set()


@pytest.mark.parametrize('case', list(CASES))
def test_resumed_run_equals_the_uninterrupted_run(dev, tmp_path, tmp_path_factory, case):
    mode = CASES[case][0]
    tag = TAG[mode]
    dir_a, dir_b = tmp_path / 'A', tmp_path / 'B'
    dir_a.mkdir()
    tr_a = _trainer(case, dev, str(tmp_path / 'logA'), seed=0)
    out_a = _train(tr_a, case, str(dir_a / 'model.pth'), resume=True)
    assert 'starting from iteration 0' in out_a
    fin_a = _final(tr_a)
    names = ['model.pth-%s-%d' % (tag, it) for it in (EVERY, ITERS)]
    assert sorted(os.listdir(str(dir_a))) == sorted(names + ['train_state'])              # max_to_keep 10 keeps both
    assert sorted(os.listdir(str(dir_a / 'train_state'))) == sorted(n + '.pt' for n in names)
    # A's directory as it stood after iteration 3
    shutil.copytree(str(dir_a), str(dir_b))
    os.remove(str(dir_b / names[1]))
    os.remove(str(dir_b / 'train_state' / (names[1] + '.pt')))
    tr_b = _trainer(case, dev, str(tmp_path / 'logB'), seed=1234)                         # other initial weights, other RNG
    assert not torch.equal(tr_b.Encoder.flat_params()[0], tr_a.Encoder.flat_params()[0])
    out_b = _train(tr_b, case, str(dir_b / 'model.pth'), resume=True)
    assert 'continuing at iteration 3 of 6' in out_b
    seen = sorted({int(l.split('[')[1].split('/')[0]) for l in out_b.split('\n') if '/%0*d]' % (5 if mode == 't_classify' else 6, ITERS) in l})
    assert seen == [4, 5, 6], (seen, out_b)
    fin_b = _final(tr_b)
    assert fin_b['consumed'] == fin_a['consumed'] and sum(fin_a['consumed'].values()) > 0
    # resume=True computes what the plain loop computes
    plain = _plain_runs(case, dev, tmp_path_factory)
    noise = _spread(plain[0], plain[1])
    fin_plain = dict(plain[0], consumed=fin_a['consumed'])
    if noise == 0.0:
        assert _spread(fin_a, fin_plain) == 0.0
        for k, a in fin_a.items():
            if isinstance(a, torch.Tensor):
                assert torch.equal(a, fin_b[k]), (case, k, _rel_diff(fin_b[k], a))
            else:
                assert a == fin_b[k], (case, k, a, fin_b[k])
    else:                                                                                 # the kernels of this case do not repeat
        _BOUNDED.add(case)
        assert len(_BOUNDED) <= 2, _BOUNDED
        for k, a in fin_a.items():
            if isinstance(a, torch.Tensor):
                d = _rel_diff(fin_b[k], a)
                print('%s %s: resumed against uninterrupted %.3g, fresh against fresh %.3g' % (case, k, d, noise))
                assert d <= 4.0 * noise, (case, k, d, noise)
            else:
                assert a == fin_b[k], (case, k)
    # B went on writing: iteration 6 with its state file, the window continued from the restored one
    assert sorted(os.listdir(str(dir_b))) == sorted(names + ['train_state'])
    st = torch.load(str(dir_b / 'train_state' / (names[1] + '.pt')), weights_only=True)
    assert st['iteration'] == ITERS and st['model_kept'] == names and st['tag'] == tag
    # a third start finds the final iteration and trains nothing
    tr_c = _trainer(case, dev, str(tmp_path / 'logC'), seed=5)
    out_c = _train(tr_c, case, str(dir_b / 'model.pth'), resume=True)
    assert 'is the final iteration' in out_c and '/%06d]' % ITERS not in out_c


def _expected_batch(name, k):
    """Batch k of the set as a fresh host loader serves it."""
    from zs_amd.dataloader import DataLoader
    dl = DataLoader(_sets()[name], 4)
    for _ in range(k):
        next(dl)
    c, x = next(dl)
    return c.long(), x.float()


@pytest.mark.parametrize('case', list(CASES))
def test_state_round_trip(dev, tmp_path, case):
    """Save at iteration 3, load into a fresh Trainer: moments, counts, counters, RNG states, batch counts and the next batch of
    every loader are exactly what was saved."""
    from zs_amd import resume
    mode, tg, _, _ = CASES[case]
    tag = TAG[mode]
    tr = _trainer(case, dev, str(tmp_path / 'log'), seed=0, iters=EVERY)
    _train(tr, case, str(tmp_path / 'model.pth'), resume=True)
    rng = torch.get_rng_state().clone(), torch.cuda.get_rng_state(dev).clone()
    ckpt = str(tmp_path / ('model.pth-%s-%d' % (tag, EVERY)))
    side = resume.state_path(ckpt)
    saved = torch.load(side, weights_only=True)
    assert saved['iteration'] == EVERY and saved['version'] == resume.FORMAT_VERSION
    for name, sd in saved['steps'].items():                                               # optimizer state and counters, no weights
        assert set(sd) <= {'enc', 'dec', 'clf', 'gen', 'patch', 'adam_step', 'seed_dev', 'step_dev', 'use_graph', 'step_no'}, (name, set(sd))
        assert all(set(v) == {'m', 'v', 't'} for v in sd.values() if isinstance(v, dict)), name
    tr2 = _trainer(case, dev, str(tmp_path / 'log2'), seed=77, iters=EVERY)
    if mode in ('patchGAN', 'autolocker'):
        tr2.stage2(autolocker=(mode == 'autolocker'))
    torch.rand(5, device=dev), torch.rand(5)                                              # move both generators off their seeded state
    tr2._load_all_nets(ckpt)
    st = tr2.load_state(side)
    assert st['iteration'] == EVERY
    fa, fb = _final(tr), _final(tr2)
    for k, a in fa.items():
        if k.startswith('loss.') or k.startswith('correct.'):
            continue                                                                      # results of a step, not state
        if isinstance(a, torch.Tensor):
            assert torch.equal(a, fb[k]), (case, k)
        else:
            assert a == fb[k], (case, k, a, fb[k])
    assert int(tr2.ae._step_dev.item()) == tr2.ae.adam_step
    assert torch.equal(torch.get_rng_state(), rng[0]) and torch.equal(torch.cuda.get_rng_state(dev), rng[1])
    assert torch.equal(saved['rng']['cpu'], rng[0]) and torch.equal(saved['rng']['cuda'], rng[1])
    used = {'patchGAN': ('source', 'target'), 'autolocker': ('source', 'target')}.get(mode, ('data',))
    assert all(tr2._consumed[n] > 0 for n in used) and tr2._consumed == saved['consumed']
    for name, loader in (('data', tr2.data_loader), ('source', tr2.source_loader), ('target', tr2.target_loader)):
        if loader is None:
            continue
        c, x = next(loader)[:2]
        ce, xe = _expected_batch(name, saved['consumed'][name])
        assert torch.equal(c.cpu().long(), ce) and torch.equal(x.cpu().float(), xe), (case, name)
    # the state saved by hand equals the one the loop wrote
    tr3 = _trainer(case, dev, str(tmp_path / 'log3'), seed=3, iters=EVERY)
    tr3._load_all_nets(ckpt)
    tr3.load_state(side)
    tr3.save_state(str(tmp_path / 'by_hand.pt'), tag=tag, iteration=EVERY, target_guided=tg)
    again = torch.load(str(tmp_path / 'by_hand.pt'), weights_only=True)

    def same(a, b, path):
        if isinstance(a, dict):
            assert set(a) == set(b), path
            for k in a:
                same(a[k], b[k], path + (k,))
        elif isinstance(a, torch.Tensor):
            assert torch.equal(a, b), path
        else:
            assert a == b, (path, a, b)
    same(saved, again, ())


def test_a_state_from_the_other_execution_path_is_refused(dev, tmp_path):
    from zs_amd import resume
    tr = _trainer('ae_host_fed', dev, str(tmp_path / 'log'), seed=0, iters=EVERY)
    _train(tr, 'ae_host_fed', str(tmp_path / 'model.pth'), resume=True)
    tr2 = _trainer('ae_eager', dev, str(tmp_path / 'log2'), seed=0)
    w0 = tr2.Encoder.flat_params()[0].clone()
    with pytest.raises(ValueError, match='use_graph'):
        _train(tr2, 'ae_eager', str(tmp_path / 'model.pth'), resume=True)
    assert torch.equal(w0, tr2.Encoder.flat_params()[0]) and tr2.ae.adam_step == 0        # refused before anything was loaded
    sd = tr.ae.state_dict()
    with pytest.raises(ValueError, match='use_graph'):
        tr2.ae.load_state_dict(sd)
    tr3 = _trainer('ae_host_fed', dev, str(tmp_path / 'log3'), seed=0, batch_size=2)
    with pytest.raises(ValueError, match='batch_size'):
        tr3.load_state(resume.state_path(str(tmp_path / 'model.pth-ae-3')))


@pytest.mark.parametrize('case', ['ae_host_fed', 'patchgan_tg'])
def test_snapshot_is_ordered_before_the_next_step(dev, tmp_path, monkeypatch, case):
    """The host runs ahead of the GPU (no logged iteration between the checkpoint and the end): the iteration-3 checkpoint of a
    six-iteration run (the captured autoencoder step; the eager stage-2 steps) holds the weights, and its state file the
    moments, a three-iteration run ends with.  A snapshot that raced the next step's Adam differs."""
    from zs_amd import resume
    monkeypatch.setenv('ZS_LOG_EVERY', '1000')
    tag = TAG[CASES[case][0]]
    six = _trainer(case, dev, str(tmp_path / 'log6'), seed=0)
    _train(six, case, str(tmp_path / 'six' / 'model.pth'), resume=True)
    three = _trainer(case, dev, str(tmp_path / 'log3'), seed=0, iters=EVERY)
    os.makedirs(str(tmp_path / 'three'))
    _train(three, case, str(tmp_path / 'three' / 'model.pth'))
    ckpt = str(tmp_path / 'six' / ('model.pth-%s-3' % tag))
    ck = torch.load(ckpt, weights_only=True)
    stepped = {'ae_host_fed': ('encoder', 'decoder'), 'patchgan_tg': ('generator', 'patch_discriminator')}[case]
    for key, n6, n3 in zip(resume.NET_NAMES, six.nets(), three.nets()):
        if key in stepped:
            assert not torch.equal(n6.flat_params()[0], n3.flat_params()[0]), key            # six went on training
        pre = 'module.' if key in ('patch_discriminator', 'target_classifier') else ''
        for k, v in n3.state_dict().items():
            assert torch.equal(ck[key][pre + k], v.cpu()), (key, k)
    st = torch.load(resume.state_path(ckpt), weights_only=True)
    if case == 'ae_host_fed':
        saved, opts = st['steps']['ae'], {'enc': three.ae.opt['enc'], 'dec': three.ae.opt['dec']}
        assert saved['adam_step'] == 3 and int(saved['step_dev']) == 3
        assert torch.equal(saved['seed_dev'], three.ae._seed_dev.cpu())
    else:
        saved, opts = st['steps']['s2'], {'gen': three.s2.gen_opt, 'patch': three.s2.patch_opt}
        assert saved['step_no'] == three.s2.step_no
    for name, o in opts.items():
        assert float(o.m.abs().max()) > 0
        assert torch.equal(saved[name]['m'], o.m.cpu()) and torch.equal(saved[name]['v'], o.v.cpu()), name
        assert saved[name]['t'] == o.t


def test_files_on_return_and_default_run_unchanged(dev, tmp_path):
    from zs_amd import resume
    tr = _trainer('ae_host_fed', dev, str(tmp_path / 'log'), seed=0)
    _train(tr, 'ae_host_fed', str(tmp_path / 'r' / 'model.pth'), resume=True)
    left = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path / 'r')) for f in fs]
    assert len(left) == 4 and not [f for f in left if f.endswith('.tmp')], left
    tr.save_model(str(tmp_path / 'sync.pth'), 'ae', ITERS)                                # the synchronous writer, as ever
    sync = torch.load(str(tmp_path / ('sync.pth-ae-%d' % ITERS)), weights_only=True)
    ck = torch.load(str(tmp_path / 'r' / ('model.pth-ae-%d' % ITERS)), weights_only=True)
    assert list(ck) == list(sync)
    for key in sync:
        assert list(ck[key]) == list(sync[key]), key
        for k, v in sync[key].items():
            assert ck[key][k].dtype == v.dtype and ck[key][k].shape == v.shape and torch.equal(ck[key][k], v), (key, k)
            assert ck[key][k].untyped_storage().nbytes() == v.numel() * v.element_size()  # a tensor of its own, not a view of the flat buffer
    st = torch.load(resume.state_path(str(tmp_path / 'r' / ('model.pth-ae-%d' % ITERS))), weights_only=True)
    assert {'version', 'tag', 'iteration', 'target_guided', 'autolocker', 'world', 'batch_size', 'dtype', 'g_mode', 'enc_mode',
            'use_graph', 'flat_len', 'steps', 'consumed', 'rng', 'model_kept'} == set(st)
    # the default run: same file names as ever, no state directory
    tr2 = _trainer('ae_host_fed', dev, str(tmp_path / 'log2'), seed=0)
    os.makedirs(str(tmp_path / 'd'))
    out = _train(tr2, 'ae_host_fed', str(tmp_path / 'd' / 'model.pth'))
    assert 'resume' not in out
    assert sorted(os.listdir(str(tmp_path / 'd'))) == ['model.pth-ae-3', 'model.pth-ae-6']
    assert tr2._writer is None and tr2._snap is None


def test_a_failing_writer_raises_from_train(dev, tmp_path):
    blocker = tmp_path / 'blocker'
    blocker.write_text('a file where the checkpoint directory should be')
    tr = _trainer('ae_host_fed', dev, str(tmp_path / 'log'), seed=0)
    with pytest.raises(OSError):
        _train(tr, 'ae_host_fed', str(blocker / 'model.pth'), resume=True)
    assert tr._writer._thread is None                                                     # nothing left running


def test_main_resume_end_to_end(dev, tmp_path, monkeypatch, capsys):
    """main.py --train_ae --synthetic --resume twice in one directory, the first run cut short by an hps file with fewer
    enc_pretrain_iters, against one uninterrupted run."""
    sys.path.insert(0, ROOT)
    import main
    monkeypatch.chdir(tmp_path)

    def hps_file(iters):
        p = str(tmp_path / ('hps_%d.json' % iters))
        json.dump(_hps(iters, n_speakers=4)._asdict(), open(p, 'w'))
        return p

    def run(ckpt_dir, iters, seed):
        torch.manual_seed(seed)
        main.main(['--train_ae', '--synthetic', '--resume', '--hps_path', hps_file(iters), '--ckpt_dir', str(tmp_path / ckpt_dir),
                   '--dtype', 'bf16'])
        return capsys.readouterr().out

    assert 'starting from iteration 0' in run('whole', ITERS, 0)
    assert 'starting from iteration 0' in run('cut', EVERY, 0)
    out = run('cut', ITERS, 99)
    assert 'continuing at iteration 3 of 6' in out and 'pre_AE:[000006/000006]' in out and 'pre_AE:[000003/' not in out
    from zs_amd import resume
    for d in ('whole', 'cut'):
        assert sorted(os.listdir(str(tmp_path / d))) == ['model.pth-ae-3', 'model.pth-ae-6', 'train_state']
    a, b = (torch.load(str(tmp_path / d / 'model.pth-ae-6'), weights_only=True) for d in ('whole', 'cut'))
    for key in a:
        for k in a[key]:
            assert torch.equal(a[key][k], b[key][k]), (key, k)
    sa, sb = (torch.load(resume.state_path(str(tmp_path / d / 'model.pth-ae-6')), weights_only=True) for d in ('whole', 'cut'))
    for name in ('enc', 'dec'):
        for k in ('m', 'v'):
            assert torch.equal(sa['steps']['ae'][name][k], sb['steps']['ae'][name][k]), (name, k)
    assert sa['steps']['ae']['adam_step'] == sb['steps']['ae']['adam_step'] == ITERS
    assert torch.equal(sa['steps']['ae']['seed_dev'], sb['steps']['ae']['seed_dev']) and sa['consumed'] == sb['consumed']
