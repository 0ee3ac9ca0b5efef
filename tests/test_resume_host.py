"""Host logic of resumable training (zs_amd.resume, DataLoader.skip, main.py --resume): no GPU.

DataLoader.skip(k) against k calls of next(); the search for the newest checkpoint that has a train-state file; validation of a
state file against the run that loads it (stub objects, no device); the command line's refusals; the rolling window of
max_to_keep continued from a restored model_kept."""
import copy
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Items(object):
    """n items (speaker i, a [2, 3] array filled with i): the batch served names the items it holds."""

    def __init__(self, n):
        self.n = n

    def __getitem__(self, i):
        assert 0 <= i < self.n, i
        return (np.int64(i), np.full((2, 3), float(i), dtype=np.float32))

    def __len__(self):
        return self.n


# (n items, batch size, world): one batch (index stays 0), a wrap in the middle of the skipped batches, two ranks
SKIP_CASES = [(4, 4, 1), (5, 4, 1), (8, 4, 1), (14, 2, 1), (15, 2, 1), (23, 3, 2), (12, 3, 2), (64, 4, 2)]


@pytest.mark.parametrize('n,B,world', SKIP_CASES)
def test_skip_equals_k_calls_of_next(n, B, world):
    import zs_amd  # noqa: F401
    from zs_amd.dataloader import DataLoader
    from zs_amd.pool import batch_items
    for rank in range(world):
        for k in (0, 1, 2, 3, 5, 7, 11, 40):
            a, b = DataLoader(_Items(n), B, rank=rank, world=world), DataLoader(_Items(n), B, rank=rank, world=world)
            for _ in range(k):
                next(a)
            b.skip(k)
            assert b.index == a.index, (k, rank, a.index, b.index)
            ca, xa = next(a)
            cb, xb = next(b)
            assert torch.equal(ca, cb) and torch.equal(xa, xb)
            assert ca.tolist() == batch_items(n, B, rank, world, k)            # the closed form the pool serves
            # from a position in the middle of a pass too
            b.skip(k)
            for _ in range(k):
                next(a)
            assert b.index == a.index
    one = DataLoader(_Items(4), 4)
    one.skip(9)
    assert one.index == 0
    with pytest.raises(ValueError):
        one.skip(-1)


def _touch(path, payload=None):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save(payload if payload is not None else {}, path)


def test_find_resumable_picks_the_newest_checkpoint_with_a_state_file(tmp_path):
    import zs_amd  # noqa: F401
    from zs_amd import resume
    d = str(tmp_path / 'ck')
    model_path = os.path.join(d, 'model.pth')
    assert resume.find_resumable(model_path, 'ae') is None                     # no directory at all: start from 0
    os.makedirs(d)
    assert resume.find_resumable(model_path, 'ae') is None                     # empty directory
    for it in (3, 6, 12):
        _touch('%s-ae-%d' % (model_path, it))
        _touch(resume.state_path('%s-ae-%d' % (model_path, it)))
    _touch(model_path + '-ae-15')                                              # no state file
    _touch(model_path + '-s2-99')                                              # another tag, with a state file
    _touch(resume.state_path(model_path + '-s2-99'))
    _touch(model_path + '-ae-18.tmp')                                          # a killed writer's leftovers
    _touch(resume.state_path(model_path + '-ae-18') + '.tmp')
    _touch(model_path + '-ae-21')
    _touch(resume.state_path(model_path + '-ae-21') + '.tmp')                  # checkpoint written, state file not yet
    _touch(os.path.join(d, 'other.pth-ae-30'))                                 # another model name
    _touch(resume.state_path(os.path.join(d, 'other.pth-ae-30')))
    ckpt, state, it = resume.find_resumable(model_path, 'ae')
    assert (ckpt, it) == (model_path + '-ae-12', 12)
    assert state == os.path.join(d, 'train_state', 'model.pth-ae-12.pt')
    assert resume.find_resumable(model_path, 's2')[2] == 99
    assert resume.find_resumable(model_path, 'tclf') is None
    # an existing test lists the checkpoint directory by prefix: state files must not show up there
    assert not [f for f in os.listdir(d) if f.startswith('model.pth-ae-') and f.endswith('.pt')]


def _stub_trainer(**over):
    net = lambda n: types.SimpleNamespace(flat_params=lambda n=n: (torch.zeros(n), torch.zeros(n)))
    kw = dict(hps=types.SimpleNamespace(batch_size=4), dtype='bf16', g_mode='targeted_residual', enc_mode='multilabel_binary',
              ae=types.SimpleNamespace(use_graph=True), nets=lambda: [net(8 * (i + 1)) for i in range(6)])
    kw.update(over)
    return types.SimpleNamespace(**kw)


def test_validate_names_the_field_that_differs():
    import zs_amd  # noqa: F401
    from zs_amd import resume
    expect = resume.describe(_stub_trainer(), 'ae', False, False)
    assert expect['version'] == resume.FORMAT_VERSION and expect['world'] == 1 and expect['flat_len']['decoder'] == 16
    resume.validate(copy.deepcopy(expect), expect)                             # an unaltered file passes
    for field, value in (('version', resume.FORMAT_VERSION + 1), ('tag', 's2'), ('world', 2), ('batch_size', 8), ('dtype', 'fp32'),
                         ('enc_mode', 'one_hot'), ('g_mode', 'naive'), ('use_graph', False), ('target_guided', True),
                         ('autolocker', True)):
        st = copy.deepcopy(expect)
        st[field] = value
        with pytest.raises(ValueError, match=field):
            resume.validate(st, expect)
        st = copy.deepcopy(expect)
        del st[field]
        with pytest.raises(ValueError, match=field):
            resume.validate(st, expect)
    st = copy.deepcopy(expect)
    st['flat_len']['generator'] += 4
    with pytest.raises(ValueError, match=r'flat_len\[generator\]'):
        resume.validate(st, expect)
    # the same through describe(): a run built otherwise refuses the file
    for over, field in ((dict(dtype='fp32'), 'dtype'), (dict(ae=types.SimpleNamespace(use_graph=False)), 'use_graph'),
                        (dict(hps=types.SimpleNamespace(batch_size=2)), 'batch_size')):
        with pytest.raises(ValueError, match=field):
            resume.validate(copy.deepcopy(expect), resume.describe(_stub_trainer(**over), 'ae', False, False))


def test_command_line_accepts_and_refuses_resume():
    sys.path.insert(0, ROOT)
    import main
    p = main.build_parser()
    for stage in ('--train_ae', '--train_p', '--train_tgat', '--train_c'):
        for extra in ([], ['--device_data']):
            args = p.parse_args(['--resume', stage] + extra)
            assert args.resume
            main.check_resume(args)
    assert not p.parse_args(['--train_ae']).resume
    main.check_resume(p.parse_args(['--train', '--load_model']))               # without --resume nothing is refused
    hps = ['--hps_path', os.path.join(ROOT, 'hps', 'zerospeech_english.json')]
    for argv, word in ((['--resume', '--train'], '--train'), (['--resume', '--train_ae', '--load_model'], '--load_model'),
                       (['--resume', '--train_ae', '--train_p'], 'exactly one'), (['--resume'], 'exactly one'),
                       (['--resume', '--test'], 'exactly one')):
        with pytest.raises(ValueError, match=word):
            main.check_resume(p.parse_args(argv))
        with pytest.raises(ValueError, match=word):                            # main() refuses before hps are read or anything is built
            main.main(argv + hps)


def test_restored_window_removes_the_right_checkpoint_and_its_state_file(tmp_path):
    import zs_amd  # noqa: F401
    from zs_amd import resume
    model_path = str(tmp_path / 'model.pth')
    paths = ['%s-ae-%d' % (model_path, it) for it in (3, 6, 9, 12)]
    for p in paths[:3]:
        _touch(p)
        _touch(resume.state_path(p))
    kept = list(paths[1:3])                                                    # what a state file written at iteration 9 recorded (max_keep 3)
    _touch(paths[3])
    _touch(resume.state_path(paths[3]))
    drop = resume.roll_window(kept, paths[3], 3)
    assert drop == [paths[1]] and kept == [paths[2], paths[3]]
    for p in drop:
        resume.remove_checkpoint(p)
    assert not os.path.exists(paths[1]) and not os.path.exists(resume.state_path(paths[1]))
    for p in (paths[0], paths[2], paths[3]):                                   # iteration 3 left the window before: not this save's to remove
        assert os.path.exists(p) and os.path.exists(resume.state_path(p))
    # a window that is not full removes nothing; a checkpoint without a state file is removed alone
    kept = []
    assert resume.roll_window(kept, paths[0], 3) == [] and kept == [paths[0]]
    os.remove(resume.state_path(paths[0]))
    resume.remove_checkpoint(paths[0])
    assert not os.path.exists(paths[0])


def test_save_model_continues_a_restored_window(tmp_path):
    """Trainer.save_model itself (tiny nets on the CPU: one parameter `w` each) on a restored model_kept."""
    import zs_amd  # noqa: F401
    from zs_amd import resume
    from zs_amd.model import ZsModule
    from zs_amd.trainer import Trainer

    class Net(ZsModule):
        def __init__(self):
            super(Net, self).__init__(dtype='fp32')
            self.w = torch.nn.Parameter(torch.ones(2))

    tr = Trainer.__new__(Trainer)
    tr.Encoder, tr.Decoder, tr.Generator, tr.SpeakerClassifier, tr.PatchDiscriminator, tr.TargetClassifier = (Net() for _ in range(6))
    model_path = str(tmp_path / 'model.pth')
    old = [model_path + '-ae-3', model_path + '-ae-6']
    for p in old:
        _touch(p)
        _touch(resume.state_path(p))
    tr.model_kept, tr.max_keep = list(old), 3
    tr.save_model(model_path, 'ae', 9)
    assert tr.model_kept == [old[1], model_path + '-ae-9']
    assert not os.path.exists(old[0]) and not os.path.exists(resume.state_path(old[0]))
    assert os.path.exists(old[1]) and os.path.exists(resume.state_path(old[1])) and os.path.exists(model_path + '-ae-9')
    ck = torch.load(model_path + '-ae-9', weights_only=True)
    assert set(ck) == {'encoder', 'decoder', 'generator', 'classifier', 'patch_discriminator', 'target_classifier'}
    assert set(ck['patch_discriminator']) == {'module.w'} and set(ck['encoder']) == {'w'}
