"""The host side of the weight averages (--ema / --use_ema): command line, train-state validation, the choice of the checkpoint
entry a net is loaded from, and the place of the two new ZsAdam fields.  No GPU."""
import copy
import ctypes
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _main():
    sys.path.insert(0, ROOT)
    import main
    return main


def test_parser_accepts_a_decay_in_range_and_refuses_the_rest(capsys):
    main = _main()
    p = main.build_parser()
    a = p.parse_args(['--train_ae', '--ema', '0.999'])
    assert a.ema == 0.999 and a.use_ema is False
    assert p.parse_args(['--train_ae', '--ema', '0']).ema == 0.0
    assert p.parse_args(['--train_ae']).ema is None
    for bad in ('1', '-0.1', 'x', 'nan', '1.5'):
        with pytest.raises(SystemExit):
            p.parse_args(['--train_ae', '--ema', bad])
        assert '--ema' in capsys.readouterr().err
    assert p.parse_args(['--test_single', '--use_ema']).use_ema is True
    assert p.parse_args(['--train_tgat', '--load_model', '--use_ema', '--ema', '0.999']).use_ema is True
    import zs_amd  # noqa: F401
    from zs_amd.hps import make_hps
    assert len(make_hps()._fields) == 32 and 'ema' not in make_hps()._fields     # a flag, not an hps key


def test_ema_needs_a_training_mode():
    main = _main()
    p = main.build_parser()
    for mode in main.TRAIN_MODES:
        main.check_ema(p.parse_args(['--' + mode, '--ema', '0.9']))
    main.check_ema(p.parse_args(['--test_single']))                              # no --ema: nothing to check
    for argv in (['--ema', '0.9'], ['--test_single', '--ema', '0.9'], ['--convert_dir', 'd', '--use_ema', '--ema', '0.9']):
        with pytest.raises(ValueError, match='--ema'):
            main.check_ema(p.parse_args(argv))
    for argv in (['--test_single', '--use_ema'], ['--cross_test', '--use_ema'], ['--convert_dir', 'd', '--use_ema'],
                 ['--train_tgat', '--load_model', '--use_ema', '--ema', '0.999'], ['--train_ae', '--test', '--use_ema']):
        main.check_ema(p.parse_args(argv))
    for argv in (['--use_ema'], ['--train_ae', '--use_ema'], ['--train_ae', '--use_ema', '--ema', '0.9'], ['--preprocess', '--use_ema']):
        with pytest.raises(ValueError, match='--use_ema'):                       # it would be ignored
            main.check_ema(p.parse_args(argv))
    with pytest.raises(ValueError, match='--ema'):                               # through the runner: before hps or anything is built
        main.argument_runner(['--test', '--ema', '0.5', '--hps_path', '/nonexistent/hps.json'])


def _stub_trainer(**over):
    net = lambda n: types.SimpleNamespace(flat_params=lambda n=n: (torch.zeros(n), torch.zeros(n)))
    kw = dict(hps=types.SimpleNamespace(batch_size=4), dtype='bf16', g_mode='targeted_residual', enc_mode='multilabel_binary',
              ae=types.SimpleNamespace(use_graph=True), nets=lambda: [net(8 * (i + 1)) for i in range(6)])
    kw.update(over)
    return types.SimpleNamespace(**kw)


def test_validate_compares_the_decay():
    import zs_amd  # noqa: F401
    from zs_amd import resume
    off = resume.describe(_stub_trainer(), 'ae', False, False)
    off_none = resume.describe(_stub_trainer(ema=None), 'ae', False, False)
    on = resume.describe(_stub_trainer(ema=0.5), 'ae', False, False)
    assert 'ema' not in off and 'ema' not in off_none and on['ema'] == 0.5     # recorded only when on
    assert set(on) - set(off) == {'ema'}
    assert resume.FORMAT_VERSION == 1 and 'ema' not in resume.FIELDS
    resume.validate(copy.deepcopy(off), off)                                     # a file without 'ema' for an off run
    resume.validate(copy.deepcopy(on), on)
    other = resume.describe(_stub_trainer(ema=0.9), 'ae', False, False)
    for state, expect, said in ((on, other, ('0.5', '0.9')), (on, off, ('0.5', 'None')), (off, on, ('None', '0.5'))):
        with pytest.raises(ValueError, match=r'train state: ema is %s in the file, %s in this run' % said):
            resume.validate(copy.deepcopy(state), expect)


def test_key_choice_prefers_the_average_and_falls_back_per_net():
    import zs_amd  # noqa: F401
    from zs_amd import resume
    keys = ['encoder', 'decoder', 'generator', 'classifier', 'patch_discriminator', 'target_classifier', 'encoder_ema', 'decoder_ema']
    got = resume.ema_keys(keys, resume.NET_NAMES, 'ck')
    assert got == {'encoder': 'encoder_ema', 'decoder': 'decoder_ema', 'generator': 'generator', 'classifier': 'classifier',
                   'patch_discriminator': 'patch_discriminator', 'target_classifier': 'target_classifier'}
    assert resume.ema_keys(keys + ['generator_ema'], ('generator', 'encoder'))['generator'] == 'generator_ema'
    assert resume.ema_keys(iter(keys), ('decoder',), 'ck') == {'decoder': 'decoder_ema'}
    with pytest.raises(ValueError, match='some/dir/model.pth-ae-3'):
        resume.ema_keys(keys[:6], resume.NET_NAMES, 'some/dir/model.pth-ae-3')


def test_netopt_refuses_a_decay_outside_the_range():
    import zs_amd  # noqa: F401
    from zs_amd.optim import check_ema
    assert check_ema(None) is None and check_ema(0) == 0.0 and check_ema('0.25') == 0.25
    for bad in (1.0, -0.1, float('nan'), 2):
        with pytest.raises(ValueError, match='ema'):
            check_ema(bad)


def test_zsadam_ends_with_the_average():
    """ema and ema_decay come after every earlier field, so a caller that zeroes the struct and fills the old fields has it off."""
    import zs_amd  # noqa: F401
    from zs_amd import _lib as L
    S = L.STRUCTS['ZsAdam']
    names = [f[0] for f in S._fields_]
    assert names[-2:] == ['ema', 'ema_decay'] and names[-3] == 'max_blocks'
    assert dict(S._fields_)['ema'] is ctypes.c_void_p and dict(S._fields_)['ema_decay'] is ctypes.c_float
    assert S.ema.offset >= S.max_blocks.offset + 4 and S.ema_decay.offset == S.ema.offset + 8
    z = S()
    assert z.ema is None and z.ema_decay == 0.0
