"""The checkpoint file on the host (Trainer.save_model, _load_all_nets and load_model): no GPU.

Six tiny ZsModules on the CPU, of differing widths so that a swapped net is noticed: a Linear, a BatchNorm1d (its running
statistics and its int64 num_batches_tracked lie outside the flat parameter storage, between the flat entries) and a Conv1d.
Stand-in optimizers carry `.ema` for every net but target_classifier."""
import io
import types
from contextlib import redirect_stdout

import pytest
import torch

NETS = ('encoder', 'decoder', 'generator', 'classifier', 'patch_discriminator', 'target_classifier')
ATTRS = ('Encoder', 'Decoder', 'Generator', 'SpeakerClassifier', 'PatchDiscriminator', 'TargetClassifier')
WRAPPED = ('patch_discriminator', 'target_classifier')


def _tiny_nets(seed):
    import zs_amd  # noqa: F401
    from zs_amd.model import ZsModule

    class Tiny(ZsModule):
        def __init__(self, w):
            super(Tiny, self).__init__(dtype='fp32')
            self.a = torch.nn.Linear(w, 3)
            self.bn = torch.nn.BatchNorm1d(w)
            self.b = torch.nn.Conv1d(2, w, 3)
            self.flat_params()

    g = torch.Generator().manual_seed(seed)
    nets = [Tiny(3 + i) for i in range(6)]
    for i, net in enumerate(nets):
        flat = net.flat_params()[0]
        flat.copy_(torch.randn(flat.shape, generator=g))
        net.bn.running_mean.copy_(torch.randn(3 + i, generator=g))
        net.bn.num_batches_tracked.fill_(100 * seed + i)
    return nets


class _Opt(object):
    def __init__(self, net, g):
        self.ema = torch.randn(net.flat_params()[0].shape, generator=g)

    def reset_ema(self):
        pass


def _trainer(seed, ema=None):
    """A Trainer around six tiny nets, without its __init__ (which needs the GPU); ema: with the stand-in optimizers."""
    from zs_amd.trainer import Trainer
    tr = Trainer.__new__(Trainer)
    nets = _tiny_nets(seed)
    for attr, net in zip(ATTRS, nets):
        setattr(tr, attr, net)
    tr.model_kept, tr.max_keep, tr.ema, tr.s2, tr.tclf, tr.tclf_loaded = [], 10, ema, None, None, False
    if ema is not None:
        g = torch.Generator().manual_seed(seed + 1000)
        enc, dec, gen, clf, patch, _ = [_Opt(n, g) for n in nets]
        tr.ae = types.SimpleNamespace(opt={'enc': enc, 'dec': dec})
        tr.clf = types.SimpleNamespace(opt=clf)
        tr.s2 = types.SimpleNamespace(gen_opt=gen, patch_opt=patch)
    return tr


def _expected(tr):
    """The rule of the file, restated: state_dict() per net, `module.` on the two wrapped nets, then `<net>_ema` for every net
    with an average: opt.ema[offs[k]:offs[k] + numel] for an entry of the flat storage, the raw value for a buffer."""
    nets = dict(zip(NETS, tr.nets()))
    want = {}
    for key, net in nets.items():
        pre = 'module.' if key in WRAPPED else ''
        want[key] = {pre + k: v.detach().clone() for k, v in net.state_dict().items()}
    for key, opt in tr.ema_opts().items():
        pre = 'module.' if key in WRAPPED else ''
        offs = nets[key]._zs['offsets']
        want[key + '_ema'] = {pre + k: (opt.ema[offs[k]:offs[k] + v.numel()].view(v.shape) if k in offs else v).detach().clone()
                              for k, v in nets[key].state_dict().items()}
    return want


def _assert_file_is(got, want):
    assert list(got) == list(want)
    for key in want:
        assert list(got[key]) == list(want[key]), key
        for k, v in want[key].items():
            t = got[key][k]
            assert t.dtype == v.dtype and t.shape == v.shape and torch.equal(t, v), (key, k)
            assert t.untyped_storage().nbytes() == v.numel() * v.element_size(), (key, k)       # a tensor of its own, not a view


@pytest.fixture(scope='module')
def saved(tmp_path_factory):
    """(trainer with averages, the path save_model wrote, the file loaded), once; nobody changes them."""
    tr = _trainer(1, ema=0.5)
    model_path = str(tmp_path_factory.mktemp('ckpt') / 'model.pth')
    tr.save_model(model_path, 'ae', 7)
    assert tr.model_kept == [model_path + '-ae-7']
    return tr, model_path + '-ae-7', torch.load(model_path + '-ae-7', weights_only=True)


def test_save_model_writes_the_file_the_rule_describes(saved):
    tr, _, ck = saved
    want = _expected(tr)
    assert list(want) == list(NETS) + ['encoder_ema', 'decoder_ema', 'generator_ema', 'classifier_ema', 'patch_discriminator_ema']
    assert 'module.bn.num_batches_tracked' in want['patch_discriminator_ema'] and 'bn.running_mean' in want['encoder_ema']
    assert want['encoder']['bn.num_batches_tracked'].dtype == torch.int64
    assert not torch.equal(want['encoder']['a.weight'], want['encoder_ema']['a.weight'])
    _assert_file_is(ck, want)


def test_without_averages_the_file_has_the_six_nets(tmp_path):
    tr = _trainer(2)
    tr.save_model(str(tmp_path / 'model.pth'), 's2', 3)
    ck = torch.load(str(tmp_path / 'model.pth-s2-3'), weights_only=True)
    assert list(ck) == list(NETS)
    _assert_file_is(ck, _expected(tr))


def test_load_all_nets_restores_every_entry(saved):
    tr, path, ck = saved
    other = _trainer(3)
    assert not torch.equal(other.Encoder.a.weight, tr.Encoder.a.weight)
    other._load_all_nets(path)
    for key, net, src in zip(NETS, other.nets(), tr.nets()):
        got, want = net.state_dict(), src.state_dict()
        assert list(got) == list(want)
        for k, v in want.items():
            assert got[k].dtype == v.dtype and torch.equal(got[k], v), (key, k)
            if k in net._zs['offsets']:                                                  # it went into the flat storage the kernels read
                assert got[k].data_ptr() == net.flat_params()[0][net._zs['offsets'][k]:].data_ptr(), (key, k)


def test_load_model_takes_the_averages_where_the_file_has_them(saved):
    tr, path, ck = saved
    said = {}
    loaded = {}
    for use in (True, False):
        loaded[use] = _trainer(4)
        buf = io.StringIO()
        with redirect_stdout(buf):
            loaded[use].load_model(path, ', '.join(NETS), use_ema=use)
        said[use] = buf.getvalue().split('\n')
    assert said[False] == ['[Trainer] - load model from ' + path, '[Trainer] - ' + ''.join('[%s], ' % k for k in NETS) + 'Loaded!', '']
    assert said[True][1] == ('[Trainer] - [encoder_ema], [decoder_ema], [generator_ema], [classifier_ema], '
                             '[patch_discriminator_ema], [target_classifier], Loaded!')
    assert loaded[True].tclf_loaded and loaded[False].tclf_loaded
    for key, net_avg, net_raw in zip(NETS, loaded[True].nets(), loaded[False].nets()):
        pre = 'module.' if key in WRAPPED else ''
        entry = key + '_ema' if key != 'target_classifier' else key
        for k, v in net_avg.state_dict().items():
            assert torch.equal(v, ck[entry][pre + k]), (key, k)
        for k, v in net_raw.state_dict().items():
            assert torch.equal(v, ck[key][pre + k]), (key, k)
    # the target classifier of another file, a net the list leaves out, and an entry that does not fit: printed, not raised
    some = _trainer(5)
    w0 = some.Decoder.flat_params()[0].clone()
    broken = dict(ck, generator={'nothing': torch.zeros(1)})
    torch.save(broken, path + '.broken')
    buf = io.StringIO()
    with redirect_stdout(buf):
        some.load_model(path + '.broken', 'encoder, generator, target_classifier', clf_path=path)
    assert buf.getvalue().split('\n')[1] == '[Trainer] - [encoder], [generator - X] (RuntimeError), [target_classifier_another], Loaded!'
    assert torch.equal(some.Decoder.flat_params()[0], w0)
    assert torch.equal(some.TargetClassifier.a.weight, ck['target_classifier']['module.a.weight'])
