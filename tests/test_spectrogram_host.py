"""Stage-2 generator mode 'spectrogram' without a GPU: the Spectrogram_Patcher module (reference model/model.py:505-549), its
state_dict against the fixture captured from the reference (tests/golden/spectrogram_small.npz, tools/make_golden_spectrogram.py),
the fixture's layout, and a restatement of the patcher's forward pinned to the fixture's eval output (the GPU tests use the same
restatement in fp64 as the yardstick of the config-5-sized step)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def patcher_ref(sd, x, c, ns):
    """Spectrogram_Patcher.forward restated on torch ops (any dtype / device): x [B, c_in, T], c [B] -> [B, c_out, T]."""
    import zs_oracle as O
    lin = lambda h, n: O.linear_t(h, sd[n + '.weight'], sd[n + '.bias'])
    col = lambda e: e.unsqueeze(2)
    e1, e2 = sd['emb1.weight'][c], sd['emb2.weight'][c]
    out = lin(x, 'input_layer')
    for a, b in (('dense1', 'dense2'), ('dense3', 'dense4')):
        h = torch.nn.functional.leaky_relu(lin(out + col(e1), a), ns)
        h = torch.nn.functional.leaky_relu(lin(h + col(e1), b), ns)
        out = O.instance_norm(h) + out
    rnn = O.bigru(out + col(e2), sd, 'RNN.')
    cat = torch.cat([out, rnn, col(e2).expand(-1, -1, out.shape[2])], dim=1)
    h = torch.nn.functional.leaky_relu(lin(cat, 'dense5'), ns)
    return torch.sigmoid(lin(h, 'linear'))


def _fixture():
    return load_golden('spectrogram_small.npz')


def test_patcher_builds_with_reference_state_dict():
    from zs_amd.model import Spectrogram_Patcher
    d, m = _fixture()
    P = Spectrogram_Patcher(c_in=m['c_in'], c_h=m['c_h'], c_a=m['c_a'], ns=m['ns'], seg_len=m['seg_len'], dtype='fp32')
    assert P.c_a == m['c_a'] and P.c_in == 513 and P.c_out == 513
    shapes = {k: list(v.shape) for k, v in P.state_dict().items()}
    assert shapes == m['shapes']                                  # same keys, same shapes
    P.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in d.items() if k.startswith('P.')})
    assert not any('ins_norm' in k for k in shapes)               # InstanceNorm1d without affine: no parameters
    # the trainer's wiring (trainer.py:77-78) at the english hps
    from zs_amd.hps import make_hps
    hps = make_hps()
    Q = Spectrogram_Patcher(ns=hps.ns, c_in=513, c_h=hps.emb_size, c_a=hps.n_target_speakers, seg_len=hps.seg_len, dtype='fp32')
    assert tuple(Q.input_layer.weight.shape) == (hps.emb_size, 513) and tuple(Q.dense5.weight.shape) == (hps.emb_size, 3 * hps.emb_size)
    assert tuple(Q.RNN.weight_hh_l0.shape) == (3 * hps.emb_size // 2, hps.emb_size // 2)


def test_patcher_has_no_cpu_path():
    from zs_amd import _lib
    from zs_amd.model import Spectrogram_Patcher
    if torch.cuda.is_available():
        pytest.skip('has GPU')
    P = Spectrogram_Patcher(c_in=513, c_h=64, c_a=2, ns=0.01, dtype='fp32')
    with pytest.raises(_lib.ZsError, match='no CPU fallback'):
        P(torch.rand(1, 513, 8), torch.zeros(1, dtype=torch.int64))


def test_fixture_layout():
    d, m = _fixture()
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'spectrogram_small.npz')) < 1 << 20
    B, T, Te, F = m['B'], m['T'], m['T_eval'], m['c_in']
    assert m['shift'] == m['n_speakers'] - m['c_a'] and m['n_class'] == m['c_a']
    assert d['eval.xq'].shape == (B, F, Te) and d['eval.xq'].dtype == np.uint8 and d['eval.out'].shape == (B, 513, Te)
    for k in ('g.xdq', 'tg.xdq', 'tg.xtq'):
        assert d[k].shape == (B, F, T) and d[k].dtype == np.uint8 and d[k].min() >= 1 and d[k].max() <= 15
    c = d['g.c']
    assert c.shape == (B,) and c.min() >= m['shift'] and c.max() < m['shift'] + m['c_a']
    assert [d['g.mask.%d' % i].shape for i in range(6)] == [(B, ch) for ch in (64, 128, 256, 512, 512, 32)]
    for key in ('g.grad', 'g.step', 'tg.grad', 'tg.step'):
        assert sorted(t[0] for t in m['fixed'][key]) == sorted(m['shapes'])
        assert all(t[1] == m['shapes'][t[0]] for t in m['fixed'][key])
    for k in ('g.loss', 'g.loss_adv', 'g.loss_clf', 'g.norm', 'tg.loss'):
        assert d[k].dtype == np.float32 and np.isfinite(d[k])
    assert abs(float(d['g.loss']) - float(d['g.loss_adv']) - float(d['g.loss_clf'])) < 1e-6


def test_restatement_matches_fixture_eval_forward():
    d, m = _fixture()
    sd = {k[2:]: torch.from_numpy(v).double() for k, v in d.items() if k.startswith('P.')}
    x = torch.from_numpy(d['eval.xq']).double() / 16
    y = patcher_ref(sd, x, torch.from_numpy(d['eval.c']), m['ns'])
    err = (y - torch.from_numpy(d['eval.out']).double()).abs().max().item()
    assert err < 1e-5, err
