"""Stage-2 autolocker mode (reference trainer.py:563-611) without a GPU: the fixture captured from the reference
(tests/golden/autolocker_small.npz, tools/make_golden_autolocker.py), the exact form of its BCE loss on hard units, a restatement
of the step with oracle/zs_oracle.py pieces under torch autograd pinned to the fixture (the yardstick of the GPU tests), and the
enc_mode check that runs before any device work."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import load_golden, sub_sd

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def fixed_point(d, m, key):
    """{name: fp64 tensor} of a fixed-point group of the fixture (q * step per tensor)."""
    if key + '@q8' in d:
        q = d[key + '@q8'].astype(np.int64)
    else:
        planes = d[key + '@q16'].astype(np.int64)
        q = ((planes[0] << 8) | planes[1]).astype(np.uint16).view(np.int16).astype(np.int64)
    out, o = {}, 0
    for name, shape, step in m['fixed'][key]:
        n = int(np.prod(shape)) if shape else 1
        out[name] = torch.from_numpy(q[o:o + n].reshape(shape) * step)
        o += n
    assert o == q.size
    return out


def al_restate(d, m, g_mode, gen_sd=None):
    """One autolocker iteration on oracle pieces: returns (x_gen, re_enc, enc_act, loss, dLoss/dx_gen, generator grads dict,
    clip norm, clipped grads dict).  fp32, CPU, the fixture's uniform draws."""
    import zs_oracle as O
    ns, sl, E = m['ns'], m['seg_len'], m['enc_size']
    enc_sd, dec_sd = sub_sd(d, 'enc.'), sub_sd(d, 'dec.')
    gsd = {k: v.clone().requires_grad_(True) for k, v in (gen_sd or sub_sd(d, 'gen.%s.' % g_mode)).items()}
    x_s = torch.from_numpy(d['xq_s']).float() / 16
    c_t = torch.from_numpy(d['c_t']).long()
    U1, U2 = torch.from_numpy(d[g_mode + '.U1']), torch.from_numpy(d[g_mode + '.U2'])
    enc_act, _ = O.encoder_forward(enc_sd, x_s, ns, 0.0, E, sl, U=U1, training=True)
    x_gen = O.gen_step(dec_sd, gsd, enc_act, c_t, m['n_speakers'] - m['n_target_speakers'], ns, sl, g_mode=g_mode)
    re_enc, _ = O.encoder_forward(enc_sd, x_gen, ns, 0.0, E, sl, U=U2, training=True)
    loss = torch.nn.functional.binary_cross_entropy(re_enc, enc_act.detach())
    names = list(gsd)
    gs = torch.autograd.grad(loss, [x_gen] + [gsd[k] for k in names])
    norm, clipped = O.clip_grad_norm(list(gs[1:]), m['max_grad_norm'])
    return (x_gen.detach(), re_enc.detach(), enc_act.detach(), loss.detach(), gs[0], dict(zip(names, gs[1:])), norm,
            dict(zip(names, clipped)))


def _fixture():
    return load_golden('autolocker_small.npz')


@pytest.mark.parametrize('g_mode', ['targeted_residual', 'targeted'])
def test_golden_loss_is_mismatch_count(g_mode):
    d, m = _fixture()
    re, act = d[g_mode + '.re_enc'], d[g_mode + '.enc_act']
    assert set(np.unique(re)) <= {0, 1} and set(np.unique(act)) <= {0, 1}
    N = re.size
    mism = int((re != act).sum())
    assert 0 < mism < N
    assert d[g_mode + '.loss'] == np.float32(100.0 * mism / N)


@pytest.mark.parametrize('g_mode', ['targeted_residual', 'targeted'])
def test_golden_reenc_gradient_is_pm_1e12_over_n(g_mode):
    d, m = _fixture()
    g, re, act = d[g_mode + '.dre_enc'], d[g_mode + '.re_enc'].astype(np.float32), d[g_mode + '.enc_act'].astype(np.float32)
    N = g.size
    want = np.float32(np.float32(1e12) * (re - act)) / np.float32(N)            # (x - y) / 1e-12 / N at the mismatches, else 0
    np.testing.assert_array_equal(np.abs(g), np.abs(want))
    np.testing.assert_array_equal(np.sign(g), np.sign(re - act))
    assert set(np.unique(np.abs(g))) == {0.0, np.float32(1e12 / N)}


@pytest.mark.parametrize('g_mode', ['targeted_residual', 'targeted'])
def test_oracle_restatement_matches_golden(g_mode):
    torch.set_num_threads(4)
    d, m = _fixture()
    x_gen, re_enc, enc_act, loss, dx, grads, norm, clipped = al_restate(d, m, g_mode)
    np.testing.assert_allclose(x_gen.numpy(), d[g_mode + '.x_gen'], atol=1e-5, rtol=0)
    np.testing.assert_array_equal(re_enc.numpy().astype(np.uint8), d[g_mode + '.re_enc'])
    np.testing.assert_array_equal(enc_act.numpy().astype(np.uint8), d[g_mode + '.enc_act'])
    assert loss.item() == float(d[g_mode + '.loss'])
    gdx = fixed_point(d, m, g_mode + '.dx_gen')['dx_gen']
    assert float((dx.double() - gdx).abs().max()) <= 2e-3 * float(gdx.abs().max())
    assert abs(float(norm) - float(d[g_mode + '.gnorm'])) <= 1e-3 * float(d[g_mode + '.gnorm'])
    gold = fixed_point(d, m, g_mode + '.gclip')
    assert set(gold) == set(clipped)
    for k, v in clipped.items():
        sc = float(gold[k].abs().max())
        assert float((v.double() - gold[k]).abs().max()) <= 5e-3 * sc + 1e-12, k        # fp32 sums of +-1e12 terms


def test_autolocker_needs_multilabel_binary():
    """Every other enc_mode is refused with ValueError before any device work (stub nets: no tensor is ever made)."""
    from zs_amd.stage2 import AutolockerStep
    from zs_amd.trainer import Trainer
    for mode in ('one_hot', 'binary', 'continues'):
        enc = types.SimpleNamespace(enc_mode=mode)
        with pytest.raises(ValueError, match='multilabel_binary'):
            AutolockerStep(enc, None, None, None, None, 'targeted_residual')
        tr = Trainer.__new__(Trainer)
        tr.s2, tr.hps, tr.g_mode, tr.enc_mode = None, types.SimpleNamespace(patch_iters=3), 'targeted_residual', mode
        tr.Encoder, tr.Decoder, tr.Generator, tr.PatchDiscriminator = enc, None, None, None
        with pytest.raises(ValueError, match='multilabel_binary'):
            tr.train('unused', mode='autolocker', target_guided=True)
        assert tr.s2 is None


def test_tacotron_mode_still_not_implemented():
    from zs_amd.trainer import Trainer
    tr = Trainer.__new__(Trainer)
    tr.hps = types.SimpleNamespace()
    with pytest.raises(NotImplementedError):
        tr.train('unused', mode='train_Tacotron')
