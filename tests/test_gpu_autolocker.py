"""Stage-2 autolocker mode (reference trainer.py:563-611) on the GPU: the encoder's input gradient (EncoderEngine.backward_input)
against oracle autograd, one AutolockerStep.al_step per g_mode against tests/golden/autolocker_small.npz (captured from the
reference by tools/make_golden_autolocker.py), a full-size step, and Trainer.train(mode='autolocker').

Tolerances.  Input gradient, fp32: 5e-3 of its scale, from enc_act (dbits, through the MBV backward) and from the pre-activation
enc (dlogits).  bf16: from enc only, by cosine and norm within BF16_DX, about 2x the error measured on the MI355X (the elementwise
error, 0.35-0.85 of scale, comes from a few entries: the InstanceNorm backwards over 4-16 rows cancel in bf16).  From enc_act the MBV
backward's weight y0 (1 - y0) / tau is largest at the units nearest a tie, and there a bf16 rounding of the logits moves it by its
own size (measured 0.43-0.97 of scale on random dbits): no bf16 yardstick exists for that product.
al step, fp32: the loss and both encodes' units exactly, the clipped generator gradient by cosine >= 0.999 and norm within 1e-2
(measured 0.999995 and 2e-5), Adam's update within 0.1 lr where the reference's clipped gradient is above 1e-3 of its tensor's scale
(elsewhere the sign of the first Adam update is rounding; measured 0.011 lr).
al step, bf16: the same product decides the direction of the gradient (the loss's gradient lives on the mismatched units, weighted
by y0 (1 - y0) / tau, so the few mismatches nearest a tie carry it) and a unit within bf16 rounding of a tie takes the other value
(measured: 121 mismatches against the reference's 126, clipped cosine -0.22 and 0.53).  So bf16 checks the mismatch count within
BF16_FLIPS, the loss = 100 * mismatches / N, a finite clipped gradient of norm max_grad_norm and Adam steps of at most lr."""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from conftest import load_golden, sub_sd

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

G_MODES = ('targeted_residual', 'targeted')
# bf16 input gradient from enc, per seg_len: (min cosine, max |norm ratio - 1|), about 2x the measured 1 - cosine and norm error
# (seg_len 128: cosine 0.944-0.963, norm ratio 1.05; seg_len 32, four rows per InstanceNorm in the last blocks: 0.779-0.825, 0.61-0.72)
BF16_DX = {128: (0.88, 0.12), 32: (0.55, 0.8)}
BF16_FLIPS = 12        # bf16 al step: |mismatches - reference mismatches| (of 256 units; measured 5)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def _cos(a, b):
    a, b = torch.as_tensor(a).double().cpu().reshape(-1), torch.as_tensor(b).double().cpu().reshape(-1)
    return float(a @ b) / max(float(a.norm() * b.norm()), 1e-300)


def _sync_all():
    torch.cuda.synchronize()


# ---- encoder input gradient ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('seg_len', [128, 32])
@pytest.mark.parametrize('c_in', [80, 513])
def test_encoder_input_gradient_vs_oracle(dev, c_in, seg_len, dtype):
    import zs_oracle as O
    from zs_amd.model import Encoder
    torch.manual_seed(c_in + seg_len)
    E, B, T, ns = 8, 2, seg_len, 0.01
    enc = Encoder(c_in=c_in, c_h1=16, c_h2=32, c_h3=16, ns=ns, dp=0.0, enc_size=E, seg_len=seg_len, enc_mode='multilabel_binary',
                  dtype=dtype).to(dev)
    enc.train()
    ee = enc._engine()
    x = torch.rand(B, T, c_in) * 0.98 + 1e-3
    T4 = (((T + 1) // 2 + 1) // 2 + 1) // 2
    G = O.gumbel_from_uniform(torch.rand(B, T4, E, 2))
    _, bits_f32, _ = ee.forward(x.to(dev).contiguous(), True, noise=G.to(dev).contiguous(), noise_kind=0, seed=3)
    db = torch.randn(B, T4, E).to(ee.ctx.tdt)
    dl = torch.randn(B, T4, 2 * E).to(ee.ctx.tdt)
    dbits = ee.ctx.act('test_dbits', B, T4, E)
    dbits.valid().copy_(db.to(dev))
    dlog = ee.ctx.act('test_dlog', B, T4, 2 * E)
    dlog.valid().copy_(dl.to(dev))
    flat, gflat = enc.flat_params()
    gflat.copy_(torch.randn_like(gflat))                     # any content: backward_input must leave it as it is
    g0, p0 = gflat.clone(), flat.clone()
    _sync_all()
    dx_b = ee.backward_input(dbits).clone() if dtype == 'fp32' else None
    dx = ee.backward_input(dlogits=dlog)
    _sync_all()
    assert dx.shape == (B, T, c_in) and dx.dtype == torch.float32 and dx.is_contiguous()
    assert torch.equal(gflat, g0) and torch.equal(flat, p0)
    sd = {k: v.detach().cpu() for k, v in enc.state_dict().items()}
    xr = x.permute(0, 2, 1).contiguous().requires_grad_(True)
    act, logits = O.encoder_forward(sd, xr, ns, 0.0, E, seg_len, G=G, training=True)
    if dtype == 'fp32':
        assert torch.equal(act.permute(0, 2, 1), bits_f32.cpu())
        ref_b, = torch.autograd.grad((act * db.float().permute(0, 2, 1)).sum(), xr, retain_graph=True)
        err_b = _rel(dx_b.cpu(), ref_b.permute(0, 2, 1))
        print('[dx] c_in %d seg_len %d %s from enc_act: max|d| / scale %.3g' % (c_in, seg_len, dtype, err_b))
        assert err_b <= 5e-3, err_b
    ref, = torch.autograd.grad((logits * dl.float().permute(0, 2, 1)).sum(), xr)
    err = _rel(dx.cpu(), ref.permute(0, 2, 1))
    cos, rn = _cos(dx.cpu(), ref.permute(0, 2, 1)), float(dx.double().norm().cpu() / ref.double().norm())
    print('[dx] c_in %d seg_len %d %s from enc: max|d| / scale %.3g, cos %.5f, norm ratio %.4f' % (c_in, seg_len, dtype, err, cos, rn))
    if dtype == 'fp32':
        assert err <= 5e-3, err
    else:
        assert cos >= BF16_DX[seg_len][0] and abs(rn - 1.0) <= BF16_DX[seg_len][1], (cos, rn)


# ---- one al step against the golden ---------------------------------------------------------------------------------------------
class _Hps(object):
    def __init__(self, m):
        self.max_grad_norm, self.lr, self.n_speakers, self.n_target_speakers = m['max_grad_norm'], m['lr'], m['n_speakers'], m['n_target_speakers']
        self.beta_dis = self.beta_clf = self.beta_gen = 1.0
        self.lambda_ = 10.0


def fixed_point(d, m, key):
    from test_autolocker_host import fixed_point as fp
    return fp(d, m, key)


def _al_nets(dev, d, m, g_mode, dtype):
    from zs_amd.model import Decoder, Encoder
    from zs_amd.patch import PatchDiscriminator
    kw = dict(ns=m['ns'], seg_len=m['seg_len'], dtype=dtype)
    enc = Encoder(c_in=m['c_in'], c_h1=m['c_h1'], c_h2=m['c_h2'], c_h3=m['c_h3'], dp=0.0, enc_size=m['enc_size'],
                  enc_mode='multilabel_binary', **kw).to(dev)
    dec = Decoder(c_in=m['enc_size'], c_out=m['c_in'], c_h=m['c_h'], c_a=m['n_speakers'], **kw).to(dev)
    gen = Decoder(c_in=m['enc_size'], c_out=m['c_in'], c_h=m['c_h'], c_a=m['n_target_speakers'],
                  output_mask=(g_mode == 'targeted_residual'), **kw).to(dev)
    enc.load_state_dict(sub_sd(d, 'enc.'))
    dec.load_state_dict(sub_sd(d, 'dec.'))
    gen.load_state_dict(sub_sd(d, 'gen.%s.' % g_mode))
    D = PatchDiscriminator(n_class=m['n_target_speakers'], ns=m['ns'], seg_len=m['seg_len'], dtype=dtype).to(dev)
    return enc, dec, gen, D


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('g_mode', G_MODES)
def test_al_step_golden(dev, g_mode, dtype):
    import zs_oracle as O
    from zs_amd.stage2 import AutolockerStep
    d, m = load_golden('autolocker_small.npz')
    enc, dec, gen, D = _al_nets(dev, d, m, g_mode, dtype)
    al = AutolockerStep(enc, dec, gen, D, _Hps(m), g_mode)
    btf = lambda k: (torch.from_numpy(d[k]).float() / 16).permute(0, 2, 1).contiguous().to(dev)
    x_s, x_t = btf('xq_s'), btf('xq_t')
    c_t = torch.from_numpy(d['c_t']).long().to(dev)
    G = {i: O.gumbel_from_uniform(torch.from_numpy(d['%s.U%d' % (g_mode, i)])).contiguous().to(dev) for i in (1, 2, 3)}
    frozen = {n: net.flat_params()[0].clone() for n, net in (('enc', enc), ('dec', dec), ('D', D))}
    enc_g = enc.flat_params()[1].clone()
    p0 = gen.flat_params()[0].clone()
    loss = al.al_step(x_s, c_t, update=False, noise=G[1], noise_kind=0, seed=5, noise2=G[2])
    _sync_all()
    lo = al.last
    enc_act, re_enc = lo['enc_act'].cpu().permute(0, 2, 1), lo['re_enc'].cpu().permute(0, 2, 1)
    N = re_enc.numel()
    ref_mism = int((d[g_mode + '.re_enc'] != d[g_mode + '.enc_act']).sum())
    mism = int((re_enc != enc_act).sum())
    assert abs(loss.item() - 100.0 * mism / N) <= 1e-5 * loss.item()              # the loss is the mismatch count, on any dtype
    # the clipped generator gradient
    names = [k for k, _ in gen.named_parameters()]
    gold = fixed_point(d, m, g_mode + '.gclip')
    g_now = {k: gen.grad_view(k).detach().double().cpu() for k in names}
    norm = float(torch.sqrt(sum((v ** 2).sum() for v in g_now.values())))
    coef = min(1.0, m['max_grad_norm'] / (norm + 1e-6))
    mine = torch.cat([g_now[k].reshape(-1) * coef for k in names])
    ref = torch.cat([gold[k].reshape(-1) for k in names])
    cos, rn = _cos(mine, ref), float(mine.norm() / ref.norm())
    print('[al] %s %s: loss %.6f (ref %.6f), mismatches %d (ref %d), |g| %.4g (ref %.4g), clipped cos %.6f, norm ratio %.6f' %
          (g_mode, dtype, loss.item(), float(d[g_mode + '.loss']), mism, ref_mism, norm, float(d[g_mode + '.gnorm']), cos, rn))
    assert np.isfinite(norm) and norm > 0
    if dtype == 'fp32':
        assert loss.item() == float(d[g_mode + '.loss'])
        np.testing.assert_array_equal(enc_act.numpy().astype(np.uint8), d[g_mode + '.enc_act'])
        np.testing.assert_array_equal(re_enc.numpy().astype(np.uint8), d[g_mode + '.re_enc'])
        assert _rel(lo['x_gen'].cpu().permute(0, 2, 1), torch.from_numpy(d[g_mode + '.x_gen'])) <= 1e-4
        assert _cos(lo['dx_gen'].cpu().permute(0, 2, 1), fixed_point(d, m, g_mode + '.dx_gen')['dx_gen']) >= 0.999
        assert cos >= 0.999 and abs(rn - 1.0) <= 1e-2
    else:
        assert abs(mism - ref_mism) <= BF16_FLIPS and abs(rn * float(ref.norm()) - m['max_grad_norm']) <= 1e-3 * m['max_grad_norm']
    # Adam's first update
    al.gen_opt.step(m['max_grad_norm'])
    _sync_all()
    upd = gen.flat_params()[0].double().cpu() - p0.double().cpu()
    lr = m['lr']
    gupd = fixed_point(d, m, g_mode + '.upd')
    o = 0
    worst = 0.0
    for k, p in gen.named_parameters():
        n = p.numel()
        u = upd[gen._zs['offsets'][k]:gen._zs['offsets'][k] + n].reshape(p.shape)
        assert torch.isfinite(u).all() and float(u.abs().max()) <= 1.01 * lr
        mask = gold[k].abs() > 1e-3 * float(gold[k].abs().max())
        if dtype == 'fp32' and mask.any():
            worst = max(worst, float((u - gupd[k])[mask].abs().max()))
        o += n
    print('[al] %s %s: Adam update max|d| / lr %.3g' % (g_mode, dtype, worst / lr))
    assert worst <= 0.1 * lr
    # nothing else moved: Encoder, Decoder, discriminator weights and the encoder's gradient buffer
    _sync_all()
    for n, net in (('enc', enc), ('dec', dec), ('D', D)):
        assert torch.equal(net.flat_params()[0], frozen[n]), n
    assert torch.equal(enc.flat_params()[1], enc_g)
    # the target-guided half: tg_step with the same optimizer, no clip
    p1 = gen.flat_params()[0].clone()
    tg = al.tg_step(x_t, c_t, noise=G[3], noise_kind=0, seed=6)
    _sync_all()
    assert abs(tg.item() - float(d[g_mode + '.tg_loss'])) <= (1e-4 if dtype == 'fp32' else 2e-2) * float(d[g_mode + '.tg_loss'])
    assert torch.isfinite(gen.flat_params()[0]).all() and not torch.equal(gen.flat_params()[0], p1)


# ---- full size -----------------------------------------------------------------------------------------------------------------
def test_al_step_full_size_bf16_finite(dev, tmp_path):
    """english hps with enc_size = emb_size = 1024, B = 128, bf16: one al step.  The loss's gradient is +-1e12 / N on the
    mismatched units; the clip norm's sum of squares must stay finite and the updated generator too."""
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    B = 128
    hps = make_hps(enc_size=1024, emb_size=1024, batch_size=B)
    tr = Trainer(hps, None, 'targeted_residual', hps.enc_mode, log_dir=str(tmp_path / 'log'), dtype='bf16', device=dev)
    s2 = tr.stage2(autolocker=True)
    g = torch.Generator().manual_seed(3)
    x_s = torch.rand(B, 128, 513, generator=g).to(dev)
    c_t = torch.randint(hps.n_speakers - hps.n_target_speakers, hps.n_speakers, (B,), generator=g).to(dev)
    p0 = tr.Generator.flat_params()[0].clone()
    e0 = tr.Encoder.flat_params()[0].clone()
    loss = s2.al_step(x_s, c_t, update=True, seed=11)
    _sync_all()
    sq = float(s2.gen_opt.sq.item())
    print('[al full] loss %.4f, |g|^2 %.4g' % (loss.item(), sq))
    assert np.isfinite(loss.item()) and 0.0 <= loss.item() <= 100.0
    assert np.isfinite(sq) and sq > 0
    p1 = tr.Generator.flat_params()[0]
    assert torch.isfinite(p1).all() and not torch.equal(p1, p0)
    assert torch.equal(tr.Encoder.flat_params()[0], e0)


# ---- the training loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('g_mode', ['targeted_residual', 'spectrogram', 'naive'])
def test_trainer_autolocker_loop_checkpoints(dev, tmp_path, monkeypatch, g_mode):
    from zs_amd.dataloader import DataLoader, SyntheticDataset
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    monkeypatch.setenv('ZS_CKPT_EVERY', '2')
    hps = make_hps(enc_size=8, emb_size=32, n_speakers=4, n_target_speakers=2, batch_size=2, patch_iters=3, max_to_keep=5)
    src = DataLoader(SyntheticDataset(16, seg_len=128, n_speakers=2, seed=1), 2)
    tgt = DataLoader(SyntheticDataset(16, seg_len=128, n_speakers=2, seed=2, speaker_offset=(0 if g_mode == 'naive' else 2)), 2)
    tr = Trainer(hps, None, g_mode, hps.enc_mode, log_dir=str(tmp_path / 'log'), dtype='fp32', device=dev)
    tr.add_duo_loader(src, tgt)
    before = {n: net.flat_params()[0].clone() for n, net in (('enc', tr.Encoder), ('dec', tr.Decoder), ('gen', tr.Generator),
                                                             ('D', tr.PatchDiscriminator))}
    buf = io.StringIO()
    with redirect_stdout(buf):
        tr.train(str(tmp_path / 'm.pth'), 'train', mode='autolocker', target_guided=True)
    txt = buf.getvalue()
    assert 'patch_G:[000003/000003], re_enc=' in txt and 'tg_rec=' in txt
    assert os.path.exists(str(tmp_path / 'm.pth-s2-2')) and not os.path.exists(str(tmp_path / 'm.pth-s2-3'))
    ck = torch.load(str(tmp_path / 'm.pth-s2-2'), map_location='cpu', weights_only=True)
    assert all(torch.isfinite(v).all() for v in ck['generator'].values())
    _sync_all()
    for n, net in (('enc', tr.Encoder), ('dec', tr.Decoder), ('D', tr.PatchDiscriminator)):
        assert torch.equal(net.flat_params()[0], before[n]), n
    assert not torch.equal(tr.Generator.flat_params()[0], before['gen'])
