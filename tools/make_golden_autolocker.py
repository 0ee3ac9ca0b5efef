"""Generate tests/golden/autolocker_small.npz by running the REFERENCE Encoder / Decoder (model/model.py:284-489) as Encoder,
Decoder and Generator of the stage-2 autolocker mode, CPU only, and restating one iteration of trainer.py:563-611 with them:

    enc_act = Encoder(x_s);  x_gen = gen_step(enc_act, c_t);  re_enc = Encoder(x_gen);  loss = BCELoss(re_enc, enc_act.detach())
    backward;  clip_grad_norm(Generator, max_grad_norm);  Adam(lr, (0.5, 0.9)).step()
    target guided:  loss_rec = mean|gen_step(Encoder(x_t), c_t) - x_t|;  backward;  the same Adam, no clip.

Per g_mode ('targeted_residual', 'targeted'; prefix '<g_mode>.'): the uniform draws of the three encodes (captured by seed replay,
model/model.py:96), x_gen, re_enc, the loss, dLoss/dre_enc, dLoss/dx_gen, the generator's clipped gradients and its clip norm, Adam's
first update, and the target-guided loss and update.  enc_dp = 0 (no dropout draws).  Parameters are shared by both modes
('enc.', 'dec.'; the generators 'gen.<g_mode>.').

Size.  Reduced widths, seg_len 128, B = 2.  Parameters are rounded to 3 significant bits and spectrograms are multiples of 1/16
(exact fp32 data).  Gradients are stored as fixed point with 11 bits per tensor, Adam updates with 5 bits (see
make_golden_encmodes.put_fixed); x_gen, re_enc, the losses and dLoss/dre_enc are exact fp32.  The seeds are chosen so that every
unit of both encodes is decided by a margin of at least MIN_MARGIN in (logit + Gumbel) units: a restatement in fp32 takes the same
decisions.  Run:
    python tools/make_golden_autolocker.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import make_golden_encmodes as ME  # noqa: E402  (puts oracle/ and the reference on sys.path; coarse / put_fixed / write_npz)
import make_golden as MG  # noqa: E402
import zs_oracle as O  # noqa: E402

from model.model import Decoder, Encoder  # noqa: E402  (the reference)

OUT = os.path.join(ROOT, 'tests', 'golden', 'autolocker_small.npz')
SHAPE = dict(c_in=80, c_h1=16, c_h2=32, c_h3=16, seg_len=128)
E, C_H, N_SPK, N_TGT = 8, 32, 4, 2
NS, LR, MAX_NORM, BETAS = 0.01, 1e-4, 5.0, (0.5, 0.9)
B, T = 2, 128
G_MODES = ('targeted_residual', 'targeted')
MIN_MARGIN = 2e-3
GRAD_BITS, STEP_BITS = 11, 5


def margin(enc_logits, U):
    """min over units of |(l0 + g0) - (l1 + g1)|: how far every hard decision of the MBV is from a tie."""
    lg = enc_logits.permute(0, 2, 1).reshape(enc_logits.shape[0], enc_logits.shape[2], E, 2)
    a = lg + O.gumbel_from_uniform(U)
    return float((a[..., 0] - a[..., 1]).abs().min())


def encode(enc, x, seed):
    """Encoder(x) in train mode with its torch.rand draw replayed from `seed`: (enc_act, enc, U)."""
    torch.manual_seed(seed)
    act, logits = enc(x)
    torch.manual_seed(seed)
    U = torch.rand(x.size(0), logits.size(2), E, 2)
    return act, logits, U


def gen_step(dec, gen, g_mode, enc_act, c):
    """trainer.py:272-284."""
    shift = N_SPK - N_TGT
    x_dec = dec(enc_act, c)
    if g_mode == 'targeted':
        return x_dec + gen(enc_act, c - shift)
    return x_dec + x_dec * gen(enc_act, c - shift)


def one_mode(out, meta, g_mode, enc, dec, x_s, c_t, x_t, seed0):
    torch.manual_seed(700 + G_MODES.index(g_mode))
    gen = ME.coarse(Decoder(c_in=E, c_out=SHAPE['c_in'], c_h=C_H, c_a=N_TGT, ns=NS, seg_len=SHAPE['seg_len'],
                            output_mask=(g_mode == 'targeted_residual')))
    p0 = {k: v.detach().clone() for k, v in gen.state_dict().items()}
    out.update(MG.sd_np('gen.%s.' % g_mode, gen))
    opt = torch.optim.Adam(gen.parameters(), lr=LR, betas=BETAS)
    for s in range(seed0, seed0 + 1000, 3):
        for net in (enc, dec, gen):
            net.zero_grad()
        enc_act, enc1, U1 = encode(enc, x_s, s)
        x_gen = gen_step(dec, gen, g_mode, enc_act, c_t)
        x_gen.retain_grad()
        re_enc, enc2, U2 = encode(enc, x_gen, s + 1)
        re_enc.retain_grad()
        if min(margin(enc1.detach(), U1), margin(enc2.detach(), U2)) >= MIN_MARGIN:
            break
    else:
        raise RuntimeError('no seed with decisions %g away from a tie' % MIN_MARGIN)
    loss = torch.nn.BCELoss()(re_enc, enc_act.detach())
    loss.backward()
    N = re_enc.numel()
    mism = int((re_enc.detach() != enc_act.detach()).sum())
    assert float(loss) == np.float32(100.0 * mism / N), (float(loss), mism, N)
    assert set(np.unique(np.abs(re_enc.grad.numpy()))) <= {0.0, np.float32(1e12 / N)}, np.unique(re_enc.grad.numpy())
    gnorm = torch.nn.utils.clip_grad_norm_(gen.parameters(), MAX_NORM)          # the reference's grad_clip (utils.py:53-55)
    gclip = {k: p.grad.detach().clone() for k, p in gen.named_parameters()}
    opt.step()
    upd = {k: (p.detach() - p0[k]) for k, p in gen.named_parameters()}
    pfx = g_mode + '.'
    out.update({pfx + 'U1': U1.numpy(), pfx + 'U2': U2.numpy(), pfx + 'x_gen': x_gen.detach().numpy(),
                pfx + 're_enc': re_enc.detach().numpy().astype(np.uint8), pfx + 'enc_act': enc_act.detach().numpy().astype(np.uint8),
                pfx + 'loss': np.float32(loss.item()), pfx + 'dre_enc': re_enc.grad.numpy(), pfx + 'gnorm': np.float32(gnorm.item())})
    ME.put_fixed(out, meta, pfx + 'dx_gen', [('dx_gen', x_gen.grad.numpy())], GRAD_BITS)
    ME.put_fixed(out, meta, pfx + 'gclip', [(k, v.numpy()) for k, v in gclip.items()], GRAD_BITS)
    ME.put_fixed(out, meta, pfx + 'upd', [(k, v.numpy()) for k, v in upd.items()], STEP_BITS)
    print('[golden] %s: seed %d, %d / %d units flipped, loss %.6f, |g| %.4g' % (g_mode, s, mism, N, loss.item(), gnorm.item()))
    # ---- target guided (trainer.py:597-603): the same Adam, no clip
    p1 = {k: v.detach().clone() for k, v in gen.state_dict().items()}
    for net in (enc, dec, gen):
        net.zero_grad()
    enc_tf, _, U3 = encode(enc, x_t, s + 2)
    loss_rec = torch.mean(torch.abs(gen_step(dec, gen, g_mode, enc_tf, c_t) - x_t))
    loss_rec.backward()
    opt.step()
    out.update({pfx + 'U3': U3.numpy(), pfx + 'tg_loss': np.float32(loss_rec.item())})
    ME.put_fixed(out, meta, pfx + 'tg_upd', [(k, (p.detach() - p1[k]).numpy()) for k, p in gen.named_parameters()], STEP_BITS)
    meta['seed.' + g_mode] = s


def main():
    torch.set_num_threads(1)
    out, meta = {}, dict(SHAPE, enc_size=E, c_h=C_H, n_speakers=N_SPK, n_target_speakers=N_TGT, ns=NS, lr=LR, max_grad_norm=MAX_NORM,
                         betas=list(BETAS), B=B, T=T, enc_dp=0.0, g_modes=list(G_MODES))
    torch.manual_seed(500)
    enc = ME.coarse(Encoder(ns=NS, dp=0.0, enc_size=E, enc_mode='multilabel_binary', **SHAPE))
    torch.manual_seed(600)
    dec = ME.coarse(Decoder(c_in=E, c_out=SHAPE['c_in'], c_h=C_H, c_a=N_SPK, ns=NS, seg_len=SHAPE['seg_len']))
    enc.train(); dec.train()
    out.update(MG.sd_np('enc.', enc))
    out.update(MG.sd_np('dec.', dec))
    g = torch.Generator().manual_seed(801)
    xq_s = torch.randint(1, 16, (B, SHAPE['c_in'], T), generator=g).to(torch.uint8)
    xq_t = torch.randint(1, 16, (B, SHAPE['c_in'], T), generator=g).to(torch.uint8)
    c_t = torch.tensor([3, 2])
    out.update({'xq_s': xq_s.numpy(), 'xq_t': xq_t.numpy(), 'c_t': c_t.numpy()})
    for i, gm in enumerate(G_MODES):
        one_mode(out, meta, gm, enc, dec, xq_s.float() / 16, c_t, xq_t.float() / 16, 9000 + 100 * i)
    out['meta'] = np.array(json.dumps(meta, sort_keys=True))
    ME.write_npz(OUT, out)
    print('[golden] ->', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
