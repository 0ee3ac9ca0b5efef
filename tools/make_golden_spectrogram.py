"""Generate tests/golden/spectrogram_small.npz by running the REFERENCE Spectrogram_Patcher (model/model.py:505-549), the
stage-2 generator of g_mode 'spectrogram', with the reference's PatchDiscriminator, CPU only, with the helpers of
oracle/make_golden.py and tools/make_golden_encmodes.py.  Only data is written:
  - the patcher's initial parameters ('P.*') and its state_dict key -> shape map (meta['shapes']);
  - one eval forward of a batch ('eval.*');
  - one G step of --train_p (trainer.py:514-533): x_gen = x_dec + G(x_dec, c - shift), loss = beta_clf * CE(D_clf(x_gen), c - shift)
    - beta_gen * mean D(x_gen), clip_grad_norm(G, 5), Adam(lr, (0.5, 0.9)) -- the losses, the clip norm, every parameter gradient
    and the parameter update ('g.*');
  - the target-guided step that follows it (trainer.py:535-541): loss_rec = mean|x_dec + G(x_dec, c - shift) - x_t|, Adam without
    clipping, the same optimizer state ('tg.*').
x_dec stands for the decoder's output: the patcher sees nothing else, and the Encoder / Decoder get no gradient in these steps.

Size.  The patcher starts from parameters rounded to 3 significant bits and the spectrograms are multiples of 1/16 in (0, 1),
stored as uint8 sixteenths: exact fp32 data for both sides.  The 10.9 M discriminator weights are regenerated from a seed
(oracle/zs_oracle.py synthetic_patch_sd) and its Dropout2d keep masks are stored.  Gradients are per-tensor fixed point with 11
bits (at most 4.9e-4 of the tensor's max |value|) and Adam updates with 5 bits (1 / 30 of the tensor's largest update); losses and the eval forward are
exact fp32.  The archive is written with fixed zip metadata, so a re-run reproduces it byte for byte.  Run:
    python tools/make_golden_spectrogram.py
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import make_golden_encmodes as ME  # noqa: E402  (puts oracle/ and the reference on sys.path; coarse / put_fixed / write_npz)
import make_golden as MG  # noqa: E402
import zs_oracle as O  # noqa: E402

sys.modules.setdefault('tensorboardX', types.SimpleNamespace(SummaryWriter=object))
from model.model import PatchDiscriminator, Spectrogram_Patcher  # noqa: E402  (the reference)

OUT = os.path.join(ROOT, 'tests', 'golden', 'spectrogram_small.npz')
C_IN, C_H, C_A, N_SPK, SEG = 513, 64, 2, 4, 128
NS, DP, LR, MAX_NORM, BETAS = 0.01, 0.1, 1e-4, 5.0, (0.5, 0.9)
B, T, T_EVAL = 2, 128, 40
D_SEED = 7
GRAD_BITS, STEP_BITS = 11, 5


def sixteenths(g, *shape):
    """uint8 q in [1, 15]: the spectrogram q / 16."""
    return torch.randint(1, 16, shape, generator=g).to(torch.uint8)


def main():
    torch.set_num_threads(1)
    out, meta = {}, dict(c_in=C_IN, c_h=C_H, c_a=C_A, n_speakers=N_SPK, shift=N_SPK - C_A, seg_len=SEG, ns=NS, dp=DP, lr=LR,
                         max_grad_norm=MAX_NORM, betas=list(BETAS), B=B, T=T, T_eval=T_EVAL, d_seed=D_SEED, n_class=C_A,
                         beta_clf=1.0, beta_gen=1.0)
    torch.manual_seed(800)
    P = ME.coarse(Spectrogram_Patcher(c_in=C_IN, c_h=C_H, c_a=C_A, ns=NS, seg_len=SEG))
    out.update(MG.sd_np('P.', P))
    meta['shapes'] = {k: list(v.shape) for k, v in P.state_dict().items()}
    p0 = {k: v.detach().clone() for k, v in P.state_dict().items()}
    shift = N_SPK - C_A
    g = torch.Generator().manual_seed(801)

    # ---- eval forward (trainer.py:212-213 post-filters the decoded spectrogram with c - testing_shift_c) --------------------------
    xq = sixteenths(g, B, C_IN, T_EVAL)
    ce = torch.tensor([1, 0])
    P.eval()
    with torch.no_grad():
        y = P(xq.float() / 16, ce)
    out.update({'eval.xq': xq.numpy(), 'eval.c': ce.numpy(), 'eval.out': y.numpy()})
    print('[golden] eval forward', tuple(y.shape))

    # ---- one G step of --train_p -----------------------------------------------------------------------------------------------
    P.train()
    D = PatchDiscriminator(n_class=C_A, ns=NS, dp=DP, seg_len=SEG)
    D.load_state_dict(O.synthetic_patch_sd(C_A, seed=D_SEED))
    D.train()
    drops = [MG._MaskDrop(DP) for _ in range(6)]
    for i, d in enumerate(drops):
        setattr(D, 'drop%d' % (i + 1), d)
    xdq = sixteenths(g, B, C_IN, T)
    c_t = torch.tensor([shift + 1, shift + 0])                   # target speakers (absolute ids)
    masks = [(torch.rand(B, ch, generator=g) >= DP).float() for ch in (64, 128, 256, 512, 512, 32)]
    opt = torch.optim.Adam(P.parameters(), lr=LR, betas=BETAS)
    x_dec = xdq.float() / 16
    x_gen = x_dec + P(x_dec, c_t - shift)                         # trainer.py:283-284
    for d, m in zip(drops, masks):
        d.queue.append(m)
    D_f, f_logits = D(x_gen, classify=True)
    loss_adv = -torch.mean(D_f)
    loss_clf = torch.nn.CrossEntropyLoss()(f_logits, c_t - shift)
    loss = 1.0 * loss_clf + 1.0 * loss_adv
    P.zero_grad()
    loss.backward()
    ME.put_fixed(out, meta, 'g.grad', [(k, p.grad.numpy()) for k, p in P.named_parameters()], GRAD_BITS)
    norm = torch.nn.utils.clip_grad_norm_(P.parameters(), MAX_NORM)
    opt.step()
    p1 = {k: v.detach().clone() for k, v in P.state_dict().items()}
    steps = [(k, (p1[k].double() - p0[k].double()).numpy()) for k in p0]
    assert all(np.abs(s).max() <= LR * (1 + 1e-3) for _, s in steps)
    ME.put_fixed(out, meta, 'g.step', steps, STEP_BITS)
    out.update({'g.xdq': xdq.numpy(), 'g.c': c_t.numpy(), 'g.loss': np.float32(loss.item()), 'g.loss_adv': np.float32(loss_adv.item()),
                'g.loss_clf': np.float32(loss_clf.item()), 'g.norm': np.float32(norm.item())})
    for i, m in enumerate(masks):
        out['g.mask.%d' % i] = m.numpy().astype(np.uint8)
    print('[golden] G step: loss %.6f (adv %.6f, clf %.6f), |g| %.5f' % (loss.item(), loss_adv.item(), loss_clf.item(), norm.item()))

    # ---- the target-guided step that follows (trainer.py:535-541): the same Adam, no clipping -------------------------------------
    tdq = sixteenths(g, B, C_IN, T)
    xtq = sixteenths(g, B, C_IN, T)
    x_dec_tf, x_t = tdq.float() / 16, xtq.float() / 16
    loss_rec = torch.mean(torch.abs(x_dec_tf + P(x_dec_tf, c_t - shift) - x_t))
    P.zero_grad()
    loss_rec.backward()
    ME.put_fixed(out, meta, 'tg.grad', [(k, p.grad.numpy()) for k, p in P.named_parameters()], GRAD_BITS)
    opt.step()
    steps = [(k, (v.detach().double() - p1[k].double()).numpy()) for k, v in P.state_dict().items()]
    assert all(np.abs(s).max() <= 2 * LR for _, s in steps)                 # second Adam step: |m_hat / sqrt(v_hat)| < 2
    ME.put_fixed(out, meta, 'tg.step', steps, STEP_BITS)
    out.update({'tg.xdq': tdq.numpy(), 'tg.xtq': xtq.numpy(), 'tg.loss': np.float32(loss_rec.item())})
    print('[golden] target-guided step: loss_rec %.6f' % loss_rec.item())

    out['meta'] = np.array(json.dumps(meta, sort_keys=True))
    ME.write_npz(OUT, out)
    print('done ->', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
