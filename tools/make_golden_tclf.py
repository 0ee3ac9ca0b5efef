"""Generate tests/golden/tclf_small.npz by running the REFERENCE TargetClassifier (model/model.py:176-228) and one step of its
t_classify loop (trainer.py:613-642), CPU only, with the helpers of oracle/make_golden.py.  Only data is written.

The classifier is TargetClassifier(n_class=3, ns=0.01, dp=0.8, seg_len=128).  Its 10.9 M parameters are regenerated from a seed
by oracle.synthetic_patch_sd(3, SEED) (the PatchDiscriminator's parameter set: the same keys, conv7 included), so the fixture holds:
  * eval logits of the reference for B_EVAL inputs (Dropout2d off);
  * one t_classify step on B_TRAIN segments: the raw speaker ids (below 100, 100 and 101), the relabelled targets
    (c[c < 100] = 102; c - shift_c with shift_c = 100), the six Dropout2d keep masks (make_golden's stand-in replaces drop1..drop6,
    so the masks are known), the train-mode logits and CE loss, the norm and a strided 512-entry sample of every parameter
    gradient (conv7 has none: the forward never uses it), the total norm that clip_grad_norm_(max_norm = 5) sees, and the norm and
    the same strided sample of Adam's first update (lr 1e-4, betas (0.5, 0.9)) of every parameter.
The archive is written with fixed zip metadata, so a re-run reproduces it byte for byte.  Run:
    python tools/make_golden_tclf.py
"""
import io
import json
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import make_golden as MG  # noqa: E402  (puts the reference on sys.path; helpers check / _MaskDrop)
import zs_oracle as O  # noqa: E402

sys.modules.setdefault('tensorboardX', types.SimpleNamespace(SummaryWriter=object))
from model.model import TargetClassifier  # noqa: E402  (the reference)
from utils import grad_clip  # noqa: E402  (the reference)

OUT = os.path.join(ROOT, 'tests', 'golden', 'tclf_small.npz')
NS, DP, SEG, N_CLASS, SEED = 0.01, 0.8, 128, 3, 13
N_SPEAKERS, N_TARGET = 102, 2
LR, BETAS, MAX_NORM = 1e-4, (0.5, 0.9), 5.0
B_EVAL, B_TRAIN = 3, 6
C_RAW = [5, 100, 101, 57, 101, 99]                  # below 100 ('None'), V001, V002
CHANS = [64, 128, 256, 512, 512, 32]


def x_input(*shape, generator):
    """Spectrogram-like inputs in (0, 1) on a 1/16 grid (exact data that compresses to a fraction of the bytes of U[0, 1))."""
    return (torch.floor(torch.rand(*shape, generator=generator) * 16) + 0.5) / 16


def sample(t):
    flat = t.reshape(-1)
    return flat[::max(1, flat.numel() // 512)][:512].numpy().copy()


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (reproducible bytes)."""
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def main():
    torch.set_num_threads(4)
    sd = O.synthetic_patch_sd(N_CLASS, seed=SEED, seg_len=SEG)
    T = TargetClassifier(n_class=N_CLASS, ns=NS, dp=DP, seg_len=SEG)
    T.load_state_dict(sd)
    g = torch.Generator().manual_seed(SEED)
    out = {}

    # ---- eval logits (trainer.py:231-235): the real Dropout2d modules, off in eval mode
    x_eval = x_input(B_EVAL, 513, SEG, generator=g)
    T.eval()
    with torch.no_grad():
        lg_eval = T(x_eval)
    _, o_eval = O.patch_discriminator_forward(sd, x_eval, NS, SEG, classify=True, dp=DP, training=False)
    MG.check('tclf eval logits', o_eval, lg_eval, 2e-5)
    out.update(x_eval=x_eval.numpy(), logits_eval=lg_eval.numpy())

    # ---- one t_classify step (trainer.py:615-628) with known keep masks
    drops = [MG._MaskDrop(DP) for _ in range(6)]
    for i, d in enumerate(drops):
        setattr(T, 'drop%d' % (i + 1), d)
    T.train()
    x = x_input(B_TRAIN, 513, SEG, generator=g)
    masks = [(torch.rand(B_TRAIN, ch, generator=g) >= DP).float() for ch in CHANS]
    for d, mk in zip(drops, masks):
        d.queue.append(mk)
    c = torch.tensor(C_RAW, dtype=torch.int64)
    cl = c.clone()
    cl[cl < 100] = 102
    y = cl - (N_SPEAKERS - N_TARGET)
    opt = torch.optim.Adam(T.parameters(), lr=LR, betas=BETAS)
    before = {k: p.detach().clone() for k, p in T.named_parameters()}
    logits = T(x)
    loss = torch.nn.CrossEntropyLoss()(logits, y)
    T.zero_grad()
    loss.backward()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in T.named_parameters()}
    norm = float(torch.sqrt(sum((gr.double() ** 2).sum() for gr in grads.values())))
    grad_clip([T], MAX_NORM)
    opt.step()
    _, o_lg = O.patch_discriminator_forward(sd, x, NS, SEG, classify=True, dp=DP, training=True, drop_masks=masks)
    MG.check('tclf train logits', o_lg, logits.detach(), 2e-5)
    out.update(x_train=x.numpy(), c_raw=c.numpy(), target=y.numpy(), logits_train=logits.detach().numpy(),
               loss=np.float32(loss.item()), clip_norm=np.float32(norm))
    for li, mk in enumerate(masks):
        out['mask.%d' % li] = mk.numpy().astype(np.uint8)
    for k, gr in grads.items():
        out['g.norm.' + k] = np.float32(gr.double().norm().item())
        out['g.sample.' + k] = sample(gr)
        upd = T.state_dict()[k].detach() - before[k]
        out['upd.norm.' + k] = np.float32(upd.double().norm().item())
        out['upd.sample.' + k] = sample(upd)
    out['meta'] = np.array(json.dumps(dict(ns=NS, dp=DP, seg_len=SEG, n_class=N_CLASS, seed=SEED, n_speakers=N_SPEAKERS,
                                            n_target_speakers=N_TARGET, lr=LR, betas=list(BETAS), max_grad_norm=MAX_NORM)))
    print('  loss %.6f  clip norm %.5f  eval logits %s' % (loss.item(), norm, lg_eval.numpy().round(4).tolist()))
    save_npz(OUT, out)
    print('  wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
