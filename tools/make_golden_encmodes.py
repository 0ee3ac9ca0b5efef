"""Generate tests/golden/encmodes_small.npz by running the REFERENCE Encoder in its 'one_hot', 'binary' and 'continues'
modes (model/model.py:457-472), CPU only, with the helpers of oracle/make_golden.py.  Only data is written: per mode and
enc_size the reference's parameters, eval forwards (enc_act, enc) at several lengths with the uniform draw U captured by seed
replay, one pretrain_AE step per mode at dp = 0 (loss, every gradient, the clip norms, the parameter update of Adam), for
binary E = 6 one SpeakerClassifier forward + CE with the gradient on `enc` (classifier width E^2), and every state_dict's
key -> shape map.

Size.  Every reference module is built from a fixed seed and its initial parameters are rounded to 3 significant bits
(exact fp32 data for the reference and the kernels, a fraction of the bytes after compression); the inputs x are multiples of
1/16; eval forwards use one sample; every train step uses the same batch.  Parameters that equal another case's are stored
once ('enc.', 'dec0.'), the rest under the case's prefix.  Outputs the tests compare to a tolerance of their tensor's scale are
stored as fixed point per tensor (put_fixed): the train step's gradients and the classifier's gradient on enc with 11 bits,
an error of at most 4.9e-4 of the tensor's max |value| (the tests allow 2e-3); Adam's first update (at most lr in magnitude)
with 5 bits, an error of at most lr / 30 (the tests allow 0.1 lr).  Outputs compared bit for bit (enc, enc_act, U), the
losses and the clip norms are exact fp32.
The archive is written with fixed zip metadata, so a re-run reproduces it byte for byte.  Run:
    python tools/make_golden_encmodes.py
"""
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import make_golden as MG  # noqa: E402  (puts the reference on sys.path; helpers sd_np / sd_t / check)
from model.model import Decoder, Encoder, SpeakerClassifier  # noqa: E402  (the reference)

OUT = os.path.join(ROOT, 'tests', 'golden', 'encmodes_small.npz')
SHAPE = dict(c_in=80, c_h1=16, c_h2=32, c_h3=16, seg_len=128)
NS, TAU = 0.01, 0.1
CASES = [('one_hot', 6), ('one_hot', 96), ('binary', 6), ('binary', 16), ('continues', 8)]
TRAIN = [('one_hot', 96), ('binary', 6), ('continues', 8)]      # one pretrain_AE step per mode
LENGTHS = [24, 128, 201]
SEED_ENC, SEED_DEC = 500, 600
B_EVAL = 1
COND_TOL = 2e-4                   # fp32 vs fp64 reference gradients of a train step, of scale
GRAD_BITS, STEP_BITS = 11, 5      # fixed-point widths of the stored gradients and Adam updates (see above)


def t8(T):
    return (((T + 1) // 2 + 1) // 2 + 1) // 2


def noise_shape(mode, B, T4, E):
    return {'one_hot': (B, T4, E), 'binary': (B, T4, E, E)}.get(mode)


def restate(mode, enc, U, E):
    """enc [B, n_lin, T'] + U -> enc_act [B, E, T'] (gumbel_softmax with tau = 0.1, model/model.py:93-110)."""
    if mode == 'continues':
        return torch.nn.functional.leaky_relu(enc, negative_slope=NS)
    B, _, T4 = enc.shape
    lg = enc.permute(0, 2, 1)
    if mode == 'binary':
        lg = lg.reshape(B, T4, E, E)
    y = torch.softmax((lg + (-torch.log(-torch.log(U + 1e-20) + 1e-20))) / TAU, dim=-1)
    hard = torch.zeros_like(y).scatter_(-1, y.max(dim=-1)[1].unsqueeze(-1), 1.0)
    out = (hard - y).detach() + y
    if mode == 'binary':
        out = torch.clamp(out.sum(2), min=0, max=1)
    return out.permute(0, 2, 1)


def coarse(module, bits=3):
    """Round the module's parameters to `bits` significant bits (still exact fp32 data; a quarter of the bytes compressed)."""
    with torch.no_grad():
        for p in module.parameters():
            m, e = np.frexp(p.detach().double().numpy())
            p.copy_(torch.from_numpy(np.ldexp(np.rint(np.ldexp(m, bits)), e - bits)).float())
    return module


def x_input(*shape):
    """Spectrogram-like input in (0, 1): multiples of 1/16."""
    return torch.randint(1, 16, shape).float() / 16


def put_fixed(out, meta, key, named, bits):
    """A group of tensors (name -> array) as fixed point, one scale per tensor: value = q * step with
    |error| <= max|tensor| / (2 (2^(bits-1) - 1)).  The q of all tensors are concatenated in order into one array: bits <= 8,
    key@q8 = q (int8); otherwise key@q16 = the two bytes of q (int16, two's complement) as uint8 planes [2, n], high byte first
    (deflate compresses the planes apart better).  meta['fixed'][key] = [[name, shape, step], ...]; fixed_point() in the tests
    reads it back."""
    qs, table = [], []
    qmax = 2 ** (bits - 1) - 1
    for name, t in named:
        a = np.asarray(t, dtype=np.float64)
        step = float(np.abs(a).max()) / qmax
        q = (np.zeros(a.shape) if step == 0.0 else np.clip(np.rint(a / step), -qmax, qmax)).astype(np.int64)
        assert np.abs(q * step - a).max() <= 0.5 * step * (1 + 1e-9), (key, name)
        qs.append(q.ravel())
        table.append([name, list(a.shape), step])
    q = np.concatenate(qs)
    if bits <= 8:
        out[key + '@q8'] = q.astype(np.int8)
    else:
        u = (q & 0xffff).astype(np.uint16)
        out[key + '@q16'] = np.stack([(u >> 8).astype(np.uint8), (u & 0xff).astype(np.uint8)])
    meta.setdefault('fixed', {})[key] = table


def put_shared(out, shared, tag, sd):
    """Parameters equal to a stored shared one are not stored again; the first occurrence becomes the shared one."""
    for k, v in sd.items():
        if shared + k not in out:
            out[shared + k] = v
        elif not np.array_equal(out[shared + k], v):
            out[tag + k] = v


def make_enc(mode, E, dp):
    torch.manual_seed(SEED_ENC)
    return coarse(Encoder(ns=NS, dp=dp, enc_size=E, enc_mode=mode, **SHAPE))


def gen_eval(out, meta, mode, E, seed0, xs):
    """Every case is built from the same seed, so its layers up to the RNN equal the other cases' (stored once, 'enc.');
    the case stores its `linear` ('<mode>_<E>.enc.linear.*')."""
    tag = '%s_%d' % (mode, E)
    enc = make_enc(mode, E, 0.5).eval()
    put_shared(out, 'enc.', tag + '.enc.', MG.sd_np('', enc))
    meta['shapes'][tag] = {k: list(v.shape) for k, v in enc.state_dict().items()}
    B = B_EVAL
    for T in LENGTHS:
        x = xs[T]
        torch.manual_seed(seed0 + T)
        with torch.no_grad():
            act, logits = enc(x)
        shp = noise_shape(mode, B, t8(T), E)
        if shp is not None:
            torch.manual_seed(seed0 + T)
            U = torch.rand(shp)                                   # the forward's single torch.rand draw (model/model.py:96)
            out['%s.U.%d' % (tag, T)] = U.numpy()
        else:
            U = None
        assert torch.equal(restate(mode, logits, U, E), act), '%s T=%d: restatement != reference' % (tag, T)
        out['%s.enc_act.%d' % (tag, T)] = act.numpy()
        out['%s.enc.%d' % (tag, T)] = logits.numpy()
        print('  %s T=%d: enc %s, enc_act %s' % (tag, T, tuple(logits.shape), tuple(act.shape)))
    return enc


def fp64_grad_error(enc, dec, x, c, seed):
    """The step's gradients recomputed by the reference in fp64 (same parameters, batch and noise draw): {name: grad}, the
    decoder's names prefixed 'dec.'.  A fixture step must have fp32 gradients close to these (COND_TOL of scale): the tau = 0.1
    straight-through gradient can amplify fp32 rounding, and a draw where it does is no yardstick for the kernels."""
    import copy
    e64, d64 = copy.deepcopy(enc).double(), copy.deepcopy(dec).double()
    rand32 = torch.rand

    def rand(*a, requires_grad=False, **kw):                      # the same fp32 uniform draw, promoted
        return rand32(*a, dtype=torch.float32, **kw).double().requires_grad_(requires_grad)
    torch.manual_seed(seed)
    torch.set_default_dtype(torch.float64)                        # (the reference's GRU zero state follows the default)
    torch.rand = rand
    try:
        xin = x.double().requires_grad_(True)
        act, _ = e64(xin)
        loss = torch.mean(torch.abs(d64(act, c) - xin))
        loss.backward()
    finally:
        torch.rand = rand32
        torch.set_default_dtype(torch.float32)
    out = {k: p.grad.clone() for k, p in e64.named_parameters() if p.grad is not None}
    out.update({'dec.' + k: p.grad.clone() for k, p in d64.named_parameters() if p.grad is not None})
    return out, act.detach().float()


def gen_train(out_all, meta, mode, E, seed0, x, c):
    out = dict(out_all)                                           # merged back only if the draw is accepted
    """One pretrain_AE step (trainer.py:322-332) with dropout off, so U is the only draw."""
    tag = 'train_%s' % mode
    lr, max_norm, B, T, c_h, n_spk = 1e-4, 5.0, 3, 32, 32, 4
    enc = make_enc(mode, E, 0.0).train()                          # initial parameters: 'enc.' + '<tag>.enc0.' (its linear)
    put_shared(out, 'enc.', tag + '.enc0.', MG.sd_np('', enc))
    torch.manual_seed(SEED_DEC)
    dec = coarse(Decoder(c_in=E, c_out=SHAPE['c_in'], c_h=c_h, c_a=n_spk, ns=NS, seg_len=SHAPE['seg_len'])).train()
    put_shared(out, 'dec0.', tag + '.dec0.', MG.sd_np('', dec))
    p0 = {('enc', k): v.detach().clone() for k, v in enc.state_dict().items()}
    p0.update({('dec', k): v.detach().clone() for k, v in dec.state_dict().items()})
    opt = torch.optim.Adam(list(enc.parameters()) + list(dec.parameters()), lr=lr, betas=(0.5, 0.9))
    cond, act64 = fp64_grad_error(enc, dec, x, c, seed0 + 100)             # before the fp32 step below changes the parameters
    torch.manual_seed(seed0 + 100)
    xin = x.clone().requires_grad_(True)
    enc_act, _ = enc(xin)
    if mode != 'continues' and not torch.equal(act64, enc_act.detach()):
        return False                                              # a near-tie: the fp64 step discretised differently
    x_dec = dec(enc_act, c)
    loss = torch.mean(torch.abs(x_dec - xin))
    enc.zero_grad(); dec.zero_grad()
    loss.backward()
    for net, name in ((enc, 'genc'), (dec, 'gdec')):
        put_fixed(out, meta, '%s.%s' % (tag, name), [(k, p.grad.numpy() if p.grad is not None else np.zeros(p.shape, np.float32))
                                                    for k, p in net.named_parameters()], GRAD_BITS)
    worst = max((float((p.grad.double() - cond[k]).abs().max()) / max(float(cond[k].abs().max()), 1e-30), k)
                for k, p in list(enc.named_parameters()) + [('dec.' + k, p) for k, p in dec.named_parameters()]
                if p.grad is not None and float(cond[k].abs().max()) >= 1e-6)
    ne = torch.nn.utils.clip_grad_norm_(enc.parameters(), max_norm)
    nd = torch.nn.utils.clip_grad_norm_(dec.parameters(), max_norm)
    opt.step()
    for net, name in ((enc, 'enc'), (dec, 'dec')):
        steps = [(k, (v.double() - p0[(name, k)].double()).numpy()) for k, v in net.state_dict().items()]
        assert all(np.abs(st).max() <= lr * (1 + 1e-3) for _, st in steps), name
        put_fixed(out, meta, '%s.%s1_step' % (tag, name), steps, STEP_BITS)
    shp = noise_shape(mode, B, t8(T), E)
    if shp is not None:
        torch.manual_seed(seed0 + 100)
        out[tag + '.U'] = torch.rand(shp).numpy()
    out[tag + '.loss'] = np.float32(loss.item())
    out[tag + '.norm_enc'] = np.float32(ne.item()); out[tag + '.norm_dec'] = np.float32(nd.item())
    meta['train'][mode] = dict(enc_size=E, c_h=c_h, n_spk=n_spk, B=B, T=T, lr=lr, max_grad_norm=max_norm, seed=seed0)
    print('  %s E=%d: loss %.6f, |g_enc| %.5f, |g_dec| %.5f, fp32 vs fp64 gradients: worst %.2g of scale (%s)' %
          (tag, E, loss.item(), ne.item(), nd.item(), worst[0], worst[1]))
    if worst[0] > COND_TOL:
        return False
    out_all.update(out)
    return True


def gen_classifier(out, meta, enc_bin, seed0):
    """SpeakerClassifier on the binary encoder's pre-activation (c_in = E^2, trainer.py:78-80) + CE, gradient on enc."""
    E, T, B, n_class, c_h = enc_bin.enc_size, 128, 3, 4, 32
    torch.manual_seed(seed0)
    clf = coarse(SpeakerClassifier(c_in=E * E, c_h=c_h, n_class=n_class, dp=0.0, ns=NS, seg_len=SHAPE['seg_len'])).train()
    x = x_input(B, SHAPE['c_in'], T)
    y = torch.randint(0, n_class, (B,))
    with torch.no_grad():
        _, enc = enc_bin(x)
    enc = enc.clone().requires_grad_(True)
    logits = clf(enc)
    loss = torch.nn.CrossEntropyLoss()(logits, y)
    loss.backward()
    out.update(MG.sd_np('clf.', clf))
    put_fixed(out, meta, 'clf.denc', [('denc', enc.grad.numpy())], GRAD_BITS)
    out.update({'clf.y': y.numpy(), 'clf.enc': enc.detach().numpy(), 'clf.logits': logits.detach().numpy(),
                'clf.loss': np.float32(loss.item())})
    meta['clf'] = dict(c_in=E * E, c_h=c_h, n_class=n_class, enc_size=E, B=B, T=T)
    meta['shapes']['classifier_binary_6'] = {k: list(v.shape) for k, v in clf.state_dict().items()}
    print('  classifier c_in=%d: loss %.6f' % (E * E, loss.item()))


def write_npz(path, arrays):
    """np.savez_compressed layout, with fixed zip dates and key order (np.savez stamps the current time)."""
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue())


def main():
    torch.set_num_threads(1)
    out = {}
    meta = dict(SHAPE, ns=NS, tau=TAU, cases=[list(c) for c in CASES], lengths=LENGTHS, B=B_EVAL, shapes={}, train={})
    encs = {}
    print('[golden] eval forwards')
    torch.manual_seed(400)
    xs = {T: x_input(B_EVAL, SHAPE['c_in'], T) for T in LENGTHS}
    for T in LENGTHS:
        out['x.%d' % T] = xs[T].numpy()
    for i, (mode, E) in enumerate(CASES):
        encs[(mode, E)] = gen_eval(out, meta, mode, E, 500 + 10 * i, xs)
    print('[golden] pretrain_AE steps')
    torch.manual_seed(700)
    x, c = x_input(3, SHAPE['c_in'], 32), torch.randint(0, 4, (3,))            # the batch of every train step (B = 3, T = 32)
    out['train.x'], out['train.c'] = x.numpy(), c.numpy()
    for i, (mode, E) in enumerate(TRAIN):
        seed = 700 + 100 * i                                      # the first noise draw whose fp32 step is accurate (COND_TOL)
        while not gen_train(out, meta, mode, E, seed, x, c):
            seed += 1
    print('[golden] classifier on the binary encoding')
    gen_classifier(out, meta, encs[('binary', 6)], 900)
    out['meta'] = np.array(json.dumps(meta, sort_keys=True))
    write_npz(OUT, out)
    print('done ->', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
