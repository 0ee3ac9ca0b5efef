"""enc_mode 'one_hot', 'binary' and 'continues' on the GPU: the discretiser kernels (zs_gumbel_st_fwd / _bwd), the Encoder module,
one train_ae step, graph capture, ragged inference and the Trainer surface, against tests/golden/encmodes_small.npz (captured
from the reference by tools/make_golden_encmodes.py).

Fixture layout (tools/make_golden_encmodes.py): parameters shared between cases are stored once ('enc.', 'dec0.'); the
train step's gradients and Adam updates and the classifier's gradient on enc are per-tensor fixed point (fixed_point() below),
within 4.9e-4 of the tensor's max |value| (gradients) and lr / 30 (updates) of the reference's fp32 values.

Bits: given the reference's logits and Gumbel noise the kernel's encoding is identical to the reference's; an element may only
differ where the argmax is a near-tie (the two largest (l + g) / tau of its group within 1e-5 relative), and every such element
is counted.  Module / train-step bounds are those of test_gpu_model.py (1e-3 of scale forward, 2e-3 of scale gradients)."""
import numpy as np
import pytest
import torch

from conftest import load_golden, sub_sd

pytestmark = pytest.mark.gpu

NS, TAU = 0.01, 0.1
CASES = [('one_hot', 6), ('one_hot', 96), ('binary', 6), ('binary', 16), ('continues', 8)]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def gold():
    return load_golden('encmodes_small.npz')


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


def _gumbel(U):
    return -torch.log(-torch.log(U + 1e-20) + 1e-20)


def _mode_id(mode):
    from zs_amd import _lib as L
    return {'one_hot': L.ZS_ENC_ONE_HOT, 'binary': L.ZS_ENC_BINARY, 'continues': L.ZS_ENC_CONTINUES}[mode]


def _n_lin(mode, E):
    return E * E if mode == 'binary' else E


def _groups(mode, s, E):
    """[rows, n_lin] -> [rows, groups, E]."""
    return s.reshape(s.shape[0], -1, E)


def _near_tie_rows(mode, a, E, rel=1e-5, abs_bound=0.0):
    """Rows [rows] in which some softmax group's two largest entries of a (any monotone image of (l + g)) are within
    rel * |largest| + abs_bound."""
    top = _groups(mode, a, E).topk(2, dim=-1).values
    gap = top[..., 0] - top[..., 1]
    return (gap <= rel * top[..., 0].abs() + abs_bound).any(dim=-1)


def _fwd(dev, mode, logits, E, G=None, dtype='fp32', seed=0):
    """zs_gumbel_st_fwd on fp32 logits [rows, n_lin] -> (bits_f32 [rows, E], y [rows, n_lin], s [rows, E])."""
    from zs_amd import _lib as L
    rows = logits.shape[0]
    lg = logits.contiguous().to(dev)
    Gd = G.reshape(rows, -1).contiguous().to(dev) if G is not None else None
    bits = torch.full((rows, E), -7.0, device=dev)
    y = torch.zeros(rows, _n_lin(mode, E), device=dev)
    s = torch.zeros(rows, E, device=dev)
    L.call('zs_gumbel_st_fwd', 'ZsGumbelStFwd', torch.cuda.current_stream().cuda_stream, dtype=L.ZS_F32, mode=_mode_id(mode),
           logits=L.ptr(lg), ld=lg.shape[1], logits_f32=1, noise=L.ptr(Gd), noise_kind=(0 if Gd is not None else 2), seed=seed,
           rows=rows, E=E, tau=TAU, slope=NS, bits_f32=L.ptr(bits), y=(L.ptr(y) if mode != 'continues' else None),
           s=(L.ptr(s) if mode == 'binary' else None))
    torch.cuda.synchronize()
    return bits.cpu(), y, s, lg


def _sd_eval(d, tag):
    sd = sub_sd(d, 'enc.')
    sd.update(sub_sd(d, tag + '.enc.'))
    return sd


def _encoder(m, mode, E, dtype, dev, sd, dp=0.5):
    from zs_amd.model import Encoder
    enc = Encoder(c_in=m['c_in'], c_h1=m['c_h1'], c_h2=m['c_h2'], c_h3=m['c_h3'], ns=NS, dp=dp, enc_size=E, seg_len=m['seg_len'],
                  enc_mode=mode, dtype=dtype).to(dev)
    enc.load_state_dict(sd)
    return enc


def _check_bits(mode, E, got, ref, s_ref, rel=1e-5, abs_bound=0.0):
    """got / ref [rows, E]; s_ref [rows, n_lin] = (l + g) in the reference's fp32.  Returns the number of excused elements."""
    if mode == 'continues':
        assert torch.equal(got, ref)
        return 0
    bad = (got != ref)
    if not bad.any():
        return 0
    tie = _near_tie_rows(mode, s_ref, E, rel, abs_bound)
    rows_bad = bad.any(dim=1)
    assert bool(tie[rows_bad].all()), 'encoding differs from the reference away from an argmax near-tie (%d rows)' % \
        int((rows_bad & ~tie).sum())
    return int(bad.sum())


# ---- 1. kernel forward on the reference's logits ----------------------------------------------------------------------------
@pytest.mark.parametrize('mode,E', CASES)
def test_kernel_bits_equal_reference(dev, gold, mode, E):
    d, m = gold
    tag = '%s_%d' % (mode, E)
    excused = total = 0
    for T in m['lengths']:
        enc = torch.from_numpy(d['%s.enc.%d' % (tag, T)])                                   # [B, n_lin, T']
        B, n_lin, T4 = enc.shape
        logits = enc.permute(0, 2, 1).reshape(B * T4, n_lin)
        ref = torch.from_numpy(d['%s.enc_act.%d' % (tag, T)]).permute(0, 2, 1).reshape(B * T4, E)
        G = _gumbel(torch.from_numpy(d['%s.U.%d' % (tag, T)])) if mode != 'continues' else None
        bits, _, _, _ = _fwd(dev, mode, logits, E, G)
        if mode == 'continues':
            assert torch.equal(bits, torch.nn.functional.leaky_relu(logits, NS))
        a = (logits + G.reshape(B * T4, n_lin)) / TAU if G is not None else None
        excused += _check_bits(mode, E, bits, ref, a)
        total += ref.numel()
    print('%s: %d/%d elements excused as argmax near-ties' % (tag, excused, total))


def test_kernel_bf16_bits_and_padding(dev, gold):
    """Compute-dtype output (bits, ld_bits, bits_fill_cols): bf16 encoding equals the fp32 one, the padding columns are zero."""
    from zs_amd import _lib as L
    d, m = gold
    for mode, E in (('one_hot', 96), ('binary', 6), ('continues', 8)):
        tag = '%s_%d' % (mode, E)
        enc = torch.from_numpy(d['%s.enc.%d' % (tag, 201)])
        B, n_lin, T4 = enc.shape
        logits = enc.permute(0, 2, 1).reshape(B * T4, n_lin).contiguous()
        G = _gumbel(torch.from_numpy(d['%s.U.%d' % (tag, 201)])) if mode != 'continues' else None
        f32, _, _, _ = _fwd(dev, mode, logits, E, G)
        ldb = ((E + 31) // 32) * 32 + 32
        out = torch.full((B * T4, ldb), 3.0, dtype=torch.bfloat16, device=dev)
        lg = logits.to(dev)
        Gd = G.reshape(B * T4, -1).contiguous().to(dev) if G is not None else None
        L.call('zs_gumbel_st_fwd', 'ZsGumbelStFwd', torch.cuda.current_stream().cuda_stream, dtype=L.ZS_BF16, mode=_mode_id(mode),
               logits=L.ptr(lg), ld=n_lin, logits_f32=1, noise=L.ptr(Gd), noise_kind=0, rows=B * T4, E=E, tau=TAU, slope=NS,
               bits=L.ptr(out), ld_bits=ldb, bits_fill_cols=ldb - 16)
        torch.cuda.synchronize()
        o = out.float().cpu()
        assert torch.equal(o[:, :E], f32.to(torch.bfloat16).float()), tag
        assert (o[:, E:ldb - 16] == 0).all() and (o[:, ldb - 16:] == 3.0).all(), tag


# ---- 2. kernel backward against fp64 autograd --------------------------------------------------------------------------------
def _restate64(mode, l, g, E):
    """fp64 restatement, l / g [rows, n_lin] -> enc [rows, E] (straight-through, model/model.py:93-110, 457-472)."""
    if mode == 'continues':
        return torch.nn.functional.leaky_relu(l, NS)
    y = torch.softmax(_groups(mode, l + g, E) / TAU, dim=-1)
    hard = torch.zeros_like(y).scatter_(-1, y.max(dim=-1)[1].unsqueeze(-1), 1.0)
    out = (hard - y).detach() + y
    return torch.clamp(out.sum(1), 0, 1) if mode == 'binary' else out[:, 0]


@pytest.mark.parametrize('mode,E', [('one_hot', 6), ('one_hot', 96), ('one_hot', 1024), ('binary', 6), ('binary', 16),
                                    ('binary', 64), ('continues', 8), ('continues', 1024)])
def test_kernel_backward_matches_fp64_autograd(dev, mode, E):
    from zs_amd import _lib as L
    gen = torch.Generator().manual_seed(E + 7)
    rows, n_lin = 37, _n_lin(mode, E)
    logits = torch.randn(rows, n_lin, generator=gen) * 0.5
    G = _gumbel(torch.rand(rows, n_lin, generator=gen)) if mode != 'continues' else None
    bits, y, s, lg = _fwd(dev, mode, logits, E, G)
    dout = torch.randn(rows, E, generator=gen)
    ld = ((n_lin + 31) // 32) * 32
    dl = torch.full((rows, ld), 5.0, device=dev)
    dd = dout.to(dev)
    yy, ld_y = (lg, n_lin) if mode == 'continues' else (y, n_lin)
    L.call('zs_gumbel_st_bwd', 'ZsGumbelStBwd', torch.cuda.current_stream().cuda_stream, dtype=L.ZS_F32, mode=_mode_id(mode),
           dbits=L.ptr(dd), ld_dbits=E, y=L.ptr(yy), ld_y=ld_y, s=(L.ptr(s) if mode == 'binary' else None), rows=rows, E=E, tau=TAU,
           slope=NS, dlogits=L.ptr(dl), ld=ld, fill_cols=ld)
    torch.cuda.synchronize()
    dl = dl.cpu()
    l64 = logits.double().requires_grad_(True)
    g64 = G.double() if G is not None else None
    out = _restate64(mode, l64, g64, E)
    if mode != 'continues':                                  # (leaky_relu's fp64 product rounds differently: no bit compare)
        assert torch.equal(out.float(), bits), 'forward of the fp64 restatement differs (tie in the random draw?)'
    out.backward(dout.double())
    ref = l64.grad
    scale = ref.abs().max().item()
    err = (dl[:, :n_lin].double() - ref).abs().max().item()
    print('%s E=%d: dlogits max|d| %.3g of scale %.3g' % (mode, E, err, scale))
    assert err <= 1e-5 * scale, (err, scale)
    assert (dl[:, n_lin:] == 0).all()


# ---- 3. module forward against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,E', CASES)
def test_module_forward_vs_reference(dev, gold, mode, E):
    d, m = gold
    tag = '%s_%d' % (mode, E)
    enc = _encoder(m, mode, E, 'fp32', dev, _sd_eval(d, tag)).eval()
    excused = 0
    for T in m['lengths']:
        x = torch.from_numpy(d['x.%d' % T]).to(dev)
        ref_enc = torch.from_numpy(d['%s.enc.%d' % (tag, T)])
        ref_act = torch.from_numpy(d['%s.enc_act.%d' % (tag, T)])
        U = torch.from_numpy(d['%s.U.%d' % (tag, T)]) if mode != 'continues' else None
        act, logits = enc(x, U=(U.to(dev) if U is not None else None))
        logits, act = logits.cpu(), act.cpu()
        assert logits.shape == ref_enc.shape and act.shape == ref_act.shape
        err = (logits - ref_enc).abs().max().item()
        assert err <= 1e-3 * ref_enc.abs().max().item(), (T, err)
        B, n_lin, T4 = ref_enc.shape
        if mode == 'continues':
            assert torch.equal(act, torch.nn.functional.leaky_relu(logits, NS))
            assert (act - ref_act).abs().max().item() <= 1e-3 * ref_act.abs().max().item()
            continue
        assert set(np.unique(act.numpy())) <= {0.0, 1.0}
        s_ref = ref_enc.permute(0, 2, 1).reshape(B * T4, n_lin) + _gumbel(U).reshape(B * T4, n_lin)
        bound = 4 * err + 1e-5 * s_ref.abs().max().item()           # end-to-end logit error + device log() in the noise
        excused += _check_bits(mode, E, act.permute(0, 2, 1).reshape(B * T4, E), ref_act.permute(0, 2, 1).reshape(B * T4, E),
                               s_ref, rel=0.0, abs_bound=bound)
    print('%s: %d elements excused as argmax near-ties' % (tag, excused))


# ---- 4. one train_ae step against the reference ------------------------------------------------------------------------------
def _grad_dict(net):
    return {k: net.grad_view(k).detach().cpu().clone() for k, _ in net.named_parameters()}


@pytest.mark.parametrize('mode', ['one_hot', 'binary', 'continues'])
def test_train_step_vs_reference(dev, gold, mode):
    from zs_amd.model import Decoder
    from zs_amd.trainer import AEStep
    d, m = gold
    tm = m['train'][mode]
    E, tag = tm['enc_size'], 'train_' + mode
    sd = sub_sd(d, 'enc.')
    sd.update(sub_sd(d, tag + '.enc0.'))
    enc = _encoder(m, mode, E, 'fp32', dev, sd, dp=0.0)
    dec = Decoder(c_in=E, c_out=m['c_in'], c_h=tm['c_h'], c_a=tm['n_spk'], ns=NS, seg_len=m['seg_len'], dtype='fp32').to(dev)
    dsd = sub_sd(d, 'dec0.')
    dsd.update(sub_sd(d, tag + '.dec0.'))
    dec.load_state_dict(dsd)
    p0 = {'enc': {k: v.detach().cpu().double().clone() for k, v in enc.state_dict().items()},
          'dec': {k: v.detach().cpu().double().clone() for k, v in dec.state_dict().items()}}
    ae = AEStep(enc, dec, lr=tm['lr'], max_grad_norm=tm['max_grad_norm'])
    x = torch.from_numpy(d['train.x']).permute(0, 2, 1).contiguous().to(dev)
    c = torch.from_numpy(d['train.c']).to(dev)
    G = _gumbel(torch.from_numpy(d[tag + '.U'])).contiguous().to(dev) if mode != 'continues' else None
    loss = ae.step(x, c, noise=G, noise_kind=0, update=False)
    torch.cuda.synchronize()
    assert abs(loss.item() - float(d[tag + '.loss'])) < 1e-5, (loss.item(), float(d[tag + '.loss']))
    worst = ('', 0.0)
    grefs = {'enc': fixed_point(d, m, tag + '.genc'), 'dec': fixed_point(d, m, tag + '.gdec')}
    for net, name in ((enc, 'enc'), (dec, 'dec')):
        assert set(grefs[name]) == set(k for k, _ in net.named_parameters())
        for k, g in _grad_dict(net).items():
            ref = grefs[name][k]
            scale = ref.abs().max().item()
            if scale < 1e-6:
                assert g.abs().max().item() < 1e-5, (k, g.abs().max().item())
                continue
            e = (g.double() - ref).abs().max().item() / scale
            worst = max(worst, (name + '.' + k, e), key=lambda t: t[1])
            assert e < 2e-3, 'grad %s.%s rel err %.3g' % (name, k, e)
    print('%s: worst grad rel err %s %.3g' % (mode, worst[0], worst[1]))
    sq = ae.grad_norms()
    torch.cuda.synchronize()
    for v, key in ((sq[0], '.norm_enc'), (sq[1], '.norm_dec')):
        ref = float(d[tag + key])
        assert abs(float(v.item()) ** 0.5 - ref) < 2e-3 * ref, (key, float(v.item()) ** 0.5, ref)
    ae.optimizer_step()
    torch.cuda.synchronize()
    lr = tm['lr']
    for net, name in ((enc, 'enc'), (dec, 'dec')):
        steps = fixed_point(d, m, '%s.%s1_step' % (tag, name))
        for k, p in net.state_dict().items():
            err = (p.detach().cpu().double() - (p0[name][k] + steps[k])).abs()
            sig = grefs[name][k].abs() > 1e-5
            assert err.max().item() <= 2.1 * lr, (k, err.max().item())
            if sig.any():
                assert err[sig].max().item() <= 0.1 * lr, (k, err[sig].max().item())
    assert not torch.equal(enc.state_dict()['linear.weight'].cpu().double(), p0['enc']['linear.weight'])


def test_speaker_classifier_on_binary_encoding(dev, gold):
    """SpeakerClassifier on the binary E = 6 encoder's pre-activation (c_in = E^2 = 36, trainer.py:78-80): logits, CE and the
    gradient on enc against the reference."""
    from zs_amd import _lib as L
    from zs_amd.model import SpeakerClassifier
    d, m = gold
    cm = m['clf']
    clf = SpeakerClassifier(c_in=cm['c_in'], c_h=cm['c_h'], n_class=cm['n_class'], dp=0.0, ns=NS, seg_len=m['seg_len'],
                            dtype='fp32').to(dev)
    keys = m['shapes']['classifier_binary_6']
    clf.load_state_dict({k: torch.from_numpy(d['clf.' + k]) for k in keys})
    clf.train()
    enc = torch.from_numpy(d['clf.enc'])                                               # [B, 36, 16]
    eng = clf._engine()
    out = eng.forward(clf.input_act(enc.permute(0, 2, 1).contiguous().to(dev)), True)
    B = enc.shape[0]
    ref_logits = torch.from_numpy(d['clf.logits'])
    assert (out.valid()[:, 0, :].cpu() - ref_logits).abs().max().item() <= 1e-3 * ref_logits.abs().max().item()
    y = torch.from_numpy(d['clf.y']).to(dev)
    loss, corr = torch.zeros(1, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    dl = torch.zeros(B, out.ld, device=dev)
    L.call('zs_softmax_ce', 'ZsSoftmaxCE', torch.cuda.current_stream().cuda_stream, logits=out.ptr(), ld=out.ld, target=L.ptr(y), B=B,
           n_class=cm['n_class'], loss_out=L.ptr(loss), dlogits=L.ptr(dl), ldg=out.ld, grad_scale=1.0, correct_out=L.ptr(corr))
    dx = eng.backward(dl, out.ld, need_dx=True, param_grads=False)
    torch.cuda.synchronize()
    assert abs(loss.item() - float(d['clf.loss'])) < 1e-5
    ref = fixed_point(d, m, 'clf.denc')['denc']
    got = dx.valid().permute(0, 2, 1).cpu().double()
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() <= 2e-3 * ref.abs().max().item()


# ---- 5. graph capture ---------------------------------------------------------------------------------------------------------
def test_one_hot_graph_replay_equals_eager(dev):
    """bf16 one_hot train_ae: the captured step (device seed through seed_ptr) replays bit for bit like the same launches issued
    eagerly, and the noise changes between steps."""
    from zs_amd.model import Decoder, Encoder
    from zs_amd.trainer import AEStep
    res = []
    for graph_warmup in (2, 10 ** 9):
        torch.manual_seed(0)
        enc = Encoder(c_in=80, c_h1=16, c_h2=64, c_h3=32, ns=0.01, dp=0.5, enc_size=96, seg_len=128, enc_mode='one_hot',
                      dtype='bf16').to(dev)
        dec = Decoder(c_in=96, c_out=80, c_h=64, c_a=4, ns=0.01, seg_len=128, dtype='bf16').to(dev)
        ae = AEStep(enc, dec, lr=1e-3, max_grad_norm=5.0, use_graph=True)
        ae.graph_warmup = graph_warmup
        g = torch.Generator().manual_seed(1)
        losses = []
        for i in range(6):
            x = torch.rand(4, 128, 80, generator=g).to(dev)
            c = torch.randint(0, 4, (4,), generator=g).to(dev)
            losses.append(ae.step(x, c).item())
        res.append((losses, enc.flat_params()[0].clone(), dec.flat_params()[0].clone(), len(ae._graphs)))
    (la, ea, da, na), (lb, eb, db, nb) = res
    assert na == 1 and nb == 0
    assert la == lb, (la, lb)
    assert torch.equal(ea, eb) and torch.equal(da, db)
    assert len(set(la)) == len(la)


# ---- 6. ragged inference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['one_hot', 'binary'])
def test_encode_batch_equals_fragment_by_fragment(dev, tmp_path, mode):
    from zs_amd import convert as cv
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    torch.manual_seed(5)
    E = 16
    hps = make_hps(enc_size=E, emb_size=32, n_speakers=4, n_target_speakers=2)
    tr = Trainer(hps, None, 'targeted_residual', mode, log_dir=str(tmp_path / 'log'), dtype='fp32', device=dev)
    rng = np.random.RandomState(11)
    lens = [int(n) for n in rng.randint(30, 701, size=20)]
    specs = [np.clip(rng.rand(n, 513).astype(np.float32), 1e-8, 1) for n in lens]
    tail = (E,) if mode == 'one_hot' else (E, E)
    base = _gumbel(torch.rand((64,) + tail, generator=torch.Generator().manual_seed(1234))).to(dev)

    def noise_fn(n, t, e):                 # every batch position reads the same field, so a fragment's noise is base[:T']
        assert e == E and t <= base.shape[0]
        return base[:t].unsqueeze(0).expand((n, t) + tail).contiguous()

    encs, _ = cv.encode_batch(specs, tr, 128, noise_fn=noise_fn, max_batch=8)
    checked = 0
    for u, spec in enumerate(specs):
        frags = cv.fragments(len(spec), 128) if len(spec) > 128 else [(0, len(spec))]
        o8 = 0
        for a, b in frags:
            tp = (((b - a + 1) // 2 + 1) // 2 + 1) // 2
            x = torch.from_numpy(np.ascontiguousarray(spec[a:b].T[None])).float().to(dev)
            act, _ = tr.Encoder(x, G=base[:tp].unsqueeze(0).contiguous())
            assert np.array_equal(encs[u][o8:o8 + tp], act[0].T.cpu().numpy()), (u, a, b)
            checked += 1
            o8 += tp
        assert o8 == encs[u].shape[0]
    assert checked > 20 and any(n < 128 for n in lens) and any(n > 256 for n in lens)


# ---- 7. Trainer surface ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['one_hot', 'binary', 'continues'])
def test_trainer_surface(dev, tmp_path, mode):
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    torch.manual_seed(0)
    E, B = 6, 4
    hps = make_hps(enc_size=E, emb_size=32, n_speakers=4, n_target_speakers=2, batch_size=B, max_to_keep=5)
    tr = Trainer(hps, None, 'targeted_residual', mode, log_dir=str(tmp_path / 'log'), dtype='fp32', device=dev)
    want = E * E if mode == 'binary' else E                      # trainer.py:78-80
    assert tr.SpeakerClassifier.c_in == want and tr.Encoder.linear.out_features == want
    g = torch.Generator().manual_seed(3)
    x = torch.rand(B, 128, 513, generator=g).to(dev)
    c = torch.randint(0, 4, (B,), generator=g).to(dev)
    lc, corr = tr.clf.d_step(x, c, alpha_dis=1.0)
    lr_, lc2, _ = tr.clf.g_step(x, c, 0.5)
    torch.cuda.synchronize()
    assert all(np.isfinite(v.item()) for v in (lc, lr_, lc2))
    s2 = tr.stage2()
    c_t = torch.randint(hps.n_speakers - hps.n_target_speakers, hps.n_speakers, (B,), generator=g).to(dev)
    r = s2.d_step(x, x.flip(0).contiguous(), c_t)
    rg = s2.g_step(x, x.flip(0).contiguous(), c_t)
    lrec = s2.tg_step(x.flip(0).contiguous(), c_t)
    torch.cuda.synchronize()
    assert all(np.isfinite(r[k].item()) for k in ('w_dis', 'gp', 'real_loss_clf'))
    assert np.isfinite(rg['loss_adv'].item()) and np.isfinite(lrec.item())
    tr.save_model(str(tmp_path / 'm.pth'), 's1', 1)
    tr2 = Trainer(hps, None, 'targeted_residual', mode, log_dir=str(tmp_path / 'log'), dtype='fp32', device=dev)
    tr2.load_model(str(tmp_path / 'm.pth-s1-1'), 'encoder, decoder, generator, classifier')
    for a, b in ((tr.Encoder, tr2.Encoder), (tr.SpeakerClassifier, tr2.SpeakerClassifier), (tr.Generator, tr2.Generator)):
        assert torch.equal(a.flat_params()[0], b.flat_params()[0])
    tr2.set_eval()
    xe = torch.rand(1, 513, 128, generator=g).to(dev)
    torch.manual_seed(9)
    e1 = tr.encoder_test_step(xe.permute(0, 2, 1).cpu())
    torch.manual_seed(9)
    e2 = tr2.encoder_test_step(xe.permute(0, 2, 1).cpu())
    assert e1.shape == (1, E, 16) and np.array_equal(e1, e2)


def test_main_train_ae_synthetic_one_hot(dev, tmp_path, monkeypatch, capsys):
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import main
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('ZS_CKPT_EVERY', '4')
    hp = json.load(open(os.path.join(root, 'hps', 'zerospeech_english_1024.json')))
    hp.update(n_speakers=2, n_target_speakers=2, batch_size=16, enc_pretrain_iters=4, max_to_keep=3, enc_size=64, emb_size=128)
    p = str(tmp_path / 'hps_onehot.json')
    json.dump(hp, open(p, 'w'))
    main.main(['--train_ae', '--synthetic', '--enc_mode', 'one_hot', '--hps_path', p, '--ckpt_dir', str(tmp_path / 'ck'),
               '--dtype', 'bf16'])
    out = capsys.readouterr().out
    assert 'pre_AE:[000004/000004]' in out and 'one_hot' in out
    ck = torch.load(str(tmp_path / 'ck' / 'model.pth-ae-4'), map_location='cpu', weights_only=True)
    assert tuple(ck['encoder']['linear.weight'].shape)[0] == 64
