"""The weight average inside the Adam kernels (ZsAdam.ema): zs_adam_clip and zs_adam_pack over hand-built flat buffers of small
layers, the counted training step of a small Encoder + Decoder on every execution path, and one stage-2 D and G step.

The average is e_new = fma(p_new - e, 1 - decay, e) with p_new - e rounded once and 1 - decay formed in fp32.  The value check
takes the kernel's own fp32 p_new and the e it started from, forms diff = fp32(p_new - e) and one = fp32(1) - fp32(decay) in fp32
and ref = float64(diff) * float64(one) + float64(e) in fp64.  The bound is ONE fp32 ulp at |ref| (floor 2^-126): the fused
multiply-add is correctly rounded, so half an ulp is its true error, and the other half covers the fp64 rounding of ref.  No
measured tolerance enters."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(40, 33), (130, 65), (128, 513), (513, 96)]
CASES = ['k1', 'k2', 'k3', 'k5', 'k7', 'mixed']


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


def ema_ref(p_new, e0, decay):
    """(ref fp64, tol fp64): the recursion's value and one fp32 ulp at |ref| (floor 2^-126), per element."""
    one = torch.tensor(1.0, dtype=torch.float32) - torch.tensor(decay, dtype=torch.float32)          # formed in fp32
    diff = p_new.float() - e0.float()                                                               # one fp32 rounding
    ref = diff.double() * one.double().to(diff.device) + e0.double()
    _, ex = torch.frexp(ref.abs())                                                                   # |ref| in [2^(ex-1), 2^ex)
    tol = torch.where(ref == 0, torch.zeros_like(ref), torch.ldexp(torch.ones_like(ref), ex - 24)).clamp_min(2.0 ** -126)
    return ref, tol


def assert_ema(e, p_new, e0, decay, what):
    ref, tol = ema_ref(p_new, e0, decay)
    err = (e.double() - ref).abs()
    worst = float((err / tol).max())
    print('%s: worst |e - ref| = %.3f ulp' % (what, worst))
    assert bool((err <= tol).all()), (what, worst)


def _params(case):
    """[(name, shape)] in flat-buffer order: the layers' parameters with an embedding / plain biases between them, so that range
    jobs and the alignment gaps of odd-sized parameters occur."""
    if case != 'mixed':
        k = int(case[1:])
        out = []
        for i, (co, ci) in enumerate(SHAPES):
            out += [('c%d.w' % i, (co, ci, k) if k > 1 else (co, ci)), ('c%d.b' % i, (co,))]
            if i == 1:
                out.append(('emb', (5, 7)))
        return out
    out = [('s2.w', (130, 65, 3)), ('s2.b', (130,)), ('emb', (3, 9)), ('st.w', (40, 33, 5)), ('st.b', (40,))]
    for g, H in (('g32.', 32), ('g24.', 24)):
        for sfx in ('', '_reverse'):
            out += [(g + 'weight_ih_l0' + sfx, (3 * H, 40)), (g + 'weight_hh_l0' + sfx, (3 * H, H)), (g + 'bias_ih_l0' + sfx, (3 * H,)),
                    (g + 'bias_hh_l0' + sfx, (3 * H,))]
    return out


class _Net(object):
    """One set of clones: flat p / g / m / v, the layers over it and their packed buffers."""

    def __init__(self, case, dtype, dev, init):
        from zs_amd.layers import ConvLayer, Ctx, GruLayer, rup
        self.ctx = Ctx(dev, dtype)
        offs, n = {}, 0
        for name, shape in _params(case):
            offs[name] = n
            n += rup(int(torch.Size(shape).numel()), 4)
        self.n = n
        self.flat, self.g, self.m, self.v = (torch.zeros(n, device=dev) for _ in range(4))
        self.init = init(n)
        P = {k: self.flat[o:o + torch.Size(s).numel()].view(s) for (k, s), o in zip(_params(case), offs.values())}
        G = {k: self.g[o:o + torch.Size(s).numel()].view(s) for (k, s), o in zip(_params(case), offs.values())}
        self.layers = []
        if case != 'mixed':
            for i in range(len(SHAPES)):
                self.layers.append(ConvLayer(self.ctx, P['c%d.w' % i], P['c%d.b' % i], G['c%d.w' % i], G['c%d.b' % i]))
        else:
            self.layers.append(ConvLayer(self.ctx, P['s2.w'], P['s2.b'], G['s2.w'], G['s2.b'], split2=True))
            self.layers.append(ConvLayer(self.ctx, P['st.w'], P['st.b'], G['st.w'], G['st.b'], stride=2))
            self.layers += [GruLayer(self.ctx, P, G, 'g32.'), GruLayer(self.ctx, P, G, 'g24.')]
        self.sq = torch.zeros(1, device=dev)
        self.part = torch.zeros(1024, dtype=torch.float64, device=dev)
        self.e_store = torch.zeros(n + 4, device=dev)                # the average: [0, n) is 16-byte aligned, [1, n + 1) is not

    def operands(self):
        from zs_amd.engine import operands_of
        return operands_of(self.layers)

    def reset(self):
        """p, g, m, v back to the initial values, the operands packed in full from them, the average's storage filled with -7."""
        from zs_amd import _lib as L
        from zs_amd.layers import pack_operands
        for t, s in zip((self.flat, self.g, self.m, self.v), self.init):
            t.copy_(s)
        self.sq.zero_()
        self.e_store.fill_(-7.0)
        with L.pack_batch(self.ctx.stream):
            pack_operands(self.ctx, *self.operands())

    def ema(self, e0, shift):
        """The view of the average's storage at element `shift` (0: aligned, 1: not), holding e0."""
        e = self.e_store[shift:shift + self.n]
        e.copy_(e0)
        return e

    def buffers(self):
        out = {'p': self.flat, 'g': self.g, 'm': self.m, 'v': self.v, 'sq': self.sq}
        for i, l in enumerate(self.layers):
            for name in ('wf', 'wd', 'bias_p', 'wih_f', 'wih_d', 'whh_f', 'whh_t', 'bih', 'bhh'):
                if getattr(l, name, None) is not None:
                    out['%d.%s' % (i, name)] = getattr(l, name)
        return out

    def snapshot(self):
        return {k: v.clone() for k, v in self.buffers().items()}

    def adam(self, max_norm, step, wcg, ema=None, decay=None):
        from zs_amd import _lib as L
        kw = dict(p=L.ptr(self.flat), g=L.ptr(self.g), m=L.ptr(self.m), v=L.ptr(self.v), n=self.n, lr=1e-3, beta1=0.5, beta2=0.9,
                  eps=1e-8, bc1=1.0, bc2=1.0, sumsq=L.ptr(self.sq), max_norm=max_norm, write_clipped_grad=wcg, step_ptr=L.ptr(step),
                  grad_scale=1.0)
        if ema is not None:
            kw.update(ema=L.ptr(ema), ema_decay=decay)
        return kw


def _init(dev):
    def init(n):
        g = torch.Generator().manual_seed(1234)
        return [(torch.randn(n, generator=g) * s).to(dev) for s in (0.1, 1.0, 0.05)] + [(torch.rand(n, generator=g) ** 2 * 0.01).to(dev)]
    return init


def _run_clip(A, kw):
    """zs_sqnorm + zs_adam_clip + the full pack."""
    from zs_amd import _lib as L
    from zs_amd.layers import pack_operands
    st = A.ctx.stream
    L.check(L.lib().zs_sqnorm(L.ptr(A.g), A.n, L.ptr(A.part), L.ptr(A.sq), st), 'zs_sqnorm')
    L.call('zs_adam_clip', 'ZsAdam', st, **kw)
    with L.pack_batch(st):
        pack_operands(A.ctx, *A.operands())


def _run_pack(B, plan, kw):
    """zs_sqnorm_stage1 + zs_adam_pack."""
    from zs_amd import _lib as L
    st = B.ctx.stream
    n_part = L.lib().zs_sqnorm_stage1(L.ptr(B.g), B.n, L.ptr(B.part), st)
    assert 0 < n_part <= 1024
    plan.launch(L.STRUCTS['ZsAdam'](**kw), L.ptr(B.part), n_part, st)


def _same(a, b, what):
    for k, x in a.items():
        assert torch.equal(x, b[k]), (k, what)


@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
@pytest.mark.parametrize('case', CASES)
def test_kernels_average_alike_and_perturb_nothing(dev, case, dtype):
    """(a) zs_sqnorm + zs_adam_clip + full pack and (b) zs_sqnorm_stage1 + zs_adam_pack from the same p, g, m, v and a random e0:
    p, g, m, v, the norm, every packed buffer in full and the average bit-equal; (c) all but the average bit-equal to the same
    launches with ema = NULL; (d) with the average one float off 16-byte alignment (the one-element branch) the same bits
    everywhere; (e) the average within one ulp of the fp64 recursion on the kernel's own p_new; and it moved."""
    from zs_amd import _lib as L
    from zs_amd.optim import AdamPackPlan
    A, B = _Net(case, dtype, dev, _init(dev)), _Net(case, dtype, dev, _init(dev))
    plan = AdamPackPlan(B.flat, B.ctx, *B.operands())
    assert not plan.rest_w and not plan.rest_v
    kinds = [j.kind for j in plan.jobs]
    assert L.ZS_APJ_WEIGHT in kinds and L.ZS_APJ_RANGE in kinds and (case != 'mixed' or L.ZS_APJ_VECTOR in kinds)
    e0 = (torch.randn(A.n, generator=torch.Generator().manual_seed(99)) * 0.1).to(dev)
    steps = {t: torch.full((1,), t, dtype=torch.int32, device=dev) for t in (1, 7)}
    for decay, max_norm, t, wcg in itertools.product((0.9, 0.999), (0.01, 0.0), (1, 7), (0, 1)):
        what = (decay, max_norm, t, wcg)
        # (c)'s side: the launches without the average
        A.reset()
        B.reset()
        _run_clip(A, A.adam(max_norm, steps[t], wcg))
        _run_pack(B, plan, B.adam(max_norm, steps[t], wcg))
        torch.cuda.synchronize()
        plain_a, plain_b = A.snapshot(), B.snapshot()
        _same(plain_a, plain_b, what)
        assert float(A.e_store.min()) == float(A.e_store.max()) == -7.0 and float(B.e_store.max()) == -7.0      # never touched
        # (a), (b): with the average, 16-byte aligned
        A.reset()
        B.reset()
        ea, eb = A.ema(e0, 0), B.ema(e0, 0)
        assert ea.data_ptr() % 16 == 0 and eb.data_ptr() % 16 == 0
        _run_clip(A, A.adam(max_norm, steps[t], wcg, ea, decay))
        _run_pack(B, plan, B.adam(max_norm, steps[t], wcg, eb, decay))
        torch.cuda.synchronize()
        _same(A.buffers(), B.buffers(), what)
        assert torch.equal(ea, eb), what
        _same(plain_a, A.buffers(), what)                                        # (c)
        _same(plain_b, B.buffers(), what)
        assert float(A.e_store[A.n:].min()) == -7.0 and float(B.e_store[B.n:].max()) == -7.0      # nothing behind the n floats
        assert_ema(ea, A.flat, e0, decay, '%s %s %r' % (case, dtype, what))      # (e)
        assert not torch.equal(ea, e0) and not torch.equal(A.flat, A.init[0]), what
        aligned = ea.clone()
        # (d): the average one float further on
        A.reset()
        B.reset()
        ea, eb = A.ema(e0, 1), B.ema(e0, 1)
        assert ea.data_ptr() % 16 == 4 and eb.data_ptr() % 16 == 4
        _run_clip(A, A.adam(max_norm, steps[t], wcg, ea, decay))
        _run_pack(B, plan, B.adam(max_norm, steps[t], wcg, eb, decay))
        torch.cuda.synchronize()
        assert torch.equal(ea, aligned) and torch.equal(eb, aligned), what
        _same(plain_a, A.buffers(), what)
        _same(plain_b, B.buffers(), what)
        for net in (A, B):                                                       # nothing outside the n floats
            assert float(net.e_store[0]) == -7.0 and float(net.e_store[net.n + 1:].min()) == -7.0 == float(net.e_store[net.n + 1:].max())


@pytest.mark.parametrize('decay', [1.0, -0.1])
def test_a_decay_outside_the_range_is_refused_by_both_entry_points(dev, decay):
    from zs_amd import _lib as L
    from zs_amd.optim import AdamPackPlan
    assert L.ZS_EINVAL == -1
    N = _Net('k1', 'bf16', dev, _init(dev))
    plan = AdamPackPlan(N.flat, N.ctx, *N.operands())
    e0 = torch.full((N.n,), 0.25, device=dev)
    N.reset()
    e = N.ema(e0, 0)
    step = torch.ones(1, dtype=torch.int32, device=dev)
    before = N.snapshot()
    kw = N.adam(0.01, step, 0, e, decay)
    with pytest.raises(L.ZsError, match=r'zs_adam_clip failed \(-1\).*ema_decay'):
        L.call('zs_adam_clip', 'ZsAdam', N.ctx.stream, **kw)
    with pytest.raises(L.ZsError, match=r'zs_adam_pack failed \(-1\).*ema_decay'):
        plan.launch(L.STRUCTS['ZsAdam'](**kw), None, 0, N.ctx.stream)
    torch.cuda.synchronize()
    _same(before, N.buffers(), decay)                                            # nothing was written
    assert torch.equal(e, e0)
    # without the average the field is not looked at: a struct from an older caller is off whatever its tail holds
    kw.pop('ema')
    L.call('zs_adam_clip', 'ZsAdam', N.ctx.stream, **kw)
    torch.cuda.synchronize()
    assert not torch.equal(before['p'], N.flat) and torch.equal(e, e0)


# ---- counted steps ------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _train(dev, knob, graph_warmup, ema, steps=3):
    """Three counted steps of the small autoencoder; cached.  Returns dict(losses, p / m / v per net after the last step and, with
    an average, per step the (p, ema) of each net read back after it, and the initial weights)."""
    key = (knob, graph_warmup, ema)
    if key in _RUNS:
        return _RUNS[key]
    from zs_amd import _lib as L
    from zs_amd.model import Decoder, Encoder
    from zs_amd.trainer import AEStep
    prev = L.set_option('adam_pack', knob)
    try:
        torch.manual_seed(0)
        enc = Encoder(c_in=80, c_h1=16, c_h2=64, c_h3=32, ns=0.01, dp=0.5, enc_size=32, seg_len=128, enc_mode='multilabel_binary',
                      dtype='bf16').to(dev)
        dec = Decoder(c_in=32, c_out=80, c_h=64, c_a=4, ns=0.01, seg_len=128, dtype='bf16').to(dev)
        ae = AEStep(enc, dec, lr=1e-3, max_grad_norm=5.0, use_graph=True, ema=ema)
        ae.graph_warmup = graph_warmup
        out = {'losses': [], 'trace': [], 'w0': {n: ae.opt[n].net.flat_params()[0].clone() for n in ('enc', 'dec')}}
        if ema is not None:
            for n in ('enc', 'dec'):
                assert ae.opt[n].ema.dtype == torch.float32 and torch.equal(ae.opt[n].ema, out['w0'][n])
                assert ae.opt[n].ema.data_ptr() != ae.opt[n].net.flat_params()[0].data_ptr()
        else:
            assert ae.opt['enc'].ema is None and 'ema' not in ae.opt['enc'].state_dict()
        g = torch.Generator().manual_seed(1)
        for _ in range(steps):
            x = torch.rand(4, 128, 80, generator=g).to(dev)
            c = torch.randint(0, 4, (4,), generator=g).to(dev)
            out['losses'].append(ae.step(x, c).item())
            torch.cuda.synchronize()
            if ema is not None:
                out['trace'].append({n: (ae.opt[n].net.flat_params()[0].clone(), ae.opt[n].ema.clone()) for n in ('enc', 'dec')})
        assert len(ae._graphs) == (1 if graph_warmup == 2 else 0)
        out['final'] = {n: tuple(t.clone() for t in (ae.opt[n].net.flat_params()[0], ae.opt[n].m, ae.opt[n].v)) for n in ('enc', 'dec')}
        _RUNS[key] = out
        return out
    finally:
        L.set_option('adam_pack', prev)


@pytest.mark.parametrize('knob', [1, 0], ids=['pack', 'clip'])
@pytest.mark.parametrize('graph_warmup', [2, 10 ** 9], ids=['graph', 'eager'])
def test_counted_steps_with_the_average(dev, graph_warmup, knob):
    """Three counted steps with ema = 0.9 on each of the four paths (captured or eager x zs_adam_pack or zs_adam_clip): losses, p, m
    and v bit-equal to the run without the average, the average bit-equal to the captured zs_adam_pack run's, and after every step
    within the bound of one recursion step from the average before it and the p read back after it."""
    on, off = _train(dev, knob, graph_warmup, 0.9), _train(dev, knob, graph_warmup, None)
    assert on['losses'] == off['losses'] and len(set(on['losses'])) == 3
    for n in ('enc', 'dec'):
        assert all(torch.equal(a, b) for a, b in zip(on['final'][n], off['final'][n])), n
    first = _train(dev, 1, 2, 0.9)
    for n in ('enc', 'dec'):
        e_prev = on['w0'][n]
        for i, tr in enumerate(on['trace']):
            p, e = tr[n]
            assert torch.equal(e, first['trace'][i][n][1]), (n, i)
            assert_ema(e, p, e_prev, 0.9, '%s step %d' % (n, i + 1))
            assert not torch.equal(e, p) and not torch.equal(e, e_prev), (n, i)
            e_prev = e


# ---- stage 2 ------------------------------------------------------------------------------------------------------------------
def _stage2_once(dev, tmp_path, ema):
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    hps = make_hps(enc_size=8, emb_size=32, n_speakers=4, n_target_speakers=2, batch_size=2, patch_iters=2, n_patch_steps=2, max_to_keep=5)
    torch.manual_seed(0)
    tr = Trainer(hps, None, hps.g_mode, hps.enc_mode, log_dir=str(tmp_path / ('log_%s' % ema)), dtype='bf16', device=dev, ema=ema)
    s2 = tr.stage2()
    w0 = {'gen': tr.Generator.flat_params()[0].clone(), 'patch': tr.PatchDiscriminator.flat_params()[0].clone()}
    g = torch.Generator().manual_seed(5)
    x_s, x_t = (torch.rand(2, 128, 513, generator=g).to(dev) for _ in range(2))
    c_t = torch.tensor([2, 3], device=dev)
    s2.d_step(x_s, x_t, c_t)
    s2.g_step(x_s, x_t, c_t)
    torch.cuda.synchronize()
    return tr, s2, w0


def test_stage2_generator_and_critic_average(dev, tmp_path):
    """One D step and one G step at the smallest stage-2 configuration: the weights bit-equal to the run without the average, each
    average one recursion step from its initial copy of the weights; every other average still equals its net's weights."""
    tr, s2, w0 = _stage2_once(dev, tmp_path, 0.9)
    tr_off, s2_off, w0_off = _stage2_once(dev, tmp_path, None)
    assert s2_off.gen_opt.ema is None and s2_off.patch_opt.ema is None and tr_off.ema_opts() == {}
    assert set(tr.ema_opts()) == {'encoder', 'decoder', 'generator', 'classifier', 'patch_discriminator'}
    for name, opt, net, net_off in (('gen', s2.gen_opt, tr.Generator, tr_off.Generator),
                                    ('patch', s2.patch_opt, tr.PatchDiscriminator, tr_off.PatchDiscriminator)):
        assert torch.equal(w0[name], w0_off[name])
        p = net.flat_params()[0]
        assert torch.equal(p, net_off.flat_params()[0]) and not torch.equal(p, w0[name]), name
        assert opt.t == 1
        assert_ema(opt.ema, p, w0[name], 0.9, 'stage 2 ' + name)
        assert not torch.equal(opt.ema, w0[name]) and not torch.equal(opt.ema, p), name
    for key in ('encoder', 'decoder', 'classifier'):                             # never stepped: the average is the weights
        opt = tr.ema_opts()[key]
        assert torch.equal(opt.ema, opt.net.flat_params()[0]), key
