"""zs_adam_pack (clip + Adam + operand re-pack in one launch) against the launches it replaces, bit for bit: the kernel over
hand-built flat buffers of small layers, the counted training step of a small Encoder + Decoder with the "adam_pack" knob on and
off, and the re-pack of an operand the fused launch cannot express (the encoder's bank_d)."""
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

    def operands(self):
        from zs_amd.engine import operands_of
        return operands_of(self.layers)

    def reset(self):
        """p, g, m, v back to the initial values and the operands packed in full from them."""
        from zs_amd import _lib as L
        from zs_amd.layers import pack_operands
        for t, s in zip((self.flat, self.g, self.m, self.v), self.init):
            t.copy_(s)
        self.sq.zero_()
        with L.pack_batch(self.ctx.stream):
            pack_operands(self.ctx, *self.operands())

    def buffers(self):
        out = {'p': self.flat, 'g': self.g, 'm': self.m, 'v': self.v, 'sq': self.sq}
        for i, l in enumerate(self.layers):
            for name in ('wf', 'wd', 'bias_p', 'wih_f', 'wih_d', 'whh_f', 'whh_t', 'bih', 'bhh'):
                if getattr(l, name, None) is not None:
                    out['%d.%s' % (i, name)] = getattr(l, name)
        return out

    def adam(self, max_norm, step, gs, wcg):
        from zs_amd import _lib as L
        return dict(p=L.ptr(self.flat), g=L.ptr(self.g), m=L.ptr(self.m), v=L.ptr(self.v), n=self.n, lr=1e-3, beta1=0.5, beta2=0.9,
                    eps=1e-8, bc1=1.0, bc2=1.0, sumsq=L.ptr(self.sq), max_norm=max_norm, write_clipped_grad=wcg, step_ptr=L.ptr(step),
                    grad_scale=gs)


@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
@pytest.mark.parametrize('case', CASES)
def test_kernel_equals_the_launches_it_replaces(dev, case, dtype):
    """(a) zs_sqnorm + zs_adam_clip + zs_pack_weight_batch + the bias copies against (b) zs_sqnorm + zs_adam_pack and (c)
    zs_sqnorm_stage1 + zs_adam_pack finishing the norm itself, from the same p, g, m, v and fully packed operands: p, g, m, v, the
    norm and every packed buffer in full (padding and slack included) and every bias copy must be equal bit for bit."""
    from zs_amd import _lib as L
    from zs_amd.layers import pack_operands
    from zs_amd.optim import AdamPackPlan

    def init(n):
        g = torch.Generator().manual_seed(1234)
        return [(torch.randn(n, generator=g) * s).to(dev) for s in (0.1, 1.0, 0.05)] + [(torch.rand(n, generator=g) ** 2 * 0.01).to(dev)]

    A, B = _Net(case, dtype, dev, init), _Net(case, dtype, dev, init)
    plan = AdamPackPlan(B.flat, B.ctx, *B.operands())
    assert not plan.rest_w and not plan.rest_v
    kinds = [j.kind for j in plan.jobs]
    assert L.ZS_APJ_WEIGHT in kinds and L.ZS_APJ_RANGE in kinds and (case != 'mixed' or L.ZS_APJ_VECTOR in kinds)
    lib = L.lib()
    st = A.ctx.stream
    steps = {t: torch.full((1,), t, dtype=torch.int32, device=dev) for t in (1, 7)}
    for max_norm, t, gs, wcg, fold in itertools.product((0.01, 0.0), (1, 7), (1.0, 0.5), (0, 1), (0, 1)):
        A.reset()
        B.reset()
        L.check(lib.zs_sqnorm(L.ptr(A.g), A.n, L.ptr(A.part), L.ptr(A.sq), st), 'zs_sqnorm')
        L.call('zs_adam_clip', 'ZsAdam', st, **A.adam(max_norm, steps[t], gs, wcg))
        with L.pack_batch(st):
            pack_operands(A.ctx, *A.operands())
        b = L.STRUCTS['ZsAdam'](**B.adam(max_norm, steps[t], gs, wcg))
        if fold:
            n_part = lib.zs_sqnorm_stage1(L.ptr(B.g), B.n, L.ptr(B.part), st)
            assert 0 < n_part <= 1024
            plan.launch(b, L.ptr(B.part), n_part, st)
        else:
            L.check(lib.zs_sqnorm(L.ptr(B.g), B.n, L.ptr(B.part), L.ptr(B.sq), st), 'zs_sqnorm')
            plan.launch(b, None, 0, st)
        torch.cuda.synchronize()
        what = (max_norm, t, gs, wcg, fold)
        bb = B.buffers()
        for k, x in A.buffers().items():
            assert torch.equal(x, bb[k]), (k, what)
        assert not torch.equal(A.flat, A.init[0]), what


def _train(dev, knob, graph_warmup, steps=3, bank=False):
    from zs_amd import _lib as L
    from zs_amd.model import Decoder, Encoder
    from zs_amd.trainer import AEStep
    prev = L.set_option('adam_pack', knob)
    try:
        torch.manual_seed(0)
        enc = Encoder(c_in=80, c_h1=16, c_h2=64, c_h3=32, ns=0.01, dp=0.5, enc_size=32, seg_len=128, enc_mode='multilabel_binary',
                      dtype='bf16').to(dev)
        dec = Decoder(c_in=32, c_out=80, c_h=64, c_a=4, ns=0.01, seg_len=128, dtype='bf16').to(dev)
        ae = AEStep(enc, dec, lr=1e-3, max_grad_norm=5.0, use_graph=True)
        ae.graph_warmup = graph_warmup
        if bank:
            enc._engine()._bank_operand()
        g = torch.Generator().manual_seed(1)
        losses = []
        for _ in range(steps):
            x = torch.rand(4, 128, 80, generator=g).to(dev)
            c = torch.randint(0, 4, (4,), generator=g).to(dev)
            losses.append(ae.step(x, c).item())
        torch.cuda.synchronize()
        return ae, enc, dec, losses
    finally:
        L.set_option('adam_pack', prev)


@pytest.mark.parametrize('graph_warmup', [2, 10 ** 9], ids=['graph', 'eager'])
def test_counted_steps_equal_with_the_knob_on_and_off(dev, graph_warmup):
    """Three counted steps (two eager + one captured and replayed, or all three eager) with adam_pack = 1 and = 0 from the same
    initial state: every loss, every parameter, m and v bit-equal, and the packed operands equal to a full pack."""
    res = []
    for knob in (1, 0):
        ae, enc, dec, losses = _train(dev, knob, graph_warmup)
        assert len(ae._graphs) == (1 if graph_warmup == 2 else 0)
        res.append((losses, [t.clone() for net in ('enc', 'dec') for t in
                             (ae.opt[net].net.flat_params()[0], ae.opt[net].m, ae.opt[net].v, ae.opt[net].sq)]))
        if knob:
            for net in (enc, dec):
                eng = net._engine()
                assert eng.adam_plan is not None and not eng.adam_plan.rest_w
                bufs = [v['dst'] for op in eng.operands()[0] for v in op['views']] + [cp['dst'] for vc in eng.operands()[1] for cp in vc['copies']]
                fused = [b.clone() for b in bufs]
                eng.pack()
                torch.cuda.synchronize()
                assert all(torch.equal(a, b) for a, b in zip(fused, bufs))
    (la, ta), (lb, tb) = res
    assert la == lb, (la, lb)
    assert len(set(la)) == len(la)
    assert all(torch.equal(a, b) for a, b in zip(ta, tb))


def test_bank_operand_is_repacked_behind_the_fused_launch(dev):
    """An encoder engine with the bank's data-gradient operand allocated: after a fused step, bank_d equals what a full pack() of
    the new weights gives (zs_pack_weight jobs behind the fused launch), and the step equals the knob-off step."""
    ae, enc, dec, losses = _train(dev, 1, 10 ** 9, steps=2, bank=True)
    eng = enc._engine()
    assert eng.adam_plan is not None and len(eng.adam_plan.rest_w) == 7 and not dec._engine().adam_plan.rest_w
    fused = eng.bank_d.clone()
    eng.pack()
    torch.cuda.synchronize()
    assert torch.equal(fused, eng.bank_d) and fused.float().abs().sum().item() > 0
    ae0, enc0, _, losses0 = _train(dev, 0, 10 ** 9, steps=2, bank=True)
    assert losses == losses0 and torch.equal(enc.flat_params()[0], enc0.flat_params()[0])
    assert torch.equal(fused, enc0._engine().bank_d)
