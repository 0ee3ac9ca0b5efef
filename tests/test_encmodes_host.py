"""enc_mode 'one_hot', 'binary' and 'continues' on the host (no GPU): Encoder construction and state_dict against the reference's
key -> shape maps in tests/golden/encmodes_small.npz, the noise checks, and a torch restatement of the three discretisers
(model/model.py:93-110, 457-472) pinned to the fixture."""
import pytest
import torch

from conftest import load_golden

NS, TAU = 0.01, 0.1
CASES = [('one_hot', 6), ('one_hot', 96), ('binary', 6), ('binary', 16), ('continues', 8)]


@pytest.fixture(scope='module')
def gold():
    return load_golden('encmodes_small.npz')


def _small(mode, E):
    import zs_amd  # noqa: F401
    from zs_amd.model import Encoder
    return Encoder(c_in=80, c_h1=16, c_h2=32, c_h3=16, ns=NS, dp=0.5, enc_size=E, seg_len=128, enc_mode=mode)


def restate(mode, enc, U, E):
    """enc [B, n_lin, T'] (+ U [B, T', E] / [B, T', E, E]) -> enc_act [B, E, T'], differentiable (straight-through)."""
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


@pytest.mark.parametrize('mode,E', CASES)
def test_state_dict_matches_reference(gold, mode, E):
    _, m = gold
    ref = m['shapes']['%s_%d' % (mode, E)]
    sd = _small(mode, E).state_dict()
    assert sorted(sd.keys()) == sorted(ref.keys())
    assert {k: list(v.shape) for k, v in sd.items()} == ref


def test_reference_default_mode_constructs():
    import zs_amd  # noqa: F401
    from zs_amd.model import Encoder
    enc = Encoder()
    assert enc.enc_mode == 'continues' and tuple(enc.linear.weight.shape) == (512, 512 + 2 * 128)


def test_gumbel_t_is_not_built():
    with pytest.raises(NotImplementedError, match='gumbel_t'):
        _small('gumbel_t', 8)
    with pytest.raises(NotImplementedError):
        _small('no_such_mode', 8)


@pytest.mark.parametrize('mode,E,good,bad', [('one_hot', 6, (2, 4, 6), (2, 4, 6, 2)), ('binary', 6, (2, 4, 6, 6), (2, 4, 36)),
                                             ('one_hot', 96, (2, 4, 96), (2, 5, 96))])
def test_noise_shape_checked_on_the_host(mode, E, good, bad):
    from zs_amd import _lib as L
    enc = _small(mode, E)
    x = torch.rand(2, 80, 32)                                    # T' = 4
    for kw in ('U', 'G'):
        with pytest.raises(ValueError, match='shape'):
            enc(x, **{kw: torch.rand(bad)})
    with pytest.raises(L.ZsError):                               # the right shape passes the check; the CPU module then refuses
        enc(x, U=torch.rand(good))


def test_continues_takes_no_noise():
    enc = _small('continues', 8)
    with pytest.raises(ValueError, match='no noise'):
        enc(torch.rand(2, 80, 32), U=torch.rand(2, 4, 8))
    with pytest.raises(ValueError, match='no noise'):
        enc(torch.rand(2, 80, 32), G=torch.rand(2, 4, 8))


def test_binary_width_limit():
    with pytest.raises(ValueError):
        _small('binary', 65)


@pytest.mark.parametrize('mode,E', CASES)
def test_restatement_reproduces_fixture(gold, mode, E):
    d, m = gold
    tag = '%s_%d' % (mode, E)
    for T in m['lengths']:
        enc = torch.from_numpy(d['%s.enc.%d' % (tag, T)])
        U = torch.from_numpy(d['%s.U.%d' % (tag, T)]) if mode != 'continues' else None
        assert torch.equal(restate(mode, enc, U, E), torch.from_numpy(d['%s.enc_act.%d' % (tag, T)])), T


@pytest.mark.parametrize('mode,E', CASES)
def test_restatement_backward_is_the_closed_form(gold, mode, E):
    """Autograd of the restatement equals the backward formulas the kernel implements (fp64)."""
    d, _ = gold
    tag = '%s_%d' % (mode, E)
    enc = torch.from_numpy(d['%s.enc.%d' % (tag, 24)]).double().requires_grad_(True)
    U = torch.from_numpy(d['%s.U.%d' % (tag, 24)]).double() if mode != 'continues' else None
    act = restate(mode, enc, U, E)
    dout = torch.randn(act.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    act.backward(dout)
    B, n_lin, T4 = enc.shape
    lg = enc.detach().permute(0, 2, 1).reshape(B * T4, n_lin)
    g = dout.permute(0, 2, 1).reshape(B * T4, E)
    if mode == 'continues':
        want = torch.where(lg > 0, g, g * NS)
    else:
        G = -torch.log(-torch.log(U + 1e-20) + 1e-20)
        y = torch.softmax((lg + G.reshape(B * T4, n_lin)).reshape(B * T4, -1, E) / TAU, dim=-1)
        if mode == 'binary':
            hard = torch.zeros_like(y).scatter_(-1, y.max(dim=-1)[1].unsqueeze(-1), 1.0)
            s = hard.sum(1)
            g = g * ((s >= 0) & (s <= 1)).double()
        gg = g.unsqueeze(1)
        want = (y * (gg - (gg * y).sum(-1, keepdim=True)) / TAU).reshape(B * T4, n_lin)
    got = enc.grad.permute(0, 2, 1).reshape(B * T4, n_lin)
    assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize('mode', ['one_hot', 'binary', 'continues'])
def test_fixture_train_step_covers_every_parameter(gold, mode):
    """The train step's fixed-point gradient / update groups name every Encoder parameter with the reference's shape, and decode
    to finite values whose first Adam step is at most lr."""
    import numpy as np
    d, m = gold
    tm = m['train'][mode]
    shapes = m['shapes']['%s_%d' % (mode, tm['enc_size'])]
    for key in ('genc', 'enc1_step'):
        table = m['fixed']['train_%s.%s' % (mode, key)]
        assert {name: shape for name, shape, _ in table} == shapes
        q = d['train_%s.%s@%s' % (mode, key, 'q16' if key == 'genc' else 'q8')]
        assert q.shape[-1] == sum(int(np.prod(s)) for _, s, _ in table)
        if key == 'enc1_step':
            assert max(step * 15 for _, _, step in table) <= tm['lr'] * (1 + 1e-3)
