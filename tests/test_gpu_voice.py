"""Voice adaptation on the device (zs_amd.voice; csrc/zs_voice.hip):

1. zs_voice_gather against numpy, exact: the cursor's batch, the wrap of the item table, the zero columns, both operand types;
2. zs_voice_adam against the launches it replaces (zs_emb_scatter into row 0, zs_adam_clip), bit for bit, and its norm against fp64;
3. DecoderEngine.backward(param_grads=False): the embedding sums of the full backward, no gradient buffer written;
4. one VoiceStep iteration against the oracle (decoder_forward under autograd, l1_loss, clip, AdamState);
5. the eager and the captured iteration, bit for bit; the logging cadence changes nothing;
6. an adaptation run leaves every Encoder and Decoder tensor of the trainer as it was;
7. a planted voice is recovered: the loss falls as it falls in the oracle;
8. main.py --adapt_voice, then --convert_dir / --synth_dir with --voice."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the repository root and oracle/ on sys.path)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 128


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


def _stream():
    return torch.cuda.current_stream().cuda_stream


TDT = {'fp32': torch.float32, 'bf16': torch.bfloat16}


# ---- 1. zs_voice_gather ------------------------------------------------------------------------------------------------------------------
class _Gather(object):
    """A pool, packed units (every byte random: the unused high bits of a row's last byte too) and an item table of n entries on the
    host and the device; outputs filled with a sentinel, with a guard behind them; x one float off 16-byte alignment when x_off."""

    def __init__(self, dev, E, ld_bits, dtype, F, n=7, B=3, seg=SEG, row_extra=0, x_off=0, seed=0):
        from zs_amd import _lib as L
        rng = np.random.RandomState(seed)
        self.L, self.dev, self.E, self.ld, self.dtype, self.F, self.n, self.B, self.seg = L, dev, E, ld_bits, dtype, F, n, B, seg
        self.U = seg // 8
        frames_total = 3 * seg + 40
        n_units = frames_total // 8
        self.nbytes = (E + 7) // 8
        self.row_bytes = self.nbytes + row_extra
        self.pool = rng.rand(frames_total, F).astype(np.float32)
        self.packed = rng.randint(0, 256, size=(n_units, self.row_bytes)).astype(np.uint8)
        self.first = (8 * rng.randint(0, (frames_total - seg) // 8 + 1, size=n)).astype(np.int64)
        self.ufirst = rng.randint(0, n_units - self.U + 1, size=n).astype(np.int64)
        self.first[0], self.ufirst[0] = frames_total - seg, n_units - self.U          # the last admissible rows are read
        d = lambda a: torch.from_numpy(a).to(dev)
        self.pool_d, self.packed_d, self.first_d, self.ufirst_d = d(self.pool), d(self.packed), d(self.first), d(self.ufirst)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        self.nx, self.nb, self.x_off = B * seg * F, B * self.U * ld_bits, x_off
        self.xbuf = torch.full((x_off + self.nx + 64,), -3.0, dtype=torch.float32, device=dev)
        self.bbuf = torch.full((self.nb + 64,), -3.0, dtype=TDT[dtype], device=dev)

    def args(self, **change):
        L = self.L
        kw = dict(dtype=(L.ZS_F32 if self.dtype == 'fp32' else L.ZS_BF16), pool=L.ptr(self.pool_d), packed=L.ptr(self.packed_d),
                  row_bytes=self.row_bytes, first=L.ptr(self.first_d), ufirst=L.ptr(self.ufirst_d), n=self.n, cursor=L.ptr(self.cursor),
                  B=self.B, seg_len=self.seg, F=self.F, E=self.E, x=L.ptr(self.xbuf, self.x_off), bits=L.ptr(self.bbuf), ld_bits=self.ld,
                  advance=1)
        kw.update(change)
        return kw

    def launch(self, **change):
        self.L.call('zs_voice_gather', 'ZsVoiceGather', _stream(), **self.args(**change))

    def want(self, k):
        items = [(k * self.B + b) % self.n for b in range(self.B)]
        x = np.stack([self.pool[self.first[i]:self.first[i] + self.seg] for i in items])
        bits = np.zeros((self.B, self.U, self.ld), dtype=np.float32)
        for b, i in enumerate(items):
            rows = self.packed[self.ufirst[i]:self.ufirst[i] + self.U, :self.nbytes]
            bits[b, :, :self.E] = np.unpackbits(rows, axis=1, count=self.E, bitorder='little')
        return x, bits

    def check(self, k):
        x, bits = self.want(k)
        gx = self.xbuf.cpu().numpy()
        gb = self.bbuf.float().cpu().numpy()
        assert np.array_equal(gx[self.x_off:self.x_off + self.nx].reshape(x.shape), x), 'x of batch %d' % k
        assert np.array_equal(gb[:self.nb].reshape(bits.shape), bits), 'bits of batch %d' % k
        assert (gx[:self.x_off] == -3.0).all() and (gx[self.x_off + self.nx:] == -3.0).all() and (gb[self.nb:] == -3.0).all(), 'guard'

    def untouched(self):
        return bool((self.xbuf == -3.0).all()) and bool((self.bbuf.float() == -3.0).all())


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('E, ld_bits, F, row_extra, x_off', [(6, 32, 513, 0, 0), (13, 16, 80, 1, 1), (13, 32, 513, 0, 3), (1024, 1024, 80, 0, 0),
                                                             (1024, 1056, 513, 2, 0)])
def test_gather_equals_numpy(dev, dtype, E, ld_bits, F, row_extra, x_off):
    """n = 7 items, B = 3: four launches serve batches 0..3 (items 0 1 2 | 3 4 5 | 6 0 1 | 2 3 4: the table wraps) and leave the
    cursor at 4; advance = 0 serves batch 4 and leaves it there; a cursor set by the host is honoured."""
    g = _Gather(dev, E, ld_bits, dtype, F, row_extra=row_extra, x_off=x_off, seed=E + F)
    for k in range(4):
        g.launch()
        g.check(k)
    assert int(g.cursor.item()) == 4
    g.launch(advance=0)
    g.check(4)
    assert int(g.cursor.item()) == 4
    g.cursor.fill_(2 ** 40 + 5)                                            # far past the table: (k B + b) mod n in 64 bits
    g.launch()
    g.check(2 ** 40 + 5)
    assert int(g.cursor.item()) == 2 ** 40 + 6


def test_gather_more_samples_than_items(dev):
    g = _Gather(dev, 8, 32, 'fp32', 80, n=2, B=4, seed=9)
    g.launch()
    g.check(0)
    g.launch()
    g.check(1)


def test_gather_refuses_malformed_structs(dev):
    from zs_amd import _lib as L
    g = _Gather(dev, 13, 32, 'bf16', 513, seed=2)
    one = lambda t: L.ptr(t) + 1
    cases = [dict(pool=None), dict(packed=None), dict(first=None), dict(ufirst=None), dict(cursor=None), dict(x=None), dict(bits=None),
             dict(dtype=7), dict(B=0), dict(F=0), dict(E=0), dict(n=0), dict(seg_len=0), dict(seg_len=SEG + 4), dict(seg_len=-8),
             dict(ld_bits=8), dict(ld_bits=36), dict(row_bytes=1), dict(pool=one(g.pool_d)), dict(x=one(g.xbuf)),
             dict(bits=L.ptr(g.bbuf, 1)), dict(first=L.ptr(g.first_d) + 4), dict(ufirst=L.ptr(g.ufirst_d) + 4), dict(cursor=L.ptr(g.cursor) + 4)]
    for change in cases:
        with pytest.raises(L.ZsError, match='zs_voice_gather'):
            g.launch(**change)
    torch.cuda.synchronize()
    assert g.untouched() and int(g.cursor.item()) == 0
    g.launch()
    g.check(0)


# ---- 2. zs_voice_adam --------------------------------------------------------------------------------------------------------------------
def _adam_pair(dev, B, C, max_norm_of, steps, seed):
    """zs_voice_adam (rows at five separate addresses) against five zs_emb_scatter(idx = 0) + zs_adam_clip over the same values laid
    out as one buffer, fed the sumsq the kernel reports, `len(steps)` updates in a row.  max_norm_of(norm) -> max_norm."""
    import ctypes
    from zs_amd import _lib as L
    rng = np.random.RandomState(seed)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    n = 5 * C
    p0, m0, v0 = rng.randn(n), 0.1 * rng.randn(n), 0.01 * rng.rand(n)
    rows = [d(p0[k * C:(k + 1) * C]) for k in range(5)]                       # five allocations
    ptrs = (ctypes.c_void_p * 5)(*[r.data_ptr() for r in rows])
    mA, vA, gA, sqA = d(m0), d(v0), torch.full((n,), 9.0, device=dev), torch.zeros(1, device=dev)
    pB, mB, vB, gB = d(p0), d(m0), d(v0), torch.full((n,), 9.0, device=dev)
    idx = torch.zeros(B, dtype=torch.int64, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    kw = dict(lr=1e-2, beta1=0.5, beta2=0.9, eps=1e-8, bc1=1.0, bc2=1.0)
    for t in steps:
        e = rng.randn(5, B, C).astype(np.float32) * rng.choice([1e-3, 1.0, 30.0])
        e_d = d(e)
        g64 = e.astype(np.float64).sum(axis=1)                                  # (for the size of the norm only)
        max_norm = float(max_norm_of(float(np.sqrt((g64 ** 2).sum()))))
        step.fill_(t)
        L.call('zs_voice_adam', 'ZsVoiceAdam', _stream(), emb_sum=L.ptr(e_d), B=B, C=C, row=ptrs, m=L.ptr(mA), v=L.ptr(vA), g=L.ptr(gA),
               sumsq=L.ptr(sqA), max_norm=max_norm, step_ptr=L.ptr(step), **kw)
        for k in range(5):
            L.call('zs_emb_scatter', 'ZsEmbScatter', _stream(), emb_sum=L.ptr(e_d, k * B * C), emb_ld=C, idx=L.ptr(idx), B=B,
                   demb=L.ptr(gB, k * C), demb_ld=C, n_rows=1, C=C, accumulate=0)
        L.call('zs_adam_clip', 'ZsAdam', _stream(), p=L.ptr(pB), g=L.ptr(gB), m=L.ptr(mB), v=L.ptr(vB), n=n, sumsq=L.ptr(sqA),
               max_norm=max_norm, write_clipped_grad=0, step_ptr=L.ptr(step), **kw)
        torch.cuda.synchronize()
        assert torch.equal(gA, gB), 'g at step %d' % t
        assert torch.equal(torch.cat(rows), pB) and torch.equal(mA, mB) and torch.equal(vA, vB), 'p, m, v at step %d' % t
        sq64 = float((gB.double() ** 2).sum().item())
        rel = abs(float(sqA.item()) - sq64) / sq64
        print('B %d C %d step %d max_norm %.3g: |sumsq - fp64| / fp64 = %.3g' % (B, C, t, max_norm, rel))
        assert rel <= 1e-6
        yield max_norm, float(np.sqrt(sq64)), pB.clone()


@pytest.mark.parametrize('B', [1, 37])
@pytest.mark.parametrize('C', [64, 1024])
def test_voice_adam_equals_scatter_and_adam_clip(dev, B, C):
    """Clipping active (max_norm half the norm), inactive (twice the norm) and disabled (0 and negative), step counts 1 and 7."""
    for name, fn in (('active', lambda nrm: 0.5 * nrm), ('inactive', lambda nrm: 2.0 * nrm), ('off', lambda nrm: 0.0), ('off', lambda nrm: -1.0)):
        for max_norm, nrm, _ in _adam_pair(dev, B, C, fn, (1, 7), seed=B + C):
            assert {'active': 0.0 < max_norm < nrm, 'inactive': max_norm > nrm, 'off': max_norm <= 0.0}[name]
    # clipping changes the update, and only when it is active
    run = lambda fn: [p for _, _, p in _adam_pair(dev, B, C, fn, (7,), seed=3)][0]
    off, inactive, active = run(lambda nrm: 0.0), run(lambda nrm: 2.0 * nrm), run(lambda nrm: 0.5 * nrm)
    assert torch.equal(off, inactive) and not torch.equal(off, active)


def test_voice_adam_refuses_malformed_structs(dev):
    import ctypes
    from zs_amd import _lib as L
    C, B = 64, 2
    t = lambda n, val=5.0: torch.full((n,), val, device=dev)
    e, m, v, g, sq = t(5 * B * C), t(5 * C), t(5 * C), t(5 * C), t(1)
    rows = t(5 * C)
    ptrs = lambda missing=None: (ctypes.c_void_p * 5)(*[None if k == missing else L.ptr(rows, k * C) for k in range(5)])
    ok = dict(emb_sum=L.ptr(e), B=B, C=C, row=ptrs(), m=L.ptr(m), v=L.ptr(v), g=L.ptr(g), lr=1e-3, beta1=0.5, beta2=0.9, eps=1e-8,
              bc1=0.5, bc2=0.1, sumsq=L.ptr(sq), max_norm=5.0)
    for change in (dict(emb_sum=None), dict(m=None), dict(v=None), dict(g=None), dict(sumsq=None), dict(row=ptrs(3)), dict(B=0), dict(C=0),
                   dict(C=20000), dict(bc1=0.0), dict(bc2=0.0)):
        with pytest.raises(L.ZsError, match='zs_voice_adam'):
            L.call('zs_voice_adam', 'ZsVoiceAdam', _stream(), **dict(ok, **change))
    torch.cuda.synchronize()
    assert all(bool((x == 5.0).all()) for x in (rows, m, v, g, sq))
    L.call('zs_voice_adam', 'ZsVoiceAdam', _stream(), **ok)                    # host-side bias corrections
    torch.cuda.synchronize()
    assert float(sq.item()) == pytest.approx(5 * C * (5.0 * B) ** 2, rel=1e-6) and bool((g == 5.0 * B).all())


# ---- a small decoder and a synthetic set --------------------------------------------------------------------------------------------------
def _decoder(dev, dtype, F=80, c_h=64, E=8, n_spk=3, seed=0, seg=SEG):
    from zs_amd.model import Decoder
    torch.manual_seed(seed)
    return Decoder(c_in=E, c_out=F, c_h=c_h, c_a=n_spk, ns=0.01, seg_len=seg, dtype=dtype).to(dev)


def _vset(dev, F=80, E=8, lens=(300, 128, 200, 90), seed=0, seg=SEG, n_items=64):
    """Random spectrograms in (0, 1) and random units; the utterance of 90 frames is left out."""
    from zs_amd import voice
    rng = np.random.RandomState(seed)
    specs = [(rng.rand(n, F) * 0.98 + 1e-3).astype(np.float32) for n in lens]
    units = [rng.randint(0, 2, size=((n - 1) // 8 if n > seg else (n + 7) // 8, E)).astype(np.float32) for n in lens]
    packed = [np.packbits(u != 0, axis=1, bitorder='little') for u in units]
    return voice.VoiceSet(specs, packed, seg, dev, n_items=n_items, seed=seed), specs, units


def test_voice_set_serves_the_planned_segments(dev):
    from zs_amd import voice
    vs, specs, units = _vset(dev, F=513, seed=4)
    assert vs.left_out == [3] and vs.kept == [0, 1, 2] and vs.n == 64 and vs.n_frames_kept == 628
    dec = _decoder(dev, 'fp32', F=513)
    st = voice.VoiceStep(dec, vs, 3, voice.init_rows(dec.state_dict()), use_graph=False)
    pool, packed = vs.pool.cpu().numpy(), vs.packed.cpu().numpy()
    for k in range(3):
        bits = st.gather()
        x, b = st.x.cpu().numpy(), bits.valid().float().cpu().numpy()
        for i in range(3):
            it = (3 * k + i) % vs.n
            f, u = int(vs.first[it]), int(vs.ufirst[it])
            assert np.array_equal(x[i], pool[f:f + SEG])
            assert np.array_equal(b[i], np.unpackbits(packed[u:u + SEG // 8], axis=1, count=8, bitorder='little'))
            # ... and these are rows of one utterance, its units those of its frames
            j = [j for j in range(3) if any(np.array_equal(x[i][0], r) for r in specs[j][::8])]
            assert len(j) == 1
            t = int(np.nonzero((specs[j[0]] == x[i][0]).all(axis=1))[0][0])
            assert t % 8 == 0 and np.array_equal(x[i], specs[j[0]][t:t + SEG]) and np.array_equal(b[i], units[j[0]][t // 8:t // 8 + SEG // 8])
    assert int(st.cursor.item()) == 3
    with pytest.raises(ValueError, match='no utterance'):
        voice.VoiceSet(specs[3:], [np.zeros((12, 2), np.uint8)], SEG, dev)


# ---- 3. backward(param_grads=False) -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype, F', [('fp32', 80), ('bf16', 513), ('fp32', 513), ('bf16', 80)])
def test_backward_without_param_grads(dev, dtype, F):
    from zs_amd import voice
    vs, _, _ = _vset(dev, F=F, seed=1)
    dec = _decoder(dev, dtype, F=F)
    st = voice.VoiceStep(dec, vs, 4, voice.init_rows(dec.state_dict(), 1), use_graph=False)
    de = st.de
    gflat = st.dec.flat_params()[1]

    def run(param_grads):
        bits = st.gather(advance=0)
        dl = st.l1_loss(de.forward(bits, st.cidx, True))
        de.backward(dl, need_dbits=False, param_grads=param_grads)
        torch.cuda.synchronize()
        return de._embsum.clone()

    full = run(True)
    assert bool((gflat != 0).any())                                          # the full backward writes the gradients
    gflat.fill_(-77.0)
    torch.cuda.synchronize()
    mine = run(False)
    assert torch.equal(mine, full) and bool((full[:5 * 4 * 64] != 0).any())
    assert bool((gflat == -77.0).all())                                      # no gradient buffer written, the embedding tables' included
    again = run(True)
    assert torch.equal(again, full) and not bool((gflat == -77.0).all())


# ---- 4. one iteration against the oracle ---------------------------------------------------------------------------------------------------
def _oracle_step(sd, rows, enc_act, x_bft, lr, max_norm, adam=None):
    """loss, row gradients, clipped update of the five rows in the oracle: decoder_forward with the rows as speaker 0, l1_loss,
    clip_grad_norm over the five rows together, AdamState."""
    import zs_oracle as O
    rows = [r.clone().requires_grad_(True) for r in rows]
    sd1 = dict(sd)
    for k, r in enumerate(rows):
        sd1['emb%d.weight' % (k + 1)] = r.reshape(1, -1)
    c = torch.zeros(enc_act.shape[0], dtype=torch.int64)
    xdec = O.decoder_forward(sd1, enc_act, c, 0.01, SEG)
    loss = O.l1_loss(xdec, x_bft)
    grads = torch.autograd.grad(loss, rows)
    adam = adam or O.AdamState(rows, lr=lr, betas=(0.5, 0.9))
    _, clipped = O.clip_grad_norm(grads, max_norm)
    new = adam.update([r.detach() for r in rows], clipped)
    return float(loss.detach()), xdec.detach(), [g.detach() for g in grads], new, adam


MARGIN = 2e-3


def _separate_targets(vs, sd, rows0, B):
    """The gradient of mean |x_dec - x| is sign(x_dec - x): where a target lies closer to the output than the output's own error,
    device and oracle may take opposite signs.  That is a property of the loss, not of a kernel, so the targets of the first batch
    are moved until every one is at least 2 MARGIN from the oracle's output (MARGIN = 2e-3 is twice the forward bound of 1e-3 of the
    scale, which is below 1) -- the conditioning tests/test_gpu_convert_dir.py applies to its trim thresholds.  Changes the set's
    pool in place."""
    import zs_oracle as O
    pool = vs.pool.cpu()
    sd1 = dict(sd)
    for k, r in enumerate(rows0):
        sd1['emb%d.weight' % (k + 1)] = r.reshape(1, -1)
    packed = vs.packed.cpu().numpy()
    U = SEG // 8
    bits = torch.from_numpy(np.stack([np.unpackbits(packed[int(vs.ufirst[b]):int(vs.ufirst[b]) + U], axis=1, count=8, bitorder='little')
                                      for b in range(B)]).astype(np.float32))
    with torch.no_grad():
        xd = O.decoder_forward(sd1, bits.permute(0, 2, 1), torch.zeros(B, dtype=torch.int64), 0.01, SEG).permute(0, 2, 1)     # [B, SEG, F]
    for _ in range(4):                                   # (overlapping segments share pool rows: repeat until nothing is near)
        moved = 0
        for b in range(B):
            seg = pool[int(vs.first[b]):int(vs.first[b]) + SEG]
            near = (xd[b] - seg).abs() < 2 * MARGIN
            seg[near] = xd[b][near] + 4 * MARGIN
            moved += int(near.sum())
        if not moved:
            break
    assert all(((xd[b] - pool[int(vs.first[b]):int(vs.first[b]) + SEG]).abs() >= 2 * MARGIN).all() for b in range(B))
    vs.pool.copy_(pool)


@pytest.mark.parametrize('F, seed', [(80, 6), (513, 6), (513, 8), (80, 9)])
def test_one_step_against_the_oracle(dev, F, seed):
    """Bounds of tests/test_gpu_model.py: the output within 1e-3 of its scale, each row's gradient within 2e-3 of its scale, on
    targets that are not within the output's error of the output (_separate_targets) and on weights at which the fp32 oracle is
    itself trustworthy: the leaky-ReLU kinks make the gradient discontinuous too, and at one of the seeds tried (decoder seed 5,
    F = 513) the fp32 oracle is 2.4e-3 to 5.5e-3 of scale from the same oracle run in fp64 -- as far as the device was from it
    (2.4e-3 on emb1) -- against 1e-5 at every other seed.  So the test asserts that the fp32 oracle is within 2e-4 of scale (a tenth
    of the bound) of the fp64 one before it compares the device with it.  The
    update is checked in two parts, so that a gradient element near zero (whose sign decides a first Adam step of +-lr) cannot
    fail it: the oracle's AdamState fed the device's own gradient must give the device's rows to within 1e-3 of the step size lr
    (fp32 rounding of the update's few operations is some 1e-6 of it) plus one ulp of the row."""
    import zs_oracle as O
    from zs_amd import voice
    vs, _, _ = _vset(dev, F=F, seed=2)
    dec = _decoder(dev, 'fp32', F=F, seed=seed)
    sd = {k: v.detach().cpu().clone() for k, v in dec.state_dict().items()}
    rows0 = voice.init_rows(sd)
    lr, max_norm = 1e-2, 0.002
    _separate_targets(vs, sd, rows0, 2)
    st = voice.VoiceStep(dec, vs, 2, rows0, lr=lr, max_grad_norm=max_norm, use_graph=False)
    xdec = st.forward_backward()
    st.adam()
    torch.cuda.synchronize()
    bits = st.de.tape['bits'].valid().float().cpu()                            # [B, T', E]
    x = st.x.cpu()
    loss, o_xdec, o_g, _, _ = _oracle_step(sd, rows0, bits.permute(0, 2, 1), x.permute(0, 2, 1), lr, max_norm)
    e = (xdec.valid().cpu().permute(0, 2, 1) - o_xdec).abs().max().item() / o_xdec.abs().max().item()
    print('F %d: x_dec rel err %.3g, loss %.6f (oracle %.6f)' % (F, e, float(st._loss.item()), loss))
    assert e < 1e-3
    assert (o_xdec - x.permute(0, 2, 1)).abs().min().item() >= MARGIN
    assert abs(float(st._loss.item()) - loss) <= 1e-3 * o_xdec.abs().max().item()     # a mean of |x_dec - x|: no further than x_dec is
    g = st.g.cpu().reshape(5, -1)
    _, _, o_g64, _, _ = _oracle_step({k: v.double() for k, v in sd.items()}, [r.double() for r in rows0], bits.double().permute(0, 2, 1),
                                     x.double().permute(0, 2, 1), lr, max_norm)
    for k in range(5):
        scale = o_g[k].abs().max().item()
        assert (o_g[k].double() - o_g64[k]).abs().max().item() <= 2e-4 * scale, 'the fp32 oracle is ill-conditioned here (emb%d)' % (k + 1)
        ek = (g[k] - o_g[k]).abs().max().item() / scale
        print('  emb%d gradient rel err %.3g (scale %.3g)' % (k + 1, ek, scale))
        assert scale > 1e-6 and ek < 2e-3
    nrm = float(torch.sqrt((g.double() ** 2).sum()))
    assert abs(float(st.sumsq.item()) ** 0.5 - nrm) < 1e-5 * nrm
    print('  gradient norm %.4g, max_norm %.3g' % (nrm, max_norm))
    assert nrm > max_norm                                                       # the clip is active in this step
    adam = O.AdamState(rows0, lr=lr, betas=(0.5, 0.9))
    _, clipped = O.clip_grad_norm([g[k] for k in range(5)], max_norm)
    want = adam.update(rows0, clipped)
    for k, r in enumerate(st.rows()):
        d = np.abs(r - want[k].numpy())
        assert (d <= 1e-3 * lr + np.abs(want[k].numpy()) * 2.0 ** -23).all(), (k, d.max())
        assert np.abs(r - rows0[k].numpy()).max() > 0.5 * lr                    # the rows moved, by a first Adam step
    assert int(st._step_dev.item()) == 1 and int(st.cursor.item()) == 1        # (zs_step_counters is _launches' last call)


# ---- 5. eager against captured ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_eager_equals_captured(dev, dtype):
    """Six iterations: eager; two eager + capture + four replays, the loss read after every one; the same with the loss read once."""
    from zs_amd import voice
    vs, _, _ = _vset(dev, F=80, seed=3)
    dec = _decoder(dev, dtype, seed=7)
    rows0 = voice.init_rows(dec.state_dict())
    mk = lambda graph: voice.VoiceStep(dec, vs, 3, rows0, lr=1e-2, max_grad_norm=0.002, use_graph=graph)
    a, b, c = mk(False), mk(True), mk(True)
    la = a.run(6, log_every=1)
    lb = b.run(6, log_every=1)
    lc = c.run(6, log_every=0)
    torch.cuda.synchronize()
    assert b._graph is not None and c._graph is not None and a._graph is None
    assert [i for i, _ in la] == [1, 2, 3, 4, 5, 6] and la == lb and lc == [la[-1]]
    assert len({l for _, l in la}) == 6 and all(np.isfinite(l) for _, l in la)
    for s in (b, c):
        assert all(np.array_equal(x, y) for x, y in zip(a.rows(), s.rows()))
        assert torch.equal(a.m, s.m) and torch.equal(a.v, s.v) and torch.equal(a.cursor, s.cursor) and torch.equal(a._step_dev, s._step_dev)
    assert int(a.cursor.item()) == 6 and int(a._step_dev.item()) == 7 and bool((a.m != 0).any())
    # the decoder the steps were made from was never written
    assert all(torch.equal(v, dec.state_dict()[k]) for k, v in a.dec.state_dict().items() if k not in voice.EMB_KEYS)


# ---- 7. a planted voice ------------------------------------------------------------------------------------------------------------------------
PLANT = dict(seed=2, K=24, lr=0.1, n_utt=4, B=4, c_h=32, E=8, F=80, max_norm=5.0)


def _planted(seed, n_utt, c_h, E, F):
    """A random small decoder (CPU state dict), random units of n_utt utterances of exactly SEG frames, and their spectrograms as the
    oracle decodes them with a hidden row set."""
    import zs_oracle as O
    from zs_amd.model import Decoder
    torch.manual_seed(seed)
    sd = {k: v.detach().clone() for k, v in Decoder(c_in=E, c_out=F, c_h=c_h, c_a=4, ns=0.01, seg_len=SEG, dtype='fp32').state_dict().items()}
    g = torch.Generator().manual_seed(seed + 100)
    hidden = [torch.randn(c_h, generator=g) for _ in range(5)]
    units = (torch.rand(n_utt, SEG // 8, E, generator=g) < 0.5).float()
    sd1 = dict(sd)
    for k, r in enumerate(hidden):
        sd1['emb%d.weight' % (k + 1)] = r.reshape(1, -1)
    with torch.no_grad():
        x = O.decoder_forward(sd1, units.permute(0, 2, 1), torch.zeros(n_utt, dtype=torch.int64), 0.01, SEG)       # [n, F, SEG]
    return sd, units, x.permute(0, 2, 1).contiguous()


def _oracle_run(sd, rows0, units, x, items, B, K, lr, max_norm):
    """K iterations in the oracle over the batch sequence of the item table: the losses."""
    rows, adam, losses = [r.clone() for r in rows0], None, []
    for k in range(K):
        it = [items[(k * B + b) % len(items)] for b in range(B)]
        loss, _, _, rows, adam = _oracle_step(sd, rows, units[it].permute(0, 2, 1), x[it].permute(0, 2, 1), lr, max_norm, adam)
        losses.append(loss)
    return losses


def test_planted_voice_is_recovered(dev):
    """Targets decoded by the oracle from a hidden row set; adaptation from the mean of the table's rows.  The same K iterations run in
    the oracle on the CPU, over the same batches: its loss must fall by at least 20 % (seed, K and lr were chosen for that on the
    CPU), and the device's loss by at least half of that relative fall."""
    from zs_amd import voice
    from zs_amd.model import Decoder
    P = PLANT
    sd, units, x = _planted(P['seed'], P['n_utt'], P['c_h'], P['E'], P['F'])
    packed = [np.packbits(u.numpy() != 0, axis=1, bitorder='little') for u in units]
    vs = voice.VoiceSet([s.numpy() for s in x], packed, SEG, dev, n_items=32, seed=P['seed'])
    assert vs.left_out == [] and not (vs.first % SEG).any()
    items = (vs.first // SEG).tolist()
    rows0 = voice.init_rows(sd)
    o = _oracle_run(sd, rows0, units, x, items, P['B'], P['K'] + 1, P['lr'], P['max_norm'])
    o_fall = (o[0] - o[-1]) / o[0]
    print('oracle: loss %.5f -> %.5f after %d iterations, a fall of %.1f %%' % (o[0], o[-1], P['K'], 100 * o_fall))
    assert o_fall >= 0.20
    dec = Decoder(c_in=P['E'], c_out=P['F'], c_h=P['c_h'], c_a=4, ns=0.01, seg_len=SEG, dtype='fp32').to(dev)
    dec.load_state_dict(sd)
    st = voice.VoiceStep(dec, vs, P['B'], rows0, lr=P['lr'], max_grad_norm=P['max_norm'])
    hist = st.run(P['K'] + 1, log_every=1)                                       # the loss of iteration k is taken before its update
    g = [l for _, l in hist]
    g_fall = (g[0] - g[-1]) / g[0]
    print('device: loss %.5f -> %.5f, a fall of %.1f %%' % (g[0], g[-1], 100 * g_fall))
    assert abs(g[0] - o[0]) < 1e-3 * o[0]                                       # the same start: the first loss precedes every update
    assert g_fall >= 0.5 * o_fall


# ---- 6. and 8.: a trainer, a checkpoint, wav files --------------------------------------------------------------------------------------------
SEG_E2E = 32


def _trainer(tmp_path, seed=0):
    from zs_amd.hps import make_hps
    from zs_amd.trainer import Trainer
    torch.manual_seed(seed)
    hps = make_hps(enc_size=8, emb_size=32, n_speakers=4, n_target_speakers=2, seg_len=SEG_E2E, batch_size=4)
    return Trainer(hps, None, 'targeted_residual', 'multilabel_binary', log_dir=str(tmp_path / 'log'), dtype='fp32',
                   device=torch.device('cuda:0')), hps


def _voiced(rng, n, lead, trail, f0=300.0, sr=16000):
    t = np.arange(n) / float(sr)
    y = 0.3 * np.sin(2 * np.pi * f0 * t) + 0.1 * np.sin(2 * np.pi * 2.7 * f0 * t) + 0.01 * rng.randn(n)
    y[:lead] = 0.0
    if trail:
        y[n - trail:] = 0.0
    return y.astype(np.float32)


def _folder(tmp_path):
    from scipy.io import wavfile
    rng = np.random.RandomState(41)
    d = tmp_path / 'in'
    d.mkdir()
    wavfile.write(str(d / 'a16.wav'), 16000, (_voiced(rng, 15000, 2000, 1500, sr=16000) * 32767).astype(np.int16))
    wavfile.write(str(d / 'b22.wav'), 22050, _voiced(rng, 24000, 1000, 3000, sr=22050, f0=210.0))
    wavfile.write(str(d / 'one.wav'), 16000, np.array([1000], dtype=np.int16))             # too short after trimming: left out
    wavfile.write(str(d / 'short.wav'), 16000, _voiced(rng, 3000, 0, 0))                     # fewer than seg_len frames: left out
    s2id = tmp_path / 'speaker2id.json'
    s2id.write_text(json.dumps({'S015': 0, 'S020': 1, 'V001': 2, 'V002': 3}))
    return d, str(s2id)


def _field_noise(E, seed=1234, T=64):
    U = torch.rand(T, E, 2, generator=torch.Generator().manual_seed(seed))
    base = (-torch.log(-torch.log(U + 1e-20) + 1e-20)).cuda()

    def noise_fn(n, t, e):
        assert e == E and t <= base.shape[0]
        return base[:t].unsqueeze(0).expand(n, t, E, 2).contiguous()
    return noise_fn


def test_adaptation_leaves_the_trainer_frozen(dev, tmp_path, capsys):
    from zs_amd import preprocess as P, voice
    tr, hps = _trainer(tmp_path, seed=2)
    d, _ = _folder(tmp_path)
    before = {n: {k: v.detach().clone() for k, v in net.state_dict().items()} for n, net in (('enc', tr.Encoder), ('dec', tr.Decoder))}
    wavs = [P.read_wav(str(d / n)) for n in ('a16.wav', 'b22.wav', 'one.wav', 'short.wav')]
    path, meta = voice.adapt(tr, SEG_E2E, None, 'NEW', str(tmp_path / 'voices'), speaker2id={'V001': 2}, iters=6, init='V001', lr=1e-2,
                             log_every=2, wavs=wavs)
    torch.cuda.synchronize()
    for n, net in (('enc', tr.Encoder), ('dec', tr.Decoder)):
        sd = net.state_dict()
        assert set(sd) == set(before[n]) and all(torch.equal(sd[k], v) for k, v in before[n].items()), n
    assert tr.Decoder.c_a == 4 and not tr.Decoder.training
    rows, m2 = voice.load_voice(path, c_h=32, digest=voice.decoder_digest(tr.Decoder.state_dict()))
    assert m2 == meta and meta['iterations'] == 6 and meta['init'] == 'V001' and meta['utterances'] == 2 and meta['left_out'] == 2
    assert meta['seg_len'] == SEG_E2E and meta['frames'] > 2 * SEG_E2E and np.isfinite(meta['final_loss'])
    start = voice.init_rows(tr.Decoder.state_dict(), 2)
    assert all(r.shape == (32,) and np.isfinite(r).all() and np.abs(r - s.numpy()).max() > 1e-3 for r, s in zip(rows, start))
    out = capsys.readouterr().out
    assert 'left out' in out and out.count('loss_rec') == 3                      # iterations 2, 4 and 6
    with pytest.raises(ValueError, match='already'):
        voice.adapt(tr, SEG_E2E, None, 'V001', str(tmp_path / 'voices'), speaker2id={'V001': 2}, iters=1, wavs=wavs)
    with pytest.raises(ValueError, match='nothing to adapt to'):
        voice.adapt(tr, SEG_E2E, None, 'X', str(tmp_path / 'voices'), iters=1, wavs=wavs[3:])
    assert os.listdir(str(tmp_path / 'voices')) == ['NEW.voice.npz']


def test_adapt_voice_then_convert_end_to_end(dev, tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import main as M
    from zs_amd import convert as cv, preprocess as P, voice
    from zs_amd.hps import hp
    d, s2id = _folder(tmp_path)
    tr, hps = _trainer(tmp_path, seed=5)
    hps_path = str(tmp_path / 'hps.json')
    json.dump(hps._asdict(), open(hps_path, 'w'))
    tr.save_model(str(tmp_path / 'model.pth'), 's2', 1)
    ckpt = str(tmp_path / 'model.pth-s2-1')
    monkeypatch.setattr(hp, 'n_iter', 4)
    common = ['--hps_path', hps_path, '--speaker2id_path', s2id, '--ckpt_pth', ckpt, '--g_mode', 'targeted_residual']
    files = lambda: sorted(os.listdir(str(tmp_path)))
    listed, ckpt_bytes = files(), open(ckpt, 'rb').read()
    # the same command twice: the same rows, bit for bit
    for vd in ('v1', 'v2'):
        M.main(['--adapt_voice', 'NEW', '--adapt_dir', str(d), '--adapt_iters', '6', '--adapt_lr', '0.01', '--voice_dir', str(tmp_path / vd)] + common)
    r1, m1 = voice.load_voice(str(tmp_path / 'v1' / 'NEW.voice.npz'))
    r2, m2 = voice.load_voice(str(tmp_path / 'v2' / 'NEW.voice.npz'))
    assert m1 == m2 and all(np.array_equal(a, b) for a, b in zip(r1, r2)) and m1['init'] == 'mean' and m1['utterances'] == 2
    # nothing else was written: the checkpoint, hps and speaker2id files are as they were
    assert files() == sorted(listed + ['v1', 'v2']) and open(ckpt, 'rb').read() == ckpt_bytes
    vfile = str(tmp_path / 'v1' / 'NEW.voice.npz')
    # conversion and synthesis with the voice as a target beside a table speaker
    res = tmp_path / 'result'
    M.main(['--convert_dir', str(d), '--enc_only', '--voice', 'NEW=' + vfile, '--t_speaker', 'NEW,V001', '--result_dir', str(res)] + common)
    out = os.path.join(os.path.join(str(res), './english/'), 'convert')
    man = json.load(open(os.path.join(out, 'convert_dir.json')))
    assert man['targets'] == ['NEW', 'V001'] and man['voices'] == {'NEW': 4} and man['enc_only'] is True
    for t in ('NEW', 'V001'):
        assert sorted(os.listdir(os.path.join(out, t))) == ['a16.txt', 'a16.wav', 'b22.txt', 'b22.wav', 'short.txt', 'short.wav']
    units = tmp_path / 'units'
    units.mkdir()
    os.replace(os.path.join(out, 'NEW', 'a16.txt'), str(units / 'a16.txt'))
    M.main(['--synth_dir', str(units), '--enc_only', '--voice', 'NEW=' + vfile, '--t_speaker', 'NEW', '--result_dir', str(res)] + common)
    sman = json.load(open(os.path.join(str(res), './english/', 'synth', 'synth_dir.json')))
    assert sman['voices'] == {'NEW': 4} and os.path.getsize(os.path.join(str(res), './english/', 'synth', 'NEW', 'a16.wav')) > 44
    # a voice with the generator, and a voice fitted to other weights, are refused
    with pytest.raises(ValueError, match='enc_only'):
        M.main(['--convert_dir', str(d), '--voice', 'NEW=' + vfile, '--t_speaker', 'NEW', '--result_dir', str(res)] + common)
    tr_other, _ = _trainer(tmp_path, seed=6)
    with pytest.raises(ValueError, match='digest'):
        voice.add_voices(tr_other, {'NEW': vfile})
    assert tr_other.Decoder.c_a == 4
    # the spectrograms: NEW is the decoder with a table row overwritten by the file's rows; V001 is what it is without voices
    tr_v = cv.get_trainer(hps_path, ckpt, 'targeted_residual', 'multilabel_binary')
    tr_0 = cv.get_trainer(hps_path, ckpt, 'targeted_residual', 'multilabel_binary')
    old = tr_v.Decoder
    ids = voice.add_voices(tr_v, {'NEW': vfile})
    assert ids == {'NEW': 4} and tr_v.voices == {'NEW': 4} and tr_v.Decoder.c_a == 5 and tr_v.Decoder is not old
    sd_v, sd_0 = tr_v.Decoder.state_dict(), tr_0.Decoder.state_dict()
    for k in sd_0:
        assert torch.equal(sd_v[k][:4] if k in voice.EMB_KEYS else sd_v[k], sd_0[k]), k
    wavs = [P.read_wav(str(d / n)) for n in ('a16.wav', 'b22.wav', 'short.wav')]
    specs, _ = cv._wav_features([w for w, _ in wavs], [r for _, r in wavs], dev)
    noise = lambda: _field_noise(8)
    _, new_v = cv.encode_batch(specs, tr_v, SEG_E2E, decode_speakers=[4, 4, 4], noise_fn=noise())
    _, v001_v = cv.encode_batch(specs, tr_v, SEG_E2E, decode_speakers=[2, 2, 2], noise_fn=noise())
    _, v001_0 = cv.encode_batch(specs, tr_0, SEG_E2E, decode_speakers=[2, 2, 2], noise_fn=noise())
    with torch.no_grad():
        for i, k in enumerate(voice.EMB_KEYS):
            dict(tr_0.Decoder.named_parameters())[k][1].copy_(torch.from_numpy(r1[i]))
    tr_0.Decoder.mark_dirty()
    _, new_0 = cv.encode_batch(specs, tr_0, SEG_E2E, decode_speakers=[1, 1, 1], noise_fn=noise())
    for a, b, c, e in zip(new_v, new_0, v001_v, v001_0):
        assert a.shape == b.shape == c.shape and np.array_equal(a, b) and np.array_equal(c, e) and not np.array_equal(a, c)
