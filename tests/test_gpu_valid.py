"""Held-out validation on the GPU: zs_eval_accum against fp64 numpy, the validation value against the oracle and the public modules,
and the Trainer surface -- above all that a run with validation computes, bit for bit, what it computes without.

Trainer cases are six-iteration runs on small nets (the hps of tests/test_gpu_resume.py) with a validation of two batches of four
segments every two iterations."""
import ctypes
import io
import json
import os
import shutil
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS, M, B = 6, 2, 4


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


# ---- zs_eval_accum ---------------------------------------------------------------------------------------------------------------
class _Tables(object):
    def __init__(self, dev, B, n_spk, E):
        from zs_amd import _lib as L
        self.work = torch.full((B * L.ZS_EVAL_PARTS,), float('nan'), dtype=torch.float64, device=dev)     # scratch: never read before written
        self.spk_sum = torch.zeros(n_spk, dtype=torch.float64, device=dev)
        self.spk_cnt = torch.zeros(n_spk, dtype=torch.int64, device=dev)
        self.ones = torch.zeros(max(E, 1), dtype=torch.int64, device=dev)
        self.flips = torch.zeros(max(E, 1), dtype=torch.int64, device=dev)
        self.words = torch.zeros(3, dtype=torch.int64, device=dev)             # rows, pairs, bad

    def host(self):
        torch.cuda.synchronize()
        w = self.words.cpu().numpy()
        return dict(spk_sum=self.spk_sum.cpu().numpy(), spk_cnt=self.spk_cnt.cpu().numpy(), ones=self.ones.cpu().numpy(),
                    flips=self.flips.cpu().numpy(), rows=int(w[0]), pairs=int(w[1]), bad=int(w[2]))


def _struct(t, xdec, x, c, n_spk, bits, F, over=()):
    """The ZsEvalAccum of one call: xdec [B, T, ld_dec], x [B, T, ldx] (F valid columns), bits [B, T4, E] or None."""
    from zs_amd import _lib as L
    Bn, T = xdec.shape[:2]
    kw = dict(x_dec=L.ptr(xdec), ld_dec=xdec.shape[2], x=L.ptr(x), ldx=x.shape[2], c=L.ptr(c), B=Bn, T=T, F=F, n_speakers=n_spk,
              work=L.ptr(t.work), spk_sum=L.ptr(t.spk_sum), spk_cnt=L.ptr(t.spk_cnt), bad=L.ptr(t.words, 2))
    if bits is not None:
        kw.update(bits_f32=L.ptr(bits), T4=bits.shape[1], E=bits.shape[2], ones=L.ptr(t.ones), flips=L.ptr(t.flips),
                  rows=L.ptr(t.words, 0), pairs=L.ptr(t.words, 1))
    kw.update(dict(over))
    return L.STRUCTS['ZsEvalAccum'](**{k: v for k, v in kw.items() if v is not None})


def _call(s):
    from zs_amd import _lib as L
    fn = L.lib().zs_eval_accum
    return fn(ctypes.addressof(s), torch.cuda.current_stream().cuda_stream)


def _reference(xdec, x, c, n_spk, bits, F):
    """fp64 numpy on the exact fp32 inputs (host arrays)."""
    d = np.abs(xdec[:, :, :F].astype(np.float64) - x[:, :, :F].astype(np.float64)).sum(axis=(1, 2))
    spk_sum, spk_cnt, bad = np.zeros(n_spk), np.zeros(n_spk, dtype=np.int64), 0
    for b, s in enumerate(c):
        if 0 <= s < n_spk:
            spk_sum[s] += d[b]
            spk_cnt[s] += 1
        else:
            bad += 1
    out = dict(spk_sum=spk_sum, spk_cnt=spk_cnt, bad=bad)
    if bits is not None:
        on = bits != 0
        out.update(ones=on.sum(axis=(0, 1)), flips=(on[:, 1:] != on[:, :-1]).sum(axis=(0, 1)), rows=on.shape[0] * on.shape[1],
                   pairs=on.shape[0] * (on.shape[1] - 1))
    return out


SHAPES = {  # B, T, F, n_speakers, c, E, T4
    'odd_F_ordered_pass': (5, 9, 513, 7, [3, 0, 3, 6, 3], 10, 2),             # speaker 3 three times, 1 2 4 5 absent
    'training_T4': (3, 128, 80, 4, [1, 0, 1], 1024, 16),
    'no_pairs': (1, 1, 1, 1, [0], 1, 1),
}


def _inputs(dev, name, seed=0):
    Bn, T, F, n_spk, c, E, T4 = SHAPES[name]
    g = torch.Generator().manual_seed(seed)
    ld_dec, ldx = F + 7, F + 3                                                 # both > F; rows of x not 16-byte aligned
    xdec = torch.rand(Bn, T, ld_dec, generator=g) * 1.3 - 0.1                  # (not multiples of 2^-24: the fp32 difference rounds)
    x = torch.rand(Bn, T, ldx, generator=g) / 3.0
    xdec[:, :, F:] = float('nan')                                              # a kernel that reads the padding columns fails
    x[:, :, F:] = 1e30
    bits = (torch.rand(Bn, T4, E, generator=g) < 0.3).float()
    if E >= 4:
        bits[:, :, 0] = 0.0                                                    # a dead unit, an always-on one, one that flips at every frame
        bits[:, :, 1] = 1.0
        bits[:, :, 2] = (torch.arange(T4) % 2).float()[None, :]
    return xdec.to(dev), x.to(dev), torch.tensor(c, dtype=torch.int64, device=dev), n_spk, bits.to(dev), F


@pytest.mark.parametrize('name', list(SHAPES))
def test_eval_accum_against_fp64(dev, name):
    xdec, x, c, n_spk, bits, F = _inputs(dev, name)
    ref = _reference(xdec.cpu().numpy(), x.cpu().numpy(), c.cpu().numpy(), n_spk, bits.cpu().numpy(), F)
    t = _Tables(dev, xdec.shape[0], n_spk, bits.shape[2])
    assert _call(_struct(t, xdec, x, c, n_spk, bits, F)) == 0
    one = t.host()
    E = bits.shape[2]
    # each term is one fp32 subtraction (relative error <= 2^-24 = 6e-8), the sums are in double: 1e-6 leaves more than 10x
    nz = ref['spk_sum'] != 0
    rel = (np.abs(one['spk_sum'] - ref['spk_sum'])[nz] / ref['spk_sum'][nz]).max()           # per speaker
    print('%s: spk_sum max relative error %.3g' % (name, rel))
    assert rel <= 1e-6
    assert np.array_equal(one['spk_sum'] == 0, ref['spk_cnt'] == 0)              # absent speakers stay exactly zero
    assert np.array_equal(one['spk_cnt'], ref['spk_cnt']) and one['bad'] == 0
    assert np.array_equal(one['ones'][:E], ref['ones']) and np.array_equal(one['flips'][:E], ref['flips'])
    assert one['rows'] == ref['rows'] and one['pairs'] == ref['pairs']
    if name == 'no_pairs':
        assert one['pairs'] == 0 and one['flips'][0] == 0
    if E >= 4:
        T4 = bits.shape[1]
        assert one['ones'][0] == 0 and one['ones'][1] == one['rows'] and one['flips'][2] == xdec.shape[0] * (T4 - 1)
    # a second call accumulates: twice the integers, the summed doubles
    assert _call(_struct(t, xdec, x, c, n_spk, bits, F)) == 0
    two = t.host()
    for k in ('spk_cnt', 'ones', 'flips', 'rows', 'pairs'):
        assert np.array_equal(np.asarray(two[k]), 2 * np.asarray(one[k])), k
    assert (np.abs(two['spk_sum'] - 2 * ref['spk_sum'])[nz] / (2 * ref['spk_sum'][nz])).max() <= 1e-6 and not two['spk_sum'][~nz].any()
    # fresh tables: identical bits (no floating-point atomics, a fixed order)
    t2 = _Tables(dev, xdec.shape[0], n_spk, E)
    assert _call(_struct(t2, xdec, x, c, n_spk, bits, F)) == 0
    again = t2.host()
    assert again['spk_sum'].tobytes() == one['spk_sum'].tobytes()
    # without bits_f32 the unit tables are left alone
    t3 = _Tables(dev, xdec.shape[0], n_spk, E)
    assert _call(_struct(t3, xdec, x, c, n_spk, None, F)) == 0
    plain = t3.host()
    assert plain['spk_sum'].tobytes() == one['spk_sum'].tobytes() and plain['rows'] == 0 and plain['pairs'] == 0 and not plain['ones'].any()


def test_eval_accum_skips_speaker_ids_outside_the_tables(dev):
    xdec, x, c, n_spk, bits, F = _inputs(dev, 'odd_F_ordered_pass')
    t = _Tables(dev, 5, n_spk, 10)
    assert _call(_struct(t, xdec, x, c, n_spk, bits, F)) == 0
    good = t.host()
    c_bad = c.clone()
    c_bad[1], c_bad[3] = -1, n_spk                                             # speakers 0 and 6 lose their only sample
    t2 = _Tables(dev, 5, n_spk, 10)
    assert _call(_struct(t2, xdec, x, c_bad, n_spk, bits, F)) == 0
    got = t2.host()
    assert got['bad'] == 2 and list(got['spk_cnt']) == [0, 0, 0, 3, 0, 0, 0]
    assert got['spk_sum'][3].tobytes() == good['spk_sum'][3].tobytes() and got['spk_sum'][0] == 0 and got['spk_sum'][6] == 0
    assert np.array_equal(got['ones'], good['ones']) and got['rows'] == good['rows']
    from zs_amd import validation
    with pytest.raises(ValueError, match='speaker id'):                        # the host raises after the D2H
        validation.finish(got, 9, F)


def test_eval_accum_refuses_malformed_structs(dev):
    from zs_amd import _lib as L
    xdec, x, c, n_spk, bits, F = _inputs(dev, 'odd_F_ordered_pass')
    t = _Tables(dev, 5, n_spk, 10)
    fn = L.lib().zs_eval_accum
    assert fn(None, None) == L.ZS_EINVAL
    for over in (dict(x_dec=0), dict(x=0), dict(c=0), dict(work=0), dict(spk_sum=0), dict(spk_cnt=0), dict(bad=0), dict(B=0), dict(B=-1),
                 dict(T=0), dict(F=0), dict(F=-3), dict(ld_dec=F - 1), dict(ldx=F - 1), dict(n_speakers=0), dict(n_speakers=-2),
                 dict(ones=0), dict(flips=0), dict(rows=0), dict(pairs=0), dict(T4=0), dict(E=0)):
        assert _call(_struct(t, xdec, x, c, n_spk, bits, F, over)) == L.ZS_EINVAL, over
        assert 'zs_eval_accum' in L.last_error()
    got = t.host()
    assert not got['spk_cnt'].any() and got['rows'] == 0 and got['bad'] == 0     # nothing was launched


# ---- the Trainer surface ---------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _cadence(monkeypatch):
    monkeypatch.setenv('ZS_CKPT_EVERY', '2')
    monkeypatch.setenv('ZS_LOG_EVERY', '1')


def _hps(iters=ITERS, **kw):
    from zs_amd.hps import make_hps
    d = dict(enc_size=8, emb_size=32, n_speakers=102, n_target_speakers=2, batch_size=B, enc_pretrain_iters=iters, max_to_keep=10)
    d.update(kw)
    return make_hps(**d)


_SETS = {}


def _sets():
    from zs_amd.dataloader import SyntheticDataset
    from zs_amd.validation import ValidSet
    if not _SETS:
        _SETS['data'] = SyntheticDataset(96, seg_len=128, n_speakers=102, seed=0)
        _SETS['valid'] = ValidSet.from_dataset(SyntheticDataset(M * B, seg_len=128, n_speakers=102, seed=3), M, B, 102)
    return _SETS


def _trainer(dev, log_dir, seed=0, graphs=True, pooled=False, every=2, dtype='bf16', enc_mode=None, **hps_kw):
    """A fresh Trainer on a fresh loader at position 0, torch seeded with `seed` first.  every=None: no validation."""
    from zs_amd.dataloader import DataLoader
    from zs_amd.pool import DevicePool, PoolLoader
    from zs_amd.trainer import Trainer
    from zs_amd.validation import ValidConfig
    hps, sets = _hps(**hps_kw), _sets()
    loader = PoolLoader(DevicePool([sets['data']], dev), sets['data'], hps.batch_size) if pooled else DataLoader(sets['data'], hps.batch_size)
    torch.manual_seed(seed)
    tr = Trainer(hps, loader, hps.g_mode, enc_mode or hps.enc_mode, log_dir=log_dir, dtype=dtype, device=dev,
                 valid=None if every is None else ValidConfig(every, M, sets['valid']))
    tr.ae.use_graph = graphs
    return tr


def _train(tr, model_path, **kw):
    """tr.train(mode='pretrain_AE'); returns (what it printed, the exact logged training losses)."""
    losses, log = [], tr._log

    def keep(iteration, iters, fmt, info, head=()):
        losses.extend(info.values())
        return log(iteration, iters, fmt, info, head)
    tr._log = keep
    buf = io.StringIO()
    with redirect_stdout(buf):
        tr.train(model_path, 'train', mode='pretrain_AE', **kw)
    torch.cuda.synchronize()
    tr._log = log
    return buf.getvalue().replace('\r', '\n'), losses


def _final(tr, dev):
    out = {}
    for name, net in zip(('enc', 'dec', 'gen', 'clf', 'D', 'tclf'), tr.nets()):
        out['w.' + name] = net.flat_params()[0].clone()
    for name, o in (('enc', tr.ae.opt['enc']), ('dec', tr.ae.opt['dec'])):
        out['m.' + name], out['v.' + name], out['t.' + name] = o.m.clone(), o.v.clone(), o.t
    out.update({'adam_step': tr.ae.adam_step, 'seed_dev': tr.ae._seed_dev.clone(), 'step_dev': tr.ae._step_dev.clone(),
                'loss.ae': tr.ae._loss.clone(), 'rng.cpu': torch.get_rng_state().clone(), 'rng.cuda': torch.cuda.get_rng_state(dev).clone(),
                'consumed': dict(tr._consumed)})
    return out


def _same(fa, fb):
    for k, a in fa.items():
        if isinstance(a, torch.Tensor):
            assert torch.equal(a, fb[k]), k
        else:
            assert a == fb[k], (k, a, fb[k])


@pytest.mark.parametrize('mode', ['eager', 'host_fed', 'pool_fed'])
def test_validation_does_not_disturb_the_run(dev, tmp_path, mode):
    """Six iterations from one seed with a validation after iterations 2, 4 and 6 (eager, captured, replayed) and without: every
    weight, Adam moment, counter, both of torch's generator states and every logged training loss are bit-identical."""
    graphs, pooled = mode != 'eager', mode == 'pool_fed'
    finals, logged = [], []
    for every in (2, None):
        d = tmp_path / ('v%s' % every)
        d.mkdir()
        tr = _trainer(dev, str(d / 'log'), seed=0, graphs=graphs, pooled=pooled, every=every)
        out, losses = _train(tr, str(d / 'model.pth'))
        finals.append(_final(tr, dev))
        logged.append(losses)
        recs = [json.loads(l) for l in open(str(d / 'valid.jsonl'))] if every else []
        assert (sorted(os.listdir(str(d))) == ['log', 'model.pth-ae-2', 'model.pth-ae-4', 'model.pth-ae-6'] + (['model.pth-ae-best', 'valid.jsonl'] if every else []))
        if every:
            assert [r['iteration'] for r in recs] == [2, 4, 6] and out.count('valid:[') == 3
            assert tr.ae.use_graph == graphs and (tr._vstep._captured is not None) == graphs
            assert tr.best_loss == min(r['valid_loss_rec'] for r in recs)
        else:
            assert 'valid' not in out and tr._vstep is None
        del tr
    assert len(logged[0]) == ITERS and logged[0] == logged[1]
    _same(finals[1], finals[0])


def _record(tr, iteration=0):
    buf = io.StringIO()
    with redirect_stdout(buf):
        return tr.validate(iteration)


@pytest.mark.parametrize('graphs', [True, False])
def test_validation_repeats(dev, tmp_path, graphs):
    """No training step in between: the eager first pass, the captured second and the replayed third return one record."""
    tr = _trainer(dev, str(tmp_path / 'log'), graphs=graphs)
    recs = [_record(tr) for _ in range(3)]
    assert recs[0] == recs[1] == recs[2]
    assert (tr._vstep._captured is not None) == graphs
    r = recs[0]
    assert 0.0 < r['valid_loss_rec'] < 1.0 and r['valid_loss_rec_worst'] >= r['valid_loss_rec']
    assert sum(v['count'] for v in r['per_speaker'].values()) == M * B
    assert 0 <= r['valid_dead_bits'] <= 8 and 0.0 <= r['valid_bit_entropy'] <= 8.0 and 0.0 <= r['valid_flip_rate'] <= 1.0
    assert tr.ae.adam_step == 0 and int(tr.ae._step_dev.item()) == 0 and int(tr.ae._seed_dev.item()) == 0


def _module_loss(tr, dev):
    """mean |Decoder(Encoder(x, seed=VALID_SEED + m)) - x| over the validation set through the public modules in eval mode; the
    difference in fp32 as the kernel takes it, the sum in double."""
    from zs_amd.validation import VALID_SEED
    vs = _sets()['valid']
    tr.set_eval()
    total = 0.0
    for m in range(M):
        x = vs.x[m].to(dev).permute(0, 2, 1)                                   # [B, F, T]
        act, _ = tr.Encoder(x, seed=VALID_SEED + m)
        xdec = tr.Decoder(act, vs.c[m].to(dev))
        total += float((xdec - x).abs().double().sum())
    return total / vs.x[:M].numel()


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_validation_value_equals_the_public_modules(dev, tmp_path, dtype):
    """The same launches on the same inputs, so the same x_dec bits in fp32 and in bf16: only the order of the double sum differs.
    N = 2 * 4 * 128 * 513 = 5.3e5 terms, each partial sum rounded to 2^-53 relative: at most N * 2^-53 = 5.8e-11 relative."""
    tr = _trainer(dev, str(tmp_path / 'log'), dtype=dtype, graphs=False)
    got = _record(tr)['valid_loss_rec']
    want = _module_loss(tr, dev)
    print('%s: validation %.17g, public modules %.17g, relative difference %.3g' % (dtype, got, want, abs(got - want) / want))
    assert abs(got - want) <= 5.8e-11 * want


def test_validation_value_against_the_oracle_continues(dev, tmp_path):
    """enc_mode 'continues' draws no noise: the validation value against the oracle's eval-mode forward in fp32 on the same weights
    and set, to the bound tests/test_gpu_model.py holds the training loss to against the reference (|loss - oracle| < 1e-5)."""
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import zs_oracle as O
    tr = _trainer(dev, str(tmp_path / 'log'), dtype='fp32', enc_mode='continues', graphs=False)
    rec = _record(tr)
    assert not {'valid_bit_entropy', 'valid_dead_bits', 'valid_flip_rate'} & set(rec)
    hps, vs = tr.hps, _sets()['valid']
    esd = {k: v.detach().cpu() for k, v in tr.Encoder.state_dict().items()}
    dsd = {k: v.detach().cpu() for k, v in tr.Decoder.state_dict().items()}
    losses = []
    with torch.no_grad():
        for m in range(M):
            x = vs.x[m].permute(0, 2, 1).contiguous()
            # the oracle's encoder ends in the multilabel_binary head; its second output is the pre-activation the 'continues' head
            # (leaky_relu, model/model.py:457-472) takes.  U only feeds the unused head (and keeps torch's generator out of it).
            _, enc = O.encoder_forward(esd, x, hps.ns, hps.enc_dp, hps.enc_size // 2, hps.seg_len, U=torch.full((B, 16, hps.enc_size // 2, 2), 0.5))
            act = torch.nn.functional.leaky_relu(enc, negative_slope=hps.ns)
            losses.append(float(O.l1_loss(O.decoder_forward(dsd, act, vs.c[m], hps.ns, hps.seg_len), x)))
    want = sum(losses) / M
    print('continues: validation %.8f, oracle %.8f' % (rec['valid_loss_rec'], want))
    assert abs(rec['valid_loss_rec'] - want) < 1e-5


def _set_weights(tr, w):
    for net, flat in zip((tr.Encoder, tr.Decoder), w):
        net.flat_params()[0].copy_(flat)
        net.mark_dirty()


def test_best_checkpoint(dev, tmp_path):
    """Weights set between validations so that the loss goes down, up, down: -ae-best is written on the first and third only, loads
    with load_model, is not in model_kept and survives the window rolling past it."""
    from zs_amd import validation
    tr = _trainer(dev, str(tmp_path / 'log'), graphs=False, max_to_keep=2)
    model_path = str(tmp_path / 'model.pth')
    base = [n.flat_params()[0].clone() for n in (tr.Encoder, tr.Decoder)]
    g = torch.Generator(device=dev).manual_seed(5)
    cands = [base] + [[w + s * torch.randn(w.shape, generator=g, device=dev) for w in base] for s in (0.02, 0.05)]
    vs = tr.valid_step()
    loss = []
    for w in cands:                                                            # measured without the trainer's bookkeeping
        _set_weights(tr, w)
        loss.append(validation.finish(vs.run(), vs.T, vs.F)['valid_loss_rec'])
    assert len(set(loss)) == 3, loss
    order = sorted(range(3), key=lambda i: loss[i])
    seq = [order[1], order[2], order[0]]                                       # middle, highest, lowest
    best = validation.best_path(model_path)
    seen = []
    for it, i in zip((2, 4, 6), seq):
        _set_weights(tr, cands[i])
        rec = _record_at(tr, it, model_path)
        assert rec['valid_loss_rec'] == loss[i]
        ck = torch.load(best, weights_only=True)
        seen.append(ck['encoder']['conv2.weight'].clone())
        assert tr.best_iteration == (2 if it < 6 else 6)
    assert torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])                 # rewritten on the first and third only
    assert tr.best_loss == loss[order[0]] and tr.model_kept == []
    assert [r['iteration'] for r in validation.read_records(validation.record_path(model_path))] == [2, 4, 6]
    for it in (2, 4, 6):                                                       # max_to_keep 2: the window rolls past every periodic checkpoint but one
        tr.save_model(model_path, 'ae', it)
    assert sorted(os.listdir(str(tmp_path))) == ['log', 'model.pth-ae-6', 'model.pth-ae-best', 'valid.jsonl']
    assert best not in tr.model_kept
    _set_weights(tr, base)
    buf = io.StringIO()
    with redirect_stdout(buf):
        tr.load_model(best, 'encoder, decoder')
    assert '[encoder], [decoder]' in buf.getvalue()
    for net, w in zip((tr.Encoder, tr.Decoder), cands[order[0]]):
        assert torch.equal(net.flat_params()[0], w)


def _record_at(tr, iteration, model_path):
    buf = io.StringIO()
    with redirect_stdout(buf):
        return tr.validate(iteration, model_path)


def test_resumed_run_continues_records_and_best(dev, tmp_path):
    """Six iterations with validation, interrupted after the checkpoint at 4 and resumed by a fresh Trainer: the same weights, the same
    valid.jsonl and the same best_* as the uninterrupted run; a state file with another valid_every is refused by name."""
    from zs_amd import resume, validation
    dir_a, dir_b = tmp_path / 'A', tmp_path / 'B'
    dir_a.mkdir()
    tr_a = _trainer(dev, str(tmp_path / 'logA'), seed=0)
    out_a, _ = _train(tr_a, str(dir_a / 'model.pth'), resume=True)
    assert 'starting from iteration 0' in out_a
    names = ['model.pth-ae-%d' % it for it in (2, 4, 6)]
    assert sorted(os.listdir(str(dir_a))) == sorted(names + ['model.pth-ae-best', 'train_state', 'valid.jsonl'])
    assert sorted(os.listdir(str(dir_a / 'train_state'))) == sorted(n + '.pt' for n in names)     # the best checkpoint has no state file
    st = torch.load(resume.state_path(str(dir_a / names[2])), weights_only=True)
    assert st['valid'] == validation.describe(tr_a.valid) and st['best_loss'] == tr_a.best_loss and st['best_iteration'] == tr_a.best_iteration
    shutil.copytree(str(dir_a), str(dir_b))                                    # A's directory, cut back to the checkpoint at 4
    os.remove(str(dir_b / names[2]))
    os.remove(str(dir_b / 'train_state' / (names[2] + '.pt')))
    tr_b = _trainer(dev, str(tmp_path / 'logB'), seed=1234)
    out_b, _ = _train(tr_b, str(dir_b / 'model.pth'), resume=True)
    assert 'continuing at iteration 4 of 6' in out_b and out_b.count('valid:[') == 1
    fa, fb = _final(tr_a, dev), _final(tr_b, dev)
    for k in fa:
        if not k.startswith('rng.'):                                           # (each run's own generator states are compared in test_gpu_resume)
            _same({k: fa[k]}, fb)
    ra, rb = (validation.read_records(str(d / 'valid.jsonl')) for d in (dir_a, dir_b))
    assert [r['iteration'] for r in rb] == [2, 4, 6] and ra == rb
    assert (tr_b.best_loss, tr_b.best_iteration) == (tr_a.best_loss, tr_a.best_iteration) and tr_a.best_loss is not None
    ba, bb = (torch.load(str(d / 'model.pth-ae-best'), weights_only=True) for d in (dir_a, dir_b))
    assert all(torch.equal(ba[k][n], bb[k][n]) for k in ba for n in ba[k])
    # another valid_every: refused by name, before anything is loaded
    tr_c = _trainer(dev, str(tmp_path / 'logC'), seed=7, every=3)
    w0 = tr_c.Encoder.flat_params()[0].clone()
    with pytest.raises(ValueError, match='valid_every'):
        _train(tr_c, str(dir_b / 'model.pth'), resume=True)
    assert torch.equal(w0, tr_c.Encoder.flat_params()[0]) and tr_c.ae.adam_step == 0
    tr_d = _trainer(dev, str(tmp_path / 'logD'), seed=7, every=None)           # and a run without validation refuses a file with it
    with pytest.raises(ValueError, match='valid is on in the file'):
        _train(tr_d, str(dir_b / 'model.pth'), resume=True)


def test_main_writes_the_records(dev, tmp_path, monkeypatch, capsys):
    sys.path.insert(0, ROOT)
    import main
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('ZS_CKPT_EVERY', '3')
    hps_path = str(tmp_path / 'hps.json')
    json.dump(_hps(ITERS, n_speakers=4)._asdict(), open(hps_path, 'w'))
    torch.manual_seed(0)
    main.main(['--train_ae', '--synthetic', '--valid_every', '2', '--valid_batches', '2', '--hps_path', hps_path, '--ckpt_dir',
               str(tmp_path / 'ck'), '--dtype', 'bf16'])
    out = capsys.readouterr().out
    recs = [json.loads(l) for l in open(str(tmp_path / 'ck' / 'valid.jsonl'))]
    assert [r['iteration'] for r in recs] == [2, 4, 6] and out.count('valid:[') == 3
    assert all({'valid_loss_rec', 'valid_loss_rec_target', 'valid_loss_rec_worst', 'valid_bit_entropy', 'valid_dead_bits', 'valid_flip_rate',
                'per_speaker'} <= set(r) for r in recs)
    assert all(set(r['per_speaker']) <= {'0', '1', '2', '3'} and sum(v['count'] for v in r['per_speaker'].values()) == 2 * B for r in recs)
    assert sorted(os.listdir(str(tmp_path / 'ck'))) == ['model.pth-ae-3', 'model.pth-ae-6', 'model.pth-ae-best', 'valid.jsonl']
