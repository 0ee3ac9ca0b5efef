"""Training from a dataset held in device memory (zs_amd.pool, zs_pool_gather) against the host DataLoader it replaces.  A gather
rounds nothing: every comparison is exact."""
import functools
import io
import json
import os
import sys
from contextlib import redirect_stdout
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


class TableSet(object):
    """The host view of an item table over a host pool: item i = (speaker[i], pool[first[i] : first[i] + seg_len])."""

    def __init__(self, pool, speaker, first, seg_len):
        self.pool, self.speaker, self.first, self.seg_len = pool, speaker, first, seg_len

    def __getitem__(self, i):
        if not 0 <= i < len(self.speaker):
            raise IndexError(i)
        return (np.int64(self.speaker[i]), self.pool[self.first[i]:self.first[i] + self.seg_len])

    def __len__(self):
        return len(self.speaker)


def _gather(L, dev, pool_d, spk_d, first_d, cursor, n, B, seg, F, rank, world, advance=1):
    x = torch.empty(B, seg, F, dtype=torch.float32, device=dev)
    c = torch.empty(B, dtype=torch.int64, device=dev)
    L.call('zs_pool_gather', 'ZsPoolGather', torch.cuda.current_stream(dev).cuda_stream, pool=L.ptr(pool_d), speaker=L.ptr(spk_d),
           first=L.ptr(first_d), cursor=L.ptr(cursor), n=n, B=B, seg_len=seg, F=F, rank=rank, world=world, x=L.ptr(x), c=L.ptr(c),
           advance=advance)
    return c, x


def _abi_case(L, dev, rng, F, seg, B, world, n, frames, n_batches, shift):
    """One table on the device, both ranks: batches 0 .. n_batches-1 against DataLoader, the cursor's count, a set cursor.
    shift: the pool starts `shift` floats into its allocation.  Returns the set of source addresses modulo 16 that were read."""
    from zs_amd.dataloader import DataLoader
    pool_h = rng.rand(frames, F).astype(np.float32)
    first = rng.randint(0, frames - seg + 1, size=n).astype(np.int64)            # valid by construction: first + seg <= frames
    first[0], first[-1] = 0, frames - seg                                          # both ends of the pool are touched
    spk = rng.randint(0, 1000, size=n).astype(np.int32)
    assert first.min() >= 0 and (first + seg).max() <= frames
    buf = torch.zeros(frames * F + 4, dtype=torch.float32, device=dev)
    pool_d = buf[shift:shift + frames * F]
    pool_d.copy_(torch.from_numpy(pool_h).view(-1))
    spk_d, first_d = torch.from_numpy(spk).to(dev), torch.from_numpy(first).to(dev)
    classes = set()
    for rank in range(world):
        cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        got = [_gather(L, dev, pool_d, spk_d, first_d, cursor, n, B, seg, F, rank, world) for _ in range(n_batches)]
        dl = DataLoader(TableSet(pool_h, spk, first, seg), B, rank=rank, world=world)
        torch.cuda.synchronize()
        assert int(cursor.item()) == n_batches                                   # the cursor after m launches is m
        for k, (c, x) in enumerate(got):
            rc, rx = next(dl)
            assert rc.dtype == torch.int64 and torch.equal(c.cpu(), rc), (F, seg, world, rank, n, k)
            assert torch.equal(x.cpu(), rx), (F, seg, world, rank, n, k)
        # set from the host: batch k, and a launch that does not advance leaves the cursor alone
        k = n_batches + 3
        cursor.fill_(k)
        c, x = _gather(L, dev, pool_d, spk_d, first_d, cursor, n, B, seg, F, rank, world, advance=0)
        for _ in range(k - n_batches):
            next(dl)
        rc, rx = next(dl)
        assert int(cursor.item()) == k and torch.equal(c.cpu(), rc) and torch.equal(x.cpu(), rx), (F, seg, world, rank, n, 'set')
        classes |= {int((pool_d.data_ptr() + int(f) * F * 4) % 16) for f in first}
    return classes


@pytest.mark.parametrize('F', [513, 80])
@pytest.mark.parametrize('seg', [128, 32])
def test_kernel_serves_the_dataloader_batches_bit_for_bit(dev, F, seg):
    """zs_pool_gather through the C ABI: world 1 and 2 (both ranks), n a multiple of S = world * B, not a multiple and = S, the
    pool at every 4-byte phase of a 16-byte line: (c, x) of batches 0 .. 3P+1 equal next(DataLoader), the cursor counts the
    launches, and a cursor set from the host serves that batch."""
    from zs_amd import _lib as L
    rng = np.random.RandomState(F + seg)
    B = 3
    seen = set()
    for world in (1, 2):
        S = world * B
        for n in (4 * S, 4 * S + 2, S):
            P = max(1, -(-n // S) - 1)
            for shift in range(4):
                seen |= _abi_case(L, dev, rng, F, seg, B, world, n, frames=5 * seg + 7, n_batches=3 * P + 2, shift=shift)
    assert seen == {0, 4, 8, 12}, seen                                           # every source alignment class was read


def test_kernel_at_the_training_shape(dev):
    """B = 256 segments of 128 x 513 (the --train_ae batch, 67 MB) out of overlapping items: the launch geometry of the real shape."""
    from zs_amd import _lib as L
    rng = np.random.RandomState(1)
    seen = _abi_case(L, dev, rng, 513, 128, 256, 1, 3 * 256 + 5, frames=1500, n_batches=3, shift=0)
    assert seen == {0, 4, 8, 12}


def _ragged_store(tmp_path, seg_len, F):
    from zs_amd.dataloader import NpzStore
    rng = np.random.RandomState(5)
    lens = {'S1/a': seg_len, 'S1/b': seg_len + 5, 'V1/c': 3 * seg_len + 1, 'S2/d': 2 * seg_len}
    path = str(tmp_path / 'store.npz')
    with NpzStore(path, 'w') as st:
        for utt, n in lens.items():
            st.create_group('train/' + utt).create_dataset('lin', data=rng.rand(n, F).astype(np.float32))
    items = [(0, 'S1/a', 0), (1, 'V1/c', 2 * seg_len + 1), (0, 'S1/b', 5), (2, 'S2/d', seg_len), (1, 'V1/c', 0), (0, 'S1/b', 0),
             (2, 'S2/d', 0), (1, 'V1/c', 7), (2, 'S2/d', 3), (0, 'S1/b', 2), (1, 'V1/c', seg_len)]
    index = str(tmp_path / 'index.json')
    json.dump([{'speaker': s, 'i': u, 't': t} for s, u, t in items], open(index, 'w'))
    return path, index


def test_pool_loader_equals_dataloader_and_keeps_two_batches(dev, tmp_path):
    """PoolLoader over a ragged .npz store and over a SyntheticDataset (one pool holds both), both ranks of world 2 and world 1:
    every batch equals next(DataLoader) over three passes; the batch returned by the previous call is still intact after the
    next one, and the one returned two calls ago is the slot the current call wrote (DevicePrefetcher's contract)."""
    from zs_amd.dataloader import DataLoader, Dataset, SyntheticDataset
    from zs_amd.pool import DevicePool, PoolLoader
    seg, F = 16, 513
    path, index = _ragged_store(tmp_path, seg, F)
    ds = Dataset(path, index, seg_len=seg)
    syn = SyntheticDataset(13, seg_len=seg, n_bins=F, n_speakers=3, seed=2)
    pool = DevicePool([ds, syn], dev)
    assert pool.data.shape == (pool.plan.frames_total, F)
    for data in (ds, syn):
        for world, rank in ((1, 0), (2, 0), (2, 1)):
            B = 2
            pl = PoolLoader(pool, data, B, rank=rank, world=world, n_speakers=3)
            dl = DataLoader(data, B, rank=rank, world=world)
            P = max(1, -(-len(data) // (world * B)) - 1)
            hist = []
            for k in range(3 * P + 2):
                c, x = next(pl)
                rc, rx = next(dl)
                rc, rx = rc.long(), rx.float()
                assert c.dtype == torch.int64 and x.dtype == torch.float32 and x.shape == (B, seg, F)
                assert torch.equal(c.cpu(), rc) and torch.equal(x.cpu(), rx), (world, rank, k)
                if hist:                                                         # the previous batch survived this call
                    pc, px, prc, prx = hist[-1]
                    assert torch.equal(pc.cpu(), prc) and torch.equal(px.cpu(), prx), (world, rank, k)
                    assert px.data_ptr() != x.data_ptr()
                if len(hist) >= 2:                                               # the one before it was this call's destination
                    assert hist[-2][1].data_ptr() == x.data_ptr() and hist[-2][0].data_ptr() == c.data_ptr()
                hist.append((c, x, rc, rx))
            pl.set_cursor(1)                                                     # resume at batch 1
            c, x = next(pl)
            dl2 = DataLoader(data, B, rank=rank, world=world)
            next(dl2)
            rc, rx = next(dl2)
            assert torch.equal(c.cpu(), rc.long()) and torch.equal(x.cpu(), rx.float())


@pytest.mark.parametrize('use_graph', [True, False])
def test_pool_fed_step_equals_resident_step(dev, use_graph):
    """PoolFedStep (the gather at the head of the captured step) on a dataset that wraps twice in the run: the final loss and both
    flat parameter buffers equal AEStep.step fed the same DataLoader's batches, bit for bit, with graphs and without."""
    from zs_amd.dataloader import DataLoader, SyntheticDataset
    from zs_amd.model import Decoder, Encoder
    from zs_amd.pool import DevicePool, PoolLoader
    from zs_amd.trainer import AEStep
    ds = SyntheticDataset(32, seg_len=128, n_bins=80, n_speakers=4, seed=3)       # B = 8: three positions, nine steps = three passes
    res = []
    for mode in ('pool', 'resident'):
        torch.manual_seed(0)
        enc = Encoder(c_in=80, c_h1=16, c_h2=64, c_h3=32, ns=0.01, dp=0.5, enc_size=32, seg_len=128, enc_mode='multilabel_binary', dtype='bf16').to(dev)
        dec = Decoder(c_in=32, c_out=80, c_h=64, c_a=4, ns=0.01, seg_len=128, dtype='bf16').to(dev)
        ae = AEStep(enc, dec, lr=1e-3, max_grad_norm=5.0, use_graph=use_graph)
        if mode == 'pool':
            loader = PoolLoader(DevicePool(ds, dev), ds, 8)
            feeder = ae.pool_feeder(loader)
            for _ in range(9):
                next(feeder)
            torch.cuda.synchronize()
            assert int(loader.cursor.item()) == 9
            assert (feeder.ent is not None) == use_graph and len(ae._graphs) == 0     # one set of graphs, the feeder's
        else:
            dl = DataLoader(ds, 8)
            for _ in range(9):
                c, x = next(dl)
                ae.step(x.to(dev), c.to(dev))
            torch.cuda.synchronize()
        res.append((ae._loss.item(), enc.flat_params()[0].clone(), dec.flat_params()[0].clone(), ae.adam_step))
    assert res[0][3] == res[1][3] == 9
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


def _trainer(dev, tmp_path, hps, pooled, sets):
    """A Trainer on `sets` = (data, source, target) datasets (None where unused) through PoolLoaders or DataLoaders."""
    from zs_amd.dataloader import DataLoader
    from zs_amd.pool import DevicePool, PoolLoader
    from zs_amd.trainer import Trainer
    if pooled:
        pool = DevicePool([s for s in sets if s is not None], dev)
        mk = lambda s: PoolLoader(pool, s, hps.batch_size) if s is not None else None
    else:
        mk = lambda s: DataLoader(s, hps.batch_size) if s is not None else None
    torch.manual_seed(0)
    tr = Trainer(hps, mk(sets[0]), hps.g_mode, hps.enc_mode, log_dir=str(tmp_path / 'log'), dtype='bf16', device=dev)
    if sets[1] is not None:
        tr.add_duo_loader(mk(sets[1]), mk(sets[2]))
    return tr


@pytest.mark.parametrize('mode, line', [('pretrain_AE', 'pre_AE:[000006/000006]'), ('pretrain_C', 'pre_C:[000005/000005]')])
def test_trainer_stage1_loops_equal_the_host_loaders(dev, tmp_path, mode, line):
    """Trainer.train for pretrain_AE (the captured step: PoolFedStep against HostFedStep) and pretrain_C (next(PoolLoader) against
    the DevicePrefetcher), each from a fresh trainer (HostFedStep reads its loader two batches ahead, so a second mode on the same
    host loader would not start where the pool's cursor stands): bit-equal Encoder, Decoder and SpeakerClassifier parameters over
    the same data, which wraps in the run."""
    from zs_amd.dataloader import SyntheticDataset
    from zs_amd.hps import make_hps
    hps = make_hps(enc_size=32, emb_size=64, n_speakers=4, n_target_speakers=2, batch_size=4, enc_pretrain_iters=6, dis_pretrain_iters=5,
                   max_to_keep=3)
    ds = SyntheticDataset(12, seg_len=128, n_speakers=4, seed=1)                   # two positions: the loop wraps
    res = []
    for pooled in (True, False):
        tr = _trainer(dev, tmp_path, hps, pooled, (ds, None, None))
        before = [net.flat_params()[0].clone() for net in (tr.Encoder, tr.Decoder, tr.SpeakerClassifier)]
        with redirect_stdout(io.StringIO()) as out:
            tr.train(str(tmp_path / 'm.pth'), 'train', mode=mode)
        torch.cuda.synchronize()
        assert line in out.getvalue()
        res.append([net.flat_params()[0].clone() for net in (tr.Encoder, tr.Decoder, tr.SpeakerClassifier)])
        assert any(not torch.equal(a, b) for a, b in zip(before, res[-1]))         # it trained
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_trainer_patchgan_loop_equals_the_host_loaders(dev, tmp_path):
    """Trainer.train(mode='patchGAN', target_guided=True) with PoolLoaders against DataLoaders.  The (x_s, x_t, c_t) every d_step and
    g_step receives are recorded in both arms and must be bit-equal.  The critic's kernels are not claimed to be run-to-run
    deterministic anywhere in this tree, so the DataLoader arm is run twice first: if it repeats bit for bit, the pool arm's
    Generator and PatchDiscriminator parameters must equal it too; if it does not, the equality of the inputs is what is asserted
    (the line this test prints says which; on the MI355X runs made when it was written the arm repeated)."""
    from zs_amd.dataloader import SyntheticDataset
    from zs_amd.hps import make_hps
    hps = make_hps(enc_size=8, emb_size=32, n_speakers=4, n_target_speakers=2, batch_size=2, patch_iters=3, n_patch_steps=2, max_to_keep=5)
    src = SyntheticDataset(8, seg_len=128, n_speakers=2, seed=1)
    tgt = SyntheticDataset(8, seg_len=128, n_speakers=2, seed=2, speaker_offset=2)

    def run(pooled):
        tr = _trainer(dev, tmp_path, hps, pooled, (None, src, tgt))
        s2, seen = tr.stage2(), []
        for name in ('d_step', 'g_step'):
            def spy(x_s, x_t, c_t, _real=getattr(s2, name), _name=name):
                seen.append((_name, x_s.clone(), x_t.clone(), c_t.clone()))
                return _real(x_s, x_t, c_t)
            setattr(s2, name, spy)
        with redirect_stdout(io.StringIO()):
            tr.train(str(tmp_path / 'm.pth'), 'train', mode='patchGAN', target_guided=True)
        torch.cuda.synchronize()
        return seen, [net.flat_params()[0].clone() for net in (tr.Generator, tr.PatchDiscriminator)]

    seen_a, par_a = run(False)
    seen_b, par_b = run(False)
    seen_p, par_p = run(True)
    assert len(seen_p) == len(seen_a) == 3 * 3
    for (na, *ta), (np_, *tp) in zip(seen_a, seen_p):
        assert na == np_ and all(torch.equal(u, v) for u, v in zip(ta, tp)), na
    repeatable = all(torch.equal(u, v) for u, v in zip(par_a, par_b))
    print('patchGAN DataLoader arm repeats bit for bit: %s' % repeatable)
    if repeatable:
        assert all(torch.equal(u, v) for u, v in zip(par_a, par_p))


def test_target_range_failure_raises_before_any_launch(dev, monkeypatch):
    """A source-range speaker in the target index: RuntimeError at loader construction (and from require() for a loader built
    without the check), with no gather launched."""
    from zs_amd import pool as zp
    from zs_amd.dataloader import SyntheticDataset
    from zs_amd.stage2 import PatchGANStep
    ds = SyntheticDataset(8, seg_len=128, n_speakers=4, seed=1)                    # speakers 0..3, the targets are 2 and 3
    assert ds.spk.min() < 2
    pool = zp.DevicePool(ds, dev)
    targets = functools.partial(PatchGANStep.check_targets, SimpleNamespace(shift=2, Generator=SimpleNamespace(c_a=2)))
    launched = []
    monkeypatch.setattr(zp.L, 'call', lambda *a, **k: launched.append(a))
    with pytest.raises(RuntimeError, match='only convert to target speakers'):
        zp.PoolLoader(pool, ds, 2, n_speakers=4, check=targets)
    loader = zp.PoolLoader(pool, ds, 2, n_speakers=4)
    with pytest.raises(RuntimeError, match='only convert to target speakers'):
        loader.require(n_speakers=4, check=targets)
    with pytest.raises(ValueError, match=r'speaker index outside \[0, 3\)'):
        loader.require(n_speakers=3)
    assert not launched


@pytest.mark.parametrize('flag, line, ckpt', [('--train_ae', 'pre_AE:[000004/000004]', 'model.pth-ae-4'),
                                              ('--train_tgat', 'patch_G:[000002/000002]', 'model.pth-s2-2'),
                                              ('--train_c', 'Target Classifier:[00002/00002]', 'model.pth-tclf-2')])
def test_main_device_data_synthetic(dev, tmp_path, monkeypatch, capsys, flag, line, ckpt):
    """`python main.py --train_ae | --train_tgat | --train_c --synthetic --device_data` trains from pool loaders."""
    sys.path.insert(0, ROOT)
    import main
    from zs_amd import pool as zp
    from zs_amd.hps import make_hps
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('ZS_CKPT_EVERY', '2')
    hps = make_hps(enc_size=8, emb_size=32, n_speakers=102, n_target_speakers=2, batch_size=2, enc_pretrain_iters=4, patch_iters=2,
                   n_patch_steps=1, tclf_iters=2)
    p = str(tmp_path / 'hps.json')
    json.dump(hps._asdict(), open(p, 'w'))
    gathers = []
    real = zp.PoolLoader.gather_into
    monkeypatch.setattr(zp.PoolLoader, 'gather_into', lambda self, x, c: (gathers.append(1), real(self, x, c))[1])
    main.main([flag, '--synthetic', '--device_data', '--hps_path', p, '--ckpt_dir', str(tmp_path / 'ck'), '--dtype', 'bf16'])
    out = capsys.readouterr().out
    assert line in out
    assert os.path.exists(str(tmp_path / 'ck' / ckpt))
    assert gathers                                                                # the batches came from the pool
