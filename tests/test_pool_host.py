"""Host side of the device-resident dataset (zs_amd.pool), no GPU: the closed-form batch order against DataLoader, the pool layout
of a ragged .npz store against Dataset.__getitem__, every validation error, and the --device_data flag."""
import functools
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HPS = os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')


class Ids(object):
    """Dataset whose item i is (i, [i]): a DataLoader over it returns the item numbers it serves."""

    def __init__(self, n):
        self.n = n

    def __getitem__(self, i):
        if not 0 <= i < self.n:
            raise IndexError(i)
        return (i, np.full(1, i, dtype=np.float32))

    def __len__(self):
        return self.n


def ragged_store(tmp_path, seg_len, F=7, items=None, name='store'):
    """A small .npz store of four utterances of different lengths under train/, and an index whose items touch utterance starts
    and ends.  Returns (store path, index path, utterance lengths)."""
    import zs_amd  # noqa: F401
    from zs_amd.dataloader import NpzStore
    rng = np.random.RandomState(5)
    lens = {'S1/a': seg_len, 'S1/b': seg_len + 5, 'V1/c': 3 * seg_len + 1, 'S2/d': 2 * seg_len}
    path = str(tmp_path / (name + '.npz'))
    with NpzStore(path, 'w') as st:
        for utt, n in lens.items():
            st.create_group('train/' + utt).create_dataset('lin', data=rng.rand(n, F).astype(np.float32))
    if items is None:
        items = [(0, 'S1/a', 0), (1, 'V1/c', 2 * seg_len + 1), (0, 'S1/b', 5), (2, 'S2/d', seg_len), (1, 'V1/c', 0), (0, 'S1/b', 0),
                 (2, 'S2/d', 0), (1, 'V1/c', 7), (2, 'S2/d', 3), (0, 'S1/b', 2), (1, 'V1/c', seg_len)]
    index = str(tmp_path / (name + '_index.json'))
    json.dump([{'speaker': s, 'i': u, 't': t} for s, u, t in items], open(index, 'w'))
    return path, index, lens


def test_batch_items_is_the_dataloader_order():
    """batch_items(n, B, rank, world, k) == the items DataLoader serves at its k-th next(), for at least three passes over the
    set (wraps included), n a multiple of S = world * B, not a multiple, and n = S."""
    import zs_amd  # noqa: F401
    from zs_amd.dataloader import DataLoader
    from zs_amd.pool import batch_items
    cases = 0
    for world in (1, 2, 4):
        for B in (1, 2, 3, 5):
            S = world * B
            for n in sorted({S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 3 * S, 3 * S + 2, 5 * S, 5 * S + S - 1, 7 * S + 1}):
                P = max(1, -(-n // S) - 1)
                for rank in range(world):
                    dl = DataLoader(Ids(n), B, rank=rank, world=world)
                    for k in range(3 * P + 2):
                        assert next(dl)[0].tolist() == batch_items(n, B, rank, world, k), (n, B, rank, world, k)
                        cases += 1
    assert cases > 1000
    # the tail beyond P * S is never served (kept from the reference); n = S serves one batch forever
    assert max(max(batch_items(11, 2, 0, 1, k)) for k in range(20)) == 9
    assert all(batch_items(4, 4, 0, 1, k) == [0, 1, 2, 3] for k in range(5))
    with pytest.raises(ValueError, match='fewer than one global batch'):
        batch_items(7, 4, 0, 2, 0)


def test_planned_layout_addresses_the_frames_dataset_returns(tmp_path):
    """Two index files over one ragged store share one plan: each utterance is planned once, and every item's
    [first, first + seg_len) rows of the pool are the frames Dataset.__getitem__ returns, with its speaker."""
    import zs_amd  # noqa: F401
    from zs_amd.dataloader import Dataset, SyntheticDataset
    from zs_amd.pool import PoolPlan, item_table
    seg = 6
    path, index, lens = ragged_store(tmp_path, seg)
    index2 = str(tmp_path / 'second.json')
    json.dump([{'speaker': 1, 'i': 'V1/c', 't': 4}, {'speaker': 0, 'i': 'S1/a', 't': 0}], open(index2, 'w'))
    ds, ds2 = Dataset(path, index, seg_len=seg), Dataset(path, index2, seg_len=seg)
    syn = SyntheticDataset(5, seg_len=seg, n_bins=7, n_speakers=3, seed=4)
    plan = PoolPlan([ds, ds2, syn])
    assert len(plan.order) == len(lens) + 1 and plan.F == 7
    assert plan.frames_total == sum(lens.values()) + 5 * seg and plan.nbytes == plan.frames_total * 7 * 4
    pool = np.concatenate([plan.read(k) for k in plan.order])
    assert pool.shape == (plan.frames_total, 7)
    for d in (ds, ds2, syn):
        spk, first, seg_len = item_table(plan, d, batch_size=2, n_speakers=3)
        assert seg_len == seg and spk.dtype == np.int32 and first.dtype == np.int64 and len(spk) == len(d)
        for i in range(len(d)):
            c, x = d[i]
            assert int(spk[i]) == int(c)
            assert np.array_equal(pool[first[i]:first[i] + seg], np.asarray(x)), i


def test_every_validation_error_fires(tmp_path, monkeypatch):
    import zs_amd  # noqa: F401
    from zs_amd.dataloader import Dataset, SyntheticDataset
    from zs_amd.pool import DevicePool, PoolLoader, PoolPlan, item_table
    from zs_amd.stage2 import PatchGANStep
    from zs_amd.trainer import tclf_labels
    seg = 6
    path, index, lens = ragged_store(tmp_path, seg)
    ds = Dataset(path, index, seg_len=seg)
    plan = PoolPlan(ds)
    item_table(plan, ds, batch_size=4, world=2, n_speakers=3)                    # the valid table passes
    # t + seg_len past the end of the utterance (by one frame), and a negative t
    for bad in ((0, 'S1/b', 6), (0, 'S1/b', -1)):
        p2, i2, _ = ragged_store(tmp_path, seg, items=[(0, 'S1/a', 0), bad, (2, 'S2/d', 0)], name='bad%d' % bad[2])
        d2 = Dataset(p2, i2, seg_len=seg)
        with pytest.raises(ValueError, match='leave its utterance'):
            item_table(PoolPlan(d2), d2, batch_size=1)
    # speaker outside [0, n_speakers): the host path's message
    with pytest.raises(ValueError, match=r'speaker index outside \[0, 2\) in the batch'):
        item_table(plan, ds, batch_size=2, n_speakers=2)
    # fewer items than one global batch
    with pytest.raises(ValueError, match='fewer than one global batch'):
        item_table(plan, ds, batch_size=4, world=3)
    # the consumer's hook sees the whole speaker column: a source-range speaker among targets, and the t_classify relabel
    targets = functools.partial(PatchGANStep.check_targets, SimpleNamespace(shift=1, Generator=SimpleNamespace(c_a=2)))
    with pytest.raises(RuntimeError, match='only convert to target speakers'):
        item_table(plan, ds, batch_size=2, n_speakers=3, check=targets)
    with pytest.raises(ValueError, match='t_classify target'):
        item_table(plan, ds, batch_size=2, check=lambda c: tclf_labels(c, 4, 2, 'targeted'))   # 102 - shift_c = 100
    # PoolLoader validates at construction, before it touches its pool's device (this stand-in has none)
    stub = SimpleNamespace(plan=plan, F=plan.F, device=None, data=None)
    with pytest.raises(RuntimeError, match='only convert to target speakers'):
        PoolLoader(stub, ds, 2, n_speakers=3, check=targets)
    with pytest.raises(ValueError, match='fewer than one global batch'):
        PoolLoader(stub, ds, 4, rank=1, world=3)
    # a pool larger than the limit: the error names both numbers and comes before any allocation
    syn = SyntheticDataset(4, seg_len=8, n_bins=5, n_speakers=2)
    need = 4 * 8 * 5 * 4
    with pytest.raises(MemoryError, match=r'needs %d bytes, more than the %d bytes allowed' % (need, need - 1)):
        DevicePool(syn, 'cuda:0', max_bytes=need - 1)
    monkeypatch.setenv('ZS_POOL_MAX_GB', '1e-8')                                 # 10 bytes
    with pytest.raises(MemoryError, match=r'needs %d bytes, more than the 10 bytes allowed' % need):
        DevicePool(syn, 'cuda:0')
    # what a pool cannot hold
    with pytest.raises(TypeError, match='Dataset or SyntheticDataset'):
        PoolPlan([object()])
    with pytest.raises(NotImplementedError, match='load_mel'):
        PoolPlan(Dataset(path, index, seg_len=seg, load_mel=True))


def test_device_data_flag_parses_and_is_off_by_default():
    sys.path.insert(0, ROOT)
    import main
    args, _ = main.argument_runner(['--train_ae', '--device_data', '--synthetic', '--hps_path', HPS])
    assert args.device_data is True and args.train_ae and args.synthetic
    for flags in (['--train_ae'], ['--train_p', '--synthetic'], ['--train_c']):
        args, _ = main.argument_runner(flags + ['--hps_path', HPS])
        assert args.device_data is False
    args, _ = main.argument_runner(['--train_tgat', '--device_data', '--hps_path', HPS])
    assert args.device_data is True and args.train_tgat
