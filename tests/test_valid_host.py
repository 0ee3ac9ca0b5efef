"""Held-out validation without a GPU: the flag checks, the holdout split, the validation set, the finishing arithmetic against numpy
on hand-made tables, the record file, the `valid` entry of a train-state file, and the checkpoint names."""
import copy
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def V():
    import zs_amd  # noqa: F401
    from zs_amd import validation
    return validation


def _args(argv):
    sys.path.insert(0, ROOT)
    import main
    return main.build_parser().parse_args(argv)


# ---- flags ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('argv, word', [
    (['--valid_every', '10'], '--train_ae or --train'),
    (['--valid_every', '10', '--train_p', '--synthetic'], '--train_ae or --train'),
    (['--valid_every', '10', '--test'], '--train_ae or --train'),
    (['--train_ae', '--valid_batches', '4'], '--valid_batches needs --valid_every'),
    (['--train_ae', '--valid_index_path', 'v.json'], '--valid_index_path needs --valid_every'),
    (['--train_ae', '--valid_holdout', '5'], '--valid_holdout needs --valid_every'),
    (['--train_ae', '--valid_flag', 'test'], '--valid_flag needs --valid_every'),
    (['--train_ae', '--valid_every', '10', '--valid_index_path', 'v.json', '--valid_holdout', '5'], 'give one'),
    (['--train_ae', '--valid_every', '10', '--valid_holdout', '1'], '>= 2'),
    (['--train_ae', '--valid_every', '0', '--synthetic'], '>= 1'),
    (['--train_ae', '--valid_every', '10', '--valid_batches', '0', '--synthetic'], '>= 1'),
    (['--train_ae', '--valid_every', '10'], 'needs a validation set'),
    (['--train_ae', '--valid_every', '10', '--valid_holdout', '5', '--synthetic'], '--synthetic'),
])
def test_flag_refusals(V, argv, word):
    with pytest.raises(ValueError, match=word):
        V.check_flags(_args(argv))


@pytest.mark.parametrize('argv', [
    [], ['--train_ae'], ['--train_ae', '--synthetic', '--valid_every', '1000'], ['--train', '--synthetic', '--valid_every', '5'],
    ['--train_ae', '--valid_every', '1000', '--valid_holdout', '20', '--resume', '--ema', '0.999'],
    ['--train_ae', '--valid_every', '7', '--valid_index_path', 'v.json', '--valid_flag', 'test', '--valid_batches', '2'],
])
def test_flags_accepted(V, argv):
    V.check_flags(_args(argv))


def test_main_refuses_before_anything_is_built():
    sys.path.insert(0, ROOT)
    import main
    with pytest.raises(ValueError, match='--valid_every needs --train_ae or --train'):
        main.argument_runner(['--valid_every', '3', '--train_c'])
    assert main.build_parser().parse_args([]).valid_every is None and main.VALID_BATCHES == 8


# ---- the holdout split ---------------------------------------------------------------------------------------------------------
def _index(n_utt=7, per=3, seed=0):
    """per entries of each of n_utt utterances of 3 speakers, shuffled (an index file is in random order)."""
    rng = np.random.RandomState(seed)
    ents = [{'speaker': u % 3, 'i': 'S%03d/utt_%02d' % (u % 3, u), 't': int(t)} for u in range(n_utt) for t in rng.randint(0, 50, per)]
    return [ents[i] for i in rng.permutation(len(ents))]


@pytest.mark.parametrize('K', [2, 3, 7, 100])
def test_holdout_split(V, K):
    idx = _index()
    before = copy.deepcopy(idx)
    train, valid = V.holdout_split(idx, K)
    assert idx == before                                                        # the input is left alone
    utt = lambda es: {(e['speaker'], e['i']) for e in es}
    assert not (utt(train) & utt(valid))                                        # disjoint by utterance
    key = lambda e: json.dumps(e, sort_keys=True)
    assert sorted(map(key, train + valid)) == sorted(map(key, idx))             # the union is the input, speaker ids and all
    pos = {id(e): n for n, e in enumerate(idx)}
    for part in (train, valid):                                                 # the file's order is kept (and the very entries)
        where = [pos[id(e)] for e in part]
        assert where == sorted(where)
    utts = sorted(utt(idx))
    assert utt(valid) == set(utts[K - 1::K])
    assert len(utt(valid)) == len(utts) // K                                    # K = 100 > 7 utterances: nothing is held out
    if K == 2:
        assert len(utt(valid)) == 3 and len(valid) == 9


def test_holdout_K_below_two_is_refused(V):
    with pytest.raises(ValueError, match='>= 2'):
        V.holdout_split(_index(), 1)


# ---- the validation set --------------------------------------------------------------------------------------------------------
def _store(tmp_path, idx, frames=60):
    from zs_amd.dataloader import NpzStore
    path = str(tmp_path / 'data.npz')
    rng = np.random.RandomState(1)
    with NpzStore(path, 'w') as st:
        g = st.create_group('train')
        for name in sorted({e['i'] for e in idx}):
            g.create_dataset(name + '/lin', data=rng.rand(frames, 513).astype(np.float32))
    ipath = str(tmp_path / 'index.json')
    json.dump(idx, open(ipath, 'w'))
    return path, ipath


def test_valid_set_from_an_index_file(V, tmp_path):
    from zs_amd.dataloader import Dataset
    idx = _index()
    for e in idx:
        e['t'] = e['t'] % 40
    path, ipath = _store(tmp_path, idx)
    ds = Dataset(path, ipath, seg_len=8)
    vs = V.ValidSet.from_dataset(ds, 2, 4, n_speakers=3)
    assert tuple(vs.x.shape) == (2, 4, 8, 513) and vs.x.dtype == torch.float32 and tuple(vs.c.shape) == (2, 4) and vs.c.dtype == torch.int64
    for n in range(8):                                                          # the first M * B entries, in file order
        spk, lin = ds[n]
        assert int(vs.c.view(-1)[n]) == spk and np.array_equal(vs.x.view(8, 8, 513)[n].numpy(), lin)
    # Dataset(indexes=...) serves a part of the file; its default behaviour is unchanged
    train, valid = V.holdout_split(idx, 2)
    part = Dataset(path, ipath, seg_len=8, indexes=valid)
    assert len(part) == len(valid) and part[0][0] == valid[0]['speaker'] and len(ds) == len(idx)
    assert V.ValidSet.from_dataset(part, 1, 4, 3).digest != vs.digest
    assert V.ValidSet.from_dataset(ds, 2, 4, 3).digest == vs.digest
    # a short file, and a speaker id outside the tables: ValueError
    with pytest.raises(ValueError, match='21 items'):
        V.ValidSet.from_dataset(ds, 6, 4, 3)
    with pytest.raises(ValueError, match=r'outside \[0, 2\)'):
        V.ValidSet.from_dataset(ds, 2, 4, n_speakers=2)


def test_config_must_fit_the_run(V):
    from zs_amd.dataloader import SyntheticDataset
    vs = V.ValidSet.from_dataset(SyntheticDataset(8, seg_len=16, n_speakers=5, seed=3), 2, 4, 5)
    hps = types.SimpleNamespace(batch_size=4)
    assert V.check_config(V.ValidConfig(10, 2, vs), hps).holdout is None
    for cfg in (V.ValidConfig(0, 2, vs), V.ValidConfig(10, 3, vs), V.ValidConfig(10, 0, vs)):
        with pytest.raises(ValueError):
            V.check_config(cfg, hps)
    with pytest.raises(ValueError, match='batch_size 8'):
        V.check_config(V.ValidConfig(10, 2, vs), types.SimpleNamespace(batch_size=8))


# ---- the finishing arithmetic --------------------------------------------------------------------------------------------------
def test_finish_against_numpy(V):
    T, F, E = 16, 513, 6
    spk_sum = np.array([10.5, 0.0, 3.25, 99.0], dtype=np.float64)
    spk_cnt = np.array([3, 0, 1, 4], dtype=np.int64)                            # speaker 1 has no samples
    rows, pairs = 40, 30
    ones = np.array([0, 40, 20, 10, 1, 39], dtype=np.uint64)                    # p = 0 and p = 1: no entropy, dead
    flips = np.array([0, 0, 15, 5, 2, 2], dtype=np.uint64)
    tab = dict(spk_sum=spk_sum, spk_cnt=spk_cnt, ones=ones, flips=flips, rows=np.array([rows]), pairs=np.array([pairs]), bad=np.array([0]))
    rec = V.finish(tab, T, F, target_ids=(2, 3))
    per = spk_sum[[0, 2, 3]] / (spk_cnt[[0, 2, 3]] * T * F)
    assert rec['valid_loss_rec'] == pytest.approx(spk_sum.sum() / (spk_cnt.sum() * T * F), rel=1e-15)
    assert list(rec['per_speaker']) == ['0', '2', '3']
    assert [rec['per_speaker'][k]['loss'] for k in ('0', '2', '3')] == pytest.approx(list(per), rel=1e-15)
    assert [rec['per_speaker'][k]['count'] for k in ('0', '2', '3')] == [3, 1, 4]
    assert rec['valid_loss_rec_target'] == pytest.approx(per[1:].mean(), rel=1e-15)
    assert rec['valid_loss_rec_worst'] == pytest.approx(per.max(), rel=1e-15)
    p = ones[2:].astype(np.float64) / rows
    assert rec['valid_bit_entropy'] == pytest.approx(float(-(p * np.log2(p) + (1 - p) * np.log2(1 - p)).sum()), rel=1e-14)
    assert rec['valid_dead_bits'] == 2
    assert rec['valid_flip_rate'] == pytest.approx(flips.sum() / (pairs * E), rel=1e-15)
    # the target speakers without samples: no target mean; speaker 1 alone as target likewise
    assert V.finish(tab, T, F, target_ids=(1,))['valid_loss_rec_target'] is None
    # T4 = 1: rows = B, pairs = 0, no flip rate (and no division)
    one = dict(tab, rows=np.array([5]), pairs=np.array([0]), ones=np.array([0, 5, 2, 3, 1, 4], dtype=np.uint64), flips=np.zeros(6, dtype=np.uint64))
    r1 = V.finish(one, T, F)
    assert r1['valid_flip_rate'] is None and r1['valid_dead_bits'] == 2 and r1['valid_bit_entropy'] > 0
    # 'continues': no unit statistics in the record
    rc = V.finish(dict(spk_sum=spk_sum, spk_cnt=spk_cnt, bad=np.array([0])), T, F, units=False)
    assert not set(V.UNIT_KEYS) & set(rc) and rc['valid_loss_rec'] == rec['valid_loss_rec']
    # a skipped sample raises on the host
    with pytest.raises(ValueError, match='speaker id'):
        V.finish(dict(tab, bad=np.array([2])), T, F)
    with pytest.raises(ValueError, match='no sample'):
        V.finish(dict(tab, spk_cnt=np.zeros(4, dtype=np.int64)), T, F)


def test_table_layout_round_trip(V):
    lay, total = V.table_layout(5, 3)
    assert total == 5 + 5 + 3 + 3 + 3 and lay['spk_sum'] == (0, 5) and lay['bad'] == (total - 1, 1)
    words = np.arange(total, dtype=np.int64)
    words[:5] = np.array([1.5, 2.5, 0.0, -1.0, 1e300]).view(np.int64)
    tab = V.split_table(words, 5, 3)
    assert tab['spk_sum'].dtype == np.float64 and list(tab['spk_sum']) == [1.5, 2.5, 0.0, -1.0, 1e300]
    assert list(tab['spk_cnt']) == [5, 6, 7, 8, 9] and list(tab['flips']) == [13, 14, 15] and int(tab['pairs'][0]) == total - 2
    assert V.table_layout(4, 0)[1] == 11                                        # 'continues': no unit columns


def test_records_round_trip(V, tmp_path):
    path = V.record_path(str(tmp_path / 'model.pth'))
    assert path == str(tmp_path / 'valid.jsonl') and V.read_records(path) == []
    rec = {'valid_loss_rec': 0.1234567890123456, 'valid_loss_rec_target': None, 'valid_loss_rec_worst': 0.5, 'valid_bit_entropy': 3.25,
           'valid_dead_bits': 2, 'valid_flip_rate': 0.125, 'per_speaker': {'0': {'loss': 0.1, 'count': 3}, '7': {'loss': 0.5, 'count': 1}}}
    for it in (2, 4, 6):
        V.append_record(path, it, rec)
    got = V.read_records(path)
    assert [r['iteration'] for r in got] == [2, 4, 6]
    assert all({k: v for k, v in r.items() if k != 'iteration'} == rec for r in got)          # floats survive bit for bit
    assert len(open(path).read().splitlines()) == 3 and '\r' not in open(path).read()
    V.truncate_records(path, 4)                                                 # a run resumed at iteration 4 writes 6 again
    assert [r['iteration'] for r in V.read_records(path)] == [2, 4]
    V.truncate_records(path, 0)
    assert V.read_records(path) == [] and os.listdir(str(tmp_path)) == ['valid.jsonl']
    assert 'loss_rec=0.12346' in V.line(6, rec) and 'dead_bits=2' in V.line(6, rec) and 'target' not in V.line(6, rec)


# ---- train state ---------------------------------------------------------------------------------------------------------------
def _stub_trainer(**over):
    net = lambda n: types.SimpleNamespace(flat_params=lambda n=n: (torch.zeros(n), torch.zeros(n)))
    kw = dict(hps=types.SimpleNamespace(batch_size=4), dtype='bf16', g_mode='targeted_residual', enc_mode='multilabel_binary',
              ae=types.SimpleNamespace(use_graph=True), nets=lambda: [net(8 * (i + 1)) for i in range(6)])
    kw.update(over)
    return types.SimpleNamespace(**kw)


def test_state_entry_absent_when_off_and_each_field_named(V):
    from zs_amd import resume
    off = resume.describe(_stub_trainer(), 'ae', False, False)
    assert 'valid' not in off and 'best_loss' not in off
    assert set(off) == {'version', 'tag', 'target_guided', 'autolocker', 'world', 'batch_size', 'dtype', 'g_mode', 'enc_mode',
                        'use_graph', 'flat_len'}                               # a file written without validation is today's
    assert 'valid' not in resume.describe(_stub_trainer(valid=None), 'ae', False, False)
    vset = types.SimpleNamespace(digest='abc')
    cfg = V.ValidConfig(2, 8, vset, 20)
    on = resume.describe(_stub_trainer(valid=cfg), 'ae', False, False)
    assert on['valid'] == {'every': 2, 'batches': 8, 'digest': 'abc', 'holdout': 20}
    assert 'valid' not in resume.describe(_stub_trainer(valid=cfg), 's2', False, False)     # only pretrain_AE validates
    resume.validate(copy.deepcopy(on), on)
    for other, word in ((V.ValidConfig(3, 8, vset, 20), 'valid_every'), (V.ValidConfig(2, 4, vset, 20), 'valid_batches'),
                        (V.ValidConfig(2, 8, types.SimpleNamespace(digest='abd'), 20), 'valid_digest'),
                        (V.ValidConfig(2, 8, vset, None), 'valid_holdout'), (V.ValidConfig(2, 8, vset, 10), 'valid_holdout')):
        with pytest.raises(ValueError, match=word):
            resume.validate(copy.deepcopy(on), resume.describe(_stub_trainer(valid=other), 'ae', False, False))
    with pytest.raises(ValueError, match='valid is on in the file, off in this run'):
        resume.validate(copy.deepcopy(on), off)
    with pytest.raises(ValueError, match='valid is off in the file, on in this run'):
        resume.validate(copy.deepcopy(off), on)


def test_find_resumable_ignores_the_best_checkpoint(V, tmp_path):
    from zs_amd import resume
    model_path = str(tmp_path / 'model.pth')
    assert V.best_path(model_path) == model_path + '-ae-best'
    os.makedirs(str(tmp_path / resume.STATE_DIR))
    for name in ('model.pth-ae-4', 'model.pth-ae-best'):
        open(str(tmp_path / name), 'w').close()
        open(resume.state_path(str(tmp_path / name)), 'w').close()              # even with a state file beside it
    found = resume.find_resumable(model_path, 'ae')
    assert found is not None and found[0] == model_path + '-ae-4' and found[2] == 4
    os.remove(model_path + '-ae-4')
    assert resume.find_resumable(model_path, 'ae') is None


def test_entry_point_is_declared_and_exported():
    import zs_amd  # noqa: F401
    from zs_amd import _lib
    assert 'zs_eval_accum' in _lib.FUNCTIONS
    names = [f for f, _ in _lib._STRUCT_FIELDS['ZsEvalAccum']]
    assert names[:5] == ['x_dec', 'ld_dec', 'x', 'ldx', 'c'] and {'spk_sum', 'spk_cnt', 'bad', 'ones', 'flips', 'rows', 'pairs'} <= set(names)
    assert hasattr(_lib.lib(), 'zs_eval_accum') and _lib.ZS_EVAL_PARTS == 8


def test_main_builds_the_sets_with_a_holdout(V, tmp_path):
    """main.training_sets, the dataset construction of every --train* mode, over a small store: --valid_holdout takes its utterances out
    of the training set only, the stage-2 sets are built as without it, and a DataLoader serves each."""
    sys.path.insert(0, ROOT)
    import main
    from zs_amd.dataloader import DataLoader
    from zs_amd.hps import make_hps
    idx = _index(n_utt=12, per=4)
    for e in idx:
        e['t'] = e['t'] % 40
    path, ipath = _store(tmp_path, idx)
    src, tgt = [e for e in idx if e['speaker'] < 2], [e for e in idx if e['speaker'] == 2]
    json.dump(src, open(str(tmp_path / 'src.json'), 'w'))
    json.dump(tgt, open(str(tmp_path / 'tgt.json'), 'w'))
    hps = make_hps(batch_size=2, seg_len=8, n_speakers=3, n_target_speakers=1)
    common = ['--dataset_path', path, '--index_path', ipath, '--index_source_path', str(tmp_path / 'src.json'), '--index_target_path',
              str(tmp_path / 'tgt.json')]
    utt = lambda es: {(e['speaker'], e['i']) for e in es}
    for mode in ('--train_ae', '--train'):
        args = _args([mode, '--valid_every', '5', '--valid_holdout', '3', '--valid_batches', '2'] + common)
        V.check_flags(args)
        dataset, sourceset, targetset, valid = main.training_sets(args, hps)
        kept, held = V.holdout_split(idx, 3)
        assert dataset.indexes == kept and len(held) == 16 and not (utt(dataset.indexes) & utt(held))
        assert sourceset.indexes == src and targetset.indexes == tgt                             # stage 2 reads its own index files, whole
        assert valid.every == 5 and valid.batches == 2 and valid.holdout == 3 and tuple(valid.set.c.shape) == (2, 2)
        assert [int(c) for c in valid.set.c.view(-1)] == [e['speaker'] for e in held[:4]]
        for ds in (dataset, sourceset, targetset):
            c, x = next(DataLoader(ds, hps.batch_size))
            assert tuple(x.shape) == (2, 8, 513) and int(c[0]) == ds.indexes[0]['speaker']
    # without validation, and with an index file of its own, the training set is the whole file
    assert main.training_sets(_args(['--train_ae'] + common), hps)[3] is None
    args = _args(['--train_ae', '--valid_every', '5', '--valid_index_path', str(tmp_path / 'tgt.json'), '--valid_batches', '1'] + common)
    dataset, _, _, valid = main.training_sets(args, hps)
    assert dataset.indexes == idx and valid.holdout is None and [int(c) for c in valid.set.c.view(-1)] == [2, 2]
    # a holdout too small for M batches is refused here, before a trainer exists
    with pytest.raises(ValueError, match='16 items'):
        main.training_sets(_args(['--train_ae', '--valid_every', '5', '--valid_holdout', '3', '--valid_batches', '9'] + common), hps)
    syn = main.training_sets(_args(['--train_ae', '--synthetic', '--valid_every', '5', '--valid_batches', '1']), hps)
    assert len(syn[0]) == 64 and tuple(syn[3].set.x.shape) == (1, 2, 8, 513)
