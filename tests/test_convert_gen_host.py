"""Host-side pieces of batched conversion with the generator: the --cross_test work plan (convert.py:268-300) and the target check
that runs before anything is enqueued (trainer.py:202-203).  No GPU needed."""
import os
from types import SimpleNamespace

import pytest

import zs_amd  # noqa: F401
from zs_amd import convert as cv

STORE = {
    'train': ['S015', 'S020', 'V001', 'V002'],
    'test': ['S089', 'S130'],
    'train/S015': ['0001', '0002'], 'train/S020': ['0003'], 'train/V001': ['0004'], 'train/V002': ['0005'],
    'test/S089': ['0010'], 'test/S130': ['0012', '0011'],
}


def _keys(prefix):
    return list(STORE[prefix])


@pytest.mark.parametrize('flag', ['test', 'train'])
def test_cross_test_plan_pairs_and_paths(flag, tmp_path):
    res = str(tmp_path)
    plan = cv.cross_test_plan(_keys, flag, res)
    srcs = ['S089', 'S130'] if flag == 'test' else ['S015', 'S020']
    want = []
    for src in srcs:
        for tar in ('V001', 'V002'):
            for utt in sorted(STORE['%s/%s' % (flag, src)]):
                d = os.path.join(res, '%s_to_%s' % (src, tar))
                want.append((src, tar, utt, '%s/%s/%s/lin' % (flag, src, utt), d, os.path.join(d, '%s_%s.wav' % (tar, utt)),
                             os.path.join(d, '%s_%s.txt' % (src, utt))))
    got = [(p['src'], p['tar'], p['utt'], p['key'], p['dir'], p['wav'], p['txt']) for p in plan]
    assert got == want
    assert len(plan) == 3 * 2                                 # three source utterances, two targets
    assert not os.listdir(res)                            # a plan writes nothing


def test_cross_test_plan_rejects_unknown_flag(tmp_path):
    with pytest.raises(ValueError):
        cv.cross_test_plan(_keys, 'dev', str(tmp_path))


def test_store_keys_on_both_containers(tmp_path):
    import numpy as np
    from zs_amd.dataloader import NpzStore
    path = str(tmp_path / 's.npz')
    np.savez(path, **{'test/S130/0001/lin': np.zeros((2, 513), np.float32), 'test/S130/0002/lin': np.zeros((2, 513), np.float32),
                      'test/S089/0003/lin': np.zeros((2, 513), np.float32)})
    st = NpzStore(path, 'r')
    assert cv.store_keys(st, 'test') == ['S089', 'S130'] and cv.store_keys(st, 'test/S130') == ['0001', '0002']

    class H5Like(dict):                                   # h5py.File: f[prefix] is a group with .keys()
        pass
    h5 = H5Like({'test': {'S130': {}, 'S089': {}}})
    assert cv.store_keys(h5, 'test') == ['S089', 'S130']


def _trainer_stub(g_mode, n_speakers=6, n_target=2):
    hps = SimpleNamespace(n_speakers=n_speakers, n_target_speakers=n_target)
    c_a = n_speakers if g_mode == 'naive' else n_target
    return SimpleNamespace(g_mode=g_mode, hps=hps, Generator=SimpleNamespace(c_a=c_a))


@pytest.mark.parametrize('g_mode', ['targeted', 'targeted_residual', 'spectrogram'])
def test_target_check_of_targeted_generators(g_mode):
    tr = _trainer_stub(g_mode)
    assert cv.check_gen_targets(tr, [4, 5, 4]) == 4
    for bad in ([3], [4, 0], [5, 3]):
        with pytest.raises(RuntimeError, match='can only convert to target speakers'):
            cv.check_gen_targets(tr, bad)
    with pytest.raises(ValueError):
        cv.check_gen_targets(tr, [6])


def test_target_check_of_naive_generator():
    tr = _trainer_stub('naive')
    assert cv.check_gen_targets(tr, list(range(6))) == 0
    for bad in ([6], [-1]):
        with pytest.raises(ValueError):
            cv.check_gen_targets(tr, bad)


def test_target_check_rejects_generators_without_a_batched_path():
    with pytest.raises(NotImplementedError):
        cv.check_gen_targets(_trainer_stub('enhanced'), [4])
