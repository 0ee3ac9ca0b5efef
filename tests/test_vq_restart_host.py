"""Restarting dead codewords on the host: the numpy definition (tests/vq_restart_ref.py) on hand-computed cases, mix64
against splitmix64's published outputs, vq_train.restart_stride for every n up to 300, every refusal of --vq_restart by its message,
the combinations it accepts, the refusals of --vq_train that stay with the flag added, and the two meta fields of the codebook file
written beside a checkpoint.  No GPU."""
import os
import sys
from math import gcd

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import vq_ref as R  # noqa: E402
import vq_restart_ref as S  # noqa: E402
import vq_train_ref as T  # noqa: E402

F32 = np.float32
ZERO = (1 << 64) - S.SALT                                         # the seed whose salted sum wraps to 0: mix64(0) = 0, start = 0
GOLD = 0x9E3779B97F4A7C15


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def test_mix64_against_hand_worked_values():
    # every step of the finaliser maps 0 to 0
    assert S.mix64(0) == 0
    # splitmix64 seeded with 0 adds the golden gamma and finalises: its first two outputs are the generator's published test vector
    assert S.mix64(GOLD) == 0xE220A8397B1DCDAF and S.mix64(2 * GOLD) == 0x6E789E6AA1B965F4
    assert S.mix64(GOLD + (1 << 64)) == S.mix64(GOLD)             # unsigned 64-bit: wraps
    assert S.start_row(ZERO, 0, 7) == 0 and S.start_row(0, ZERO, 7) == 0 and S.start_row(ZERO - 5, 5, 7) == 0
    # 0xE220A8397B1DCDAF = 5 * 0x2D39BB3EB2392923: start 0 of 5 rows; one more than a multiple of 3
    assert S.start_row(GOLD - S.SALT, 0, 5) == 0 and S.start_row(GOLD, ZERO, 3) == 1


def _state(K, E, fill=5.0):
    code = np.full((K, E), fill, dtype=F32)
    return np.ones(K, dtype=F32), code.copy(), code.copy(), np.full(K, fill * fill * E, dtype=F32)


def test_nothing_dead_equality_counted_and_nan():
    x = np.arange(8, dtype=F32).reshape(4, 2)
    N, m, code, cn = _state(5, 2)
    # k: 0 live by N; 1 N == thresh exactly (not below); 2 small N but counted; 3 NaN (not below); 4 N above
    N[:] = [1.0, 0.25, 0.01, np.nan, 0.5]
    cnt = np.array([0, 0, 3, 0, 0])
    assert not S.dead(cnt, N, 0.25).any()
    (N2, m2, code2, cn2), restarted, skipped, taken = S.restart(0.25, x, None, cnt, N, m, code, cn, ZERO, 0, 1)
    assert restarted == 0 and skipped == 0 and taken == []
    assert np.array_equal(N2, N, equal_nan=True) and np.array_equal(m2, m) and np.array_equal(code2, code) and np.array_equal(cn2, cn)
    # the comparison is in fp32: 0.1 as a double is below F32(0.1), as fp32 values they are equal
    assert not S.dead([0], np.array([0.1]), 0.1).any() and S.dead([0], [np.nextafter(F32(0.1), F32(0))], 0.1).all()
    assert S.dead([0, 1, 0], [0.0, 0.0, -1.0], 0.5).tolist() == [True, False, True]


def test_one_codeword_and_the_row_by_hand():
    x = np.array([[1, 2], [3, 4], [5, 6]], dtype=F32)
    N, m, code, cn = _state(1, 2)
    N[0] = 0.125
    # start = 0xE220A8397B1DCDAF mod 3 = 1, rank 0: row 1
    (N2, m2, code2, cn2), restarted, skipped, taken = S.restart(0.5, x, None, [0], N, m, code, cn, GOLD - S.SALT, 0, 2)
    assert taken == [(0, 1)] and restarted == 1 and skipped == 0
    assert N2.tolist() == [1.0] and m2.tolist() == [[3, 4]] and code2.tolist() == [[3, 4]] and cn2.tolist() == [25.0]
    assert all(a.dtype == F32 for a in (N2, m2, code2, cn2))
    assert N.tolist() == [0.125] and code.tolist() == [[5, 5]]                                # the inputs are left alone


def test_more_dead_codewords_than_rows_and_a_skipped_row():
    x = np.array([[1, 0], [0, 2], [3, 0]], dtype=F32)
    N, m, code, cn = _state(6, 2)
    N[:] = [0.01, 1.0, 0.01, 0.01, 0.01, 0.01]                   # dead: 0, 2, 3, 4, 5 with ranks 0 .. 4
    cnt = np.array([0, 7, 0, 0, 0, 0])
    # start 0, stride 2, n = 3: rows 0, 2, 1, then rank 3 mod 3 = 0 again: 0, 2
    assert S.rows(S.dead(cnt, N, 0.1), 3, 0, 2) == [(0, 0), (2, 2), (3, 1), (4, 0), (5, 2)]
    (N2, m2, code2, cn2), restarted, skipped, taken = S.restart(0.1, x, None, cnt, N, m, code, cn, ZERO, 0, 2)
    assert restarted == 5 and skipped == 0 and N2.tolist() == [1.0] * 6
    assert code2.tolist() == [[1, 0], [5, 5], [3, 0], [0, 2], [1, 0], [3, 0]] and np.array_equal(m2, code2)
    assert cn2.tolist() == [1.0, 50.0, 9.0, 4.0, 1.0, 9.0]
    assert np.array_equal(code2[4], code2[0]) and np.array_equal(code2[5], code2[2])         # the duplicates the definition allows
    # row 2 was left out of the average for its magnitude: the two codewords that would take it stay dead and are counted
    ia = np.array([0, 1, -1], dtype=np.int32)
    (N3, m3, code3, cn3), restarted, skipped, taken = S.restart(0.1, x, ia, cnt, N, m, code, cn, ZERO, 0, 2)
    assert restarted == 3 and skipped == 2 and taken == [(0, 0), (3, 1), (4, 0)]
    assert N3.tolist() == [1.0, 1.0, F32(0.01), 1.0, 1.0, F32(0.01)] and code3[2].tolist() == [5, 5] and cn3[5] == 50.0 and m3[5].tolist() == [5, 5]
    # the device word is added to the seed: another start, the same ranks
    (_, _, code4, _), _, _, taken = S.restart(0.1, x, None, cnt, N, m, code, cn, GOLD, ZERO, 2)
    assert taken == [(0, 1), (2, 0), (3, 2), (4, 1), (5, 0)] and code4[0].tolist() == [0, 2]


def test_the_norm_is_the_averages_order():
    x = R.planted(3, 700, 2, 1.0, 5)
    N, m, code, cn = _state(2, 700)
    N[1] = 0.0
    (N2, m2, code2, cn2), _, _, taken = S.restart(0.5, x, None, [0, 0], N, m, code, cn, ZERO, 0, 1)
    assert taken == [(1, 0)] and cn2[1] == T.norm_as_update(x[:1])[0] and cn2[0] == cn[0]
    assert abs(float(cn2[1]) - float((x[0].astype(np.float64) ** 2).sum())) <= np.spacing(cn2[1])


def test_step_is_the_average_then_the_restart():
    z = R.planted(40, 6, 4, 0.3, 0)
    far = np.full((2, 6), 1000.0, dtype=F32)
    st = T.State(np.concatenate([R.planted(3, 6, 4, 0.3, 100), far]))
    shift = R.vq_shift(40, T.MAX_ABS)
    seen = []
    for t in range(5):
        idx, _ = R.assign(z, st.code, st.cnorm)
        cnt, used, restarted, skipped, taken = S.step(st, z, idx, shift, 0.5, 0.1, 3, t, S.stride(40))
        seen.append((restarted, st.N[3:].tolist()))
    # N of the two far codewords: 0.5, 0.25, 0.125, 0.0625 < 0.1 on the fourth step and not before
    assert [s[0] for s in seen[:4]] == [0, 0, 0, 2] and seen[2][1] == [0.125, 0.125] and seen[3][1] == [1.0, 1.0]
    assert np.abs(st.code[3:]).max() < 100.0


# ---- the stride ----------------------------------------------------------------------------------------------------------------------
def test_restart_stride_is_coprime_in_range_and_gives_distinct_rows():
    from zs_amd import vq_train as VT
    for n in range(1, 301):
        s = VT.restart_stride(n)
        top = max(1, int(np.floor(0.6180339887 * n)))
        assert 1 <= s <= top and gcd(s, n) == 1 and s == S.stride(n)
        assert not any(gcd(t, n) == 1 for t in range(s + 1, top + 1))                     # the largest such
        for start in (0, n // 2, n - 1):
            got = [r for _, r in S.rows(np.ones(n, bool), n, start, s)]
            assert sorted(got) == list(range(n))
    assert VT.restart_stride(256) == 157 and VT.restart_stride(4096) == 2531 and VT.restart_stride(1) == 1
    with pytest.raises(ValueError):
        VT.restart_stride(0)
    for bad in (0, 1, 1.5, -0.1, float('nan')):
        with pytest.raises(ValueError, match=r'--vq_restart must be in \(0, 1\)'):
            VT.check_restart(bad)
    assert VT.check_restart('0.25') == 0.25 and VT.check_restart(1e-6) == 1e-6


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def _args(argv):
    import main as M
    return M.build_parser().parse_args(argv)


def _codebook(tmp_path, E=8):
    from zs_amd.vq import VectorCodebook
    v = str(tmp_path / 'K4.vq.npz')
    VectorCodebook(R.planted(4, E, 2, 0.3, 1), {'enc_mode': 'continues', 'seed': 3}).save(v)
    return v


def test_vq_restart_refusals_name_the_flag(tmp_path, monkeypatch):
    import main as M
    v = _codebook(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    for argv, match in ((['--train_ae', '--vq_restart', '0.1'], '--vq_restart needs --vq_train'),
                        (['--vq_restart', '0.1'], '--vq_restart needs --vq_train'),
                        (['--vq_train', v, '--train_ae', '--vq_restart', '0'], r'--vq_restart must be in \(0, 1\) \(got 0'),
                        (['--vq_train', v, '--train_ae', '--vq_restart', '1'], r'--vq_restart must be in \(0, 1\)'),
                        (['--vq_train', v, '--train_ae', '--vq_restart', '-0.5'], r'--vq_restart must be in \(0, 1\)'),
                        (['--vq_train', v, '--train_ae', '--vq_restart', 'nan'], r'--vq_restart must be in \(0, 1\)'),
                        # what --vq_train refused before, it refuses with the flag added
                        (['--vq_train', v, '--vq_restart', '0.1'], '--vq_train .* needs --train_ae'),
                        (['--vq_train', v, '--train_ae', '--train_p', '--vq_restart', '0.1'], r'--vq_train .* \(got --train_p\)'),
                        (['--vq_train', v, '--train_ae', '--resume', '--vq_restart', '0.1'], '--vq_train cannot be combined with --resume'),
                        (['--vq_train', v, '--train_ae', '--valid_every', '10', '--vq_restart', '0.1'],
                         '--vq_train cannot be combined with --valid_every'),
                        (['--vq_train', v, '--train_ae', '--vq_beta', '0', '--vq_restart', '0.1'], r'--vq_beta must be in \(0, 10\]'),
                        (['--vq_train', v, '--train_ae', '--vq_decay', '1', '--vq_restart', '0.1'], r'--vq_decay must be in \[0, 1\)')):
        with pytest.raises(ValueError, match=match):
            M.check_vq_train(_args(argv))
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='--vq_train runs on one GPU'):
        M.check_vq_train(_args(['--vq_train', v, '--train_ae', '--vq_restart', '0.1']))
    monkeypatch.setenv('WORLD_SIZE', '1')
    ok = _args(['--vq_train', v, '--train_ae', '--vq_restart', '0.1'])
    assert M.check_vq_train(ok) is None
    with pytest.raises(ValueError, match=r"--vq_train needs enc_mode 'continues'.*one_hot"):
        M.check_vq_train(ok, 'one_hot', 8)
    with pytest.raises(ValueError, match=r'--vq_train: .*field E is 8.*c_in\) is 16'):
        M.check_vq_train(ok, 'continues', 16)
    assert _args(['--train_ae']).vq_restart is None


def test_vq_restart_accepted_with_ema_device_data_and_load_model(tmp_path, monkeypatch):
    import main as M
    from zs_amd.vq import VectorCodebook
    v = _codebook(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    args = _args(['--vq_train', v, '--train_ae', '--ema', '0.999', '--device_data', '--load_model', '--use_ema', '--synthetic', '--vq_decay', '0.5',
                  '--vq_restart', '0.01'])
    M.check_resume(args)
    M.check_ema(args)
    assert M.check_vq_train(args) is None
    cb = M.check_vq_train(args, 'continues', 8)
    assert isinstance(cb, VectorCodebook) and (cb.K, cb.E) == (4, 8) and args.vq_restart == 0.01


def test_argument_runner_refuses_the_flag_before_anything_is_built(monkeypatch):
    import main as M
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    hps = os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')
    with pytest.raises(ValueError, match='--vq_restart needs --vq_train'):
        M.argument_runner(['--train_ae', '--synthetic', '--vq_restart', '0.1', '--hps_path', hps])


# ---- the file beside a checkpoint ------------------------------------------------------------------------------------------------------
def test_meta_round_trip_with_and_without_restart(tmp_path):
    from zs_amd import vq_train as VT
    from zs_amd.vq import VectorCodebook, load_codebook
    base = VectorCodebook(R.planted(5, 8, 2, 0.3, 1), {'enc_mode': 'continues', 'seed': 3})
    bn = VT.VqBottleneck.__new__(VT.VqBottleneck)                          # ckpt_meta and to_codebook read these fields alone
    bn.base, bn.beta, bn.decay, bn.restart = base, 0.25, 0.5, 0.1
    bn.code = torch.from_numpy(base.vectors.copy())
    meta = bn.ckpt_meta(12, {'used': 4, 'restarts': 9, 'dead': 1, 'skipped': 0})
    assert meta == {'trained_iterations': 12, 'beta': 0.25, 'decay': 0.5, 'used': 4, 'restart': 0.1, 'restarts': 9}
    path = VT.ckpt_path(str(tmp_path / 'model.pth-ae-12'))
    bn.to_codebook(meta).save(path)
    back = load_codebook(path, 'continues', 8)
    assert back.meta == dict(base.meta, **meta) and back.meta['restart'] == 0.1 and back.meta['restarts'] == 9
    bn.restart = None                                                      # off: the fields of before, no more
    assert bn.ckpt_meta(12, {'used': 4}) == {'trained_iterations': 12, 'beta': 0.25, 'decay': 0.5, 'used': 4}


def test_header_declares_the_entry_point():
    import ctypes
    from zs_amd import _lib as L
    assert 'zs_vq_restart' in L.FUNCTIONS and 'ZsVqRestart' in L.STRUCTS
    f = dict(L.STRUCTS['ZsVqRestart']._fields_)
    assert f['thresh'] is ctypes.c_float and f['seed'] is ctypes.c_uint64 and f['stride'] is ctypes.c_int32 and f['n'] is ctypes.c_int64
