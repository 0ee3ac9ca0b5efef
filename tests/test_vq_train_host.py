"""Training through the vector codebook on the host: the numpy definition (tests/vq_train_ref.py) on hand-computed cases,
every refusal of main.check_vq_train by its message, the combinations it accepts, the codebook file written beside a checkpoint and
the plan's fixed-point shift.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import vq_ref as R  # noqa: E402
import vq_train_ref as T  # noqa: E402

F32 = np.float32


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def test_quantise_loss_and_gradient_by_hand():
    code = np.array([[1, 0], [0, 2]], dtype=F32)
    z = np.array([[1.5, 0.5], [0, 1], [3, 3], [-1, 0]], dtype=F32)
    idx = np.array([0, 1, 7, -1])
    q, bad = T.quantise(code, idx, 8)
    assert bad == 2 and q.shape == (4, 8) and q[:, :2].tolist() == [[1, 0], [0, 2], [0, 0], [0, 0]] and (q[:, 2:] == 0).all()
    # rows 0 and 1: (0.25 + 0.25) + (0 + 1) = 1.5; every row counts in rows * E = 8
    assert T.loss_vq(z, code, idx, 0.25) == 0.25 / 8 * 1.5
    g = T.grad_scale(0.25, 4, 2)
    assert g == F32(0.0625) and g.dtype == F32
    dq = np.full((4, 2), 2.0, dtype=F32)
    dz, bad = T.st_bwd(dq, z, code, idx, g)
    assert bad == 2 and dz.tolist() == [[2.03125, 2.03125], [2.0, 1.9375], [2, 2], [2, 2]]     # a bad row passes dq
    # bf16: one cast at the end, ties to even (2.03125 = 0x4002 is exact; 1 + 2^-8 is a tie and falls to 1, 1 + 3 * 2^-8 rises)
    assert T.bf16_round(np.array([2.03125, 1.00390625, 1.01171875], dtype=F32)).tolist() == [2.03125, 1.0, 1.015625]
    assert T.quantise(np.array([[1.00390625]], dtype=F32), [0], 8, bf16=True)[0][0, 0] == 1.0
    # the three operations are rounded one by one: g * d = 1 + 2^-22 + 2^-46 rounds to 1 + 2^-22, which dq cancels; fused, 2^-46 is left
    z1, c1, d1 = np.array([[1.0 + 2.0 ** -23]], dtype=F32), np.array([[0.0]], dtype=F32), np.array([[-(1.0 + 2.0 ** -22)]], dtype=F32)
    g1 = F32(1.0 + 2.0 ** -23)
    assert T.st_bwd(d1, z1, c1, [0], g1)[0][0, 0] == 0.0 and F32(float(g1) * float(z1[0, 0]) + float(d1[0, 0])) == F32(2.0 ** -46)


def test_ema_by_hand_K1_unused_and_starved_codewords():
    # K = 1, decay 0.5, shift 2: N' = 0.5 + 0.5 * 3 = 2, m' = 0.5 * 4 + 0.5 * (20 / 4) = 4.5, code' = 2.25
    n, m, code, cn, used = T.ema([1.0], [[4.0]], [[4.0]], [3], [[20]], 2, 0.5)
    assert n.tolist() == [2.0] and m.tolist() == [[4.5]] and code.tolist() == [[2.25]] and cn.tolist() == [5.0625] and used == 1
    assert all(a.dtype == F32 for a in (n, m, code, cn))
    # cnt = 0: N and m decay, the codeword is still m' / N' (here unchanged: both halve); not counted as used
    n, m, code, cn, used = T.ema([1.0, 1.0], [[4.0], [6.0]], [[4.0], [6.0]], [0, 2], [[0], [8]], 0, 0.5)
    assert n.tolist() == [0.5, 1.5] and m.tolist() == [[2.0], [7.0]] and used == 1
    assert code[0, 0] == 4.0 and code[1, 0] == F32(7.0 / 1.5) and cn[0] == 16.0 and cn[1] == F32(float(code[1, 0]) ** 2)
    # N' < 1e-3 leaves the row untouched (m and N still move); at exactly 1e-3 (as a double) the row is rewritten
    n, m, code, cn, used = T.ema([0.0015, 0.0025], [[9.0], [9.0]], [[5.0], [5.0]], [0, 0], [[0], [0]], 0, 0.5)
    assert n[0] == F32(0.00075) and code[0, 0] == 5.0 and m[0, 0] == 4.5
    assert float(n[1]) >= 1e-3 and code[1, 0] == F32(4.5 / float(n[1])) and cn[0] == 25.0
    # decay 0 is the k-means mean through one more rounding (m' first): within 2 fp32 spacings of vq_ref.update's mean
    x = R.planted(200, 6, 3, 0.3, 1)
    cb = R.planted(3, 6, 3, 0.3, 101)
    idx, _ = R.assign(x, cb)
    cnt, s, _ = R.accum(x, idx, 3, 30)
    n, m, code, _, used = T.ema(np.ones(3), cb, cb, cnt, s, 30, 0.0)
    mean, _, _ = R.update(cb, cnt, s, 30)
    assert np.array_equal(n, cnt.astype(F32)) and used == int((cnt > 0).sum())
    assert (np.abs(code.astype(np.float64) - mean) <= 2 * np.spacing(np.abs(mean))).all()


def test_norm_order_is_a_sum_of_squares():
    for E in (1, 6, 255, 256, 257, 1024):
        code = R.planted(5, E, 2, 1.0, E)
        got = T.norm_as_update(code)
        want = R.cnorm(code)
        assert got.dtype == F32 and (np.abs(got.astype(np.float64) - want) <= np.spacing(want)).all()
    assert T.norm_as_update(np.array([[3, 4]], dtype=F32)).tolist() == [25.0]


def test_rows_above_the_bound_are_left_out():
    z = np.array([[1, 2], [65536, 0], [0, -65535.996], [np.nan, 0], [0, -np.inf]], dtype=F32)
    ia, over = T.acc_index(z, [0, 1, 1, 0, 1])
    assert ia.tolist() == [0, -1, 1, -1, -1] and over == 3 and ia.dtype == np.int32
    st = T.State(np.array([[0, 0], [0, 1]], dtype=F32))
    cnt, used = st.step(z, np.array([0, 1, 1, 0, 1]), 30, 0.0)
    assert cnt.tolist() == [1, 1] and used == 2 and st.code.tolist() == [[1, 2], [0, float(F32(-65535.996))]]


def test_iteration_uses_the_codebook_of_the_step_before():
    z = R.planted(64, 6, 4, 0.3, 0)
    st = T.State(R.planted(5, 6, 4, 0.3, 100))
    before = st.code.copy()
    dq = np.zeros((64, 6), dtype=F32)
    out = T.iteration(st, z, dq, 0.25, 0.9, 30, 8)
    idx, _ = R.assign(z, before, R.cnorm(before))
    assert np.array_equal(out['idx'], idx) and np.array_equal(out['q'][:, :6], before[idx]) and not np.array_equal(st.code, before)
    assert out['loss_vq'] == T.loss_vq(z, before, idx, 0.25)
    assert np.array_equal(out['dz'], (T.grad_scale(0.25, 64, 6) * (z - before[idx]).astype(F32)).astype(F32))


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def _args(argv):
    import main as M
    return M.build_parser().parse_args(argv)


def _codebooks(tmp_path, E=8):
    from zs_amd.codebook import Codebook
    from zs_amd.vq import VectorCodebook
    import codebook_ref as BR
    v, b = str(tmp_path / 'K4.vq.npz'), str(tmp_path / 'K4.codebook.npz')
    VectorCodebook(R.planted(4, E, 2, 0.3, 1), {'enc_mode': 'continues', 'seed': 3}).save(v)
    Codebook(BR.planted(4, E, 2, 0.3, 1), E).save(b)
    return v, b


def test_check_vq_train_refusals_name_the_flag(tmp_path, monkeypatch):
    import main as M
    v, b = _codebooks(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    for argv, match in ((['--vq_train', v], '--vq_train .* needs --train_ae'),
                        (['--vq_train', v, '--test'], '--vq_train .* needs --train_ae'),
                        (['--vq_train', v, '--train_ae', '--train_p'], r'--vq_train .* no other --train\* mode \(got --train_p\)'),
                        (['--vq_train', v, '--train'], r'--vq_train .* \(got --train\)'),
                        (['--vq_train', v, '--train_ae', '--train_c'], r'--vq_train .* \(got --train_c\)'),
                        (['--vq_train', v, '--train_tgat'], r'--vq_train .* \(got --train_tgat\)'),
                        (['--train_ae', '--vq_beta', '0.5'], '--vq_beta needs --vq_train'),
                        (['--train_ae', '--vq_decay', '0.9'], '--vq_decay needs --vq_train'),
                        (['--vq_train', v, '--train_ae', '--resume'], '--vq_train cannot be combined with --resume'),
                        (['--vq_train', v, '--train_ae', '--valid_every', '10'], '--vq_train cannot be combined with --valid_every'),
                        (['--vq_train', v, '--train_ae', '--vq_beta', '0'], r'--vq_beta must be in \(0, 10\]'),
                        (['--vq_train', v, '--train_ae', '--vq_beta', '10.5'], r'--vq_beta must be in \(0, 10\]'),
                        (['--vq_train', v, '--train_ae', '--vq_beta', 'nan'], r'--vq_beta must be in \(0, 10\]'),
                        (['--vq_train', v, '--train_ae', '--vq_decay', '1'], r'--vq_decay must be in \[0, 1\)'),
                        (['--vq_train', v, '--train_ae', '--vq_decay', '-0.1'], r'--vq_decay must be in \[0, 1\)')):
        with pytest.raises(ValueError, match=match):
            M.check_vq_train(_args(argv))
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='--vq_train runs on one GPU'):
        M.check_vq_train(_args(['--vq_train', v, '--train_ae']))
    monkeypatch.setenv('WORLD_SIZE', '1')
    ok = _args(['--vq_train', v, '--train_ae'])
    assert M.check_vq_train(ok) is None                                     # the first call reads no file
    for mode in ('multilabel_binary', 'one_hot', 'binary'):
        with pytest.raises(ValueError, match=r"--vq_train needs enc_mode 'continues'.*%s" % mode):
            M.check_vq_train(ok, mode, 8)
    with pytest.raises(ValueError, match=r"--vq_train: enc_mode 'continues' has no units to pack"):
        M.check_vq_train(_args(['--vq_train', b, '--train_ae']), 'continues', 8)             # a bit codebook
    with pytest.raises(ValueError, match=r'--vq_train: .*field E is 8.*c_in\) is 16'):
        M.check_vq_train(ok, 'continues', 16)
    with pytest.raises(ValueError, match='--vq_train: .*not a codebook file'):
        M.check_vq_train(_args(['--vq_train', str(tmp_path / 'none.npz'), '--train_ae']), 'continues', 8)
    assert M.check_vq_train(_args(['--train_ae'])) is None and M.check_vq_train(_args(['--train_ae']), 'continues', 8) is None


def test_check_vq_train_accepts_ema_device_data_and_load_model(tmp_path, monkeypatch):
    import main as M
    from zs_amd.vq import VectorCodebook
    v, _ = _codebooks(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    args = _args(['--vq_train', v, '--train_ae', '--ema', '0.999', '--device_data', '--load_model', '--use_ema', '--synthetic', '--vq_beta', '10',
                  '--vq_decay', '0'])
    M.check_resume(args)
    M.check_ema(args)
    assert M.check_vq_train(args) is None
    cb = M.check_vq_train(args, 'continues', 8)
    assert isinstance(cb, VectorCodebook) and (cb.K, cb.E) == (4, 8) and args.vq_beta == 10.0 and args.vq_decay == 0.0


def test_argument_runner_refuses_before_anything_is_built(tmp_path, monkeypatch):
    """Through main.argument_runner with the shipped hps (enc_mode multilabel_binary, enc_size 1024): the mode, then the width."""
    import main as M
    v, _ = _codebooks(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    hps = os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')
    with pytest.raises(ValueError, match="--vq_train needs enc_mode 'continues'"):
        M.argument_runner(['--train_ae', '--synthetic', '--vq_train', v, '--hps_path', hps])
    with pytest.raises(ValueError, match=r'--vq_train: .*field E is 8.*c_in\) is 1024'):
        M.argument_runner(['--train_ae', '--synthetic', '--vq_train', v, '--hps_path', hps, '--enc_mode', 'continues'])
    args, _ = M.argument_runner(['--train_ae', '--synthetic', '--hps_path', hps])
    assert args.vq_codebook is None


# ---- the file beside a checkpoint, the plan's shift ------------------------------------------------------------------------------------
def test_trained_codebook_file_round_trip(tmp_path):
    from zs_amd import vq_train as VT
    from zs_amd.vq import VectorCodebook, load_codebook
    base = VectorCodebook(R.planted(5, 8, 2, 0.3, 1), {'enc_mode': 'continues', 'seed': 3, 'history': [[1.5, 4, 0]]})
    bn = VT.VqBottleneck.__new__(VT.VqBottleneck)                          # to_codebook reads `base` and `code` alone
    bn.base = base
    moved = (base.vectors * F32(0.5)).astype(F32)
    bn.code = torch.from_numpy(moved.copy())
    meta = {'trained_iterations': 1000, 'beta': 0.25, 'decay': 0.99, 'used': 4}
    path = VT.ckpt_path(str(tmp_path / 'model.pth-ae-1000'))
    assert path.endswith('model.pth-ae-1000.vq.npz')
    bn.to_codebook(meta).save(path)
    back = load_codebook(path, 'continues', 8)
    assert isinstance(back, VectorCodebook) and np.array_equal(back.vectors, moved) and np.array_equal(back.cnorm, R.cnorm(moved))
    assert back.meta == dict(base.meta, **meta)
    with pytest.raises(ValueError, match='vector codebook'):
        load_codebook(path, 'one_hot', 8)


def test_plan_shift_rows_and_perplexity():
    from zs_amd import vq_train as VT
    from zs_amd.vq import vq_shift
    assert VT.encoded_rows(16, 128) == 256 and VT.encoded_rows(256, 128) == 4096 and VT.encoded_rows(4, 33) == 20
    # 65536 rows 2^shift < 2^61: shift 30 up to 2^15 rows, one less per doubling after that
    for rows, want in ((1, 30), (256, 30), (4096, 30), (2 ** 15 - 1, 30), (2 ** 15, 29), (2 ** 20, 24), (2 ** 31 - 1, 14)):
        s = vq_shift(rows, 65536.0)
        assert s == want == R.vq_shift(rows, 65536.0) and rows * 65536.0 * 2.0 ** s < 2.0 ** 61
    assert VT.MAX_ABS == 65536.0 == T.MAX_ABS and VT.MIN_COUNT == T.MIN_COUNT
    assert VT.perplexity([0, 0]) == 0.0 and VT.perplexity([5, 0, 0]) == 1.0 and abs(VT.perplexity([3, 3, 3, 3]) - 4.0) < 1e-12
    for bad in (0, -1, 10.5, float('nan')):
        with pytest.raises(ValueError, match='--vq_beta'):
            VT.check_beta(bad)
    for bad in (1.0, -0.5, float('nan')):
        with pytest.raises(ValueError, match='--vq_decay'):
            VT.check_decay(bad)
    assert VT.check_beta(10) == 10.0 and VT.check_decay(0) == 0.0


def test_header_declares_the_three_entry_points():
    from zs_amd import _lib as L
    assert {'zs_vq_commit', 'zs_vq_st_bwd', 'zs_vq_ema'} <= set(L.FUNCTIONS)
    assert {'ZsVqCommit', 'ZsVqStBwd', 'ZsVqEma'} <= set(L.STRUCTS)
    assert L.ENUMS['ZS_VQ_COMMIT_PARTS'] == 1024 and L.ENUMS['ZS_VQ_MAX_ABS'] == 65536 and L.ENUMS['ZS_ABI_VERSION'] == 1
    assert dict(L.STRUCTS['ZsVqEma']._fields_)['decay'] is __import__('ctypes').c_double
