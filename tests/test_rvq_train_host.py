"""Training through the residual codebook on the host: the numpy definition (tests/rvq_train_ref.py) on hand-computed
cases, every refusal of main.check_rvq_train by its message, the combinations it accepts, the options that serve either flag, the
.rvq.npz written beside a checkpoint and --vq_train still refusing a residual file.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import rvq_ref as Q  # noqa: E402
import rvq_train_ref as RT  # noqa: E402
import vq_ref as R  # noqa: E402
import vq_train_ref as T  # noqa: E402

F32 = np.float32
HPS = os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def test_two_stages_by_hand():
    """z = (1.5, 0.5), (0, 1); stage 0 takes (1, 0) and (0, 2), stage 1 (0.5, 0.5) and (0, -1): everything is a dyadic fraction."""
    codes = [np.array([[1, 0], [0, 2]], dtype=F32), np.array([[0.5, 0.5], [0, -1]], dtype=F32)]
    z = np.array([[1.5, 0.5], [0, 1]], dtype=F32)
    c = RT.cascade(z, codes)
    assert c['idx'].tolist() == [[0, 1], [0, 1]] and c['idx_acc'].tolist() == [[0, 1], [0, 1]]
    assert c['r'][1].tolist() == [[0.5, 0.5], [0, -1]] and c['r'][2].tolist() == [[0, 0], [0, 0]]
    assert c['a'].tolist() == [[0.5, 0.5], [0, -1]]                         # a_2 = r_1 + r_2
    assert c['sq'] == [0.25 + 0.25 + 1.0, 0.0] and c['bad'] == 0 and c['over'] == 0
    lv, per = RT.losses(c['sq'], 0.25, 2, 2)
    assert lv == 0.25 / 4 * 1.5 and per == [lv, 0.0]
    q, bad = RT.operand(codes, c['idx'], 8)
    assert bad == 0 and q[:, :2].tolist() == [[1.5, 0.5], [0, 1]] and (q[:, 2:] == 0).all()
    g = RT.grad_scale(0.25, 2, 2)
    assert g == F32(0.125)
    dq = np.array([[1, 1], [2, 2]], dtype=F32)
    assert RT.st_bwd(dq, c['a'], g).tolist() == [[1.0625, 1.0625], [2, 1.875]]


def test_three_stages_the_cascade_is_snap_and_the_operand_is_reconstruct():
    codes = [R.planted(5, 6, 3, 0.3, s) * F32(0.5 ** s) for s in range(3)]
    z = R.planted(40, 6, 3, 0.3, 9)
    c = RT.cascade(z, codes)
    idx, _, rs = Q.snap(z, codes)
    assert np.array_equal(c['idx'], idx) and len(c['r']) == 4 and all(np.array_equal(a, b) for a, b in zip(c['r'], rs))
    a = (c['r'][1] + c['r'][2]).astype(F32)
    a = (a + c['r'][3]).astype(F32)                                          # a's add order: ((r_1 + r_2) + r_3)
    assert np.array_equal(c['a'], a)
    q, _ = RT.operand(codes, c['idx'], 8, bf16=True)
    want, _ = Q.reconstruct(idx, codes, None, True)
    assert np.array_equal(q[:, :6], want)
    assert RT.losses(c['sq'], 0.25, 40, 6)[0] == 0.25 / 240 * ((c['sq'][0] + c['sq'][1]) + c['sq'][2])
    for s in range(3):
        assert c['sq'][s] == float((c['r'][s + 1].astype(np.float64) ** 2).sum())


def test_the_add_order_of_a_shows():
    """r_1 = 1, r_2 = 2^-24, r_3 = 2^-24: (1 + 2^-24) rounds to 1 (half to even) twice; 1 + (2^-24 + 2^-24) would be 1 + 2^-23."""
    t = F32(2.0 ** -24)
    # stage 0 leaves r_1 = 1; stage 1 subtracts 1 - 2^-24 (exact in fp32), leaving 2^-24; stage 2 subtracts 0
    codes = [np.array([[0]], dtype=F32), np.array([[F32(1) - t]], dtype=F32), np.array([[0]], dtype=F32)]
    z = np.array([[1]], dtype=F32)
    c = RT.cascade(z, codes, idxs=[[0], [0], [0]])
    assert c['r'][1][0, 0] == 1 and c['r'][2][0, 0] == t and c['r'][3][0, 0] == t
    assert c['a'][0, 0] == F32(1) and F32(1) + (t + t) == F32(1) + F32(2.0 ** -23) != F32(1)


def test_one_codeword_per_stage():
    codes = [np.array([[1, 2, 3]], dtype=F32), np.array([[0.5, 0, -1]], dtype=F32)]
    z = np.array([[2, 2, 2], [0, 0, 0]], dtype=F32)
    c = RT.cascade(z, codes)
    assert (c['idx'] == 0).all() and c['r'][2].tolist() == [[0.5, 0, 0], [-1.5, -2, -2]]
    assert c['a'].tolist() == [[1.5, 0, -1], [-2.5, -4, -5]]
    st = RT.State(np.stack(codes))
    out = RT.iteration(st, z, np.zeros((2, 3), F32), 0.25, 0.0, 30, 8)
    assert out['used'] == [1, 1]
    assert np.array_equal(st.stages[0].code, [[1, 1, 1]]) and np.array_equal(st.stages[1].code, [[0, -1, -2]])   # decay 0: the means


def test_a_bad_index_at_stage_one():
    """Never an index: the row passes to r_2 unsubtracted, adds nothing to stage 1's loss or to a, idx_acc is -1, it is counted, and
    the frame is a zero row of the operand."""
    codes = [np.array([[1, 0], [0, 2]], dtype=F32), np.array([[0.5, 0.5], [0, -1]], dtype=F32)]
    z = np.array([[1.5, 0.5], [0, 1]], dtype=F32)
    for bad_k in (2, -1, 2 ** 30, -2 ** 31):
        c = RT.cascade(z, codes, idxs=[[0, 1], [bad_k, 1]])
        assert c['bad'] == 1 and c['idx_acc'].tolist() == [[0, 1], [-1, 1]]
        assert c['r'][2].tolist() == [[0.5, 0.5], [0, 0]] and c['a'].tolist() == [[0.5, 0.5], [0, -1]]
        assert c['sq'] == [1.5, 0.0]
        q, bad = RT.operand(codes, c['idx'], 8)
        assert bad == 1 and (q[0] == 0).all() and q[1, :2].tolist() == [0, 1]
    c = RT.cascade(z, codes, idxs=[[5, 1], [0, 1]])                         # at the first stage a is zero, r_1 is z
    assert c['r'][1][0].tolist() == [1.5, 0.5] and c['a'][0].tolist() == [1.0, 0.0] and c['idx_acc'].tolist() == [[-1, 1], [0, 1]]


def test_a_row_at_the_bound_in_r1_only():
    """z = 32768 is below ZS_VQ_MAX_ABS; code_0 = -32768 leaves r_1 = 65536: stage 0 accumulates the row, stage 1 does not."""
    codes = [np.array([[-32768, 0], [0, 0]], dtype=F32), np.array([[1, 1], [0, 0]], dtype=F32)]
    z = np.array([[32768, 0], [0.25, 0.5]], dtype=F32)
    c = RT.cascade(z, codes, idxs=[[0, 1], [0, 1]])
    assert c['r'][1][0].tolist() == [65536, 0] and c['over'] == 1
    assert c['idx_acc'].tolist() == [[0, 1], [-1, 1]]
    assert c['r'][2][0].tolist() == [65535, -1]                              # it is quantised like any other
    for v in (np.inf, np.nan, -70000.0):
        z2 = z.copy()
        z2[1, 1] = v
        c = RT.cascade(z2, codes, idxs=[[0, 1], [0, 1]])
        assert c['idx_acc'].tolist() == [[0, -1], [-1, -1]] and c['over'] == 3


def test_the_three_roundings_of_dz():
    """g a rounded, dq + that rounded, then the cast: each differs from the fused or the exact result."""
    g = F32(1) + F32(2.0 ** -12)
    a = np.array([[g]], dtype=F32)                                            # g a = 1 + 2^-11 + 2^-24: a tie, to even: 1 + 2^-11
    dq = np.array([[F32(-1)]], dtype=F32)
    assert float(g) * float(g) == 1 + 2.0 ** -11 + 2.0 ** -24
    assert RT.st_bwd(dq, a, g)[0, 0] == F32(2.0 ** -11)                       # a fused multiply-add would give 2^-11 + 2^-24
    one24 = np.array([[F32(2.0 ** 24)]], dtype=F32)
    assert RT.st_bwd(one24, np.array([[F32(1)]], dtype=F32), F32(1))[0, 0] == F32(2.0 ** 24)       # 2^24 + 1: a tie, to even
    dq2 = np.array([[F32(2.0 ** 24) + F32(2)]], dtype=F32)                    # odd in units of 2: the tie goes up
    assert RT.st_bwd(dq2, np.array([[F32(1)]], dtype=F32), F32(1))[0, 0] == F32(2.0 ** 24) + F32(4)
    # the cast: 1 + 2^-8 is a tie between bf16 1 and 1 + 2^-7 and goes to even; the fp32 sum is kept without bf16
    one = np.array([[F32(1)]], dtype=F32)
    assert RT.st_bwd(one, one, F32(2.0 ** -8))[0, 0] == F32(1) + F32(2.0 ** -8)
    assert RT.st_bwd(one, one, F32(2.0 ** -8), bf16=True)[0, 0] == F32(1)
    assert RT.st_bwd(one, one, F32(3 * 2.0 ** -8), bf16=True)[0, 0] == F32(1) + F32(2.0 ** -6)


def test_one_stage_is_the_single_stage_definition():
    z, code = R.planted(50, 6, 4, 0.3, 1), R.planted(7, 6, 4, 0.3, 2)
    idx, _ = R.assign(z, code, R.cnorm(code))
    idx[3] = 7
    c = RT.cascade(z, [code], idxs=[idx])
    dq = np.random.RandomState(0).standard_normal((50, 6)).astype(F32)
    for bf16 in (False, True):
        want, _ = T.st_bwd(dq, z, code, idx, T.grad_scale(0.25, 50, 6), bf16)
        assert np.array_equal(RT.st_bwd(dq, c['a'], RT.grad_scale(0.25, 50, 6), bf16), want)
    ia, _ = T.acc_index(z, idx)
    ia[3] = -1
    assert np.array_equal(c['idx_acc'][0], ia)
    assert abs(RT.losses(c['sq'], 0.25, 50, 6)[0] - T.loss_vq(z, code, idx, 0.25)) <= 1e-6 * T.loss_vq(z, code, idx, 0.25)
    assert np.array_equal(RT.operand([code], c['idx'], 8)[0], T.quantise(code, idx, 8)[0])


def test_an_iteration_reads_the_codebooks_the_step_before_left_and_seeds_the_stages_apart():
    vec = np.stack([R.planted(4, 6, 2, 0.3, 1), R.planted(4, 6, 2, 0.3, 2) * F32(0.1)])
    z = R.planted(64, 6, 2, 0.3, 5)
    st = RT.State(vec)
    out = RT.iteration(st, z, np.zeros((64, 6), F32), 0.25, 0.9, 30, 8, restart=0.5, seed=3, seed_dev=0, stride=39)
    c = RT.cascade(z, list(vec))
    assert np.array_equal(out['idx'], c['idx']) and np.array_equal(out['q'][:, :6], Q.reconstruct(c['idx'], list(vec))[0])
    assert not np.array_equal(st.stages[0].code, vec[0]) and not np.array_equal(st.stages[1].code, vec[1])
    assert RT.stage_seed(3, 0) == 3 and RT.stage_seed(3, 1) == 3 + 0x9E3779B97F4A7C15
    assert RT.stage_seed(2 ** 64 - 1, 1) == 0x9E3779B97F4A7C15 - 1                             # mod 2^64


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def _args(argv):
    import main as M
    return M.build_parser().parse_args(argv)


def _files(tmp_path, E=8):
    from zs_amd.codebook import Codebook
    from zs_amd.rvq import ResidualCodebook
    from zs_amd.vq import VectorCodebook
    import codebook_ref as BR
    r, v, b = str(tmp_path / 'K4x2.rvq.npz'), str(tmp_path / 'K4.vq.npz'), str(tmp_path / 'K4.codebook.npz')
    ResidualCodebook(np.stack([R.planted(4, E, 2, 0.3, 1), R.planted(4, E, 2, 0.3, 2) * F32(0.1)]), {'enc_mode': 'continues', 'seed': 3}).save(r)
    VectorCodebook(R.planted(4, E, 2, 0.3, 1), {'enc_mode': 'continues', 'seed': 3}).save(v)
    Codebook(BR.planted(4, E, 2, 0.3, 1), E).save(b)
    return r, v, b


def test_check_rvq_train_refusals_name_the_flag(tmp_path, monkeypatch):
    import main as M
    r, v, b = _files(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    for argv, match in ((['--rvq_train', r, '--vq_train', v, '--train_ae'], '--rvq_train cannot be combined with --vq_train'),
                        (['--rvq_train', r], '--rvq_train .* needs --train_ae'),
                        (['--rvq_train', r, '--test'], '--rvq_train .* needs --train_ae'),
                        (['--rvq_train', r, '--train_ae', '--train_p'], r'--rvq_train .* no other --train\* mode \(got --train_p\)'),
                        (['--rvq_train', r, '--train'], r'--rvq_train .* \(got --train\)'),
                        (['--rvq_train', r, '--train_ae', '--train_c'], r'--rvq_train .* \(got --train_c\)'),
                        (['--rvq_train', r, '--train_tgat'], r'--rvq_train .* \(got --train_tgat\)'),
                        (['--rvq_train', r, '--train_ae', '--resume'], '--rvq_train cannot be combined with --resume'),
                        (['--rvq_train', r, '--train_ae', '--valid_every', '10'], '--rvq_train cannot be combined with --valid_every'),
                        (['--rvq_train', r, '--train_ae', '--vq_beta', '0'], r'--vq_beta must be in \(0, 10\]'),
                        (['--rvq_train', r, '--train_ae', '--vq_decay', '1'], r'--vq_decay must be in \[0, 1\)'),
                        (['--rvq_train', r, '--train_ae', '--vq_restart', '1'], r'--vq_restart must be in \(0, 1\)')):
        with pytest.raises(ValueError, match=match):
            M.check_rvq_train(_args(argv))
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='--rvq_train runs on one GPU'):
        M.check_rvq_train(_args(['--rvq_train', r, '--train_ae']))
    monkeypatch.setenv('WORLD_SIZE', '1')
    ok = _args(['--rvq_train', r, '--train_ae'])
    assert M.check_rvq_train(ok) is None                                    # the first call reads no file
    for mode in ('multilabel_binary', 'one_hot', 'binary'):
        with pytest.raises(ValueError, match=r"--rvq_train needs enc_mode 'continues'.*%s" % mode):
            M.check_rvq_train(ok, mode, 8)
    with pytest.raises(ValueError, match=r"--rvq_train: .*K4\.vq\.npz is no residual codebook \(kind 'vector'\)"):
        M.check_rvq_train(_args(['--rvq_train', v, '--train_ae']), 'continues', 8)
    with pytest.raises(ValueError, match=r"--rvq_train: enc_mode 'continues' has no units to pack"):
        M.check_rvq_train(_args(['--rvq_train', b, '--train_ae']), 'continues', 8)            # a bit codebook, in its own words
    with pytest.raises(ValueError, match=r'--rvq_train: .*field E is 8.*c_in\) is 16'):
        M.check_rvq_train(ok, 'continues', 16)
    with pytest.raises(ValueError, match='--rvq_train: .*not a codebook file'):
        M.check_rvq_train(_args(['--rvq_train', str(tmp_path / 'none.npz'), '--train_ae']), 'continues', 8)
    assert M.check_rvq_train(_args(['--train_ae'])) is None and M.check_rvq_train(_args(['--train_ae']), 'continues', 8) is None


def test_the_options_serve_either_flag_and_are_refused_without_both(tmp_path, monkeypatch):
    import main as M
    r, v, _ = _files(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    for flag, val in (('--vq_beta', '0.5'), ('--vq_decay', '0.9'), ('--vq_restart', '0.1')):
        with pytest.raises(ValueError, match='%s needs --vq_train' % flag):                     # the words the earlier tests pin
            M.check_vq_train(_args(['--train_ae', flag, val]))
        for train, path in (('--rvq_train', r), ('--vq_train', v)):
            args = _args(['--train_ae', train, path, flag, val])
            assert M.check_vq_train(args) is None and M.check_rvq_train(args) is None


def test_check_rvq_train_accepts_ema_device_data_and_load_model(tmp_path, monkeypatch):
    import main as M
    from zs_amd.rvq import ResidualCodebook
    r, _, _ = _files(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    args = _args(['--rvq_train', r, '--train_ae', '--ema', '0.999', '--device_data', '--load_model', '--use_ema', '--synthetic', '--vq_beta', '10',
                  '--vq_decay', '0', '--vq_restart', '0.25'])
    M.check_resume(args)
    M.check_ema(args)
    assert M.check_vq_train(args) is None and M.check_rvq_train(args) is None
    assert M.check_vq_train(args, 'continues', 8) is None
    cb = M.check_rvq_train(args, 'continues', 8)
    assert isinstance(cb, ResidualCodebook) and (cb.S, cb.K, cb.E) == (2, 4, 8) and args.vq_beta == 10.0 and args.vq_restart == 0.25


def test_argument_runner_refuses_before_anything_is_built(tmp_path, monkeypatch):
    """Through main.argument_runner with the shipped hps (enc_mode multilabel_binary, enc_size 1024): the mode, then the width."""
    import main as M
    r, v, _ = _files(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    with pytest.raises(ValueError, match="--rvq_train needs enc_mode 'continues'"):
        M.argument_runner(['--train_ae', '--synthetic', '--rvq_train', r, '--hps_path', HPS])
    with pytest.raises(ValueError, match=r'--rvq_train: .*field E is 8.*c_in\) is 1024'):
        M.argument_runner(['--train_ae', '--synthetic', '--rvq_train', r, '--hps_path', HPS, '--enc_mode', 'continues'])
    with pytest.raises(ValueError, match='--rvq_train cannot be combined with --vq_train'):
        M.argument_runner(['--train_ae', '--synthetic', '--rvq_train', r, '--vq_train', v, '--hps_path', HPS, '--enc_mode', 'continues'])
    args, _ = M.argument_runner(['--train_ae', '--synthetic', '--hps_path', HPS])
    assert args.vq_codebook is None and args.rvq_train is None


def test_vq_train_still_refuses_a_residual_file(tmp_path, monkeypatch):
    import main as M
    r, _, _ = _files(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    with pytest.raises(ValueError, match=r"--vq_train: .*K4x2\.rvq\.npz is a residual codebook \(kind 'residual'\): training through a residual"):
        M.check_vq_train(_args(['--train_ae', '--vq_train', r]), 'continues', 8)


# ---- the file beside a checkpoint ------------------------------------------------------------------------------------------------------
def test_trained_codebook_file_round_trip_and_its_removal(tmp_path):
    from zs_amd import resume, rvq_train as VT
    from zs_amd.rvq import ResidualCodebook
    from zs_amd.vq import load_codebook
    base = ResidualCodebook(np.stack([R.planted(5, 8, 2, 0.3, 1), R.planted(5, 8, 2, 0.3, 2), R.planted(5, 8, 2, 0.3, 3)]),
                            {'enc_mode': 'continues', 'seed': 3, 'bits_per_unit': 4.5})
    bn = VT.RvqBottleneck.__new__(VT.RvqBottleneck)                        # to_codebook reads `base` and `code` alone
    bn.base, bn.beta, bn.decay, bn.restart = base, 0.25, 0.99, 0.1
    moved = (base.vectors * F32(0.5)).astype(F32)
    bn.code = torch.from_numpy(moved.copy())
    meta = bn.ckpt_meta(1000, {'used': [4, 3, 5], 'restarts': 7})
    assert meta == {'trained_iterations': 1000, 'beta': 0.25, 'decay': 0.99, 'used': [4, 3, 5], 'restart': 0.1, 'restarts': 7}
    ckpt = str(tmp_path / 'model.pth-ae-1000')
    path = VT.ckpt_path(ckpt)
    assert path.endswith('model.pth-ae-1000.rvq.npz') and bn.kind == 'residual'
    bn.to_codebook(meta).save(path)
    back = load_codebook(path, 'continues', 8)
    assert isinstance(back, ResidualCodebook) and back.S == 3 and np.array_equal(back.vectors, moved)
    assert np.array_equal(back.cnorm, np.stack([R.cnorm(m) for m in moved])) and back.meta == dict(base.meta, **meta)
    assert back.with_stages(1).stages == 1                                   # the file --rvq_stages reads
    open(ckpt, 'w').close()
    resume.remove_checkpoint(ckpt)
    assert not os.path.exists(ckpt) and not os.path.exists(path)


def test_the_bottleneck_wants_a_residual_codebook():
    from zs_amd import rvq_train as VT
    from zs_amd.vq import VectorCodebook
    with pytest.raises(ValueError, match='a residual codebook'):
        VT.RvqBottleneck(VectorCodebook(R.planted(4, 8, 2, 0.3, 1), {'enc_mode': 'continues'}), rows=4)
