"""Quantiser dropout on the host: the numpy definition (tests/rvq_drop_ref.py) on hand-computed cases -- the draw, the
threshold, the distribution of the counts, the masked cascade --, every refusal of --rvq_dropout by its message and the combinations it
accepts, include/zs_amd_rvq_drop.h against the C compiler and the binding's tables, and the launch sequence of RvqBottleneck with and
without dropout.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import rvq_drop_ref as D  # noqa: E402
import rvq_train_ref as RT  # noqa: E402
import vq_ref as R  # noqa: E402
import vq_restart_ref as X  # noqa: E402

F32 = np.float32
HPS = os.path.join(ROOT, 'hps', 'zerospeech_english_1024.json')


# ---- the draw ------------------------------------------------------------------------------------------------------------------------
def test_the_draw_by_hand():
    """u_b for a few (seed, word at seed_ptr, b), worked out once with 64-bit integers and written down here; mix64 is the one the
    restart's definition (tests/vq_restart_ref.py) has."""
    assert D.SALT == int.from_bytes(b'RVQ_DROP', 'big') == 5933019028717195088
    cases = (((0, 0, 0), 0xebde58b13e0a4905), ((1, 0, 0), 0xf0f68564c5a32c49), ((0, 7, 3), 0xe30bb51375b807af),
             ((2 ** 64 - 1, 5, 4095), 0x7b4ed5b7f3422bbd), ((3, 0x123456789ABCDEF0, 17), 0xe2730fc2fe1eb5b4))
    for (seed, word, b), u in cases:
        assert D.u_of(seed, word, b) == u == X.mix64((seed + word + D.SALT + b * 0x9E3779B97F4A7C15) & D.M64)
    # the top 24 bits against thr, the low 32 modulo S
    u = 0xebde58b13e0a4905
    assert u >> 40 == 15457880 and u & 0xFFFFFFFF == 1040861445
    assert D.count_of(u, 15457880, 4) == 4 and D.count_of(u, 15457881, 4) == 1 + 1040861445 % 4 == 2
    assert D.count_of(u, 15457881, 1) == 1 and D.count_of(u, 15457881, 8) == 1 + 1040861445 % 8 == 6
    # seed and the device word are added: the same sum, the same draw; the sample index is spread by the golden ratio
    assert np.array_equal(D.draw(0, 1, 8, 3, D.threshold(0.5)), D.draw(1, 0, 8, 3, D.threshold(0.5)))
    assert D.draw(0, 0, 8, 3, D.threshold(0.5)).tolist() == [3, 1, 2, 3, 2, 2, 3, 3]
    assert D.draw(0, 1, 8, 3, D.threshold(0.5)).tolist() == [3, 3, 3, 3, 2, 3, 3, 3]
    assert D.draw(0, 0, 8, 3, D.threshold(0.5)).dtype == np.int32


def test_the_threshold_and_either_side_of_it():
    assert D.threshold(1.0) == 2 ** 24 and D.threshold(0.5) == 2 ** 23 and D.threshold(2.0 ** -24) == 1 and D.threshold(0.3) == 5033164
    assert D.threshold(np.nextafter(1.0, 0.0)) == 2 ** 24 - 1
    thr, S = D.threshold(0.3), 5
    below, at = ((thr - 1) << 40) | 0xFFFFFFFFFF, (thr << 40) | 7                 # the largest u that drops, a u that does not
    assert D.count_of(below, thr, S) == 1 + 0xFFFFFFFF % S == 1 and D.count_of(at, thr, S) == S
    assert D.count_of(at, thr + 1, S) == 1 + 7 % S == 3
    # P = 1: the 24 bits are always below 2^24, so every sample drops (to a count that may be S itself)
    for u in (0, D.M64, (2 ** 24 - 1) << 40, 0xebde58b13e0a4905):
        assert D.count_of(u, D.threshold(1.0), 4) == 1 + (u & 0xFFFFFFFF) % 4
    s = D.draw(9, 2, 512, 4, D.threshold(1.0))
    assert np.array_equal(s, [1 + (D.u_of(9, 2, b) & 0xFFFFFFFF) % 4 for b in range(512)]) and set(s.tolist()) == {1, 2, 3, 4}


def test_the_counts_at_s4_b4096_p_half():
    """Deterministic: the counts of this seed, written down.  Every value occurs; S takes the samples that do not drop and a quarter of
    those that do: 0.5 + 0.5 / 4 = 0.625 of 4096 = 2560 on average, with a standard deviation of sqrt(4096 * 0.625 * 0.375) = 31."""
    s = D.draw(0, 0, 4096, 4, D.threshold(0.5))
    cnt = np.bincount(s, minlength=5)
    assert cnt.tolist() == [0, 498, 555, 549, 2494]
    dropped = sum(1 for b in range(4096) if (D.u_of(0, 0, b) >> 40) < 2 ** 23)
    assert cnt[4] == (4096 - dropped) + sum(1 for b in range(4096) if (D.u_of(0, 0, b) >> 40) < 2 ** 23 and (D.u_of(0, 0, b) & 0xFFFFFFFF) % 4 == 3)
    assert abs(cnt[4] - 2560) < 4 * 31 and abs(dropped - 2048) < 4 * 32
    assert D.active(s, 4, 3).tolist() == [3 * 4096, 3 * (4096 - 498), 3 * (4096 - 498 - 555), 3 * 2494]
    assert np.bincount(D.draw(5, 9, 4096, 4, D.threshold(0.5)), minlength=5).tolist() == [0, 485, 504, 520, 2587]


# ---- the masked cascade ----------------------------------------------------------------------------------------------------------------
CODES = [np.array([[1, 0], [0, 2]], dtype=F32), np.array([[0.5, 0.5], [0, -1]], dtype=F32), np.array([[0.25, 0], [0, 0.5]], dtype=F32)]
Z = np.array([[1.5, 0.5], [0, 1], [0.25, 2.75]], dtype=F32)
IDXS = [[0, 1, 1], [0, 1, 0], [0, 1, 1]]


def test_the_masked_cascade_by_hand():
    """S = 3, three samples of one row with s_use = (1, 3, 2); everything is a dyadic fraction.  Sample 0 stops behind stage 0: r_2 = r_3
    = r_1 and a = r_1; sample 2 stops behind stage 1."""
    c = D.cascade(Z, CODES, [1, 3, 2], 1, idxs=IDXS)
    assert c['idx'].tolist() == IDXS                                          # the assignment is complete: all rows, every stage
    assert c['idx_acc'].tolist() == [[0, 1, 1], [-1, 1, 0], [-1, 1, -1]]
    assert c['r'][1].tolist() == [[0.5, 0.5], [0, -1], [0.25, 0.75]]
    assert c['r'][2].tolist() == [[0.5, 0.5], [0, 0], [-0.25, 0.25]]
    assert c['r'][3].tolist() == [[0.5, 0.5], [0, -0.5], [-0.25, 0.25]]
    assert c['a'].tolist() == [[0.5, 0.5], [0, -1.5], [0, 1]]
    assert c['sq'] == [0.5 + 1.0 + 0.625, 0.125, 0.25] and c['bad'] == 0 and c['over'] == 0
    q, bad = D.operand(CODES, c['idx'], [1, 3, 2], 1, 8)
    assert bad == 0 and q[:, :2].tolist() == [[1, 0], [0, 1.5], [0.5, 2.5]] and (q[:, 2:] == 0).all()
    assert D.active([1, 3, 2], 3, 1).tolist() == [3, 2, 1] and D.active([1, 3, 2], 3, 5).tolist() == [15, 10, 5]
    lv, per = RT.losses(c['sq'], 0.25, 3, 2)                                    # the masked mean: over all n rows, whatever took part
    assert per == [0.25 / 6 * 2.125, 0.25 / 6 * 0.125, 0.25 / 6 * 0.25] and lv == 0.25 / 6 * 2.5
    dz = RT.st_bwd(np.zeros((3, 2), F32), c['a'], F32(0.5))
    assert dz.tolist() == [[0.25, 0.25], [0, -0.75], [0, 0.5]]                 # sample 0: stage 0's residual alone


def test_all_counts_at_s_is_the_unmasked_definition_and_rows_follow_their_fragment():
    codes = [R.planted(5, 6, 3, 0.3, s) * F32(0.5 ** s) for s in range(3)]
    z = R.planted(35, 6, 3, 0.3, 9)
    full = RT.cascade(z, codes)
    c = D.cascade(z, codes, [3] * 5, 7)
    for k in ('idx', 'idx_acc', 'a'):
        assert np.array_equal(c[k], full[k])
    assert c['sq'] == full['sq'] and all(np.array_equal(a, b) for a, b in zip(c['r'], full['r']))
    assert np.array_equal(D.operand(codes, c['idx'], [3] * 5, 7, 8)[0], RT.operand(codes, full['idx'], 8)[0])
    s_use = [2, 1, 3, 1, 2]                                                    # rows 7 b .. 7 b + 6 follow sample b
    c = D.cascade(z, codes, s_use, 7)
    for b, su in enumerate(s_use):
        rows = slice(7 * b, 7 * b + 7)
        part = RT.cascade(z[rows], codes[:su], idxs=c['idx'][:su, rows])
        assert np.array_equal(c['a'][rows], part['a']) and np.array_equal(c['r'][-1][rows], part['r'][-1])
        assert np.array_equal(c['idx_acc'][:su, rows], part['idx_acc']) and (c['idx_acc'][su:, rows] == -1).all()
        assert np.array_equal(D.operand(codes, c['idx'], s_use, 7, 8)[0][rows], RT.operand(codes[:su], c['idx'][:su, rows], 8)[0])
    assert D.row_mask(s_use, 7, 35, 1).tolist() == [True] * 7 + [False] * 7 + [True] * 7 + [False] * 7 + [True] * 7


def test_bad_input_counts_only_where_the_row_takes_part():
    """A bad index and a row at ZS_VQ_MAX_ABS at a stage the sample does not use: copied, idx_acc -1, no counter moves.  A count
    outside [1, S]: zero rows in the operand, a bad frame each, and the fragment's indices are not looked at."""
    idxs = [[0, 1, 1], [7, 1, -1], [2 ** 30, 1, 9]]
    c = D.cascade(Z, CODES, [1, 3, 2], 1, idxs=idxs)
    assert c['bad'] == 1 and c['idx_acc'].tolist() == [[0, 1, 1], [-1, 1, -1], [-1, 1, -1]]     # sample 2's -1 at its active stage 1
    assert c['r'][2][2].tolist() == [0.25, 0.75] and c['a'][2].tolist() == [0.25, 0.75]
    z = Z.copy()
    z[0, 1] = np.inf
    c = D.cascade(z, CODES, [1, 3, 2], 1, idxs=IDXS)
    assert c['over'] == 1 and c['idx_acc'][:, 0].tolist() == [-1, -1, -1] and c['r'][3][0].tolist() == [0.5, np.inf]
    q, bad = D.operand(CODES, [[0, 5, 1], [0, 1, 0], [0, 1, 1]], [0, 4, 2], 1, 8)
    assert bad == 2 and (q[:2] == 0).all() and q[2, :2].tolist() == [0.5, 2.5]
    q, bad = D.operand(CODES, [[0, 1, 1], [9, 1, 0], [9, 1, 9]], [1, 3, 2], 1, 8)                # bad planes behind the count: not read
    assert bad == 0 and q[:, :2].tolist() == [[1, 0], [0, 1.5], [0.5, 2.5]]


def test_an_iteration_leaves_the_unused_stages_codebooks_to_the_rows_that_used_them():
    vec = np.stack([R.planted(4, 6, 2, 0.3, 1), R.planted(4, 6, 2, 0.3, 2) * F32(0.1)])
    z = R.planted(64, 6, 2, 0.3, 5)
    s_use = [1, 2] * 4
    st = RT.State(vec)
    out = D.iteration(st, z, np.zeros((64, 6), F32), 0.25, 0.0, 30, 8, 8, s_use)
    assert out['active'].tolist() == [64, 32]
    live = out['idx_acc'][1] >= 0
    assert live.sum() == 32 and np.array_equal(live, D.row_mask(s_use, 8, 64, 1))
    for k in np.unique(out['idx'][1][live]):                                   # decay 0: the mean of the rows that took part
        mean = out['r'][1][live & (out['idx'][1] == k)].astype(np.float64).mean(0)
        assert np.abs(st.stages[1].code[k] - mean).max() < 1e-6


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def _args(argv):
    import main as M
    return M.build_parser().parse_args(argv)


def _files(tmp_path, E=8):
    from zs_amd.rvq import ResidualCodebook
    from zs_amd.vq import VectorCodebook
    r, v = str(tmp_path / 'K4x2.rvq.npz'), str(tmp_path / 'K4.vq.npz')
    ResidualCodebook(np.stack([R.planted(4, E, 2, 0.3, 1), R.planted(4, E, 2, 0.3, 2) * F32(0.1)]), {'enc_mode': 'continues', 'seed': 3}).save(r)
    VectorCodebook(R.planted(4, E, 2, 0.3, 1), {'enc_mode': 'continues', 'seed': 3}).save(v)
    return r, v


def test_rvq_dropout_refusals_name_the_flag(tmp_path, monkeypatch):
    import main as M
    r, v = _files(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    for argv, match in ((['--train_ae', '--rvq_dropout', '0.5'], '--rvq_dropout needs --rvq_train'),
                        (['--rvq_dropout', '0.5'], '--rvq_dropout needs --rvq_train'),
                        (['--train_ae', '--vq_train', v, '--rvq_dropout', '0.5'], '--rvq_dropout cannot be combined with --vq_train'),
                        (['--train_ae', '--vq_train', v, '--rvq_train', r, '--rvq_dropout', '0.5'], '--rvq_dropout cannot be combined with --vq_train'),
                        (['--train_ae', '--rvq_train', r, '--rvq_dropout', '0'], r'--rvq_dropout must be in \(0, 1\]'),
                        (['--train_ae', '--rvq_train', r, '--rvq_dropout', '-0.5'], r'--rvq_dropout must be in \(0, 1\]'),
                        (['--train_ae', '--rvq_train', r, '--rvq_dropout', '1.0000001'], r'--rvq_dropout must be in \(0, 1\]'),
                        (['--train_ae', '--rvq_train', r, '--rvq_dropout', 'nan'], r'--rvq_dropout must be in \(0, 1\]'),
                        (['--train_ae', '--rvq_train', r, '--rvq_dropout', 'inf'], r'--rvq_dropout must be in \(0, 1\]'),
                        (['--train_ae', '--rvq_train', r, '--rvq_dropout', '1e-9'], r'--rvq_dropout must be at least 2\^-24'),
                        # what --rvq_train refuses stays refused, in its words
                        (['--train_ae', '--rvq_train', r, '--rvq_dropout', '0.5', '--resume'], '--rvq_train cannot be combined with --resume'),
                        (['--train_ae', '--rvq_train', r, '--rvq_dropout', '0.5', '--valid_every', '5'], '--rvq_train cannot be combined with --valid_every'),
                        (['--train_p', '--rvq_train', r, '--rvq_dropout', '0.5'], r'--rvq_train .* \(got --train_p\)')):
        with pytest.raises(ValueError, match=match):
            M.check_rvq_train(_args(argv))
    with pytest.raises(SystemExit):                                         # not a number: the parser's own refusal
        _args(['--train_ae', '--rvq_train', r, '--rvq_dropout', 'half'])
    # through argument_runner with the shipped hps: before hps is read, so before anything is built
    for argv, match in ((['--train_ae', '--synthetic', '--rvq_dropout', '0.5', '--hps_path', HPS], '--rvq_dropout needs --rvq_train'),
                        (['--train_ae', '--synthetic', '--rvq_train', r, '--rvq_dropout', '2', '--hps_path', str(tmp_path / 'none.json')],
                         r'--rvq_dropout must be in \(0, 1\]')):
        with pytest.raises(ValueError, match=match):
            M.argument_runner(argv)
    args, _ = M.argument_runner(['--train_ae', '--synthetic', '--hps_path', HPS])
    assert args.rvq_dropout is None


def test_rvq_dropout_is_accepted_with_everything_rvq_train_accepts(tmp_path, monkeypatch):
    import main as M
    from zs_amd.rvq import ResidualCodebook
    r, _ = _files(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    for p in ('1', '1.0', '0.5', '6e-8', '0.999'):
        args = _args(['--rvq_train', r, '--train_ae', '--rvq_dropout', p])
        assert M.check_vq_train(args) is None and M.check_rvq_train(args) is None and args.rvq_dropout == float(p)
    args = _args(['--rvq_train', r, '--train_ae', '--rvq_dropout', '0.25', '--ema', '0.999', '--device_data', '--load_model', '--use_ema', '--synthetic',
                  '--vq_beta', '10', '--vq_decay', '0', '--vq_restart', '0.25'])
    M.check_resume(args)
    M.check_ema(args)
    assert M.check_vq_train(args) is None and M.check_rvq_train(args) is None and M.check_vq_train(args, 'continues', 8) is None
    cb = M.check_rvq_train(args, 'continues', 8)
    assert isinstance(cb, ResidualCodebook) and (cb.S, cb.K, cb.E) == (2, 4, 8) and args.rvq_dropout == 0.25


def test_check_dropout_and_the_threshold_the_host_computes():
    from zs_amd import rvq_train as VT
    assert VT.check_dropout(1) == 1.0 and VT.check_dropout('0.5') == 0.5 and VT.DROP_ONE == D.THR_ONE
    for p in (1.0, 0.5, 0.3, 2.0 ** -24, float(np.nextafter(1.0, 0.0)), 0.1, 1.0 / 3.0):
        assert VT.drop_threshold(p) == D.threshold(p) and 1 <= VT.drop_threshold(VT.check_dropout(p)) <= 2 ** 24
    for bad in (0, -1, 1.5, float('nan'), float('inf'), None, 'x', 2.0 ** -25):
        with pytest.raises(ValueError, match='--rvq_dropout must be'):
            VT.check_dropout(bad)


# ---- the header and the binding ----------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_in_tables_of_their_own():
    from zs_amd import _lib
    assert _lib.DROP_FUNCTIONS == ['zs_rvq_drop_draw', 'zs_rvq_commit_drop', 'zs_rvq_gather_frag']      # include/zs_amd_rvq_drop.h, in its order
    for fn, st in (('zs_rvq_drop_draw', 'ZsRvqDropDraw'), ('zs_rvq_commit_drop', 'ZsRvqCommitDrop'), ('zs_rvq_gather_frag', 'ZsRvqGatherFrag')):
        assert _lib.DROP_PROTOS[fn][2] == st and st in _lib.DROP_STRUCTS
        assert st not in _lib.STRUCTS and st not in _lib.SEGMENT_STRUCTS and fn not in _lib.FUNCTIONS and fn not in _lib.PROTOS
    # the counts the earlier parts pin
    assert len(_lib.FUNCTIONS) == 98 and _lib.SEGMENT_FUNCTIONS == ['zs_vq_scores', 'zs_code_scores', 'zs_seg_viterbi']
    assert len(_lib.PROTOS) == 101 and _lib.ENUMS['ZS_ABI_VERSION'] == 1
    assert _lib.ENUMS['ZS_RVQ_DROP_SALT'] == _lib.ZS_RVQ_DROP_SALT == D.SALT and _lib.ZS_RVQ_DROP_THR_ONE == 2 ** 24
    # ZsRvqCommitDrop is ZsRvqCommit's fields, in order, and three more; ZsRvqGatherFrag is ZsRvqGather with s_use a pointer
    commit = [f for f, _ in _lib._STRUCT_FIELDS['ZsRvqCommit']]
    assert [f for f, _ in _lib._DROP_STRUCT_FIELDS['ZsRvqCommitDrop']] == commit + ['s_use', 'rows_per_frag', 'stage']
    assert dict(_lib._DROP_STRUCT_FIELDS['ZsRvqCommitDrop'])['s_use'] is ctypes.c_void_p
    gather = [f for f, _ in _lib._STRUCT_FIELDS['ZsRvqGather']]
    assert [f for f, _ in _lib._DROP_STRUCT_FIELDS['ZsRvqGatherFrag']] == gather
    assert dict(_lib._DROP_STRUCT_FIELDS['ZsRvqGatherFrag'])['s_use'] is ctypes.c_void_p and dict(_lib._STRUCT_FIELDS['ZsRvqGather'])['s_use'] is ctypes.c_int32
    assert [f for f, _ in _lib._DROP_STRUCT_FIELDS['ZsRvqDropDraw']] == ['seed', 'seed_ptr', 'thr', 'S', 'n_frag', 'rows_per_frag', 's_use', 'active']
    if os.path.exists(_lib.LIB_PATH):                                 # a built tree: the library exports what the header declares
        assert all(hasattr(_lib.lib(), f) for f in _lib.DROP_FUNCTIONS)
    from zs_amd import build
    assert os.path.exists(os.path.join(build.CSRC, 'zs_rvq_drop.hip')) and os.path.join(build.CSRC, 'zs_rvq_drop.hip') in build.sources()


def test_drop_header_matches_the_c_compiler(tmp_path):
    """gcc's sizeof and offsetof of every struct against the generated ctypes Structures, the constants, and the size of every
    parameter against the generated argtypes."""
    from zs_amd import _lib
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){\n' % _lib.DROP_HEADER
    for n in _lib.DROP_STRUCTS:
        src += 'printf("%s %%zu\\n", sizeof(%s));\n' % (n, n)
        for f, _ in _lib._DROP_STRUCT_FIELDS[n]:
            src += 'printf("%s.%s %%zu\\n", offsetof(%s,%s));\n' % (n, f, n, f)
    src += 'printf("salt %llu\\n", (unsigned long long)ZS_RVQ_DROP_SALT);\nprintf("one %d\\n", ZS_RVQ_DROP_THR_ONE);\nreturn 0;}\n'
    c = tmp_path / 'drop.c'
    c.write_text(src)
    subprocess.check_call(['gcc', '-Wall', '-Werror', str(c), '-o', str(tmp_path / 'drop')])
    seen = 0
    for line in subprocess.check_output([str(tmp_path / 'drop')]).decode().split('\n'):
        if not line:
            continue
        k, v = line.split()
        seen += 1
        if k == 'salt':
            assert int(v) == D.SALT == 0x5256515F44524F50
        elif k == 'one':
            assert int(v) == 2 ** 24
        elif '.' in k:
            n, f = k.split('.')
            assert getattr(_lib.DROP_STRUCTS[n], f).offset == int(v), k
        else:
            assert ctypes.sizeof(_lib.DROP_STRUCTS[k]) == int(v), k
    assert seen == 2 + sum(1 + len(_lib._DROP_STRUCT_FIELDS[n]) for n in _lib.DROP_STRUCTS) == 2 + 3 + 8 + 24 + 18
    for fn in _lib.DROP_FUNCTIONS:
        res, args, st = _lib.DROP_PROTOS[fn]
        assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_void_p] and st in _lib.DROP_STRUCTS


# ---- the launch sequence ---------------------------------------------------------------------------------------------------------------
class _HostCtx(object):
    """What RvqBottleneck reads of a layers.Ctx, on the CPU: the launches are recorded, never made."""
    stream = 0

    def __init__(self):
        from zs_amd import _lib as L
        self.device, self.tdt, self.dt, self._bufs = torch.device('cpu'), torch.float32, L.ZS_F32, {}

    def act(self, name, B, T, C):
        from zs_amd import layers
        t = self._bufs.setdefault(name, torch.zeros(B * T * 32 + 64))
        return layers.Act(t, B, T, C, 32)


def _recorded(monkeypatch, dropout, restart=None, B=3, Tq=4):
    from zs_amd import _lib as L
    from zs_amd.rvq import ResidualCodebook
    from zs_amd.rvq_train import RvqBottleneck
    calls = []

    def record(fname, sname, stream, **kw):
        cls = L.STRUCTS.get(sname) or L.SEGMENT_STRUCTS.get(sname) or L.DROP_STRUCTS[sname]
        cls(**{k: v for k, v in kw.items() if v is not None})                 # the fields exist and take these values
        calls.append((fname, sname, kw))
    monkeypatch.setattr(L, 'call', record)
    vec = np.stack([R.planted(5, 8, 2, 0.3, s) * F32(0.3 ** s) for s in range(3)])
    ctx = _HostCtx()
    bn = RvqBottleneck(ResidualCodebook(vec, {'enc_mode': 'continues'}), 0.25, 0.99, B * Tq, ctx, restart=restart, dropout=dropout)
    bits = ctx.act('z', B, Tq, 8)
    bn.forward(bits, 3, None)
    bn.backward(ctx.act('dz', B, Tq, 8))
    return bn, calls


def test_without_dropout_the_bottleneck_records_no_new_entry_point(monkeypatch):
    from zs_amd import _lib as L
    bn, calls = _recorded(monkeypatch, None, restart=0.5)
    stage = ['zs_vq_assign', 'zs_rvq_commit', 'zs_vq_accum', 'zs_vq_ema', 'zs_vq_restart']
    assert [c[0] for c in calls] == stage * 3 + ['zs_rvq_loss', 'zs_rvq_gather', 'zs_rvq_st_bwd']
    assert not [c for c in calls if c[0] in L.DROP_FUNCTIONS or c[1] in L.DROP_STRUCTS]
    assert bn.dropout is None and not hasattr(bn, 'active') and not hasattr(bn, 's_use')
    assert 'dropout' not in bn.ckpt_meta(5, {'used': [1, 1, 1], 'restarts': 0})


def test_with_dropout_the_three_take_their_places_with_fixed_arguments(monkeypatch):
    from zs_amd import _lib as L
    bn, calls = _recorded(monkeypatch, 0.3, restart=0.5)
    stage = ['zs_vq_assign', 'zs_rvq_commit_drop', 'zs_vq_accum', 'zs_vq_ema', 'zs_vq_restart']
    assert [c[0] for c in calls] == ['zs_rvq_drop_draw'] + stage * 3 + ['zs_rvq_loss', 'zs_rvq_gather_frag', 'zs_rvq_st_bwd']
    draw = calls[0][2]
    assert draw['thr'] == D.threshold(0.3) and draw['S'] == 3 and draw['n_frag'] == 3 and draw['rows_per_frag'] == 4 and draw['seed'] == 3
    assert draw['s_use'] == L.ptr(bn.s_use) and draw['active'] == L.ptr(bn.active) and bn.s_use.shape == (3,) and bn.active.shape == (3,)
    commits = [c[2] for c in calls if c[0] == 'zs_rvq_commit_drop']
    assert [c['stage'] for c in commits] == [0, 1, 2] and [c['first'] for c in commits] == [1, 0, 0]
    assert all(c['s_use'] == draw['s_use'] and c['rows_per_frag'] == 4 and c['n'] == 12 for c in commits)
    g = calls[-2][2]
    assert g['s_use'] == draw['s_use'] and g['S'] == 3 and g['n_frag'] == 3 and g['T'] == 4 and g['ld_idx'] == 12 and g['bad'] == L.ptr(bn.stat, 2)
    first = [(c[0], sorted(c[2].items(), key=str)) for c in calls]
    del calls[:]
    bn.forward(bn._bits, 3, None)                                              # a second step: the same buffers, the same arguments
    bn.backward(bn.ctx.act('dz', 3, 4, 8))
    assert [(c[0], sorted(c[2].items(), key=str)) for c in calls] == first and len(bn._s_use) == 1
    assert bn.ckpt_meta(5, {'used': [1, 1, 1], 'restarts': 0})['dropout'] == 0.3
    with pytest.raises(ValueError, match='dropout'):
        _recorded(monkeypatch, 1.5)
