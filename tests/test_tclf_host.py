"""Host logic of the target speaker classifier (--train_c / --test_classify): the command line, the t_classify relabel
(trainer.py:617-624), the fragment plan of target_classify (convert.py:379-397) and its scoring rule (convert.py:399-413).
No GPU needed."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HPS = os.path.join(ROOT, 'hps', 'zerospeech_english.json')


def test_train_c_and_test_classify_are_in_scope():
    import main
    assert 'train_c' not in main.OUT_OF_SCOPE and 'test_classify' not in main.OUT_OF_SCOPE
    for blocked in ('train_al', 'train_t', 'test_asr', 'encode'):         # still unbuilt
        assert blocked in main.OUT_OF_SCOPE


def test_load_tclf_model_name_parses():
    import main
    args, _ = main.argument_runner(['--test_classify', '--load_tclf_model_name', '/x/model.pth-tclf-3', '--hps_path', HPS])
    assert args.test_classify and args.load_tclf_model_name == '/x/model.pth-tclf-3'
    args, _ = main.argument_runner(['--train_c', '--synthetic', '--hps_path', HPS])
    assert args.train_c and args.synthetic and args.load_tclf_model_name is None and not args.train


def _ref_relabel(c, n_speakers, n_target_speakers):
    """trainer.py:617-624 restated: c[c < 100] = 102; label = c - shift_c."""
    c = torch.as_tensor(c).clone()
    c[c < 100] = 102
    return c - int(n_speakers - n_target_speakers)


def test_relabel_matches_reference_rule():
    from zs_amd.trainer import tclf_labels
    c = torch.tensor([0, 5, 57, 99, 100, 101, 42, 100])
    y = tclf_labels(c, 102, 2, 'targeted_residual')
    assert y.dtype == torch.int64 and torch.equal(y, _ref_relabel(c, 102, 2))
    assert y.tolist() == [2, 2, 2, 2, 0, 1, 2, 0]
    assert torch.equal(c, torch.tensor([0, 5, 57, 99, 100, 101, 42, 100]))        # the caller's batch is not changed
    for g_mode in ('targeted', 'spectrogram'):
        assert torch.equal(tclf_labels(np.array([3, 100, 101]), 102, 2, g_mode), torch.tensor([2, 0, 1]))


def test_relabel_raises_outside_three_classes_and_for_naive():
    from zs_amd.trainer import tclf_labels
    with pytest.raises(ValueError):
        tclf_labels(torch.tensor([0, 1, 2]), 4, 2, 'targeted_residual')            # 102 - 2 = 100: no such class
    with pytest.raises(ValueError):
        tclf_labels(torch.tensor([100, 103]), 102, 2, 'targeted')                  # 103 - 100 = 3
    with pytest.raises(ValueError):
        tclf_labels(torch.tensor([101, 5]), 102, 3, 'targeted')                    # shift 99: 101 -> 2, but 5 -> 102 -> 3
    with pytest.raises(ValueError, match='naive'):
        tclf_labels(torch.tensor([100]), 102, 2, 'naive')
    assert tclf_labels(torch.tensor([102]), 102, 2, 'targeted').tolist() == [2]


def _ref_plan(n_frames, seg_len):
    """convert.py:379-397 restated on a dummy spectrogram: the (utterance-local) first row of every fragment classified."""
    spec = np.arange(n_frames, dtype=np.float64)[:, None] * np.ones((1, 2))
    if len(spec) < seg_len:
        spec = np.concatenate((spec, np.zeros((seg_len - spec.shape[0], spec.shape[1]))), axis=0)
    starts = []
    for idx in range(0, len(spec), seg_len):
        if idx + (seg_len * 2) > len(spec):
            spec_frag = spec[idx:-1]
        else:
            spec_frag = spec[idx:idx + seg_len]
        if len(spec_frag) >= seg_len:
            frag = spec_frag[:seg_len]
            assert np.array_equal(frag[:, 0], np.arange(idx, idx + seg_len))
            starts.append(idx)
        elif idx == 0:
            raise RuntimeError('Please check if input is too short!')
    return starts


@pytest.mark.parametrize('seg_len', [128, 64])
def test_fragment_plan_matches_reference(seg_len):
    from zs_amd.convert import tclf_plan
    lengths = [seg_len + 1, seg_len + 2, 2 * seg_len - 1, 2 * seg_len, 2 * seg_len + 1, 3 * seg_len, 3 * seg_len + 1, 5 * seg_len - 7,
               700, 257, 129, 384, 385, 1000]
    plan = tclf_plan(lengths, seg_len)
    want = [(u, s) for u, n in enumerate(lengths) for s in _ref_plan(n, seg_len)]
    assert plan == want
    for u, s in plan:
        assert 0 <= s and s + seg_len <= lengths[u]                   # every row read is a real frame
    for n in (1, 9, seg_len - 1, seg_len):                            # padded to seg_len, then the tail rule leaves nothing
        with pytest.raises(RuntimeError):
            _ref_plan(n, seg_len)
        with pytest.raises(RuntimeError):
            tclf_plan([700, n], seg_len)


def _ref_score(logits, tar_speaker):
    """convert.py:399-413 restated."""
    acc = []
    for logit in logits:
        am = logit.argmax()
        clf_speaker = 'V001' if am == 0 else ('V002' if am == 1 else 'None')
        acc.append(1 if clf_speaker == tar_speaker else 0)
    return acc


def test_scoring_rule_with_ties_and_none():
    from zs_amd.convert import tclf_predict, tclf_targets
    logits = np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 1.0], [0.0, 1.0, 3.0],
                       [1.0, 1.0, 0.0],         # tie 0/1 -> V001
                       [0.0, 2.0, 2.0],         # tie 1/2 -> V002
                       [5.0, 1.0, 5.0],         # tie 0/2 -> V001
                       [-1.0, -1.0, -1.0],      # three-way tie -> V001
                       [0.0, -0.0, -1.0]], dtype=np.float32)
    assert tclf_predict(logits) == ['V001', 'V002', 'None', 'V001', 'V002', 'V001', 'V001', 'V001']
    assert tclf_targets(['V001', 'V002', 'None', 'S015', 'V003']).tolist() == [0, 1, 2, -1, -1]
    for tar in ('V001', 'V002', 'S015', 'None'):
        want = _ref_score(logits, tar)
        got = [int(p == tar) for p in tclf_predict(logits)]
        assert got == want
        t = tclf_targets([tar] * len(logits))
        assert [int(np.argmax(l) == k) for l, k in zip(logits, t)] == want      # the rule zs_tclf_score applies on the device


def test_header_declares_the_new_entry_points():
    from zs_amd import _lib
    assert {'zs_frag_gather', 'zs_tclf_score'} <= set(_lib.FUNCTIONS)
    names = lambda s: [f for f, _ in _lib._STRUCT_FIELDS[s]]
    assert names('ZsFragGather') == ['src', 'utt_stride', 'n_utt', 'T_max', 'table', 'n_frag', 'seg_len', 'dst']
    assert names('ZsTclfScore') == ['logits', 'ld', 'target', 'n_frag', 'pred', 'correct', 'count']
