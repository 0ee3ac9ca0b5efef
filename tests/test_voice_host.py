"""Voice adaptation without a GPU (zs_amd.voice, main.check_voice): the voice file and its refusals, the segment planner, the name
resolution, the extended Decoder tables, and every command-line combination that is refused before anything is built."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope='module')
def V():
    import zs_amd  # noqa: F401
    from zs_amd import voice
    return voice


def _decoder_sd(c_h=8, n_spk=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {'conv1.weight': torch.randn(2 * c_h, c_h, 3, generator=g), 'conv1.bias': torch.randn(2 * c_h, generator=g),
          'linear.weight': torch.randn(5, c_h, generator=g)}
    for i in range(1, 6):
        sd['emb%d.weight' % i] = torch.randn(n_spk, c_h, generator=g)
    return sd


# ---- the voice file ----------------------------------------------------------------------------------------------------------------
def test_voice_file_round_trip_and_refusals(V, tmp_path):
    sd = _decoder_sd()
    digest = V.decoder_digest(sd)
    rows = [np.random.RandomState(i).randn(8).astype(np.float32) for i in range(5)]
    path = str(tmp_path / 'sub' / 'ANNA.voice.npz')
    meta = V.save_voice(path, rows, {'digest': digest, 'seg_len': 128, 'iterations': 7, 'final_loss': 0.125, 'init': 'mean',
                                     'utterances': 3, 'frames': 900})
    assert meta['version'] == V.VOICE_VERSION and meta['c_h'] == 8
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ['emb1', 'emb2', 'emb3', 'emb4', 'emb5', 'meta']
        assert all(z['emb%d' % i].dtype == np.float32 and z['emb%d' % i].shape == (8,) for i in range(1, 6))
        assert json.loads(str(z['meta'])) == meta
    got, m2 = V.load_voice(path, c_h=8, digest=digest)
    assert m2 == meta and all(np.array_equal(a, b) and a.dtype == np.float32 for a, b in zip(got, rows))
    assert {'version', 'c_h', 'seg_len', 'iterations', 'final_loss', 'init', 'utterances', 'frames', 'digest'} <= set(m2)
    V.load_voice(path)                                                         # nothing to compare with: nothing refused
    with pytest.raises(ValueError, match='c_h is 8, the decoder has 16'):
        V.load_voice(path, c_h=16, digest=digest)
    with pytest.raises(ValueError, match='digest'):
        V.load_voice(path, c_h=8, digest='0' * 64)
    # the digest covers every non-embedding tensor and no embedding row
    sd2 = dict(sd, **{'emb3.weight': sd['emb3.weight'] + 1})
    assert V.decoder_digest(sd2) == digest
    sd3 = dict(sd)
    sd3['conv1.bias'] = sd['conv1.bias'].clone()
    sd3['conv1.bias'][0] += 1e-3
    assert V.decoder_digest(sd3) != digest
    assert V.decoder_digest(dict(reversed(list(sd.items())))) == digest       # key order, not insertion order
    with pytest.raises(ValueError, match='digest'):
        V.save_voice(str(tmp_path / 'x.npz'), rows, {})
    with pytest.raises(ValueError, match='rows'):
        V.save_voice(str(tmp_path / 'x.npz'), rows[:4], {'digest': digest})
    # a file of another version
    with open(str(tmp_path / 'old.npz'), 'wb') as f:
        np.savez(f, meta=np.array(json.dumps(dict(meta, version=0))), **{'emb%d' % (i + 1): r for i, r in enumerate(rows)})
    with pytest.raises(ValueError, match='version'):
        V.load_voice(str(tmp_path / 'old.npz'))


# ---- the planner -------------------------------------------------------------------------------------------------------------------
def test_planner_alignment_bounds_and_seed(V):
    seg = 128
    frames = [100, 300, 128, 129, 1000, 127, 200]
    units = [12, 37, 16, 16, 125, 16, 15]                # the last one: enough frames, too few units
    utt, t, kept, left = V.plan_items(frames, units, seg, n_items=2000, seed=5)
    assert kept == [1, 2, 3, 4] and left == [0, 5, 6]
    assert utt.dtype == np.int64 and t.dtype == np.int64 and len(utt) == len(t) == 2000
    assert set(utt.tolist()) == set(kept) and not (t % 8).any() and t.min() == 0
    for u, s in zip(utt, t):
        assert s + seg <= frames[u] and s // 8 + seg // 8 <= units[u]
    assert t[utt == 2].max() == 0 and t[utt == 3].max() == 0                 # one admissible start each
    assert t[utt == 1].max() == 168                                           # min(300 - 128, 8 * (37 - 16)) = 168
    assert t[utt == 4].max() == 872                                           # min(872, 8 * 109)
    # uniform over the admissible segments: utterance 4 has 110 of the 134
    assert abs((utt == 4).mean() - 110.0 / 134.0) < 0.05
    again = V.plan_items(frames, units, seg, n_items=2000, seed=5)
    assert np.array_equal(again[0], utt) and np.array_equal(again[1], t)
    other = V.plan_items(frames, units, seg, n_items=2000, seed=6)
    assert not (np.array_equal(other[0], utt) and np.array_equal(other[1], t))
    with pytest.raises(ValueError, match='no utterance of at least seg_len = 128'):
        V.plan_items([100, 127], [13, 16], seg)
    with pytest.raises(ValueError, match='multiple of 8'):
        V.plan_items([100], [13], 60)
    with pytest.raises(ValueError, match='n_items'):
        V.plan_items([300], [37], seg, n_items=0)


def test_item_table_check(V):
    ok = (np.array([0, 8, 64]), np.array([0, 1, 8]))
    V.check_items(ok[0], ok[1], 64, 128, 16)
    for first, ufirst, match in (([0, 72], [0, 1], 'leaves the pool'), ([-8, 0], [0, 1], 'leaves the pool'), ([0, 4], [0, 1], 'multiple of 8'),
                                 ([0, 8], [0, 9], 'packed units'), ([0, 8], [-1, 0], 'packed units'), ([], [], 'length')):
        with pytest.raises(ValueError, match=match):
            V.check_items(np.array(first, dtype=np.int64), np.array(ufirst, dtype=np.int64), 64, 128, 16)


# ---- names and tables ----------------------------------------------------------------------------------------------------------------
def test_name_resolution_order(V):
    s2id = {'S015': 0, 'V001': 2}
    voices = {'ANNA': 4, 'V001': 5}
    assert V.resolve_speaker('V001', s2id, voices) == 2                       # speaker2id first
    assert V.resolve_speaker('ANNA', s2id, voices) == 4 and V.resolve_speaker('S015', s2id) == 0
    with pytest.raises(ValueError, match='BOB'):
        V.resolve_speaker('BOB', s2id, voices)
    with pytest.raises(ValueError, match='ANNA'):
        V.resolve_speaker('ANNA', s2id)
    assert V.parse_voices(['A=x.npz', ' B = dir/y=z.npz ']) == {'A': 'x.npz', 'B': 'dir/y=z.npz'}
    for bad in (['A'], ['=x'], ['A='], ['A=x', 'A=y']):
        with pytest.raises(ValueError):
            V.parse_voices(bad)


def test_extended_state_dict_keeps_every_original_row(V):
    sd = _decoder_sd(c_h=8, n_spk=3)
    v1 = [np.full(8, 10.0 + i, dtype=np.float32) for i in range(5)]
    v2 = [np.full(8, 20.0 + i, dtype=np.float32) for i in range(5)]
    ext = V.extend_state_dict(sd, [v1, v2])
    assert set(ext) == set(sd)
    for k in sd:
        if k in V.EMB_KEYS:
            i = V.EMB_KEYS.index(k)
            assert ext[k].shape == (5, 8) and ext[k].dtype == sd[k].dtype
            assert torch.equal(ext[k][:3], sd[k])                               # bit for bit, at the same indices
            assert torch.equal(ext[k][3], torch.from_numpy(v1[i])) and torch.equal(ext[k][4], torch.from_numpy(v2[i]))
        else:
            assert ext[k] is sd[k]
    assert sd['emb1.weight'].shape == (3, 8)                                    # the input is not modified
    with pytest.raises(ValueError, match='c_h = 8'):
        V.extend_state_dict(sd, [[np.zeros(4, np.float32)] * 5])
    one = V.replace_tables(sd, v1)
    assert all(one[k].shape == (1, 8) and torch.equal(one[k][0], torch.from_numpy(v1[i])) for i, k in enumerate(V.EMB_KEYS))
    # init rows: a speaker's, or the mean of each table
    r = V.init_rows(sd, 1)
    assert all(torch.equal(r[i], sd[k][1]) for i, k in enumerate(V.EMB_KEYS))
    r = V.init_rows(sd)
    assert all(torch.equal(r[i], sd[k].mean(dim=0)) for i, k in enumerate(V.EMB_KEYS))
    with pytest.raises(ValueError, match='outside'):
        V.init_rows(sd, 3)


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def _args(argv):
    import main
    return main.build_parser().parse_args(argv)


S2ID = {'S015': 0, 'V001': 2, 'V002': 3}


@pytest.mark.parametrize('argv, match', [
    (['--adapt_voice', 'ANNA'], 'needs --adapt_dir'),
    (['--adapt_voice', 'V001', '--adapt_dir', 'd'], 'is a speaker of'),
    (['--adapt_voice', 'ANNA', '--adapt_dir', 'd', '--train_ae'], 'cannot be combined with --train_ae'),
    (['--adapt_voice', 'ANNA', '--adapt_dir', 'd', '--train'], 'cannot be combined with --train'),
    (['--adapt_voice', 'ANNA', '--adapt_dir', 'd', '--train_p'], 'cannot be combined with --train_p'),
    (['--adapt_voice', 'ANNA', '--adapt_dir', 'd', '--train_tgat'], 'cannot be combined with --train_tgat'),
    (['--adapt_voice', 'ANNA', '--adapt_dir', 'd', '--train_c'], 'cannot be combined with --train_c'),
    (['--adapt_voice', 'ANNA', '--adapt_dir', 'd', '--adapt_init', 'S999'], 'adapt_init'),
    (['--adapt_voice', 'ANNA', '--adapt_dir', 'd', '--adapt_iters', '0'], 'adapt_iters'),
    (['--adapt_voice', 'ANNA', '--adapt_dir', 'd', '--enc_mode', 'continues'], 'continues'),
    (['--adapt_voice', 'A,B', '--adapt_dir', 'd'], 'name'),
    (['--adapt_dir', 'd'], 'needs --adapt_voice'),
    (['--adapt_voice', 'ANNA', '--adapt_dir', 'd', '--convert_dir', 'c', '--enc_only'], 'run --convert_dir as a command of its own'),
    (['--adapt_voice', 'ANNA', '--adapt_dir', 'd', '--synth_dir', 'c'], 'run --synth_dir as a command of its own'),
    (['--adapt_voice', 'ANNA', '--adapt_dir', 'd', '--test_single'], 'run --test_single as a command of its own'),
    (['--adapt_voice', 'ANNA', '--adapt_dir', 'd', '--voice', 'B=b.npz', '--convert_dir', 'c', '--enc_only'], 'command of its own'),
    (['--voice', 'ANNA=a.npz'], 'needs --convert_dir or --synth_dir'),
    (['--voice', 'ANNA=a.npz', '--convert_dir', 'd'], 'needs --enc_only'),
    (['--voice', 'ANNA=a.npz', '--synth_dir', 'd'], 'needs --enc_only'),
    (['--voice', 'V002=a.npz', '--convert_dir', 'd', '--enc_only'], 'is a speaker of'),
    (['--voice', 'ANNA=a.npz', '--voice', 'ANNA=b.npz', '--convert_dir', 'd', '--enc_only'], 'twice'),
    (['--voice', 'ANNA', '--convert_dir', 'd', '--enc_only'], 'NAME=FILE'),
    (['--voice', 'ANNA=a.npz', '--convert_dir', 'd', '--enc_only', '--enc_mode', 'continues'], 'continues'),
])
def test_check_voice_refusals(argv, match):
    import main
    with pytest.raises(ValueError, match=match):
        main.check_voice(_args(argv), S2ID)


def test_check_voice_accepts_and_reads_speaker2id(tmp_path, monkeypatch):
    import main
    main.check_voice(_args([]), S2ID)
    main.check_voice(_args(['--adapt_voice', 'ANNA', '--adapt_dir', 'd', '--adapt_init', 'V001', '--adapt_iters', '3', '--adapt_lr', '0.01']), S2ID)
    main.check_voice(_args(['--voice', 'ANNA=a.npz', '--voice', 'BOB=b.npz', '--synth_dir', 'd', '--enc_only']), S2ID)
    assert main.voice_files(_args(['--voice', 'ANNA=a.npz', '--voice', 'BOB=b.npz'])) == {'ANNA': 'a.npz', 'BOB': 'b.npz'}
    # the table is read from --speaker2id_path when it is not handed in
    p = tmp_path / 's2id.json'
    p.write_text(json.dumps(S2ID))
    with pytest.raises(ValueError, match='is a speaker of'):
        main.check_voice(_args(['--adapt_voice', 'V002', '--adapt_dir', 'd', '--speaker2id_path', str(p)]))
    # a multi-rank launch
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='one GPU'):
        main.check_voice(_args(['--adapt_voice', 'ANNA', '--adapt_dir', 'd']), S2ID)
    assert main.OUT_OF_SCOPE == ['train_al', 'train_t', 'test_asr', 'encode']


def test_refused_before_anything_is_built(monkeypatch, tmp_path):
    """main() raises from argument_runner: no trainer is made (get_trainer would need a GPU and a checkpoint)."""
    import main
    import zs_amd.convert as cv
    monkeypatch.setattr(cv, 'get_trainer', lambda *a, **k: (_ for _ in ()).throw(AssertionError('built')))
    p = tmp_path / 's2id.json'
    p.write_text(json.dumps(S2ID))
    for argv, match in ((['--adapt_voice', 'ANNA'], 'needs --adapt_dir'),
                        (['--voice', 'ANNA=a.npz', '--convert_dir', str(tmp_path)], 'needs --enc_only'),
                        (['--adapt_voice', 'V001', '--adapt_dir', str(tmp_path), '--speaker2id_path', str(p)], 'is a speaker of'),
                        (['--adapt_voice', 'ANNA', '--adapt_dir', str(tmp_path), '--hps_path', os.path.join(ROOT, 'hps', 'zerospeech_english.json'),
                          '--enc_mode', 'continues'], 'continues')):
        with pytest.raises(ValueError, match=match):
            main.main(argv)


def test_use_ema_counts_adaptation_as_loading():
    import main
    main.check_ema(_args(['--use_ema', '--adapt_voice', 'ANNA', '--adapt_dir', 'd']))
    with pytest.raises(ValueError, match='--use_ema needs'):
        main.check_ema(_args(['--use_ema']))


def test_header_declares_the_entry_points():
    import zs_amd  # noqa: F401
    from zs_amd import _lib
    assert {'zs_voice_gather', 'zs_voice_adam'} <= set(_lib.FUNCTIONS)
    names = lambda s: [f for f, _ in _lib._STRUCT_FIELDS[s]]
    assert names('ZsVoiceGather') == ['dtype', 'pool', 'packed', 'row_bytes', 'first', 'ufirst', 'n', 'cursor', 'B', 'seg_len', 'F', 'E', 'x',
                                      'bits', 'ld_bits', 'advance']
    assert names('ZsVoiceAdam') == ['emb_sum', 'B', 'C', 'row', 'm', 'v', 'g', 'lr', 'beta1', 'beta2', 'eps', 'bc1', 'bc2', 'sumsq',
                                    'max_norm', 'step_ptr']
    import ctypes
    assert ctypes.sizeof(_lib.STRUCTS['ZsVoiceAdam']) == 8 + 8 + 5 * 8 + 3 * 8 + 6 * 4 + 8 + 8 + 8
    assert hasattr(_lib.lib(), 'zs_voice_gather') and hasattr(_lib.lib(), 'zs_voice_adam')
