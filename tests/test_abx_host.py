"""--score_units without a GPU: the item parser, the token-to-row rule at its boundaries, the planner of zs_amd.abx against
the brute-force enumeration of tests/abx_ref.py on a tiny corpus (every triplet in exactly one job, exactly once; the pair records
of every tiling), the aggregation from integer counts, the bitrate and main.py's refusals, which come before anything is read."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import abx_ref as R  # noqa: E402

HPS = os.path.join(ROOT, 'hps', 'zerospeech_english.json')


def _write(path, lines):
    with open(str(path), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return str(path)


def test_seconds_per_unit_is_the_reference_constant():
    from zs_amd import abx
    assert abx.seconds_per_unit() == R.P
    assert abx.MAX_LEN == 64 and abx.MAX_TILE == 4096
    assert abx.PAIR_DTYPE.itemsize == 32 and abx.JOB_DTYPE.itemsize == 24


def test_parse_items_header_blank_lines_and_bad_lines(tmp_path):
    from zs_amd import abx
    good = _write(tmp_path / 'a.item', ['#file onset offset #phone prev next speaker', '', 'f1 0.10 0.25 ae k t s0', '   ',
                                        'f2 1 2.5 b a a s1'])
    items = abx.parse_items(good)
    assert items == [{'file': 'f1', 'onset': 0.10, 'offset': 0.25, 'phone': 'ae', 'prev': 'k', 'next': 't', 'speaker': 's0'},
                     {'file': 'f2', 'onset': 1.0, 'offset': 2.5, 'phone': 'b', 'prev': 'a', 'next': 'a', 'speaker': 's1'}]
    with pytest.raises(ValueError, match=r'line 1: an item file starts with a header'):
        abx.parse_items(_write(tmp_path / 'b.item', ['f1 0.1 0.2 ae k t s0']))
    for bad in ('f1 0.1 0.2 ae k t', 'f1 0.1 0.2 ae k t s0 extra', 'f1 x 0.2 ae k t s0', 'f1 0.3 0.2 ae k t s0', 'f1 0.1 nan ae k t s0'):
        with pytest.raises(ValueError, match=r'c\.item, line 4: expected `file onset offset phone prev next speaker`'):
            abx.parse_items(_write(tmp_path / 'c.item', ['#h', 'f1 0.1 0.2 ae k t s0', '', bad]))
    with pytest.raises(ValueError, match='no header line'):
        abx.parse_items(_write(tmp_path / 'd.item', ['']))


def test_token_rows_at_the_boundaries():
    from zs_amd import abx
    rs = np.random.RandomState(0)
    P = R.P
    centre = lambda i, off=0.0: off + (i + 0.5) * P                # the definition's own expression: exact boundary values
    cases = [(centre(3), centre(5), 10, 0.0), (centre(3), centre(3), 10, 0.0), (np.nextafter(centre(3), 1), centre(5), 10, 0.0),
             (centre(3), np.nextafter(centre(5), 0), 10, 0.0), (0.0, 100.0, 10, 0.0), (-5.0, -1.0, 10, 0.0), (2.0, 3.0, 10, 0.0),
             (0.26, 0.34, 10, 0.0), (centre(0), centre(63), 100, 0.0), (centre(0), centre(64), 100, 0.0),
             (centre(2, 0.37), centre(4, 0.37), 10, 0.37), (centre(2), centre(4), 10, 0.37), (0.0, 0.36, 10, 0.37)]
    cases += [(a, a + b, int(n), float(o)) for a, b, n, o in zip(rs.uniform(-0.2, 1.2, 200), rs.uniform(0, 0.6, 200), rs.randint(1, 12, 200),
                                                                 rs.choice([0.0, 0.013, 0.25], 200))]
    for onset, offset, n, off in cases:
        want = R.token_rows(onset, offset, n, off)
        first, cnt = abx.token_rows(onset, offset, n, off)
        assert cnt == len(want), (onset, offset, n, off)
        if want:
            assert first == want[0] and want == list(range(first, first + cnt))
    assert abx.token_rows(centre(3), centre(5), 10) == (3, 3)      # a centre exactly on onset and on offset is inside
    assert abx.token_rows(centre(0), centre(63), 100)[1] == 64 and abx.token_rows(centre(0), centre(64), 100)[1] == 65


def test_collect_tokens_keeps_and_drops_by_reason():
    from zs_amd import abx
    P = R.P
    tok = lambda f, r0, n, ph='a': {'file': f, 'onset': r0 * P + 0.01, 'offset': (r0 + n) * P - 0.01, 'phone': ph, 'prev': 'x', 'next': 'y',
                                    'speaker': 's'}
    items = [tok('f', 0, 1), tok('f', 1, 64), tok('f', 0, 65), tok('g', 0, 2), tok('f', 70, 0), tok('f', 198, 5), tok('h', 3, 2, 'b')]
    t = abx.collect_tokens(items, {'f': (10, 200), 'h': (300, 10)})
    assert t.dropped == {'no_rows': 1, 'too_long': 1, 'no_file': 1}
    assert t.start.tolist() == [10, 11, 10 + 198, 303] and t.length.tolist() == [1, 64, 2, 2]      # (the file's end cuts a token)
    assert t.phones == ['a', 'b'] and t.ctxs == [('x', 'y')] and t.speakers == ['s'] and t.phone.tolist() == [0, 0, 0, 1]
    t2 = abx.collect_tokens([tok('f', 5, 2)], {'f': (0, 20)}, offsets={'f': 0.2})                    # offsets applied: two rows earlier
    assert t2.start.tolist() == [3] and t2.length.tolist() == [2]


def _corpus_tokens(seed=0):
    from zs_amd import abx
    lines, files, toks = R.tiny_corpus(seed)
    first, file_rows = 0, {}
    for stem in sorted(files):
        file_rows[stem] = (first, files[stem])
        first += files[stem]
    return lines, file_rows, toks


def _plan(tmp_path, tasks=('within', 'across'), budget=None, seed=0, max_tile=4096):
    from zs_amd import abx
    lines, file_rows, toks = _corpus_tokens(seed)
    items = abx.parse_items(_write(tmp_path / 'tiny.item', lines))
    tokens = abx.collect_tokens(items, file_rows)
    assert len(tokens) == len(toks) and sum(tokens.dropped.values()) == 0
    assert tokens.start.tolist() == [file_rows[t[0]][0] + t[1] for t in toks] and tokens.length.tolist() == [t[2] for t in toks]
    return tokens, toks, abx.plan(tokens, tasks, budget, max_tile)


def _cell_key(plan, tokens, c):
    a, b = tokens.phones[plan.cell_a[c]], tokens.phones[plan.cell_b[c]]
    key = (a, b, tokens.ctxs[plan.cell_ctx[c]], tokens.speakers[plan.cell_s[c]])
    return key if plan.cell_s2[c] < 0 else key + (tokens.speakers[plan.cell_s2[c]],)


@pytest.mark.parametrize('seed', [0, 1])
def test_planner_emits_every_triplet_exactly_once(tmp_path, seed):
    from zs_amd import abx
    tokens, toks, plan = _plan(tmp_path, seed=seed)
    ref_tokens = [(t[3], t[4], t[5]) for t in toks]
    want = {task: sorted(R.triplets(ref_tokens, task)) for task in abx.TASKS}
    assert len(want['within']) > 50 and len(want['across']) > 50
    got = {task: [] for task in abx.TASKS}
    per_cell = np.zeros(plan.cell_n.size, dtype=np.int64)
    for blk in plan.blocks:
        assert blk.jobs.size and (np.diff(tokens.ctx[blk.tok]) == 0).all()
        key = list(zip(tokens.speaker[blk.tok].tolist(), tokens.phone[blk.tok].tolist()))
        assert key == sorted(key)                                   # sorted by (speaker, phone): the sets are contiguous ranges
        for j, c in zip(blk.jobs, blk.job_cell):
            A = [a for a in range(j['a0'], j['a1']) if a != j['skip']]
            B = list(range(j['b0'], j['b1']))
            assert A and B, 'a job with an empty set'
            task = abx.TASKS[plan.cell_task[c]]
            assert (j['skip'] == j['x']) if task == 'within' else (j['skip'] == -1)
            if task == 'within':
                assert j['a0'] <= j['x'] < j['a1']
            cell = _cell_key(plan, tokens, c)
            for a in A:
                for b in B:
                    got[task].append((cell, int(blk.tok[a]), int(blk.tok[b]), int(blk.tok[j['x']])))
            per_cell[c] += len(A) * len(B)
    for task in abx.TASKS:
        assert sorted(got[task]) == want[task]                      # every triplet, in one job, once
    assert np.array_equal(per_cell, plan.cell_n)
    for ctx in (('x', 'y'),):                                       # a single phone: no triplet, no block
        assert all(tokens.ctxs[b.ctx] != ctx for b in plan.blocks)
    alone = [b for b in plan.blocks if tokens.ctxs[b.ctx] == ('q', 'r')]
    assert all(abx.TASKS[plan.cell_task[c]] == 'within' for b in alone for c in b.job_cell)      # one speaker alone: nothing across
    within_only = _plan(tmp_path, tasks='within', seed=seed)[2]
    assert set(within_only.cell_task.tolist()) == {0} and within_only.cell_n.sum() == len(want['within'])


def _check_tiling(tokens, plan, want_chunks=None):
    from zs_amd import abx
    for blk in plan.blocks:
        if want_chunks is not None:
            assert len(blk.chunks) >= want_chunks
        assert blk.chunks[0][0] == 0 and blk.chunks[-1][1] == blk.n and all(a[1] == b[0] for a, b in zip(blk.chunks, blk.chunks[1:]))
        seen = {}
        for r, c in blk.tiles():
            rows = int(blk.foff[blk.chunks[r][1]] - blk.foff[blk.chunks[r][0]])
            cols = int(blk.foff[blk.chunks[c][1]] - blk.foff[blk.chunks[c][0]])
            for W, rec in blk.tile_pairs(r, c).items():
                assert rec.dtype == abx.PAIR_DTYPE
                for q in rec:
                    x, y = divmod(int(q['dst0']), blk.n)
                    assert int(q['dst1']) == y * blk.n + x and x != y
                    assert q['La'] == blk.lens[x] and q['Lb'] == blk.lens[y] and abx.width_for(q['Lb']) == W
                    assert q['row0'] == blk.foff[x] - blk.foff[blk.chunks[r][0]] and q['col0'] == blk.foff[y] - blk.foff[blk.chunks[c][0]]
                    assert 0 <= q['row0'] and q['row0'] + q['La'] <= rows and 0 <= q['col0'] and q['col0'] + q['Lb'] <= cols
                    if r == c:
                        assert q['Lb'] <= q['La']                   # both orientations exist: the shorter token on the columns
                    seen[frozenset((x, y))] = seen.get(frozenset((x, y)), 0) + 1
        assert len(seen) == blk.n * (blk.n - 1) // 2 and set(seen.values()) <= {1}     # every unordered pair, once


def test_tiles_and_pair_records_in_one_tile_and_under_a_small_budget(tmp_path):
    tokens, toks, plan = _plan(tmp_path)
    assert all(len(b.chunks) == 1 for b in plan.blocks)
    _check_tiling(tokens, plan)
    big = max(plan.blocks, key=lambda b: b.frames)
    half = (big.frames + 1) // 2 + 2
    budget = 4 * big.n * big.n + 4 * half * half                   # the largest block in two chunks: 2 x 2 tiles, the upper three used
    tokens2, _, plan2 = _plan(tmp_path, budget=budget)
    b2 = max(plan2.blocks, key=lambda b: b.frames)
    assert len(b2.chunks) == 2 and b2.tiles() == [(0, 0), (0, 1), (1, 1)]
    _check_tiling(tokens2, plan2)
    assert [b.jobs.tolist() for b in plan2.blocks] == [b.jobs.tolist() for b in plan.blocks]      # the jobs do not depend on the tiling
    plan3 = _plan(tmp_path, max_tile=8)[2]                         # the column limit alone cuts too
    assert max(len(b.chunks) for b in plan3.blocks) > 2
    _check_tiling(tokens, plan3)


def test_a_block_that_cannot_be_tiled_is_refused_by_name(tmp_path):
    tokens, toks, plan = _plan(tmp_path)
    big = max(plan.blocks, key=lambda b: b.n)
    with pytest.raises(ValueError, match=r'the context a b has %d tokens of %d frames \(the longest %d\).*budget of %d bytes'
                       % (big.n, big.frames, int(big.lens.max()), 4 * big.n * big.n)):
        _plan(tmp_path, budget=4 * big.n * big.n)


def test_aggregation_from_given_integer_counts():
    from zs_amd import abx
    tokens = abx.Tokens([], [], [], [], [], ['a', 'b', 'c'], [('x', 'y'), ('u', 'v')], ['s0', 's1'], {})
    #        task a  b  ctx s  s2  n
    cells = [(0, 0, 1, 0, 0, -1, 4), (0, 0, 1, 1, 0, -1, 2), (0, 1, 0, 0, 1, -1, 3), (1, 0, 1, 0, 0, 1, 5), (0, 2, 0, 0, 0, -1, 1)]
    p = abx.Plan(tokens, ('within', 'across'), [], cells)
    wins2 = [8, 1, 3, 5, 0]
    out = abx.aggregate(p, wins2)
    ab = (8 / 8.0 + 1 / 4.0) / 2                                   # (a, b): two cells, unweighted
    ba, ca = 3 / 6.0, 0.0
    import math
    assert out['within'] == {'error': 100.0 * (1.0 - math.fsum([ab, ba, ca]) / 3), 'ordered_pairs': 3, 'cells': 4, 'triplets': 10}
    assert out['across'] == {'error': 100.0 * (1.0 - 0.5), 'ordered_pairs': 1, 'cells': 1, 'triplets': 5}
    ref = R.aggregate({('a', 'b', 0, 0): (8, 4), ('a', 'b', 1, 0): (1, 2), ('b', 'a', 0, 1): (3, 3), ('c', 'a', 0, 0): (0, 1)})
    assert out['within']['error'] == ref
    assert abx.aggregate(abx.Plan(tokens, ('within',), [], []), [])['within']['error'] is None


def test_bitrate_of_a_hand_made_folder(tmp_path):
    from zs_amd import abx
    _write(tmp_path / 'u1.txt', ['0 1', '0 1', '1 1', '1 0'])
    _write(tmp_path / 'u2.txt', ['0  1', '0 1 ', '1 1', '0 1'])     # blanks do not make a symbol
    _write(tmp_path / 'u1.idx.txt', ['3'])                          # not a bit unit file
    stems, rows, lines, E = abx.read_folder(str(tmp_path))
    assert stems == ['u1', 'u2'] and E == 2 and [r.shape for r in rows] == [(4, 2), (4, 2)] and rows[0].dtype == np.float32
    b = abx.bitrate(lines)
    H = -(5 / 8 * np.log2(5 / 8) + 2 / 8 * np.log2(2 / 8) + 1 / 8 * np.log2(1 / 8))
    assert b['units'] == 8 and b['symbols'] == 3
    assert abs(b['bits_per_unit'] - H) < 1e-12 and abs(b['bits_per_second'] - H / R.P) < 1e-9
    assert abx.bitrate(['a'] * 7)['bits_per_unit'] == 0.0
    with pytest.raises(ValueError, match='holds no'):
        abx.read_folder(str(tmp_path / 'nothing'))


def test_rows_at_of_every_codebook_kind():
    from zs_amd.codebook import Codebook
    from zs_amd.rvq import ResidualCodebook
    from zs_amd.vq import VectorCodebook
    from zs_amd import abx
    rs = np.random.RandomState(3)
    bits = Codebook(np.packbits(rs.randint(0, 2, (5, 12)).astype(bool), axis=1, bitorder='little'), 12)
    assert np.array_equal(bits.rows_at([4, 0, 4]), bits.packed[[4, 0, 4]])
    vec = VectorCodebook(rs.standard_normal((6, 7)).astype(np.float32))
    assert np.array_equal(vec.rows_at(np.array([5, 1])), vec.vectors[[5, 1]])
    res = ResidualCodebook(rs.standard_normal((3, 4, 5)).astype(np.float32))
    idx = np.array([[0, 1], [3, 2]])                               # two lines of two stages
    want = (res.vectors[0][[0, 3]] + res.vectors[1][[1, 2]]).astype(np.float32)
    assert np.array_equal(res.rows_at(idx), want)
    assert abx.check_metric(None) == 'hamming' and abx.check_metric(None, bits) == 'hamming' and abx.check_metric('angular', bits) == 'angular'
    assert abx.check_metric(None, vec) == 'angular' and abx.check_metric(None, res) == 'angular'
    with pytest.raises(ValueError, match='--abx_metric hamming needs bit units'):
        abx.check_metric('hamming', vec)
    with pytest.raises(ValueError, match='must be hamming or angular'):
        abx.check_metric('cosine')


def test_cli_refusals_come_before_anything_is_read(tmp_path, capsys):
    import main as M
    p = M.build_parser()

    def refused(argv, match):
        with pytest.raises(ValueError, match=match):
            M.check_score(p.parse_args(argv))
        with pytest.raises(ValueError, match=match):
            M.argument_runner(argv + ['--hps_path', HPS])

    a = p.parse_args([])
    assert all(getattr(a, f) is None for f in ('score_units',) + M.SCORE_FLAGS)
    M.check_score(a)
    for flag, v in (('abx_item', 'f'), ('abx_task', 'within'), ('abx_metric', 'hamming'), ('abx_offsets', 'o.json'), ('score_out', 's.json')):
        refused(['--' + flag, v], '--%s needs --score_units DIR' % flag)
    refused(['--score_units', 'd'], '--score_units needs --abx_item FILE')
    base = ['--score_units', 'd', '--abx_item', 'f.item']
    for other in (['--train_ae'], ['--convert_dir', 'e'], ['--synth_dir', 'e'], ['--test_encode'], ['--test'], ['--preprocess']):
        refused(base + other, 'it cannot be combined with --%s' % other[0][2:])
    for bad in ('both', 'within,within', 'within,', ''):
        refused(base + ['--abx_task=' + bad], '--abx_task takes within, across or within,across')
    with pytest.raises(SystemExit):
        p.parse_args(base + ['--abx_metric', 'cosine'])
    with pytest.raises(SystemExit):
        M.argument_runner(['--codebook', 'K4.codebook.npz', '--hps_path', HPS])
    assert '--codebook needs --convert_dir, --synth_dir or --test_encode' in capsys.readouterr().err
    args, hps = M.argument_runner(base + ['--abx_task', 'across,within', '--codebook', 'no_such.vq.npz'])     # nothing is opened yet
    assert args.score_units == 'd' and hps is None


def test_read_offsets(tmp_path):
    from zs_amd import abx
    path = str(tmp_path / 'o.json')
    with open(path, 'w') as f:
        json.dump({'a': 0.25, 'b': 1}, f)
    assert abx.read_offsets(path) == {'a': 0.25, 'b': 1.0}
    with open(path, 'w') as f:
        json.dump({'a': 'x'}, f)
    with pytest.raises(ValueError, match='--abx_offsets takes a json object'):
        abx.read_offsets(path)
