"""The plans of batched conversion without a GPU: the index tables _enqueue_encode, _gather_decoded and synth_units_batch upload are
built by host functions that return numpy arrays (convert._scatter_tables, _pack_tables, _dense_tables, _gather_index, _unit_tables,
all on convert._fragment_layout, and _vq_index_map on _pack_tables).  An off-by-one here is an out-of-bounds write on the device, so every table is checked against
values derived from fragments(), _t8 and the per-utterance rule of convert() alone."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zs_amd  # noqa: E402,F401
from zs_amd import convert as cv  # noqa: E402

SEG = 32
# shorter than MIN_LEN; at most seg_len; tails of exactly seg_len (65, 97, 129); the longest tail, 2 seg_len - 2 (63, 95); 3+ fragments
FRAMES = [5, 9, 32, 33, 63, 64, 65, 95, 97, 129, 200]
MAX_BATCH = [256, 3]


def _rule(n):
    """The (start, stop) pieces convert() sends an utterance of n frames through the network in."""
    n = max(n, cv.MIN_LEN)                                           # _pad_min
    return [(0, n)] if n <= SEG else cv.fragments(n, SEG)


RULE = [_rule(n) for n in FRAMES]
UNITS = [sum(cv._t8(b - a) for a, b in frs) for frs in RULE]         # what each utterance encodes to: the unit files of synth_dir
UNIT_RULE = [cv.unit_fragments(n, SEG) for n in UNITS]


def _frame_chunks(max_batch):
    items = [it for u, n in enumerate(FRAMES) for it in cv._frame_items(u, max(n, cv.MIN_LEN), SEG, n < cv.MIN_LEN)]
    return items, cv._split_chunks(items, SEG, max_batch)


def _unit_chunks(max_batch):
    items = [it for u, n in enumerate(UNITS) for it in cv._unit_items(u, n, SEG)]
    return items, cv._split_chunks(items, SEG // 8, max_batch)


def test_items_are_the_fragments_of_the_rule():
    items, _ = _frame_chunks(256)
    for u, frs in enumerate(RULE):
        mine = [it for it in items if it.u == u]
        assert [(it.k, it.a, it.b, it.n) for it in mine] == [(k, a, b, b - a) for k, (a, b) in enumerate(frs)]
        assert [it.trunc for it in mine] == ([cv.MIN_LEN // 8] if FRAMES[u] < cv.MIN_LEN else [None] * len(frs))
    items, _ = _unit_chunks(256)
    for u, pieces in enumerate(UNIT_RULE):
        mine = [it for it in items if it.u == u]
        assert [it.k for it in mine] == list(range(len(pieces))) and [it.n for it in mine] == pieces
        assert mine[0].a == 0 and mine[-1].b == UNITS[u] and all(p.b == q.a for p, q in zip(mine, mine[1:]))
        assert all(it.trunc is None for it in mine)


@pytest.mark.parametrize('max_batch', MAX_BATCH)
@pytest.mark.parametrize('make, full', [(_frame_chunks, SEG), (_unit_chunks, SEG // 8)])
def test_chunk_split(make, full, max_batch):
    items, chunks = make(max_batch)
    flat = [it for chunk, _ in chunks for it in chunk]
    assert sorted(flat) == sorted(items) and len(flat) == len(set(flat))         # every item exactly once
    kinds = [ragged for _, ragged in chunks]
    assert set(kinds) == {None, True} and kinds == sorted(kinds, key=lambda r: r is True)      # the plain chunks first
    for chunk, ragged in chunks:
        assert 1 <= len(chunk) <= max_batch
        if ragged is None:
            assert all(it.n == full for it in chunk)
        else:
            assert all(it.n != full for it in chunk)
    rest = [it.n for chunk, ragged in chunks if ragged for it in chunk]
    assert rest == sorted(rest, reverse=True)                        # longest first, within and across the ragged chunks
    if max_batch == 3:
        assert kinds.count(None) > 1 and kinds.count(True) > 1


def test_fragment_layout_does_not_depend_on_the_order_of_the_items():
    items, _ = _frame_chunks(256)
    counts = [7 * it.k + it.u + 1 for it in items]
    at, totals = cv._fragment_layout(items, counts, len(FRAMES))
    assert totals == [sum(c for it, c in zip(items, counts) if it.u == u) for u in range(len(FRAMES))]
    for it, s in zip(items, at):
        assert s == sum(c for jt, c in zip(items, counts) if jt.u == it.u and jt.k < it.k)
    perm = np.random.RandomState(0).permutation(len(items))
    at_p, totals_p = cv._fragment_layout([items[i] for i in perm], [counts[i] for i in perm], len(FRAMES))
    assert totals_p == totals and at_p == [at[i] for i in perm]


def _check_scatter(chunks, rule_rows, rows_of):
    """rule_rows[u][k]: the output rows of fragment k of utterance u, from the rule."""
    n_utt = len(rule_rows)
    Tm, ulens, tables, pad = cv._scatter_tables(chunks, n_utt, rows_of)
    assert ulens == [sum(r) for r in rule_rows] and Tm == max(ulens)
    assert len(tables) == len(chunks) and all(t.dtype == np.int32 and t.ndim == 1 for t in tables) and pad.dtype == np.int32
    for (chunk, _), table in zip(chunks, tables):
        T = max(rule_rows[it.u][it.k] for it in chunk)               # the chunk is padded to its longest member
        d = table.reshape(len(chunk), T)
        for i, it in enumerate(chunk):
            first, n = it.u * Tm + sum(rule_rows[it.u][:it.k]), rule_rows[it.u][it.k]     # fragment k's rows follow fragment k-1's
            assert np.array_equal(d[i, :n], np.arange(first, first + n))
            assert (d[i, n:] == -1).all()                            # -1 exactly behind a fragment's own rows
    everything = np.concatenate(tables + [pad])
    assert np.array_equal(np.sort(everything[everything >= 0]), np.arange(n_utt * Tm))       # every row of the buffer written once
    assert (pad >= 0).all() and len(pad) == n_utt * Tm - sum(ulens)


@pytest.mark.parametrize('max_batch', MAX_BATCH)
def test_scatter_tables(max_batch):
    _, chunks = _frame_chunks(max_batch)
    _check_scatter(chunks, [[8 * cv._t8(b - a) for a, b in frs] for frs in RULE], None)
    _, chunks = _unit_chunks(max_batch)
    _check_scatter(chunks, [[8 * n for n in pieces] for pieces in UNIT_RULE], lambda n: 8 * n)


@pytest.mark.parametrize('max_batch', MAX_BATCH)
def test_pack_tables(max_batch):
    _, chunks = _frame_chunks(max_batch)
    flat = [it for chunk, _ in chunks for it in chunk]
    uoffs, starts, lens = cv._pack_tables(chunks, len(FRAMES))
    assert (uoffs.dtype, starts.dtype, lens.dtype) == (np.int64, np.int64, np.int32) and len(starts) == len(lens) == len(flat)
    want = [[cv._t8(b - a) for a, b in frs] for frs in RULE]
    want[0] = [cv.MIN_LEN // 8]                                      # the 5-frame utterance: the truncation of convert()
    assert FRAMES[0] < cv.MIN_LEN and np.array_equal(uoffs, np.concatenate(([0], np.cumsum([sum(w) for w in want]))))
    for it, s, n in zip(flat, starts, lens):
        assert n == want[it.u][it.k] and s == uoffs[it.u] + sum(want[it.u][:it.k])           # in [uoffs[u], uoffs[u+1]), fragment order
        assert uoffs[it.u] <= s and s + n <= uoffs[it.u + 1]
    order = np.argsort(starts)
    assert starts[order][0] == 0 and np.array_equal((starts + lens)[order][:-1], starts[order][1:])      # no gap, no overlap
    assert (starts + lens)[order][-1] == uoffs[-1]


@pytest.mark.parametrize('max_batch', MAX_BATCH)
def test_vq_index_map(max_batch):
    """The table that gives every returned unit of a vector-codebook batch its index: src[uoffs[u]:uoffs[u + 1]] are the rows of the
    chunks' index buffers (chunk by chunk, len(chunk) x _t8(longest member) rows each) that hold utterance u's frames."""
    _, chunks = _frame_chunks(max_batch)
    uoffs, src = cv._vq_index_map(chunks, len(FRAMES))
    assert np.array_equal(uoffs, cv._pack_tables(chunks, len(FRAMES))[0]) and uoffs.dtype == np.int64
    assert src.dtype == np.int64 and src.shape == (uoffs[-1],)
    label, base = {}, 0                                              # every row of the buffers, end to end: (utterance, fragment, frame)
    for chunk, _ in chunks:
        Tp = cv._t8(max(b - a for a, b in (RULE[it.u][it.k] for it in chunk)))
        for i, it in enumerate(chunk):
            label.update({base + i * Tp + t: (it.u, it.k, t) for t in range(Tp)})
        base += len(chunk) * Tp
    assert src.min() >= 0 and src.max() < base and len(set(src.tolist())) == len(src)          # inside the buffers, no index twice
    want = [[cv._t8(b - a) for a, b in frs] for frs in RULE]
    want[0] = [cv.MIN_LEN // 8]                                      # the 5-frame utterance: the truncation of convert()
    assert FRAMES[0] < cv.MIN_LEN
    for u, counts in enumerate(want):                                # exactly the frames of utterance u, in fragment order
        assert [label[r] for r in src[uoffs[u]:uoffs[u + 1]]] == [(u, k, t) for k, n in enumerate(counts) for t in range(n)]


@pytest.mark.parametrize('max_batch', MAX_BATCH)
def test_dense_tables(max_batch):
    _, chunks = _frame_chunks(max_batch)
    starts, lens = cv._dense_tables(chunks)
    assert (starts.dtype, lens.dtype) == (np.int64, np.int32)
    at = 0
    for chunk, _ in chunks:
        Tp = cv._t8(max(b - a for a, b in (RULE[it.u][it.k] for it in chunk)))
        for i, it in enumerate(chunk):
            a, b = RULE[it.u][it.k]
            assert starts[at + i] == i * Tp and lens[at + i] == cv._t8(b - a) <= Tp         # every encoded frame: no truncation
        at += len(chunk)
    assert at == len(starts) == len(lens)


@pytest.mark.parametrize('max_batch', MAX_BATCH)
def test_unit_tables(max_batch):
    _, chunks = _unit_chunks(max_batch)
    uoffs = np.concatenate(([0], np.cumsum(UNITS))).astype(np.int64)
    starts, lens = cv._unit_tables(chunks, uoffs)
    assert (starts.dtype, lens.dtype) == (np.int64, np.int32)
    for it, s, n in zip((it for chunk, _ in chunks for it in chunk), starts, lens):
        assert n == UNIT_RULE[it.u][it.k] and s == uoffs[it.u] + sum(UNIT_RULE[it.u][:it.k])
    order = np.argsort(starts)
    assert starts[order][0] == 0 and np.array_equal((starts + lens)[order][:-1], starts[order][1:])
    assert (starts + lens)[order][-1] == uoffs[-1]


@pytest.mark.parametrize('max_batch', MAX_BATCH)
def test_gather_index(max_batch):
    _, chunks = _frame_chunks(max_batch)
    rows = [[8 * cv._t8(b - a) for a, b in frs] for frs in RULE]
    shapes = [(len(chunk), max(rows[it.u][it.k] for it in chunk)) for chunk, _ in chunks]   # a chunk's decoded buffer [n, 8 T', 513]
    out_rows = [[rows[it.u][it.k] for it in chunk] for chunk, _ in chunks]
    idx, ulens, total = cv._gather_index(chunks, out_rows, shapes, len(FRAMES))
    assert total == sum(n * ld for n, ld in shapes) and ulens == [sum(r) for r in rows]
    assert idx.dtype == np.int64 and idx.shape == (len(FRAMES), max(ulens))
    where, base = {}, 0
    for (chunk, _), (n, ld) in zip(chunks, shapes):
        for i, it in enumerate(chunk):
            where[(it.u, it.k)] = base + i * ld
        base += n * ld
    for u in range(len(FRAMES)):
        want = np.concatenate([np.arange(where[(u, k)], where[(u, k)] + n) for k, n in enumerate(rows[u])])
        assert np.array_equal(idx[u, :ulens[u]], want) and (want < total).all() and len(set(want.tolist())) == len(want)
        assert (idx[u, ulens[u]:] == total).all()                    # the zero row behind them
    valid = idx[idx < total]
    assert len(set(valid.tolist())) == len(valid)                    # no decoded row serves two frames


def test_both_folder_plans_group_alike():
    files = ['/in/f%02d.wav' % i for i in range(10)]
    sizes = [10 * (i + 1) for i in range(10)]
    for kw_c, kw_s in (({'max_batch_seconds': 120}, {'max_batch_units': 120}), ({'batch': 4}, {'batch': 4})):
        a = cv.convert_dir_plan(files, sizes, ['V001', 'V002'], '/out', **kw_c)
        b = cv.synth_dir_plan(files, sizes, ['V001', 'V002'], '/out', **kw_s)
        assert [[(it['stem'], it['target']) for it in g] for g in a['groups']] == [[(it['stem'], it['target']) for it in g] for g in b['groups']]
        assert len(a['groups']) > 1
    with pytest.raises(ValueError, match='^convert_dir_plan: 1 durations for 2 files'):
        cv.convert_dir_plan(files[:2], [1.0], ['V001'], '/out')
    with pytest.raises(ValueError, match='^synth_dir_plan: 1 unit counts for 2 files'):
        cv.synth_dir_plan(files[:2], [5], ['V001'], '/out')


def test_run_deferred_enqueues_the_next_group_before_it_writes():
    log = []

    def enqueue(g):
        log.append(('enqueue', g))
        return None if g == 2 else (g, 'fin%d' % g)                  # group 2 has nothing live

    cv._run_deferred(range(4), enqueue, lambda g, fin: log.append(('write', g, fin)))
    assert log == [('enqueue', 0), ('enqueue', 1), ('write', 0, 'fin0'), ('enqueue', 2), ('write', 1, 'fin1'), ('enqueue', 3),
                   ('write', 3, 'fin3')]
    cv._run_deferred([], enqueue, None)


def test_enqueued_slots_and_the_speaker_range():
    q = cv._Enqueued()
    assert all(getattr(q, slot) is None for slot in cv._Enqueued.__slots__)
    cv._check_speaker_range([0, 4], 5)
    for bad in ([0, 5], [-1]):
        with pytest.raises(ValueError, match=r'speaker id %d is outside \[0, n_speakers = 5\)' % bad[-1]):
            cv._check_speaker_range(bad, 5)


def test_vocoder_wait_is_freed_without_the_garbage_collector():
    """What _enqueue_vocoder returns holds a batch's pinned buffers; in a reference cycle they would wait for a collection."""
    import gc
    import weakref

    import torch

    class Done(object):
        def synchronize(self):
            pass

    done = Done()
    held = weakref.ref(done)
    w_h = torch.arange(2 * 1600, dtype=torch.float32).reshape(2, 1600)
    fin = cv._VocoderWait(done, torch.tensor([3], dtype=torch.int32), w_h, None, [5, 9], False)
    assert fin.status is None
    gc.disable()
    try:
        wavs = fin()
        assert fin.status == 3 and [len(w) for w in wavs] == [800, 1600] and np.array_equal(wavs[1], np.arange(1600, 3200))
        del fin, done
        assert held() is None
    finally:
        gc.enable()
