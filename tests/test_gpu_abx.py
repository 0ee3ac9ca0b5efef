"""--score_units on the GPU: zs_abx_dtw against the float32 restatement of tests/abx_ref.py with array_equal on integer
scores (ties everywhere, every group width, partly filled waves, both shift variants), its invalid records, the angular metric
against the float64 definition within the derived tol(E), zs_abx_rownorm, zs_abx_count against numpy exactly, and the whole command
on the tiny corpus of the host test against the brute-force enumeration."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import abx_ref as R  # noqa: E402

GUARD = 64
FILL = -12345.0
LENGTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)
# the seeds of the angular cases were chosen on the float64 reference alone (angular_case / e2e_angular_case below say how)
# At E = 1024 Gaussian rows are all but orthogonal: every g is 1/2 within 0.01, less than the margin 2 * 64 * tol asks for, so a pair with
# a choice in its DP is always left out; its pairs have one row on one side (either side), where no cell has a choice.
ANGULAR = {8: dict(seed=7, n=120, lengths=(1, 2, 3, 4, 5, 8), other=(1, 2, 3, 4, 5, 8)), 64: dict(seed=0, n=200, lengths=(1, 2, 3), other=(1, 2, 3)),
           1024: dict(seed=0, n=200, lengths=(1, 2, 3, 5, 8), other=(1,))}
E2E_ANGULAR_SEED = 0


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import zs_amd  # noqa: F401
    return torch.device('cuda:0')


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- zs_abx_dtw on integer scores ------------------------------------------------------------------------------------------------
def _int_case(n_pairs, seed, rows=200, cols=150, ld=160):
    """S of small integers (NaN in the unused columns) and n_pairs records with lengths from LENGTHS on both sides; the first records
    end at the matrix's last row and last column; every third has no mirror."""
    rs = np.random.RandomState(seed)
    S = np.full((rows, ld), np.nan, dtype=np.float32)
    S[:, :cols] = rs.randint(0, 4, size=(rows, cols))
    from zs_amd import abx
    rec = np.zeros(n_pairs, dtype=abx.PAIR_DTYPE)
    rec['La'], rec['Lb'] = rs.choice(LENGTHS, n_pairs), rs.choice(LENGTHS, n_pairs)
    rec['row0'] = (rs.uniform(size=n_pairs) * (rows - rec['La'] + 1)).astype(np.int64)
    rec['col0'] = (rs.uniform(size=n_pairs) * (cols - rec['Lb'] + 1)).astype(np.int64)
    edge = np.arange(n_pairs) % 5 == 0
    rec['row0'][edge], rec['col0'][edge] = rows - rec['La'][edge], cols - rec['Lb'][edge]
    perm = rs.permutation(2 * n_pairs)
    rec['dst0'], rec['dst1'] = perm[:n_pairs], perm[n_pairs:]
    rec['dst1'][np.arange(n_pairs) % 3 == 0] = -1
    return S, cols, rec


def _gather(g, rec):
    G = np.zeros((rec.size, int(rec['La'].max()), int(rec['Lb'].max())), dtype=g.dtype)
    for k, q in enumerate(rec):
        G[k, :q['La'], :q['Lb']] = g[q['row0']:q['row0'] + q['La'], q['col0']:q['col0'] + q['Lb']]
    return G


def _expected_out(rec, d, n_out):
    want = np.full(n_out + GUARD, FILL, dtype=np.float32)
    want[rec['dst0']] = d
    m = rec['dst1'] >= 0
    want[rec['dst1'][m]] = d[m]
    return want


@pytest.mark.parametrize('E', [3, 64])
@pytest.mark.parametrize('n_pairs', [1, 63, 64, 65, 1000])
def test_dtw_on_integer_scores_equals_the_fp32_definition(dev, n_pairs, E):
    from zs_amd import abx
    S, cols, rec = _int_case(n_pairs, 10 * n_pairs + E)
    d, _ = R.dtw_batch(_gather(R.g_hamming(S[:, :cols], E), rec), rec['La'], rec['Lb'], np.float32)
    if n_pairs == 1:
        assert d[0] == R.dtw(R.g_hamming(S[rec['row0'][0]:rec['row0'][0] + rec['La'][0], rec['col0'][0]:rec['col0'][0] + rec['Lb'][0]], E))[0]
    n_out = 2 * n_pairs
    want = _expected_out(rec, d, n_out)
    S_dev = torch.from_numpy(S).to(dev)
    w = np.asarray(abx.WIDTHS)[np.searchsorted(abx.WIDTHS, rec['Lb'])]
    if n_pairs == 1000:
        assert set(w.tolist()) == set(abx.WIDTHS) and (rec['La'] > rec['Lb']).any() and (rec['La'] < rec['Lb']).any()
    # bucketed by W as the planner emits them; every record in 64-lane groups; every record in 4-lane groups (the wide path)
    for name, launches in (('bucketed', [(int(W), rec[w == W]) for W in abx.WIDTHS if (w == W).any()]), ('64', [(0, rec)]), ('4', [(4, rec)]),
                           ('16', [(16, rec)])):
        for dpp in (0, 1):
            out = torch.full((n_out + GUARD,), FILL, dtype=torch.float32, device=dev)
            bad = torch.zeros(1, dtype=torch.int32, device=dev)
            for W, part in launches:
                abx.dtw(S_dev, cols, abx.to_device(part, dev), out[:n_out], bad, 'hamming', E, width=W, dpp=dpp)
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want), (name, dpp)
            assert int(bad[0]) == 0


def test_dtw_invalid_records_write_nan_and_count(dev):
    from zs_amd import abx
    S, cols, rec = _int_case(12, 5)
    rows = S.shape[0]
    E = 7
    d, _ = R.dtw_batch(_gather(R.g_hamming(S[:, :cols], E), rec), rec['La'], rec['Lb'], np.float32)
    broken = {1: dict(La=0), 2: dict(Lb=65), 3: dict(La=65), 4: dict(Lb=0), 5: dict(row0=rows - 1, La=2), 6: dict(col0=cols - 2, Lb=3),
              7: dict(row0=-1), 8: dict(col0=-1), 9: dict(La=-3), 10: dict(row0=2 ** 31 - 1, La=64)}
    for k, change in broken.items():
        for f, v in change.items():
            rec[f][k] = v
    n_out = 2 * rec.size
    want = _expected_out(rec, d, n_out)
    for k in broken:
        want[rec['dst0'][k]] = np.nan
        if rec['dst1'][k] >= 0:
            want[rec['dst1'][k]] = np.nan
    S_dev = torch.from_numpy(S).to(dev)
    for W in (0, 4, 16):
        out = torch.full((n_out + GUARD,), FILL, dtype=torch.float32, device=dev)
        bad = torch.full((1,), 100, dtype=torch.int32, device=dev)
        abx.dtw(S_dev, cols, abx.to_device(rec, dev), out[:n_out], bad, 'hamming', E, width=W)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want, equal_nan=True), W
        assert int(bad[0]) == 100 + len(broken)
    # a destination outside out: nothing is written there, the other destination gets NaN
    rec2 = rec[[0, 11]].copy()
    rec2['dst0'], rec2['dst1'] = [n_out, 3], [5, n_out + 7]
    out = torch.full((n_out + GUARD,), FILL, dtype=torch.float32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    abx.dtw(S_dev, cols, abx.to_device(rec2, dev), out[:n_out], bad, 'hamming', E)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.isnan(o[[3, 5]]).all() and int(bad[0]) == 2
    o[[3, 5]] = FILL
    assert (o == FILL).all()


def test_entry_points_refuse_what_they_cannot_run(dev):
    from zs_amd import _lib as L, abx
    S, cols, rec = _int_case(8, 1)
    S_dev, pairs = torch.from_numpy(S).to(dev), abx.to_device(rec, dev)
    out = torch.full((16 + GUARD,), FILL, dtype=torch.float32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    rinv = torch.ones(256, dtype=torch.float32, device=dev)
    good = dict(scores=L.ptr(S_dev), n_rows=S.shape[0], n_cols=cols, ld_s=S.shape[1], metric=0, E=8, width=0, dpp=0, pairs=L.ptr(pairs), n_pairs=8,
                out=L.ptr(out), n_out=16, bad=L.ptr(bad))
    assert L.lib().zs_abx_dtw(None, _stream()) == L.ZS_EINVAL
    for change in (dict(ld_s=cols - 1), dict(metric=2), dict(E=0), dict(width=5), dict(width=128), dict(n_pairs=-1), dict(n_rows=-1), dict(pairs=None),
                   dict(bad=None), dict(scores=None), dict(out=None), dict(metric=1), dict(metric=1, rinv_row=L.ptr(rinv)),
                   dict(scores=L.ptr(S_dev) + 2), dict(pairs=L.ptr(pairs) + 4), dict(out=L.ptr(out) + 1), dict(n_out=-1)):
        st = L.ABX_STRUCTS['ZsAbxDtw'](**{k: v for k, v in dict(good, **change).items() if v is not None})
        assert L.lib().zs_abx_dtw(ctypes.addressof(st), _stream()) == L.ZS_EINVAL, change
    st = L.ABX_STRUCTS['ZsAbxDtw'](n_pairs=0, metric=0, E=1)
    assert L.lib().zs_abx_dtw(ctypes.addressof(st), _stream()) == 0                 # zero work succeeds and launches nothing
    x = torch.ones(4, 8, dtype=torch.float32, device=dev)
    r = torch.full((4,), FILL, dtype=torch.float32, device=dev)
    assert L.lib().zs_abx_rownorm(None, _stream()) == L.ZS_EINVAL
    for change in (dict(ld_x=7), dict(E=0), dict(n=-1), dict(x=None), dict(rinv=None), dict(x=L.ptr(x) + 2)):
        st = L.ABX_STRUCTS['ZsAbxRownorm'](**{k: v for k, v in dict(dict(x=L.ptr(x), n=4, ld_x=8, E=8, rinv=L.ptr(r)), **change).items() if v is not None})
        assert L.lib().zs_abx_rownorm(ctypes.addressof(st), _stream()) == L.ZS_EINVAL, change
    st = L.ABX_STRUCTS['ZsAbxRownorm'](n=0, ld_x=8, E=8)
    assert L.lib().zs_abx_rownorm(ctypes.addressof(st), _stream()) == 0
    D = torch.zeros(4, 8, dtype=torch.float32, device=dev)
    jobs = abx.to_device(np.zeros(2, dtype=abx.JOB_DTYPE), dev)
    wins = torch.full((2,), -7, dtype=torch.int64, device=dev)
    goodc = dict(d=L.ptr(D), n=4, n_cols=8, ld_d=8, jobs=L.ptr(jobs), n_jobs=2, wins2=L.ptr(wins), bad=L.ptr(bad))
    assert L.lib().zs_abx_count(None, _stream()) == L.ZS_EINVAL
    for change in (dict(ld_d=7), dict(n_jobs=-1), dict(n=-1), dict(jobs=None), dict(wins2=None), dict(bad=None), dict(d=None),
                   dict(wins2=L.ptr(wins) + 4), dict(d=L.ptr(D) + 2)):
        st = L.ABX_STRUCTS['ZsAbxCount'](**{k: v for k, v in dict(goodc, **change).items() if v is not None})
        assert L.lib().zs_abx_count(ctypes.addressof(st), _stream()) == L.ZS_EINVAL, change
    st = L.ABX_STRUCTS['ZsAbxCount'](n_jobs=0)
    assert L.lib().zs_abx_count(ctypes.addressof(st), _stream()) == 0
    torch.cuda.synchronize()
    assert (out == FILL).all() and (r == FILL).all() and (wins == -7).all() and int(bad[0]) == 0


# ---- the angular metric ----------------------------------------------------------------------------------------------------------
def angular_case(E, seed, n, lengths, other, rows=96, cols=80):
    """Gaussian rows xa [rows, E] (row 0 zero) and xb [cols, E], n records with lengths from `lengths` (record 0: the zero row
    against one row), and the float64 reference: d64, the least cost margin of every pair's DP and the largest |cos| of the cells
    the records use.  The seed of every case is chosen so that max |cos| <= 0.9 and at most 2 % of the pairs have a margin below
    2 * 64 * tol: both conditions are properties of this reference alone."""
    from zs_amd import abx
    rs = np.random.RandomState(seed)
    xa, xb = rs.standard_normal((rows, E)).astype(np.float32), rs.standard_normal((cols, E)).astype(np.float32)
    xa[0] = 0
    rec = np.zeros(n, dtype=abx.PAIR_DTYPE)
    la, lb, swap = rs.choice(lengths, n), rs.choice(other, n), rs.uniform(size=n) < 0.5
    rec['La'], rec['Lb'] = np.where(swap, lb, la), np.where(swap, la, lb)
    rec['row0'] = 1 + (rs.uniform(size=n) * (rows - 1 - rec['La'] + 1)).astype(np.int64)
    rec['col0'] = (rs.uniform(size=n) * (cols - rec['Lb'] + 1)).astype(np.int64)
    rec['row0'][0], rec['La'][0], rec['Lb'][0] = 0, 1, 1
    rec['dst0'], rec['dst1'] = np.arange(n), -1
    c64 = R.cos64(xa, xb)
    G = _gather(np.arccos(c64) / np.pi, rec)
    d64, margin = R.dtw_batch(G, rec['La'], rec['Lb'], np.float64)
    used = _gather(np.abs(c64), rec)
    return xa, xb, rec, d64, margin, float(used.max())


@pytest.mark.parametrize('E', [8, 64, 1024])
def test_dtw_angular_within_the_derived_tolerance(dev, E):
    """|d - d64| <= tol(E) = (0.74 (2 E + 16) + 8 + (l_max + 1)) 2^-24 (abx_ref.tol), on the pairs whose float64 DP
    decided every minimum by a cost margin of at least 2 * 64 * tol."""
    from zs_amd import abx
    cfg = ANGULAR[E]
    xa, xb, rec, d64, margin, max_cos = angular_case(E, cfg['seed'], cfg['n'], cfg['lengths'], cfg['other'])
    tol = R.tol(E, max(cfg['lengths']))
    out_of = margin < 2 * 64 * tol
    print('E %d: tol %.3g, max |cos| %.3f, %d of %d pairs left out' % (E, tol, max_cos, int(out_of.sum()), rec.size))
    assert max_cos <= 0.9                                           # both conditions: on the float64 reference alone
    assert out_of.mean() <= 0.02
    xa_d, xb_d = torch.from_numpy(xa).to(dev), torch.from_numpy(xb).to(dev)
    ra, rb = abx.rownorm(xa_d), abx.rownorm(xb_d)
    S = torch.full((xa.shape[0], xb.shape[0] + 3), float('nan'), dtype=torch.float32, device=dev)
    abx.scores_tile(xa_d, xb_d, S, 'angular', E, torch.zeros(xb.shape[0], dtype=torch.float32, device=dev))
    out = torch.full((rec.size + GUARD,), FILL, dtype=torch.float32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    w = np.asarray(abx.WIDTHS)[np.searchsorted(abx.WIDTHS, rec['Lb'])]
    for W in sorted(set(w.tolist())):
        abx.dtw(S, xb.shape[0], abx.to_device(rec[w == W], dev), out[:rec.size], bad, 'angular', E, width=W, rinv_row=ra, rinv_col=rb)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[rec.size:] == FILL).all() and int(bad[0]) == 0
    # rownorm: 1 / sqrt of a sum of E squares: (E / 2 + 3) u relative; a zero row gives exactly 0
    ra_h = ra.cpu().numpy()
    assert ra_h[0] == 0.0
    want = 1.0 / np.sqrt((xa[1:].astype(np.float64) ** 2).sum(1))
    assert (np.abs(ra_h[1:] - want) <= (E / 2 + 3) * R.U * want).all()
    err = np.abs(o[:rec.size].astype(np.float64) - d64)
    print('E %d: max |d - d64| on the kept pairs %.3g' % (E, err[~out_of].max()))
    assert abs(float(o[0]) - 0.5) <= tol                            # the zero row: c = 0, g = 1/2
    assert (err[~out_of] <= tol).all(), (err[~out_of].max(), tol)
    # the same launch with the DPP shift: the same bits
    out2 = torch.full((rec.size,), FILL, dtype=torch.float32, device=dev)
    abx.dtw(S, xb.shape[0], abx.to_device(rec, dev), out2, bad, 'angular', E, width=8, rinv_row=ra, rinv_col=rb, dpp=1)
    torch.cuda.synchronize()
    assert np.array_equal(out2.cpu().numpy(), o[:rec.size])


# ---- zs_abx_count ----------------------------------------------------------------------------------------------------------------
def test_count_equals_numpy_exactly(dev):
    from zs_amd import abx
    rs = np.random.RandomState(7)
    n, cols, ld = 5, 2400, 2408
    D = np.full((n, ld), np.nan, dtype=np.float32)
    D[:, :cols] = rs.randint(0, 6, size=(n, cols)) * 0.25          # equal values everywhere
    D[2, 40] = D[2, 700] = D[3, 5] = np.nan                        # a NaN inside an A set and inside a B set
    sizes = (0, 1, 2, 63, 64, 65, 500, 1100)                       # 1100: more than one LDS tile of B
    jobs = []
    for na in sizes:
        for nb in sizes:
            a0 = int(rs.randint(0, 1200 - na + 1))
            b0 = 1200 + int(rs.randint(0, 1200 - nb + 1))
            for skip in ((a0 + na // 2) if na else a0, a0 + na, -1):       # inside A (where A has an entry), just outside, none
                jobs.append((int(rs.randint(0, n)), a0, a0 + na, b0, b0 + nb, skip))
    jobs += [(2, 0, 100, 600, 800, 40), (3, 0, 10, 0, 10, 5), (4, cols - 3, cols, 0, cols, cols - 1)]     # the row's NaN; overlapping sets; the last column
    n_good = len(jobs)
    jobs += [(-1, 0, 1, 1, 2, -1), (n, 0, 1, 1, 2, -1), (0, 5, 4, 1, 2, -1), (0, 0, cols + 1, 1, 2, -1), (0, 0, 1, -1, 2, -1), (0, 0, 1, 3, 2, -1),
             (0, 0, 1, 1, ld, -1), (0, -2, 1, 1, 2, -1)]
    rec = np.array(jobs, dtype=abx.JOB_DTYPE)
    want = np.zeros(len(jobs), dtype=np.int64)
    for k, (x, a0, a1, b0, b1, skip) in enumerate(jobs[:n_good]):
        A = np.array([a for a in range(a0, a1) if a != skip], dtype=np.int64)
        da, db = D[x, A][:, None], D[x, b0:b1][None, :]
        want[k] = 2 * int((da < db).sum()) + int((da == db).sum())
    assert want[:n_good].max() > 2 ** 20 and (want[:n_good] == 0).any()
    wins = torch.full((len(jobs) + GUARD,), -7, dtype=torch.int64, device=dev)
    bad = torch.full((1,), 10, dtype=torch.int32, device=dev)
    abx.count(torch.from_numpy(D).to(dev), cols, abx.to_device(rec, dev), wins, bad)
    torch.cuda.synchronize()
    got = wins.cpu().numpy()
    assert np.array_equal(got[:len(jobs)], want) and (got[len(jobs):] == -7).all()
    assert int(bad[0]) == 10 + len(jobs) - n_good


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _write_corpus(tmp):
    """tiny.item of the tiny corpus in the folder.  -> (item lines, {file stem: rows}, tokens)"""
    lines, files, toks = R.tiny_corpus(0)
    with open(os.path.join(tmp, 'tiny.item'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return lines, files, toks


def _brute(toks, dist_rows, tasks=('within', 'across')):
    """{task: {cell: [wins2, n]}} by the definition: dist_rows(token p, token q) -> d."""
    ref_tokens = [(t[3], t[4], t[5]) for t in toks]
    cache = {}

    def dist(p, q):
        if (p, q) not in cache:
            cache[(p, q)] = cache[(q, p)] = dist_rows(p, q)
        return cache[(p, q)]
    return {task: R.cell_counts(ref_tokens, task, dist) for task in tasks}


def _cells_of(details):
    from zs_amd import abx
    tokens, plan, wins = details['tokens'], details['plan'], details['wins2']
    out = {t: {} for t in abx.TASKS}
    for c in range(plan.cell_n.size):
        key = (tokens.phones[plan.cell_a[c]], tokens.phones[plan.cell_b[c]], tokens.ctxs[plan.cell_ctx[c]], tokens.speakers[plan.cell_s[c]])
        key = key if plan.cell_s2[c] < 0 else key + (tokens.speakers[plan.cell_s2[c]],)
        out[abx.TASKS[plan.cell_task[c]]][key] = [int(wins[c]), int(plan.cell_n[c])]
    return out


def test_score_units_hamming_equals_brute_force(dev, tmp_path, capsys):
    from zs_amd import abx
    import main as M
    tmp = str(tmp_path)
    rs = np.random.RandomState(11)
    E = 12
    lines, files, toks = _write_corpus(tmp)
    units = {}
    for stem, n in sorted(files.items()):
        units[stem] = rs.randint(0, 2, size=(n, E))
        units[stem][rs.randint(0, n, size=n // 2)] = units[stem][0]        # repeated rows: ties and zero distances
        with open(os.path.join(tmp, stem + '.txt'), 'w') as f:
            for row in units[stem]:
                f.write(' '.join(str(int(v)) for v in row) + '\n')

    def dist(p, q):
        a, b = (units[t[0]][t[1]:t[1] + t[2]] for t in (toks[p], toks[q]))
        S = (a[:, None, :] != b[None, :, :]).sum(-1)
        return R.dtw(R.g_hamming(S, E))[0]
    want = _brute(toks, dist)
    all_lines = [' '.join(str(int(v)) for v in row) for stem in sorted(units) for row in units[stem]]
    # once through the command in one tile, once under a budget that forces tiling
    M.main(['--score_units', tmp, '--abx_item', os.path.join(tmp, 'tiny.item'), '--score_out', os.path.join(tmp, 'out.json')])
    assert capsys.readouterr().out.count('[Score]') == 1
    with open(os.path.join(tmp, 'out.json')) as f:
        report = json.load(f)
    big = max(abx.plan(abx.collect_tokens(abx.parse_items(os.path.join(tmp, 'tiny.item')),
                                          {s: (0, n) for s, n in files.items()})).blocks, key=lambda b: b.frames)
    half = (big.frames + 1) // 2 + 2
    details = {}
    tiled = abx.score_units(tmp, os.path.join(tmp, 'tiny.item'), budget=4 * big.n * big.n + 4 * half * half, details=details,
                            out_path=os.path.join(tmp, 'tiled.json'))
    assert max(len(b.chunks) for b in details['plan'].blocks) == 2
    got = _cells_of(details)
    for task in abx.TASKS:
        assert got[task] == {k: v for k, v in want[task].items()}, task             # every cell's integer counts
        err = R.aggregate(want[task])
        assert tiled['tasks'][task]['error'] == err and report['tasks'][task]['error'] == err      # and the final doubles
        assert report['tasks'][task]['triplets'] == sum(v[1] for v in want[task].values()) and report['tasks'][task]['cells'] == len(want[task])
    assert report['metric'] == 'hamming' and report['files'] == sorted(files) and report['tokens'] == {
        'kept': len(toks), 'dropped': {'no_rows': 0, 'too_long': 0, 'no_file': 0}}
    b = abx.bitrate(all_lines)
    assert report['bits_per_unit'] == b['bits_per_unit'] and report['bits_per_second'] == b['bits_per_unit'] / R.P


def e2e_angular_case(seed, K=256, E=16):
    """A vector codebook of K Gaussian codewords of E columns and index files that use every codeword at most once, so that no two
    rows of the corpus are parallel.  -> (vectors, {stem: indices}, tokens, d64 [n, n], the least DP margin over all pairs, the
    largest |cos| over all pairs of rows of tokens, the least |d(A, X) - d(B, X)| over the triplets).  The seed is chosen on these
    float64 figures alone."""
    rs = np.random.RandomState(seed)
    lines, files, toks = R.tiny_corpus(0)
    vectors = rs.standard_normal((K, E)).astype(np.float32)
    perm = rs.permutation(K)
    idx, first = {}, 0
    for stem, n in sorted(files.items()):
        idx[stem] = perm[first:first + n]
        first += n
    assert first <= K
    rows = [vectors[idx[t[0]][t[1]:t[1] + t[2]]] for t in toks]
    n = len(toks)
    ctx = [t[4] for t in toks]
    pairs = [(p, q) for p in range(n) for q in range(n) if p != q and ctx[p] == ctx[q]]
    G = np.zeros((len(pairs), 4, 4))
    max_cos = 0.0
    for k, (p, q) in enumerate(pairs):
        c = R.cos64(rows[p], rows[q])
        max_cos = max(max_cos, float(np.abs(c).max()))
        G[k, :c.shape[0], :c.shape[1]] = np.arccos(c) / np.pi
    d, margin = R.dtw_batch(G, [rows[p].shape[0] for p, q in pairs], [rows[q].shape[0] for p, q in pairs], np.float64)
    d64 = np.full((n, n), np.nan)
    for k, (p, q) in enumerate(pairs):
        d64[p, q] = d[k]
    gap = np.inf
    ref_tokens = [(t[3], t[4], t[5]) for t in toks]
    for task in ('within', 'across'):
        for cell, A, B, X in R.triplets(ref_tokens, task):
            gap = min(gap, abs(d64[A, X] - d64[B, X]))
    return vectors, idx, toks, d64, float(margin.min()), max_cos, gap


def test_score_units_angular_through_index_files(dev, tmp_path):
    """The cells' integer counts equal the float64 brute force.  The inputs are chosen (E2E_ANGULAR_SEED) so that, in the float64
    reference, no triplet's two distances are closer than 2 tol, every |cos| is at most 0.9 and no DP minimum of a pair was decided by
    less than 2 (2 l_max - 1) tol -- a path cost of at most 2 l_max - 1 cells is off by less than that many tol -- so neither a path
    nor a comparison can come out differently within the derived error."""
    from zs_amd import abx
    from zs_amd.vq import VectorCodebook
    tmp = str(tmp_path)
    E, l_max = 16, 4
    vectors, idx, toks, d64, margin, max_cos, gap = e2e_angular_case(E2E_ANGULAR_SEED, E=E)
    tol = R.tol(E, l_max)
    print('tol %.3g: least margin %.3g (needs %.3g), max |cos| %.3f, least triplet gap %.3g (needs %.3g)' % (
        tol, margin, 2 * (2 * l_max - 1) * tol, max_cos, gap, 2 * tol))
    assert max_cos <= 0.9 and margin >= 2 * (2 * l_max - 1) * tol and gap >= 2 * tol
    _write_corpus(tmp)
    cb_path = os.path.join(tmp, 'K256.vq.npz')
    VectorCodebook(vectors).save(cb_path)
    for stem, ix in idx.items():
        with open(os.path.join(tmp, stem + '.idx.txt'), 'w') as f:
            f.write(''.join('%d\n' % k for k in ix))
    want = _brute(toks, lambda p, q: d64[p, q])
    details = {}
    report = abx.score_units(tmp, os.path.join(tmp, 'tiny.item'), codebook=abx.load_codebook(cb_path), details=details,
                             out_path=os.path.join(tmp, 'score.json'))
    got = _cells_of(details)
    for task in abx.TASKS:
        assert got[task] == want[task], task
        assert report['tasks'][task]['error'] == R.aggregate(want[task])
    assert report['metric'] == 'angular' and report['symbols'] == sum(len(v) for v in idx.values())
