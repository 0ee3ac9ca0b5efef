"""The definitions of ABX scoring (include/zs_amd_abx.h) restated in numpy: the frame distances, the DTW over
(cost, len) pairs in float32 in the stated operation order and in float64, the brute-force enumeration of the triplets over Python
loops, the aggregation and the tiny corpus the host and the GPU tests share.  Nothing here imports zs_amd."""
import itertools
import math

import numpy as np

U = 2.0 ** -24                                                     # the unit roundoff of fp32
ACOS_SLOPE = 0.74                                                  # >= 1 / (pi sqrt(1 - c^2)) for |c| <= 0.9027
P = 0.1                                                            # seconds per unit (8 frames of 200 samples at 16 kHz)


# ---- frame distances -------------------------------------------------------------------------------------------------------------
def g_hamming(S, E):
    """g = fl32(S / (float) E)"""
    return (np.asarray(S, dtype=np.float32) / np.float32(E)).astype(np.float32)


def rinv32(x):
    """1 / sqrt(sum x^2) in float32, 0 for a zero row (the summation order is the device's own: compare with a tolerance)."""
    s = (np.asarray(x, dtype=np.float32) ** 2).sum(axis=1, dtype=np.float32)
    with np.errstate(divide='ignore'):
        return np.where(s == 0, np.float32(0), np.float32(1) / np.sqrt(s)).astype(np.float32)


def g_angular32(S, rinv_row, rinv_col):
    """c = clamp(fl32(fl32(fl32(-0.5 S) * rinv_row[i]) * rinv_col[j]), -1, 1);  g = fl32(acosf(c) * (1 / pi))"""
    S = np.asarray(S, dtype=np.float32)
    c = ((np.float32(-0.5) * S) * np.asarray(rinv_row, dtype=np.float32)[:, None]).astype(np.float32) * np.asarray(rinv_col, dtype=np.float32)[None, :]
    c = np.clip(c.astype(np.float32), np.float32(-1), np.float32(1))
    return (np.arccos(c).astype(np.float32) * np.float32(1.0 / math.pi)).astype(np.float32)


def cos64(xa, xb):
    """The cosines of the rows of xa against the rows of xb in float64; a zero row gives 0."""
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    na, nb = np.sqrt((xa ** 2).sum(1)), np.sqrt((xb ** 2).sum(1))
    ia, ib = np.where(na == 0, 0.0, 1.0 / np.where(na == 0, 1.0, na)), np.where(nb == 0, 0.0, 1.0 / np.where(nb == 0, 1.0, nb))
    return np.clip((xa @ xb.T) * ia[:, None] * ib[None, :], -1.0, 1.0)


def g_angular64(xa, xb):
    return np.arccos(cos64(xa, xb)) / math.pi


def tol(E, l_max):
    """The bound on |d - d64| of the angular metric for tokens of at most l_max rows whose cosines lie in [-0.9, 0.9] and whose
    float64 DP takes the same path (DESIGN 41 derives it):
      the cosine:   E u |x||c| for the dot product of E terms in any order, E u / 2 + 2 u for each 1 / sqrt of a sum of E squares,
                    3 u for the three multiplications: at most (2 E + 16) u
      g:            the slope of acos / pi on the range, 0.74, times that; acosf to 4 ulp of a value below 4 and the product
                    with 1 / pi: 8 u
      d:            a mean of g's, so their error once; the partial sums are at most k, their roundings at most u k, the sum over a
                    path of len <= 2 l_max - 1 cells divided by len at most u l_max, and u for the division: (l_max + 1) u"""
    return (ACOS_SLOPE * (2 * E + 16) + 8 + (l_max + 1)) * U


# ---- DTW -------------------------------------------------------------------------------------------------------------------------
def dtw(g, dtype=np.float32):
    """d of one pair from its frame distances g [La, Lb], cell by cell as the definition reads.  -> (d, the least cost margin by
    which a minimum among more than one existing predecessor was decided; inf where none was)."""
    g = np.asarray(g, dtype=dtype)
    La, Lb = g.shape
    cost, length = np.zeros((La, Lb), dtype=dtype), np.zeros((La, Lb), dtype=np.int64)
    margin = math.inf
    for i in range(La):
        for j in range(Lb):
            if i == 0 and j == 0:
                cost[0, 0], length[0, 0] = g[0, 0], 1
                continue
            cand = [(cost[a, b], length[a, b]) for a, b in ((i - 1, j - 1), (i - 1, j), (i, j - 1)) if a >= 0 and b >= 0]
            cand.sort(key=lambda t: (t[0], t[1]))
            if len(cand) > 1:
                margin = min(margin, float(cand[1][0]) - float(cand[0][0]))
            cost[i, j] = dtype(g[i, j] + cand[0][0])               # one rounding
            length[i, j] = cand[0][1] + 1
    return dtype(cost[-1, -1] / dtype(length[-1, -1])), margin


def dtw_batch(G, La, Lb, dtype=np.float32):
    """dtw() of n pairs at once: G [n, >= max La, >= max Lb] (cells outside a pair's rectangle are ignored), La / Lb [n].  -> (d [n],
    margin [n]).  The same operations cell by cell, vectorised over the pairs."""
    G = np.asarray(G, dtype=dtype)
    La, Lb = np.asarray(La, dtype=np.int64), np.asarray(Lb, dtype=np.int64)
    n, ma, mb = G.shape[0], int(La.max()), int(Lb.max())
    big = np.iinfo(np.int64).max // 2
    cost, length = np.full((n, ma, mb), np.inf, dtype=dtype), np.full((n, ma, mb), big, dtype=np.int64)
    margin = np.full(n, np.inf)
    for i in range(ma):
        for j in range(mb):
            if i == 0 and j == 0:
                cost[:, 0, 0], length[:, 0, 0] = G[:, 0, 0], 1
                continue
            cands = [(cost[:, a, b], length[:, a, b]) for a, b in ((i - 1, j - 1), (i - 1, j), (i, j - 1)) if a >= 0 and b >= 0]
            mc, ml = cands[0]
            second = np.full(n, np.inf)
            for c, l in cands[1:]:
                better = (c < mc) | ((c == mc) & (l < ml))
                second = np.minimum(second, np.where(better, mc, c).astype(np.float64))
                mc, ml = np.where(better, c, mc), np.where(better, l, ml)
            inside = (i < La) & (j < Lb)
            if len(cands) > 1:
                margin = np.where(inside, np.minimum(margin, second - mc.astype(np.float64)), margin)
            cost[:, i, j] = (G[:, i, j] + mc).astype(dtype)
            length[:, i, j] = ml + 1
    k = np.arange(n)
    return (cost[k, La - 1, Lb - 1] / length[k, La - 1, Lb - 1].astype(dtype)).astype(dtype), margin


# ---- triplets and aggregation ----------------------------------------------------------------------------------------------------
def triplets(tokens, task):
    """Every triplet of the definition by brute force.  tokens: a list of (phone, ctx, speaker).  Yields (cell, A, B, X): cell is
    (a, b, ctx, s) for within and (a, b, ctx, s, s') for across; A, B, X index tokens."""
    n = len(tokens)
    for A, B, X in itertools.product(range(n), repeat=3):
        (pa, ca, sa), (pb, cb, sb), (px, cx, sx) = tokens[A], tokens[B], tokens[X]
        if not (ca == cb == cx) or pa == pb or px != pa or sb != sa:
            continue
        if task == 'within' and sx == sa and A != X:
            yield (pa, pb, ca, sa), A, B, X
        if task == 'across' and sx != sa:
            yield (pa, pb, ca, sa, sx), A, B, X


def cell_counts(tokens, task, dist):
    """{cell: [wins2, n]}: wins2 = the sum over the cell's triplets of 2 [d(A, X) < d(B, X)] + [d(A, X) == d(B, X)].  dist(p, q) -> d."""
    cells = {}
    for cell, A, B, X in triplets(tokens, task):
        dax, dbx = dist(A, X), dist(B, X)
        c = cells.setdefault(cell, [0, 0])
        c[0] += 2 * int(dax < dbx) + int(dax == dbx)
        c[1] += 1
    return cells


def aggregate(cells):
    """The task's error from {cell: (wins2, n)}: 100 (1 - the mean over ordered pairs (a, b) of the mean over cells of wins2 / 2n)."""
    pairs = {}
    for cell, (w, n) in cells.items():
        pairs.setdefault((cell[0], cell[1]), []).append(w / (2.0 * n))
    scores = [math.fsum(v) / len(v) for v in pairs.values()]        # exactly rounded sums: no order is left open
    return 100.0 * (1.0 - math.fsum(scores) / len(scores)) if scores else None


def token_rows(onset, offset, n_rows, file_offset=0.0):
    """The rows whose centre file_offset + (i + 0.5) P lies in [onset, offset], by trying every row."""
    return [i for i in range(n_rows) if onset <= file_offset + (i + 0.5) * P <= offset]


# ---- the tiny corpus -------------------------------------------------------------------------------------------------------------
def tiny_corpus(seed=0):
    """3 speakers, 4 phones, 3 contexts, 0 to 5 tokens per (phone, context, speaker); context ('x', 'y') holds the single phone p0 and
    context ('q', 'r') the single speaker s2.  Every speaker is one file of consecutive tokens of 1 to 4 rows.
    -> (item lines with the header, {file stem: rows}, tokens [(file, first row, rows, phone, ctx, speaker)] in file order)."""
    rng = np.random.RandomState(seed)
    speakers, phones = ['s0', 's1', 's2'], ['p0', 'p1', 'p2', 'p3']
    lines, files, tokens = ['#file onset offset #phone prev-phone next-phone speaker'], {}, []
    for s in speakers:
        row, stem = 1, 'utt_' + s                                  # (row 0 belongs to no token)
        for ctx in (('a', 'b'), ('x', 'y'), ('q', 'r')):
            for ph in phones:
                if ctx == ('x', 'y') and ph != 'p0':
                    continue
                if ctx == ('q', 'r') and s != 's2':
                    continue
                for _ in range(int(rng.randint(0, 6))):
                    n = int(rng.randint(1, 5))
                    lines.append('%s %.4f %.4f %s %s %s %s' % (stem, row * P + 0.01, (row + n) * P - 0.01, ph, ctx[0], ctx[1], s))
                    tokens.append((stem, row, n, ph, ctx, s))
                    row += n + int(rng.randint(0, 2))
        files[stem] = row + 1
    return lines, files, tokens
