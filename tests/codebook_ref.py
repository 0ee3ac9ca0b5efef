"""The definition of the unit codebook, numpy only: what zs_code_assign / zs_code_accum / zs_code_update and zs_amd.codebook.fit are
tested against.  Packed rows are convert.pack_units' (numpy.packbits(bitorder='little') along the columns); distances are taken on
the unpacked bits, so nothing here shares code with the kernels."""
import numpy as np


def row_bytes(E):
    return (E + 7) // 8


def bits(packed, E):
    p = np.asarray(packed, dtype=np.uint8)
    return np.unpackbits(p[:, :row_bytes(E)], axis=1, count=E, bitorder='little')


def pack(b):
    b = np.asarray(b)
    return np.packbits(b != 0, axis=1, bitorder='little').reshape(b.shape[0], row_bytes(b.shape[1]))


def planted(n, E, K0, flip, seed):
    r = np.random.RandomState(seed)
    cen = r.randint(0, 2, (K0, E))
    lab = r.randint(0, K0, n)
    b = cen[lab] ^ (r.rand(n, E) < flip)
    return pack(b)


def assign(units, code, E):
    """(idx int32 [n], dist int32 [n]): the codeword of least Hamming distance over the columns < E, the lowest index on ties."""
    units = np.asarray(units, dtype=np.uint8)
    c = bits(code, E).astype(np.float64)                     # 0 / 1 and sums <= 1024: exact in double
    idx = np.empty(len(units), dtype=np.int32)
    dist = np.empty(len(units), dtype=np.int32)
    for lo in range(0, len(units), 4096):
        a = bits(units[lo:lo + 4096], E).astype(np.float64)
        # |a - c| summed over the columns = ones(a) + ones(c) - 2 a.c
        d = a.sum(1)[:, None] + c.sum(1)[None, :] - 2.0 * (a @ c.T)
        idx[lo:lo + 4096] = d.argmin(1)                      # argmin: the first least entry
        dist[lo:lo + 4096] = d.min(1)
    return idx, dist


def snap(units, code, E):
    idx, dist = assign(units, code, E)
    return idx, pack(bits(code, E)[idx]), dist


def accum(units, idx, K, E):
    """(cnt int32 [K], ones int32 [K, E], bad): units with idx outside [0, K) are skipped and counted."""
    u = bits(units, E)
    idx = np.asarray(idx)
    ok = (idx >= 0) & (idx < K)
    cnt = np.bincount(idx[ok], minlength=K).astype(np.int32)
    ones = np.zeros((K, E), dtype=np.int32)
    np.add.at(ones, idx[ok], u[ok].astype(np.int32))
    return cnt, ones, int((~ok).sum())


def update(code, cnt, ones, E):
    """(new code, changed): majority vote per bit; a tie keeps the old bit; an empty cluster keeps its codeword."""
    old = bits(code, E)
    new = old.copy()
    cnt = np.asarray(cnt, dtype=np.int64)
    ones = np.asarray(ones, dtype=np.int64)
    for k in range(len(old)):
        if cnt[k] > 0:
            new[k] = np.where(2 * ones[k] > cnt[k], 1, np.where(2 * ones[k] < cnt[k], 0, old[k]))
    return pack(new), int((new != old).any(1).sum())


def init_rows(units, K, seed):
    """The first K pairwise different rows along RandomState(seed).permutation(n): their indices."""
    u = np.asarray(units, dtype=np.uint8)
    perm = np.random.RandomState(seed).permutation(len(u))
    seen, out = set(), []
    for i in perm:
        key = u[i].tobytes()
        if key not in seen:
            seen.add(key)
            out.append(int(i))
            if len(out) == K:
                return np.asarray(out, dtype=np.int64)
    raise ValueError('%d distinct rows, fewer than K = %d' % (len(seen), K))


def fit(units, K, E, iters=20, seed=0):
    """k-modes.  Returns (code, history [(total, changed, empties)], codes after every iteration, final idx).
    Per iteration: assign, accumulate, majority vote; then the empty k, in increasing order, take the units of largest distance (ties
    to the lowest unit index, each unit once).  changed counts the codewords that differ from the iteration's start."""
    units = np.asarray(units, dtype=np.uint8)
    code = units[init_rows(units, K, seed)].copy()
    code = pack(bits(code, E))
    history, codes = [], []
    for _ in range(iters):
        start = code.copy()
        idx, dist = assign(units, code, E)
        cnt, ones, _ = accum(units, idx, K, E)
        code, _ = update(code, cnt, ones, E)
        empties = np.flatnonzero(cnt == 0)
        if len(empties):
            order = np.argsort(-dist.astype(np.int64), kind='stable')       # largest distance first, the lowest index on ties
            for k, i in zip(empties, order):
                code[k] = pack(bits(units[i:i + 1], E))[0]
        changed = int((bits(code, E) != bits(start, E)).any(1).sum())
        history.append((int(dist.sum()), changed, int(len(empties))))
        codes.append(code.copy())
        if changed == 0:
            break
    idx, _ = assign(units, code, E)
    return code, history, codes, idx
