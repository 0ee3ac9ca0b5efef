"""The definition of zs_vq_restart, numpy and Python integers only: dead codewords of the vector codebook go back onto this
step's encoder rows.  What the kernel, zs_amd.vq_train.restart_stride and VqBottleneck(restart=...) are tested against, bit for bit;
nothing here shares code with them.  The codebook's average and the order of the norm's sum are tests/vq_train_ref.py's."""
from math import gcd

import numpy as np

import vq_train_ref as T

F32 = np.float32
M64 = (1 << 64) - 1
SALT = 0x5651524553544152


def mix64(z):
    """The splitmix64 finaliser on an unsigned 64-bit value."""
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def start_row(seed, seed_dev, n):
    """seed: the launch's; seed_dev: the device word added to it (0 without one).  Unsigned 64-bit with wrap-around."""
    return mix64((int(seed) + int(seed_dev) + SALT) & M64) % int(n)


def stride(n):
    """The largest s with 1 <= s <= max(1, floor(0.6180339887 n)) and gcd(s, n) == 1."""
    for s in range(max(1, int(np.floor(0.6180339887 * n))), 0, -1):
        if gcd(s, n) == 1:
            return s


def dead(cnt, N, thresh):
    """cnt[k] == 0 and N[k] < thresh as fp32 values: NaN is not dead, equality is not dead."""
    with np.errstate(invalid='ignore'):
        return (np.asarray(cnt) == 0) & (np.asarray(N, dtype=F32) < F32(thresh))


def rows(dead_mask, n, start, step):
    """(k, r(k)) of every dead codeword in rising k: r = (start + (rank mod n) step) mod n."""
    ks = np.flatnonzero(dead_mask)
    return [(int(k), (start + (j % n) * step) % n) for j, k in enumerate(ks)]


def restart(thresh, x, idx_acc, cnt, N, m, code, cnorm, seed, seed_dev, step):
    """x fp32 [n, E]; idx_acc None or int [n]; the state as the average just left it.  Returns new (N, m, code, cnorm), restarted,
    skipped and the (k, row) pairs that were taken.  A dead codeword whose row has idx_acc < 0 stays as it is."""
    x = np.asarray(x, dtype=F32)
    n = len(x)
    assert 1 <= step <= n
    N, m, code, cnorm = (np.array(a, dtype=F32) for a in (N, m, code, cnorm))
    pairs = rows(dead(cnt, N, thresh), n, start_row(seed, seed_dev, n), step)
    taken = [(k, r) for k, r in pairs if idx_acc is None or idx_acc[r] >= 0]
    if taken:
        ks, rs = (np.array(a, dtype=np.int64) for a in zip(*taken))           # (every k once: nothing is written twice)
        code[ks] = x[rs]
        m[ks] = x[rs]
        N[ks] = F32(1.0)
        cnorm[ks] = T.norm_as_update(x)[rs]
    return (N, m, code, cnorm), len(taken), len(pairs) - len(taken), taken


def step(state, z, idx, shift, decay, thresh, seed, seed_dev, step_rows):
    """The codebook's average of vq_train_ref.State for the rows z under idx, then the restart; returns (cnt, used, restarted,
    skipped, taken).  `state` moves to the next codebook."""
    ia, _ = T.acc_index(z, idx)
    cnt, used = state.step(z, idx, shift, decay)
    (state.N, state.m, state.code, state.cnorm), restarted, skipped, taken = restart(
        thresh, z, ia, cnt, state.N, state.m, state.code, state.cnorm, seed, seed_dev, step_rows)
    return cnt, used, restarted, skipped, taken
