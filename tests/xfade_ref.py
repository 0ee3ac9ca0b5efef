"""The overlapped decode windows and their cross-fade, stated in numpy: the definition tests/test_overlap_host.py and
tests/test_gpu_overlap.py hold zs_amd.convert and zs_xfade_gather to.  It shares no code with the product.

Windows.  overlap and seg_len are in spectrogram frames; Lu = seg_len // 8, Vu = overlap // 8, Hu = Lu - Vu units.  An utterance of
n <= 2 Lu units is one window (0, n).  Else a = 0; while n - a > 2 Lu: emit (a, a + Lu), a += Hu; then the tail (a, n).

Blend.  A window of m units decodes to 8 m frames.  Frame t of the utterance, 0 <= t < 8 n, lies in one window (that window's row,
copied) or in the V = 8 Vu frames windows k and k + 1 share, at j = t - 8 a_{k+1}:
    out = fl32(fl32(u_j * x_k) + fl32(w_j * x_{k+1})),   w_j = fp32((2 j + 1) / (2 V)),   u_j = fp32(1 - (2 j + 1) / (2 V)),
the weights evaluated in double and rounded once, the blend without a fused multiply-add (numpy float32 arithmetic rounds every
operation)."""
import numpy as np


def accepted(overlap, seg_len):
    Lu = seg_len // 8
    return overlap == 0 or (overlap % 8 == 0 and 8 <= overlap <= 8 * (Lu // 2))


def windows(n, seg_len, overlap):
    assert accepted(overlap, seg_len) and n >= 1
    Lu = seg_len // 8
    Hu = Lu - overlap // 8
    if n <= 2 * Lu:
        return [(0, n)]
    out, a = [], 0
    while n - a > 2 * Lu:
        out.append((a, a + Lu))
        a += Hu
    out.append((a, n))
    return out


def weights(V):
    """(w, u) as float32 arrays of V entries."""
    w = np.array([np.float32((2 * j + 1) / (2.0 * V)) for j in range(V)], dtype=np.float32)
    u = np.array([np.float32(1.0 - (2 * j + 1) / (2.0 * V)) for j in range(V)], dtype=np.float32)
    return w, u


def blend2(u_j, x_k, w_j, x_k1):
    """fl32(fl32(u_j * x_k) + fl32(w_j * x_{k+1})) on float32 arrays, frame weights [V] against rows [V, C]."""
    a = (np.asarray(u_j, np.float32)[:, None] * np.asarray(x_k, np.float32)).astype(np.float32)
    b = (np.asarray(w_j, np.float32)[:, None] * np.asarray(x_k1, np.float32)).astype(np.float32)
    return (a + b).astype(np.float32)


def blend_windows(wins, decoded):
    """The utterance's frames [8 n, C] from its windows [(a, b)] in units and what each decoded to alone, decoded[k] float32
    [8 (b - a), C]."""
    n = wins[-1][1]
    C = decoded[0].shape[1]
    out = np.full((8 * n, C), np.nan, dtype=np.float32)
    for t in range(8 * n):
        ks = [k for k, (a, b) in enumerate(wins) if 8 * a <= t < 8 * b]
        assert 1 <= len(ks) <= 2
        k = ks[0]
        if len(ks) == 1:
            out[t] = decoded[k][t - 8 * wins[k][0]]
        else:
            assert ks[1] == k + 1
            V = 8 * (wins[k][1] - wins[k + 1][0])
            j = t - 8 * wins[k + 1][0]
            w, u = weights(V)
            out[t] = blend2(u[j:j + 1], decoded[k][t - 8 * wins[k][0]][None], w[j:j + 1], decoded[k + 1][j][None])[0]
    return out


def denorm(x):
    """convert.py:56-58 in float64 (a yardstick for orders of magnitude only: the kernels' own bits are compared with each other)."""
    return np.power(10.0, (np.clip(np.asarray(x, np.float64), 0, 1) * 100.0 - 100.0 + 20.0) * 0.05)


def gather(src, i0, i1, w0, w1, cols):
    """zs_xfade_gather with denorm = 0: float32 [rows, cols] from src float32 [src_rows, >= cols] and the four tables."""
    src = np.asarray(src, np.float32)
    n_src = src.shape[0]
    out = np.zeros((len(i0), cols), dtype=np.float32)
    for r in range(len(i0)):
        a, b = int(i0[r]), int(i1[r])
        if a < 0 or a >= n_src or b < -1 or b >= n_src:
            continue                                          # no source, or a bad entry: zeros, nothing read
        if b < 0:
            out[r] = src[a, :cols]
        else:
            out[r] = blend2(np.float32(w0[r])[None], src[a, :cols][None], np.float32(w1[r])[None], src[b, :cols][None])[0]
    return out
