"""Python restatement of zs_trim's definition (include/zs_amd.h), kept beside the tests that use it: the triangle-wave reflection,
the frame mean squares taken sample by sample through it (no np.pad, no block sums), the keep rule and the bounds.  The GPU tests
compare the kernel with zs_amd.convert.trim(), which is the definition; this file pins the ABI comment's wording to it on the CPU,
and gives the margin of every frame from the threshold that the exact comparison rests on."""
import numpy as np


def refl(j, n):
    """numpy's mode='reflect' index for any pad width: P = 2 (n - 1), m = j mod P taken non-negative, m if m < n else P - m;
    n == 1 maps every j to 0."""
    j = np.asarray(j, dtype=np.int64)
    if n == 1:
        return np.zeros_like(j)
    P = 2 * (n - 1)
    m = np.mod(j, P)                          # numpy's mod of a positive modulus is non-negative
    return np.where(m < n, m, P - m)


def frame_mse(y, frame_length=2048, hop=512):
    """mse[f] = mean_{i < frame_length} y[refl(f * hop + i - frame_length / 2)]^2 for f = 0 .. n / hop, in double."""
    y = np.asarray(y, dtype=np.float64)
    n = len(y)
    f = np.arange(1 + n // hop, dtype=np.int64)
    idx = f[:, None] * hop + np.arange(frame_length, dtype=np.int64)[None, :] - frame_length // 2
    return np.mean(y[refl(idx, n)] ** 2, axis=1)


def frame_db(y, frame_length=2048, hop=512):
    """Every frame's level relative to the loudest, with both 1e-10 floors."""
    mse = frame_mse(y, frame_length, hop)
    return 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(np.maximum(1e-10, mse.max()))


def trim_bounds(y, top_db=60, frame_length=2048, hop=512):
    n = len(y)
    if n <= 0:
        return 0, 0
    kept = np.flatnonzero(frame_db(y, frame_length, hop) > -top_db)
    if kept.size == 0:
        return 0, 0
    return int(kept[0]) * hop, min(n, (int(kept[-1]) + 1) * hop)


def margin_db(y, top_db=60, frame_length=2048, hop=512):
    """The distance of the frame closest to the threshold from it, in dB (inf for an empty signal)."""
    if len(y) == 0:
        return np.inf
    return float(np.min(np.abs(frame_db(y, frame_length, hop) + top_db)))
