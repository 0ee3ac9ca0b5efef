"""Band-limited sample-rate conversion on the GPU: the resampling inside the reference's `librosa.load(sound_file, sr=hp.sr)`
(preprocess.py:227-258, convert.py:377,431) and, the other way round, the opt-in output rate of the written wavs (--out_sr).

librosa <= 0.7 resamples with resampy's 'kaiser_best': a Kaiser-windowed sinc used as a band-limited interpolator (Smith's
method), scale=False, followed by fix_length to ceil(n * sr_out / sr_in) samples.  This module restates that design; resampy is
not available to this project, so sample-level parity with it is UNPINNED (as for the STFT, mel basis and trim restatements).
Where resampy has implementation quirks (its table step is truncated to an integer number of table entries), this definition is
the plain mathematical form.  The constants live here and nowhere else.

Definition.  tab[i] = ROLLOFF * sinc(ROLLOFF * i / 512) * K[i], i = 0..32768, K the right half of numpy.kaiser(2 * 32768 + 1, BETA),
in fp64.  h(u): a = |u| * 512, i = floor(a); h = tab[i] + (a - i) * (tab[i + 1] - tab[i]) if i < 32768 else 0.  With
s = min(1, sr_out / sr_in) and n_out = ceil(n_in * sr_out / sr_in):

    y[t] = s * sum_{m < n_in} x[m] * h(s * (t * sr_in / sr_out - m)),     t < n_out, fp32; samples outside [0, n_in) are zero.

Polyphase form (what `zs_resample` executes): g = gcd(sr_in, sr_out), P = sr_out / g, H = ceil(NZ / s), t * sr_in = q * sr_out + r,
p = r / g:  y[t] = sum_{j = -H..H} bank[p][j + H] * x[q + j],  bank[p][j + H] = s * h(s * (p * g / sr_out - j)), computed here in
fp64 and rounded once to fp32.
"""
from collections import namedtuple
from math import gcd

import numpy as np

from .hps import hp

NZ = 64                               # zero crossings on either side
STEPS = 512                           # table steps per zero crossing
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
MAX_RATIO = 32                        # sr_out / sr_in within [1 / MAX_RATIO, MAX_RATIO]
MAX_BANK = 16 * 1024 * 1024           # floats in a bank

Plan = namedtuple('Plan', ['bank', 'n_phase', 'n_tap', 'H', 'bank64'])

_TABLE = None
_PLANS = {}
_DEVICE_BANKS = {}


def filter_table():
    """The fp64 filter table, NZ * STEPS + 1 entries (right half of the symmetric filter)."""
    global _TABLE
    if _TABLE is None:
        n = NZ * STEPS
        k = np.kaiser(2 * n + 1, BETA)[n:]
        t = ROLLOFF * np.sinc(ROLLOFF * np.arange(n + 1, dtype=np.float64) / STEPS) * k
        t.setflags(write=False)
        _TABLE = t
    return _TABLE


def filter_h(u):
    """h(u) of the definition for an fp64 array u."""
    tab = filter_table()
    a = np.abs(np.asarray(u, dtype=np.float64)) * STEPS
    i = np.floor(a).astype(np.int64)
    ok = i < NZ * STEPS
    i = np.where(ok, i, 0)
    return np.where(ok, tab[i] + (a - i) * (tab[i + 1] - tab[i]), 0.0)


def out_length(n_in, sr_in, sr_out):
    """ceil(n_in * sr_out / sr_in): librosa's fix_length target."""
    return -((-int(n_in) * int(sr_out)) // int(sr_in))


def check_rates(sr_in, sr_out):
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in <= 0 or sr_out <= 0:
        raise ValueError('sample rates must be positive integers (got %d -> %d)' % (sr_in, sr_out))
    if sr_out > MAX_RATIO * sr_in or sr_in > MAX_RATIO * sr_out:
        raise ValueError('resampling %d -> %d Hz: the ratio must lie within [1/%d, %d]' % (sr_in, sr_out, MAX_RATIO, MAX_RATIO))
    return sr_in, sr_out


def plan(sr_in, sr_out):
    """Plan(bank fp32 [n_phase][n_tap], n_phase, n_tap, H, bank64: the same bank before rounding), cached per rate pair."""
    sr_in, sr_out = check_rates(sr_in, sr_out)
    key = (sr_in, sr_out)
    if key not in _PLANS:
        g = gcd(sr_in, sr_out)
        P = sr_out // g
        H = -((-NZ * sr_in) // sr_out) if sr_in > sr_out else NZ            # ceil(NZ / s)
        n_tap = 2 * H + 1
        if P * n_tap > MAX_BANK:
            raise ValueError('resampling %d -> %d Hz needs a bank of %d phases x %d taps, more than %d floats'
                             % (sr_in, sr_out, P, n_tap, MAX_BANK))
        s = min(1.0, sr_out / sr_in)
        num = np.arange(P, dtype=np.int64)[:, None] * g - np.arange(-H, H + 1, dtype=np.int64)[None, :] * sr_out   # r - j * sr_out
        bank64 = s * filter_h(s * (num / float(sr_out)))
        bank = bank64.astype(np.float32)
        bank.setflags(write=False)
        bank64.setflags(write=False)
        _PLANS[key] = Plan(bank, P, n_tap, H, bank64)
    return _PLANS[key]


def device_layout(pl, sr_in, sr_out):
    """The bank as zs_resample reads it (include/zs_amd.h): [n_tap][n_phase] with column k = t mod n_phase holding the phase of
    output t, (k * sr_in / g) mod n_phase, so that consecutive outputs read consecutive floats."""
    g = gcd(sr_in, sr_out)
    phase = (np.arange(pl.n_phase, dtype=np.int64) * (sr_in // g)) % pl.n_phase
    return np.ascontiguousarray(pl.bank[phase].T)


def device_bank(sr_in, sr_out, dev):
    """The device copy of the bank in zs_resample's layout, cached per rate pair and device."""
    import torch
    key = (int(sr_in), int(sr_out), dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _DEVICE_BANKS:
        _DEVICE_BANKS[key] = torch.from_numpy(device_layout(plan(sr_in, sr_out), int(sr_in), int(sr_out))).to(dev)
    return _DEVICE_BANKS[key]


def resample_device(src, n_in, sr_in, sr_out, dst_ld, n_in_max=0):
    """One zs_resample launch on the current stream of src's device.  src fp32 [n_utt][src_ld] and n_in int32 [n_utt] are device
    tensors; returns dst fp32 [n_utt][dst_ld] (row u: out_length(n_in[u]) samples, zeros behind)."""
    import torch
    from . import _lib as L
    pl = plan(sr_in, sr_out)
    dev = src.device
    bank = device_bank(sr_in, sr_out, dev)
    dst = torch.empty(src.shape[0], dst_ld, dtype=torch.float32, device=dev)
    L.call('zs_resample', 'ZsResample', torch.cuda.current_stream(dev).cuda_stream, src=L.ptr(src), src_ld=src.shape[1], n_in=L.ptr(n_in),
           n_utt=src.shape[0], sr_in=int(sr_in), sr_out=int(sr_out), bank=L.ptr(bank), n_phase=pl.n_phase, n_tap=pl.n_tap,
           dst=L.ptr(dst), dst_ld=dst_ld, n_in_max=int(n_in_max))
    return dst


def resample_batch(wavs, sr_in, sr_out=None, device=None, to_host=True):
    """wavs: list of 1-D float arrays, all at sr_in.  One padded pinned host-to-device copy, one zs_resample launch and one copy
    back; returns a list of float32 arrays of out_length(n) samples, or with to_host=False (dst fp32 [n][ld] on the device, lengths
    int64 [n] host array) without waiting for the launch.  sr_in == sr_out returns the inputs as float32 and does not touch the
    GPU; an empty list returns an empty list."""
    sr_out = hp.sr if sr_out is None else sr_out
    sr_in, sr_out = check_rates(sr_in, sr_out)
    ys = [np.asarray(w, dtype=np.float32) for w in wavs]
    if any(y.ndim != 1 for y in ys):
        raise ValueError('resample_batch takes 1-D arrays')
    if sr_in == sr_out:
        if to_host:
            return ys
        raise ValueError('resample_batch(to_host=False) needs sr_in != sr_out: nothing runs on the device otherwise')
    if not ys:
        if to_host:
            return []
        raise ValueError('resample_batch(to_host=False) needs at least one wav')
    import torch
    from . import _lib as L
    plan(sr_in, sr_out)                                          # rate errors before the device is asked for
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if dev.type != 'cuda':
        raise L.ZsError('zs_amd.resample runs on an MI355X only (there is no CPU path)')
    lens = np.array([len(y) for y in ys], dtype=np.int32)
    n_max = int(lens.max())
    if n_max < 1:
        raise ValueError('resample_batch: every wav is empty')
    host = np.zeros((len(ys), n_max), dtype=np.float32)
    for i, y in enumerate(ys):
        host[i, :len(y)] = y
    src = torch.from_numpy(host).pin_memory().to(dev, non_blocking=True)
    n_in = torch.from_numpy(lens).pin_memory().to(dev, non_blocking=True)
    outs = np.array([out_length(n, sr_in, sr_out) for n in lens], dtype=np.int64)
    dst = resample_device(src, n_in, sr_in, sr_out, int(outs.max()), n_in_max=n_max)
    if not to_host:
        return dst, outs
    dst_h = dst.cpu().numpy()
    return [dst_h[i, :outs[i]].copy() for i in range(len(ys))]
