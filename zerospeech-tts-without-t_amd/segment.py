"""Segmentation of unit sequences under a codebook: the index sequence of a whole utterance chosen at once,

    minimise   sum_t score(t, k_t)  +  lambda * #{ t >= 1 : k_t != k_(t-1) }

an exact dynamic programme over T frames and K codewords whose output is a sequence of runs (codeword, duration).  lambda is a
continuous rate / distortion knob on a codebook that is already fitted, in the score's own units: squared Euclidean distance under
a vector codebook, Hamming bits under a bit codebook.  lambda = 0 is the per-frame nearest codeword.

The work is three HIP entry points: zs_vq_scores / zs_code_scores keep the scores of a batch (the codebooks' scores_ methods) and
zs_seg_viterbi (csrc/zs_segment.hip) chooses the paths of every utterance of the batch in one launch.  include/zs_amd_segment.h has the
definition; tests/segment_ref.py restates it in numpy fp32 and is reproduced bit for bit.  Not in the reference, which has no
temporal model of its units."""
import math
import numbers

import numpy as np
import torch

from . import _lib as L

MAX_K = L.ENUMS['ZS_SEG_MAX_K']
SCORE_BUDGET = 4 << 30                                         # bytes of fp32 scores one batch may keep


def check_lambda(lam, who='--segment'):
    """lambda as a float: a finite number >= 0 that fp32 holds (ValueError otherwise).  None stays None: no segmentation."""
    if lam is None:
        return None
    if isinstance(lam, bool) or not isinstance(lam, numbers.Real):
        raise ValueError('%s: lambda must be a number >= 0 (got %r)' % (who, lam))
    v = float(lam)
    if math.isnan(v) or math.isinf(v) or v < 0 or v > float(np.finfo(np.float32).max):
        raise ValueError('%s: lambda must be finite and >= 0 (got %r)' % (who, lam))
    return float(np.float32(v))


def check_codebook(codebook, who='--segment'):
    """What can be segmented: a bit or a vector codebook of at most ZS_SEG_MAX_K codewords."""
    if codebook is None:
        raise ValueError('%s needs a codebook (--codebook): the path is chosen among its codewords' % who)
    if getattr(codebook, 'kind', None) == 'residual':
        raise ValueError('--segment does not segment the stages of a residual codebook: use a bit or a vector codebook')
    if codebook.K > MAX_K:
        raise ValueError('--segment keeps at most %d states (ZS_SEG_MAX_K): this codebook has K = %d' % (MAX_K, codebook.K))


def check_budget(n_rows, K, budget=None, who='--segment'):
    """The fp32 scores of a batch, n_rows x K, against the budget (bytes; None: SCORE_BUDGET)."""
    budget = SCORE_BUDGET if budget is None else int(budget)
    need = 4 * int(n_rows) * int(K)
    if need > budget:
        raise ValueError('%s: the scores of this batch, %d rows x %d codewords x 4 bytes = %d bytes, exceed the budget of %d bytes: '
                         'use a smaller batch' % (who, n_rows, K, need, budget))
    return need


def work_bytes(n_units, K):
    """ZS_SEG_WORK_BYTES(n_units, K) of include/zs_amd_segment.h."""
    return int(n_units) * (8 * ((int(K) + 63) // 64) + 4)


def unit_name(codebook):
    """What lambda is measured in under this codebook."""
    return 'squared Euclidean distance' if getattr(codebook, 'kind', None) == 'vector' else 'Hamming bits'


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def viterbi(scores, uoffs, lam, row=None, K=None, bad=None):
    """zs_seg_viterbi on the current stream, no synchronisation.  scores fp32 [n_rows, ld >= K] on the device (K: the codewords,
    None: every column); uoffs int64 [n_utt + 1] (device tensor, or host values, which are uploaded); row: optional int64 device
    tensor [n_units], the score row of every unit (None: unit i is row i).  Returns (idx int32 [n_units], n_seg int32 [n_utt], cost
    double [n_utt]) on the device.  bad: int32 [1] to count refused utterances in (added to); None: a counter of the call's own."""
    lam = check_lambda(lam, 'viterbi')
    if lam is None:
        raise ValueError('viterbi: lambda is None')
    if not torch.is_tensor(scores) or not scores.is_cuda or scores.dtype != torch.float32 or scores.dim() != 2 or \
            (scores.shape[1] > 1 and scores.stride(1) != 1):
        raise ValueError('viterbi: scores must be an fp32 device tensor [rows, K] with unit column stride')
    dev = scores.device
    K = int(scores.shape[1]) if K is None else int(K)
    ld = int(scores.stride(0)) if scores.shape[0] > 1 else max(int(scores.shape[1]), K)
    if not torch.is_tensor(uoffs):
        uoffs = torch.from_numpy(np.ascontiguousarray(uoffs, dtype=np.int64)).to(dev, non_blocking=True)
    if uoffs.dtype != torch.int64 or uoffs.dim() != 1 or uoffs.numel() < 1 or not uoffs.is_contiguous():
        raise ValueError('viterbi: uoffs must be int64 [n_utt + 1]')
    n_utt = int(uoffs.numel()) - 1
    if row is not None:
        if not torch.is_tensor(row) or row.dtype != torch.int64 or row.dim() != 1 or not row.is_contiguous() or row.device != dev:
            raise ValueError('viterbi: row must be a contiguous int64 device tensor [n_units]')
        n_units = int(row.numel())
    else:
        n_units = int(scores.shape[0])
    idx = torch.empty(n_units, dtype=torch.int32, device=dev)
    n_seg = torch.empty(n_utt, dtype=torch.int32, device=dev)
    cost = torch.empty(n_utt, dtype=torch.float64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev) if bad is None else bad
    wb = work_bytes(n_units, K)
    work = torch.empty((wb + 7) // 8, dtype=torch.int64, device=dev)
    L.call('zs_seg_viterbi', 'ZsSegViterbi', _stream(dev), scores=L.ptr(scores), n_rows=int(scores.shape[0]), ld_s=ld, uoffs=L.ptr(uoffs),
           n_utt=n_utt, row=L.ptr(row), n_units=n_units, lam=lam, K=K, work=L.ptr(work), work_bytes=work.numel() * 8, idx=L.ptr(idx),
           n_seg=L.ptr(n_seg), cost=L.ptr(cost), bad=L.ptr(bad))
    return idx, n_seg, cost


def runs(idx, uoffs=None):
    """Run-length coding on the host: per utterance an int64 array [n_runs, 2] of (codeword, duration in units).  idx: the indices of
    one utterance (uoffs None -> one array), or of a batch laid end to end with uoffs [n_utt + 1] (-> a list)."""
    i = np.asarray(idx).reshape(-1).astype(np.int64)
    if uoffs is not None:
        o = np.asarray(uoffs, dtype=np.int64)
        return [runs(i[o[u]:o[u + 1]]) for u in range(len(o) - 1)]
    if i.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    cut = np.flatnonzero(np.diff(i) != 0) + 1
    start = np.concatenate([[0], cut])
    return np.stack([i[start], np.diff(np.concatenate([start, [i.size]]))], axis=1)


def expand(r):
    """The inverse of runs(): the per-unit indices int32 of runs int [n_runs, 2]."""
    r = np.asarray(r, dtype=np.int64).reshape(-1, 2)
    if (r[:, 1] < 1).any():
        raise ValueError('expand: a run of fewer than 1 unit')
    return np.repeat(r[:, 0], r[:, 1]).astype(np.int32)


def seg_path(txt):
    """<name>.seg.txt beside <name>.txt"""
    return txt[:-len('.txt')] + '.seg.txt'


def write_segments(path, r):
    """<name>.seg.txt: one line `k d` per run."""
    r = np.asarray(r, dtype=np.int64).reshape(-1, 2)
    with open(path, 'w') as f:
        for k, d in r:
            f.write('%d %d\n' % (k, d))


def read_segments(path, K):
    """The runs int64 [n_runs, 2] of a <name>.seg.txt: every line `k d`, k in [0, K), d >= 1.  ValueError naming file and line."""
    out = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            w = line.split()
            try:
                if len(w) != 2:
                    raise ValueError
                k, d = int(w[0]), int(w[1])
            except ValueError:
                raise ValueError('%s line %d: expected `codeword duration`, two integers (got %r)' % (path, n, line.rstrip('\n')))
            if not 0 <= k < K:
                raise ValueError('%s line %d: codeword %d is outside [0, %d)' % (path, n, k, K))
            if d < 1:
                raise ValueError('%s line %d: duration %d is below 1 unit' % (path, n, d))
            out.append((k, d))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def seconds_per_unit():
    """Seconds of speech one unit covers: 8 spectrogram frames of hop_length samples."""
    from .preprocess import hp
    return 8.0 * hp.hop_length / hp.sr


class SegmentStats(object):
    """The manifest's "segment" entry of a folder run: units, segments and the histogram of the segment symbols.  lam None: a run
    that read its segments (--synth_dir --segments) and does not know what they were made with."""

    def __init__(self, lam, K):
        self.lam, self.units, self.segments = (None if lam is None else float(lam)), 0, 0
        self.counts = np.zeros(int(K), dtype=np.int64)

    def add(self, r):
        r = np.asarray(r, dtype=np.int64).reshape(-1, 2)
        self.units += int(r[:, 1].sum())
        self.segments += int(r.shape[0])
        self.counts += np.bincount(r[:, 0], minlength=self.counts.size)

    def manifest(self):
        from .codebook import usage_counts
        entropy = usage_counts(self.counts)[1]
        secs = self.units * seconds_per_unit()
        return {'lambda': self.lam, 'units': self.units, 'segments': self.segments,
                'mean_run_units': (self.units / self.segments if self.segments else 0.0), 'entropy_bits_per_segment': entropy,
                'bits_per_second': (self.segments / secs * entropy if secs > 0 else 0.0)}
