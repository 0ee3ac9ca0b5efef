"""Vector codebook for enc_mode 'continues': K real-valued codewords of E columns fitted by k-means over encoder rows, and the snap of
every encoded frame to its nearest codeword in Euclidean distance.  A 'continues' model then emits sequences over at
most K symbols -- unit files of one index per line (<name>.idx.txt) -- and the Decoder can speak from those indices alone.

The work is four HIP entry points (csrc/zs_vq.hip): zs_vq_assign (nearest codeword: a GEMM on the exact-fp32 MFMA with an argmin
epilogue, the hot call), zs_vq_accum and zs_vq_update (the fixed-point sums and the means of one k-means iteration) and zs_vq_gather
(indices -> the Decoder's input operand).  The sums are int64, so a fit is bitwise reproducible.  tests/vq_ref.py is the numpy
definition.  Not in the reference, which has no codebook of any kind."""
from fractions import Fraction

import numpy as np
import torch

from . import _lib as L
from .codebook import (FORMAT_VERSION, Codebook, CodebookFile, _stream, encode_dir, first_distinct, read_npz,  # noqa: F401
                       reseed_rows, usage)       # (the file format, reseed_rows and usage are one rule for both kinds of codebook)

MAX_K = L.ENUMS['ZS_CODE_MAX_K']
MAX_E = L.ENUMS['ZS_CODE_MAX_E']
TILE_K = L.ENUMS['ZS_VQ_TILE_K']
SPLIT_N = L.ENUMS['ZS_VQ_SPLIT_N']
WORK_BYTES = L.ENUMS['ZS_VQ_WORK_BYTES']
MAX_SHIFT = 30


def host_cnorm(vectors):
    """fp32 [K]: the squared norms, summed in double on the host."""
    v = np.asarray(vectors, dtype=np.float64)
    return (v * v).sum(1).astype(np.float32)


def vq_shift(n, maxabs):
    """The fixed-point shift of a fit over n rows of magnitude <= maxabs: the largest shift, at most 30, for which
    n * maxabs * 2^shift < 2^61 -- the int64 sum of a cluster that took every row then stays below 2^61 (+ n halves of rounding)."""
    n, m = int(n), float(maxabs)
    if n < 1:
        raise ValueError('vq_shift: no rows (n = %d)' % n)
    if not np.isfinite(m) or m < 0:
        raise ValueError('vq_shift: the largest magnitude must be finite and >= 0 (got %r)' % (maxabs,))
    s, top = MAX_SHIFT, Fraction(m) * n
    while top * Fraction(2) ** s >= Fraction(2) ** 61:
        s -= 1
        if s < -64:
            raise ValueError('vq_shift: n * maxabs = %g is outside what the int64 sums hold' % float(top))
    return s


def workspace(dev):
    """A workspace for zs_vq_assign's split over K (ZS_VQ_WORK_BYTES)."""
    return torch.empty(WORK_BYTES // 8, dtype=torch.int64, device=dev)


def _check_x(x, E, what='x'):
    if not torch.is_tensor(x) or not x.is_cuda or x.dim() != 2 or x.dtype not in (torch.float32, torch.bfloat16) or x.stride(1) != 1 \
            or x.shape[1] < E or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        raise ValueError('%s must be an fp32 or bf16 device tensor [n, >= %d] with unit column stride' % (what, E))


def launch_assign(stream, dt, x, n, ld_x, code, cnorm, E=None, idx=None, dist=None, moved=None, work=None):
    """THE zs_vq_assign launch: n rows of the compute dtype dt at the device pointer x, ld_x elements apart, against code fp32 [K, E]
    and cnorm fp32 [K] (tensors).  Outputs and workspace as assign() describes them."""
    L.call('zs_vq_assign', 'ZsVqAssign', stream, dtype=dt, src_f32=0, x=x, n=n, ld_x=ld_x, code=L.ptr(code), ld_code=code.stride(0),
           cnorm=L.ptr(cnorm), K=code.shape[0], E=(int(code.shape[1]) if E is None else int(E)), idx=L.ptr(idx), dist=L.ptr(dist),
           moved=L.ptr(moved), count_moved=int(moved is not None), work=L.ptr(work),
           work_bytes=(0 if work is None else work.numel() * work.element_size()))


def assign(x, code, cnorm, idx=None, dist=None, moved=None, work=None, E=None):
    """zs_vq_assign on the current stream.  x fp32 / bf16 [n, >= E] (rows at stride(0)), code fp32 [K, E], cnorm fp32 [K]; every output
    optional: idx int32 [n], dist fp32 [n], moved int32 [1] (added to: the rows whose idx changes).  work: workspace(dev), or None for
    the row decomposition at any n."""
    E = int(code.shape[1]) if E is None else int(E)
    _check_x(x, E)
    n = int(x.shape[0])
    launch_assign(_stream(x.device), (L.ZS_F32 if x.dtype == torch.float32 else L.ZS_BF16), L.ptr(x), n,
                  (x.stride(0) if n > 1 else max(int(x.shape[1]), E)), code, cnorm, E=E, idx=idx, dist=dist, moved=moved, work=work)


def launch_scores(stream, dt, x, n, ld_x, code, cnorm, out, ld_s, E=None):
    """THE zs_vq_scores launch: launch_assign's operands; out: the device pointer of fp32 [n][ld_s], ld_s >= K."""
    L.call('zs_vq_scores', 'ZsVqScores', stream, dtype=dt, src_f32=0, x=x, n=n, ld_x=ld_x, code=L.ptr(code), ld_code=code.stride(0),
           cnorm=L.ptr(cnorm), K=code.shape[0], E=(int(code.shape[1]) if E is None else int(E)), scores=out, ld_s=ld_s)


def launch_gather(stream, dt, idx, code, start, length, n_frag, T, dst, ld_dst, bad, E=None):
    """THE zs_vq_gather launch: the operand [n_frag, T, ld_dst] of the compute dtype dt at the device pointer dst from idx int32
    [n_idx], code fp32 [K, E] and the device tables start int64 / length int32 [n_frag]; bad int32 [1] is added to."""
    L.call('zs_vq_gather', 'ZsVqGather', stream, dtype=dt, idx=L.ptr(idx), n_idx=idx.numel(), code=L.ptr(code), ld_code=code.stride(0),
           K=code.shape[0], E=(int(code.shape[1]) if E is None else int(E)), start=L.ptr(start), len=L.ptr(length), n_frag=n_frag,
           T=int(T), dst=dst, ld_dst=ld_dst, bad=L.ptr(bad))


def gather(idx, code, start, length, T, dst, bad, E=None):
    """zs_vq_gather on the current stream: dst [n_frag, T, ld] (fp32 / bf16, contiguous) from idx int32 [n_idx] and the device tables
    start int64 / length int32 [n_frag]; bad int32 [1] is added to."""
    launch_gather(_stream(dst.device), (L.ZS_F32 if dst.dtype == torch.float32 else L.ZS_BF16), idx, code, start, length, start.numel(), T,
                  L.ptr(dst), dst.shape[-1], bad, E=E)


class VectorCodebook(CodebookFile):
    """K codewords of E real columns: `vectors` fp32 [K, E] and `cnorm` fp32 [K] (the squared norms, summed in double) on the host, and
    `meta`: enc_mode, n_rows, seed, shift and the per-iteration history [(sum of distances, moved, empties)] of the fit."""
    kind = 'vector'
    label, payload, suffix, _payload_error = 'vector codebook', 'vectors', 'vq.npz', 'vectors'
    _dir_files = '*.wav'
    _fit_line = ('[Codebook] - K = %d vectors over %d rows of %d files: %d iterations, summed distance %.6g, %d symbols used, '
                 '%.3f bits per unit -> %s')

    def __init__(self, vectors, meta=None):
        v = np.asarray(vectors)
        if v.dtype != np.float32 or v.ndim != 2:
            raise ValueError('vector codebook: vectors must be float32 [K, E] (got %s %s)' % (v.dtype, v.shape))
        if not 1 <= v.shape[0] <= MAX_K:
            raise ValueError('vector codebook: K must be in [1, %d] (got %d)' % (MAX_K, v.shape[0]))
        if not 1 <= v.shape[1] <= MAX_E:
            raise ValueError('vector codebook: E must be in [1, %d] (got %d)' % (MAX_E, v.shape[1]))
        if not np.isfinite(v).all():
            raise ValueError('vector codebook: vectors holds a value that is not finite')
        self.K, self.E, self.vectors, self.meta = int(v.shape[0]), int(v.shape[1]), np.ascontiguousarray(v), dict(meta or {})
        self.cnorm = host_cnorm(self.vectors)
        self._dev = {}

    @classmethod
    def _from_payload(cls, vectors, E, meta):
        return cls(vectors, meta)                                  # the file's E is compared with the columns behind this

    @staticmethod
    def check_mode(enc_mode, who="a vector codebook serves enc_mode 'continues'"):
        """A vector codebook serves enc_mode 'continues' and no other mode; `who`: the caller's own opening of the refusal."""
        if enc_mode != 'continues':
            raise ValueError("%s: this model's enc_mode is %r" % (who, enc_mode))

    def _upload(self, dev):
        """(vectors, cnorm) on the device."""
        return torch.from_numpy(self.vectors).to(dev), torch.from_numpy(self.cnorm).to(dev)

    def units(self):
        """What batched conversion and the folder drivers do with units under this codebook (convert._VectorUnits)."""
        from .convert import _VectorUnits
        return _VectorUnits(self)

    def rows_at(self, idx):
        """The rows fp32 [n, E] of the codewords idx (integers [n] in [0, K)) on the host: what an index file stands for (zs_amd.abx)."""
        return self.vectors[np.asarray(idx, dtype=np.int64).reshape(-1)]

    def snap(self, x_dev, work=None):
        """(idx int32 [n], dist fp32 [n]) of the rows of x_dev (fp32 / bf16 [n, >= E]), on the device."""
        code, cn = self.to(x_dev.device)
        idx = torch.empty(x_dev.shape[0], dtype=torch.int32, device=x_dev.device)
        dist = torch.empty(x_dev.shape[0], dtype=torch.float32, device=x_dev.device)
        assign(x_dev, code, cn, idx=idx, dist=dist, work=work)
        return idx, dist

    def scores_(self, rows, out):
        """out[i][k] = the score zs_vq_assign computes for row i and codeword k, bitwise (one zs_vq_scores on the current stream, no
        synchronisation).  rows fp32 / bf16 [n, >= E] and out fp32 [n, >= K] on the device; the columns of out at or beyond K are not
        written.  What --segment chooses its paths from (zs_amd.segment)."""
        from .codebook import _check_scores, _scores_ld
        from .segment import check_codebook
        check_codebook(self)
        _check_x(rows, self.E, 'rows')
        n = int(rows.shape[0])
        _check_scores(out, n, self.K)
        code, cn = self.to(rows.device)
        launch_scores(_stream(rows.device), (L.ZS_F32 if rows.dtype == torch.float32 else L.ZS_BF16), L.ptr(rows), n,
                      (rows.stride(0) if n > 1 else max(int(rows.shape[1]), self.E)), code, cn, L.ptr(out), _scores_ld(out, self.K))

    @classmethod
    def _dir_rows(cls, trainer, seg_len, in_dir, batch, E):
        """The *.wav of in_dir as the encoder's fp32 rows, left on the device (convert.encode_rows_on_device).  *.txt files are
        ignored: what write_encodings writes for 'continues' carries no encoding."""
        from . import convert as cv
        return encode_dir(trainer, seg_len, in_dir, batch, lambda specs: cv.encode_rows_on_device(specs, trainer, seg_len))[:3]

    @classmethod
    def _fit(cls, x_dev, K, iters, seed, E, enc_mode):
        return fit_vectors(x_dev, K, iters=iters, seed=seed, enc_mode=enc_mode)

    def _indices(self, x_dev):
        return self.snap(x_dev, work=(workspace(x_dev.device) if x_dev.shape[0] < SPLIT_N else None))[0]


def kind_for(enc_mode):
    """The codebook class that serves enc_mode: VectorCodebook for 'continues', the bit Codebook for every other mode."""
    return VectorCodebook if enc_mode == 'continues' else Codebook


def load_codebook(path, enc_mode, E=None):
    """The codebook of a file, by the file's own fields: a VectorCodebook (field kind == 'vector') serves enc_mode 'continues' and no
    other mode, as does a zs_amd.rvq.ResidualCodebook (field kind == 'residual': S stages of vectors); a bit Codebook serves every other
    mode and is refused for 'continues' in the bit codebook's own words."""
    d = read_npz(path)
    if 'kind' in d and d['kind'].shape == () and d['kind'].dtype.kind == 'U' and str(d['kind']) == 'residual':
        from .rvq import ResidualCodebook                         # S stages of vectors (zs_amd.rvq): 'continues' and no other mode
        ResidualCodebook.check_mode(enc_mode, "%s is a residual codebook (kind 'residual'), which serves enc_mode 'continues'" % path)
        return ResidualCodebook.from_fields(d, path, E)
    if 'kind' in d or 'vectors' in d:
        VectorCodebook.check_mode(enc_mode, "%s is a vector codebook (kind 'vector'), which serves enc_mode 'continues'" % path)
        return VectorCodebook.from_fields(d, path, E)
    Codebook.check_mode(enc_mode)
    return Codebook.from_fields(d, path, E)


def init_rows(x, K, seed):
    """codebook.init_rows' rule over fp32 rows: the first K pairwise different rows along RandomState(seed).permutation(n)."""
    def rows_at(sel):
        rows = x[torch.from_numpy(sel).to(x.device)].cpu().numpy() if torch.is_tensor(x) else np.asarray(x)[sel]
        return np.ascontiguousarray(rows, dtype=np.float32)
    return first_distinct(int(x.shape[0]), K, seed, rows_at, ('rows', 'vectors'))


def fit_vectors(x_dev, K, iters=40, seed=0, on_iter=None, enc_mode='continues'):
    """k-means over x_dev (fp32 [n, E] contiguous on the device, left unchanged) -> VectorCodebook.  One amax before the loop fixes the
    fixed-point shift (vq_shift).  Per iteration zs_vq_assign (counting the rows that move), zs_vq_accum, zs_vq_update and ONE small D2H
    copy of (sum of dist | moved | changed | bad | cnt) -- a synchronisation; fitting is not a captured path.  Empty clusters, in
    increasing k, take the rows of largest dist (ties to the lowest row, each row once), decided on the host from one D2H of dist in
    the iterations that have empties.  The fit stops at moved == 0 or after `iters`.  The sum of distances is recorded, not policed:
    in fp32 it may rise by rounding at convergence.  on_iter(i, dict(start, idx, dist, cnt, code, cnorm, shift)) -- host copies of the
    iteration's starting codebook, its assignment and the codebook it produced -- is called after every iteration."""
    K, iters = int(K), int(iters)
    if not 1 <= K <= MAX_K:
        raise ValueError('fit_vectors: K must be in [1, %d] (got %d)' % (MAX_K, K))
    if iters < 1:
        raise ValueError('fit_vectors: iters must be >= 1 (got %d)' % iters)
    if not torch.is_tensor(x_dev) or not x_dev.is_cuda or x_dev.dtype != torch.float32 or x_dev.dim() != 2 or not x_dev.is_contiguous():
        raise ValueError('fit_vectors: x must be a contiguous fp32 device tensor [n, E]')
    n, E, dev = int(x_dev.shape[0]), int(x_dev.shape[1]), x_dev.device
    if not 1 <= E <= MAX_E:
        raise ValueError('fit_vectors: E must be in [1, %d] (got %d)' % (MAX_E, E))
    if not 1 <= n < 2 ** 31:
        raise ValueError('fit_vectors: %d rows, the counters are int32' % n)
    shift = vq_shift(n, float(x_dev.abs().amax().item()))
    first = init_rows(x_dev, K, seed)
    code = x_dev[torch.from_numpy(first).to(dev)].contiguous()
    cnorm = torch.from_numpy(host_cnorm(code.cpu().numpy())).to(dev)
    st = _stream(dev)
    stats = torch.empty(6 + K, dtype=torch.int32, device=dev)     # sum of dist (fp64) | moved | changed | bad | pad | cnt [K]
    total = stats[0:2].view(torch.float64)
    sums = torch.empty(K, E, dtype=torch.int64, device=dev)
    idx = torch.full((n,), -1, dtype=torch.int32, device=dev)
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    work = workspace(dev) if n < SPLIT_N else None
    history = []
    for it in range(iters):
        stats.zero_()
        sums.zero_()
        start = code.cpu().numpy() if on_iter is not None else None
        assign(x_dev, code, cnorm, idx=idx, dist=dist, moved=stats[2:3], work=work)
        total.copy_(dist.sum(dtype=torch.float64))
        L.call('zs_vq_accum', 'ZsVqAccum', st, x=L.ptr(x_dev), idx=L.ptr(idx), n=n, ld_x=E, K=K, E=E, shift=shift, cnt=L.ptr(stats, 6),
               sum=L.ptr(sums), bad=L.ptr(stats, 4))
        L.call('zs_vq_update', 'ZsVqUpdate', st, code=L.ptr(code), ld_code=E, cnorm=L.ptr(cnorm), K=K, E=E, shift=shift,
               cnt=L.ptr(stats, 6), sum=L.ptr(sums), changed=L.ptr(stats, 3))
        h = stats.cpu().numpy()                                   # the synchronisation of this iteration
        tot, moved, bad, cnt = float(h[0:2].view(np.float64)[0]), int(h[2]), int(h[4]), h[6:]
        if bad:
            raise RuntimeError('fit_vectors: zs_vq_assign gave %d indices outside [0, %d)' % (bad, K))
        empties, rows = reseed_rows(cnt, dist.cpu().numpy()) if (cnt == 0).any() else ((), ())
        if len(empties):
            e_d = torch.from_numpy(empties).to(dev)
            code[e_d] = x_dev[torch.from_numpy(rows).to(dev)]
            cnorm[e_d] = (code[e_d].double() ** 2).sum(1).float()
        history.append((tot, moved, int(len(empties))))
        if on_iter is not None:
            on_iter(it, dict(start=start, idx=idx.cpu().numpy(), dist=dist.cpu().numpy(), cnt=cnt.copy(), code=code.cpu().numpy(),
                             cnorm=cnorm.cpu().numpy(), shift=shift))
        if moved == 0:
            break
    return VectorCodebook(code.cpu().numpy(), {'enc_mode': enc_mode, 'n_rows': n, 'seed': int(seed), 'shift': int(shift),
                                               'history': [list(x) for x in history]})


def fit_dir(trainer, seg_len, in_dir, K, out_path, iters=40, seed=0, batch=64):
    """--fit_codebook for a 'continues' model: a vector codebook of K codewords over the encoder rows of a folder
    (CodebookFile.fit_dir).  The *.wav of in_dir are read and encoded as codebook.fit_dir reads them (the same plan, trimming and
    skip list); *.txt files are ignored.  Returns (VectorCodebook, the report written to fit_codebook.json)."""
    return VectorCodebook.fit_dir(trainer, seg_len, in_dir, K, out_path, iters, seed, batch)


def default_path(ckpt_dir, K):
    """{ckpt_dir}/codebooks/K<K>.vq.npz"""
    return VectorCodebook.default_path(ckpt_dir, K)
