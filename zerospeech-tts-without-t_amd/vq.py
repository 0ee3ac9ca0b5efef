"""Vector codebook for enc_mode 'continues': K real-valued codewords of E columns fitted by k-means over encoder rows, and the snap of
every encoded frame to its nearest codeword in Euclidean distance.  A 'continues' model then emits sequences over at
most K symbols -- unit files of one index per line (<name>.idx.txt) -- and the Decoder can speak from those indices alone.

The work is four HIP entry points (csrc/zs_vq.hip): zs_vq_assign (nearest codeword: a GEMM on the exact-fp32 MFMA with an argmin
epilogue, the hot call), zs_vq_accum and zs_vq_update (the fixed-point sums and the means of one k-means iteration) and zs_vq_gather
(indices -> the Decoder's input operand).  The sums are int64, so a fit is bitwise reproducible.  tests/vq_ref.py is the numpy
definition.  Not in the reference, which has no codebook of any kind."""
import json
from fractions import Fraction

import numpy as np
import torch

from . import _lib as L
from .codebook import Codebook, refuse_continues, usage  # noqa: F401  (usage: the histogram statistics are the bit codebook's)

FORMAT_VERSION = 1
MAX_K = L.ENUMS['ZS_CODE_MAX_K']
MAX_E = L.ENUMS['ZS_CODE_MAX_E']
TILE_K = L.ENUMS['ZS_VQ_TILE_K']
SPLIT_N = L.ENUMS['ZS_VQ_SPLIT_N']
WORK_BYTES = L.ENUMS['ZS_VQ_WORK_BYTES']
MAX_SHIFT = 30


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


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


def assign(x, code, cnorm, idx=None, dist=None, moved=None, work=None, E=None):
    """zs_vq_assign on the current stream.  x fp32 / bf16 [n, >= E] (rows at stride(0)), code fp32 [K, E], cnorm fp32 [K]; every output
    optional: idx int32 [n], dist fp32 [n], moved int32 [1] (added to: the rows whose idx changes).  work: workspace(dev), or None for
    the row decomposition at any n."""
    E = int(code.shape[1]) if E is None else int(E)
    _check_x(x, E)
    n = int(x.shape[0])
    L.call('zs_vq_assign', 'ZsVqAssign', _stream(x.device), dtype=(L.ZS_F32 if x.dtype == torch.float32 else L.ZS_BF16), src_f32=0,
           x=L.ptr(x), n=n, ld_x=(x.stride(0) if n > 1 else max(int(x.shape[1]), E)), code=L.ptr(code), ld_code=code.stride(0),
           cnorm=L.ptr(cnorm), K=code.shape[0], E=E, idx=L.ptr(idx), dist=L.ptr(dist), moved=L.ptr(moved),
           count_moved=int(moved is not None), work=L.ptr(work), work_bytes=(0 if work is None else work.numel() * work.element_size()))


def gather(idx, code, start, length, T, dst, bad, E=None):
    """zs_vq_gather on the current stream: dst [n_frag, T, ld] (fp32 / bf16, contiguous) from idx int32 [n_idx] and the device tables
    start int64 / length int32 [n_frag]; bad int32 [1] is added to."""
    E = int(code.shape[1]) if E is None else int(E)
    L.call('zs_vq_gather', 'ZsVqGather', _stream(dst.device), dtype=(L.ZS_F32 if dst.dtype == torch.float32 else L.ZS_BF16), idx=L.ptr(idx),
           n_idx=idx.numel(), code=L.ptr(code), ld_code=code.stride(0), K=code.shape[0], E=E, start=L.ptr(start), len=L.ptr(length),
           n_frag=start.numel(), T=int(T), dst=L.ptr(dst), ld_dst=dst.shape[-1], bad=L.ptr(bad))


class VectorCodebook(object):
    """K codewords of E real columns: `vectors` fp32 [K, E] and `cnorm` fp32 [K] (the squared norms, summed in double) on the host, and
    `meta`: enc_mode, n_rows, seed, shift and the per-iteration history [(sum of distances, moved, empties)] of the fit."""
    kind = 'vector'

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

    def save(self, path):
        with open(path, 'wb') as f:
            np.savez(f, kind=np.array('vector'), format_version=np.int64(FORMAT_VERSION), K=np.int64(self.K), E=np.int64(self.E),
                     vectors=self.vectors, meta=np.array(json.dumps(self.meta)))

    @classmethod
    def load(cls, path, E=None):
        """ValueError naming the field for a malformed file, and for a width other than E (the Decoder's c_in) when E is given."""
        return cls._from_fields(_read_npz(path), path, E)

    @classmethod
    def _from_fields(cls, d, path, E=None):
        for k in ('kind', 'format_version', 'K', 'E', 'vectors', 'meta'):
            if k not in d:
                raise ValueError('%s: vector codebook field %r is missing' % (path, k))
        if d['kind'].shape != () or d['kind'].dtype.kind != 'U' or str(d['kind']) != 'vector':
            raise ValueError("%s: vector codebook field kind must be 'vector'" % path)
        for k in ('format_version', 'K', 'E'):
            if d[k].shape != () or d[k].dtype.kind not in 'iu':
                raise ValueError('%s: vector codebook field %r must be one integer' % (path, k))
        if int(d['format_version']) != FORMAT_VERSION:
            raise ValueError('%s: vector codebook field format_version is %d, this build reads %d' %
                             (path, int(d['format_version']), FORMAT_VERSION))
        try:
            meta = json.loads(str(d['meta']))
            if not isinstance(meta, dict):
                raise ValueError('not an object')
        except ValueError as e:
            raise ValueError('%s: vector codebook field meta is not a json object (%s)' % (path, e))
        try:
            cb = cls(d['vectors'], meta)
        except ValueError as e:
            raise ValueError('%s: vector codebook field vectors: %s' % (path, e))
        if cb.K != int(d['K']):
            raise ValueError('%s: vector codebook field K is %d but vectors has %d rows' % (path, int(d['K']), cb.K))
        if cb.E != int(d['E']):
            raise ValueError('%s: vector codebook field E is %d but vectors has %d columns' % (path, int(d['E']), cb.E))
        if E is not None:
            cb.check_width(E, path)
        return cb

    def check_width(self, E, where='codebook'):
        if int(E) != self.E:
            raise ValueError("%s: codebook field E is %d, the Decoder's input width (c_in) is %d" % (where, self.E, int(E)))

    def to(self, dev):
        """(vectors, cnorm) on the device, uploaded once."""
        dev = torch.device(dev)
        t = self._dev.get(dev)
        if t is None:
            t = self._dev[dev] = (torch.from_numpy(self.vectors).to(dev), torch.from_numpy(self.cnorm).to(dev))
        return t

    def snap(self, x_dev, work=None):
        """(idx int32 [n], dist fp32 [n]) of the rows of x_dev (fp32 / bf16 [n, >= E]), on the device."""
        code, cn = self.to(x_dev.device)
        idx = torch.empty(x_dev.shape[0], dtype=torch.int32, device=x_dev.device)
        dist = torch.empty(x_dev.shape[0], dtype=torch.float32, device=x_dev.device)
        assign(x_dev, code, cn, idx=idx, dist=dist, work=work)
        return idx, dist


def _read_npz(path):
    try:
        z = np.load(path, allow_pickle=False)
        return {k: z[k] for k in z.files}
    except Exception as e:
        raise ValueError('%s is not a codebook file: %s' % (path, e))


def load_codebook(path, enc_mode, E=None):
    """The codebook of a file, by the file's own fields: a VectorCodebook (field kind == 'vector') serves enc_mode 'continues' and no
    other mode; a bit Codebook serves every other mode and is refused for 'continues' in the bit codebook's own words."""
    d = _read_npz(path)
    if 'kind' in d or 'vectors' in d:
        if enc_mode != 'continues':
            raise ValueError("%s is a vector codebook (kind 'vector'), which serves enc_mode 'continues': this model's enc_mode is %r" %
                             (path, enc_mode))
        return VectorCodebook._from_fields(d, path, E)
    refuse_continues(enc_mode)
    return Codebook.load(path, E=E)


def init_rows(x, K, seed):
    """codebook.init_rows' rule over fp32 rows: the first K pairwise different rows along RandomState(seed).permutation(n)."""
    n, K = int(x.shape[0]), int(K)
    perm = np.random.RandomState(seed).permutation(n)
    seen, out, at, step = set(), [], 0, max(4096, 4 * K)
    while at < n:
        sel = perm[at:at + step]
        rows = x[torch.from_numpy(sel).to(x.device)].cpu().numpy() if torch.is_tensor(x) else np.asarray(x)[sel]
        for i, r in zip(sel, np.ascontiguousarray(rows, dtype=np.float32)):
            key = r.tobytes()
            if key not in seen:
                seen.add(key)
                out.append(int(i))
                if len(out) == K:
                    return np.asarray(out, dtype=np.int64)
        at += step
        step *= 4
    raise ValueError('init_rows: the rows hold %d distinct vectors, fewer than K = %d' % (len(seen), K))


def reseed_rows(cnt, dist):
    """(the empty k in increasing order, the rows they take): the rows of largest dist, ties to the lowest row, each row once."""
    empties = np.flatnonzero(np.asarray(cnt) == 0)
    order = np.argsort(-np.asarray(dist, dtype=np.float64), kind='stable')[:len(empties)]
    return empties, order


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
    """--fit_codebook for a 'continues' model: a vector codebook of K codewords over the encoder rows of a folder.  The *.wav of
    in_dir are read and encoded as codebook.fit_dir reads them (the same plan, trimming and skip list); the encoder's fp32 rows stay
    on the device (convert.encode_rows_on_device).  *.txt files are ignored: what write_encodings writes for 'continues' carries no
    encoding.  Writes the codebook to out_path and the same fit_codebook.json beside it (symbols used and entropy through
    codebook.usage); returns (VectorCodebook, that report)."""
    import os
    from . import convert as cv
    from .codebook import encode_dir
    if trainer.enc_mode != 'continues':
        raise ValueError("a vector codebook serves enc_mode 'continues': this model's enc_mode is %r" % trainer.enc_mode)
    K = int(K)
    if not 1 <= K <= MAX_K:
        raise ValueError('--fit_codebook: K must be in [1, %d] (got %d)' % (MAX_K, K))
    E = int(trainer.Decoder.c_in)
    used, skipped, parts, _ = encode_dir(trainer, seg_len, in_dir, batch, lambda specs: cv.encode_rows_on_device(specs, trainer, seg_len))
    if not parts:
        raise ValueError('--fit_codebook: %s holds no usable *.wav' % in_dir)
    x_dev = torch.cat(parts, dim=0).contiguous()
    cb = fit_vectors(x_dev, K, iters=iters, seed=seed, enc_mode=trainer.enc_mode)
    cb.check_width(E, out_path)
    idx, _ = cb.snap(x_dev, work=(workspace(x_dev.device) if x_dev.shape[0] < SPLIT_N else None))
    n_used, entropy = usage(idx, K)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    cb.save(out_path)
    report = {'codebook': out_path, 'kind': 'vector', 'K': K, 'E': E, 'in_dir': in_dir, 'files': used, 'skipped': skipped,
              'n_units': int(x_dev.shape[0]), 'seed': int(seed), 'history': cb.meta['history'], 'symbols_used': n_used,
              'entropy_bits_per_unit': entropy}
    with open(os.path.join(os.path.dirname(os.path.abspath(out_path)), 'fit_codebook.json'), 'w') as f:
        json.dump(report, f, indent=1)
    print('[Codebook] - K = %d vectors over %d rows of %d files: %d iterations, summed distance %.6g, %d symbols used, %.3f bits per unit '
          '-> %s' % (K, x_dev.shape[0], len(used), len(cb.meta['history']), cb.meta['history'][-1][0], n_used, entropy, out_path))
    return cb, report


def default_path(ckpt_dir, K):
    """{ckpt_dir}/codebooks/K<K>.vq.npz"""
    import os
    return os.path.join(ckpt_dir, 'codebooks', 'K%d.vq.npz' % int(K))
