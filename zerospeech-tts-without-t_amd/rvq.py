"""Residual vector codebook for enc_mode 'continues' (DESIGN 33): S codebooks of K real-valued codewords of E columns each.  Stage 0
quantises the encoder's rows, stage s what stage s - 1 left over, so a frame is S indices -- S log2 K bits at S times the search of
one vector codebook -- and the first s' <= S of them are a valid coarser description: one fitted file and one folder of unit files
serve S bitrates.

The search of every stage is zs_vq_assign (zs_amd.vq), unchanged.  The two HIP entry points of csrc/zs_rvq.hip are the glue around it:
zs_rvq_residual (r = x - code[idx], one fp32 subtraction, in place from stage 1 on) and zs_rvq_gather (S planes of indices -> the
Decoder's input operand, the codewords added in fp32 in increasing stage).  The fit is greedy, stage by stage, each stage a
vq.fit_vectors over the residual rows, so it is bitwise reproducible.  tests/rvq_ref.py is the numpy definition.  Not in the reference,
which has no codebook of any kind."""
import numpy as np
import torch

from . import _lib as L
from .codebook import CodebookFile, _stream, usage
from .vq import MAX_E, MAX_K, SPLIT_N, VectorCodebook, _check_x, assign, fit_vectors, host_cnorm, workspace

MAX_S = L.ENUMS['ZS_RVQ_MAX_S']
MIN_S = 2


def check_stages(stages, S, who='stages'):
    """The number of stages used, 1 <= s' <= S (None: all S)."""
    if stages is None:
        return int(S)
    s = int(stages)
    if not 1 <= s <= S:
        raise ValueError('%s must be in [1, S = %d] (got %d)' % (who, S, s))
    return s


def launch_residual(stream, dt, src_f32, x, n, ld_x, idx, code, r, ld_r, bad, E=None):
    """THE zs_rvq_residual launch: n rows at the device pointer x (of the compute dtype dt, fp32 when src_f32), ld_x elements apart,
    minus code[idx] (code fp32 [K, E], idx int32 [n]: tensors) into the fp32 rows at the device pointer r, ld_r apart; bad int32 [1] is
    added to."""
    L.call('zs_rvq_residual', 'ZsRvqResidual', stream, dtype=dt, src_f32=int(src_f32), x=x, n=n, ld_x=ld_x, idx=L.ptr(idx), code=L.ptr(code),
           ld_code=code.stride(0), K=code.shape[0], E=(int(code.shape[1]) if E is None else int(E)), r=r, ld_r=ld_r, bad=L.ptr(bad))


def residual(x, idx, code, r, bad, E=None):
    """zs_rvq_residual on the current stream: r fp32 [n, >= E] = x (fp32 / bf16 [n, >= E]) - code[idx]; r may be x itself (fp32)."""
    E = int(code.shape[1]) if E is None else int(E)
    _check_x(x, E)
    _check_x(r, E, 'r')
    if r.dtype != torch.float32 or r.shape[0] != x.shape[0]:
        raise ValueError('r must be an fp32 device tensor with the rows of x')
    n = int(x.shape[0])
    launch_residual(_stream(x.device), (L.ZS_F32 if x.dtype == torch.float32 else L.ZS_BF16), 0, L.ptr(x), n,
                    (x.stride(0) if n > 1 else max(int(x.shape[1]), E)), idx, code, L.ptr(r), (r.stride(0) if n > 1 else max(int(r.shape[1]), E)),
                    bad, E=E)


def launch_gather(stream, dt, idx, s_use, code, start, length, n_frag, T, dst, ld_dst, bad):
    """THE zs_rvq_gather launch: the operand [n_frag, T, ld_dst] of the compute dtype dt at the device pointer dst from the planes idx
    int32 [S, n_idx], the codebooks code fp32 [S, K, E] and the device tables start int64 / length int32 [n_frag]; the first s_use
    stages are added; bad int32 [1] is added to."""
    ld_idx = idx.stride(0) if idx.shape[0] > 1 else idx.shape[1]          # (one plane: torch gives its only row any stride)
    L.call('zs_rvq_gather', 'ZsRvqGather', stream, dtype=dt, idx=L.ptr(idx), n_idx=idx.shape[1], ld_idx=ld_idx, S=idx.shape[0],
           s_use=int(s_use), code=L.ptr(code), ld_code=code.stride(1), plane_code=code.stride(0), K=code.shape[1], E=code.shape[2],
           start=L.ptr(start), len=L.ptr(length), n_frag=n_frag, T=int(T), dst=dst, ld_dst=ld_dst, bad=L.ptr(bad))


def gather(idx, s_use, code, start, length, T, dst, bad):
    """zs_rvq_gather on the current stream: dst [n_frag, T, ld] (fp32 / bf16, contiguous)."""
    launch_gather(_stream(dst.device), (L.ZS_F32 if dst.dtype == torch.float32 else L.ZS_BF16), idx, s_use, code, start, length, start.numel(),
                  T, L.ptr(dst), dst.shape[-1], bad)


def _stage_work(n, dev):
    return workspace(dev) if n < SPLIT_N else None


class ResidualCodebook(CodebookFile):
    """S stages of K codewords of E real columns: `vectors` fp32 [S, K, E] and `cnorm` fp32 [S, K] on the host, and `meta`: enc_mode,
    n_rows, seed, `stages` (per stage the fit history, the summed distance left behind it, the symbols used and the bits per unit)
    and bits_per_unit, their sum."""
    kind = 'residual'
    label, payload, suffix, _payload_error = 'residual codebook', 'vectors', 'rvq.npz', 'vectors'
    _dir_files = '*.wav'
    _fit_line = ('[Codebook] - K = %d vectors x %d stages over %d rows of %d files: %s iterations, summed distance %s, %d symbols used, '
                 '%.3f bits per unit -> %s')

    def __init__(self, vectors, meta=None):
        v = np.asarray(vectors)
        if v.dtype != np.float32 or v.ndim != 3:
            raise ValueError('residual codebook: vectors must be float32 [S, K, E] (got %s %s)' % (v.dtype, v.shape))
        if not MIN_S <= v.shape[0] <= MAX_S:
            raise ValueError('residual codebook: S must be in [%d, %d] (got %d)' % (MIN_S, MAX_S, v.shape[0]))
        if not 1 <= v.shape[1] <= MAX_K:
            raise ValueError('residual codebook: K must be in [1, %d] (got %d)' % (MAX_K, v.shape[1]))
        if not 1 <= v.shape[2] <= MAX_E:
            raise ValueError('residual codebook: E must be in [1, %d] (got %d)' % (MAX_E, v.shape[2]))
        if not np.isfinite(v).all():
            raise ValueError('residual codebook: vectors holds a value that is not finite')
        self.S, self.K, self.E = int(v.shape[0]), int(v.shape[1]), int(v.shape[2])
        self.vectors, self.meta = np.ascontiguousarray(v), dict(meta or {})
        self.cnorm = np.stack([host_cnorm(c) for c in self.vectors])
        self._dev = {}

    @classmethod
    def _from_payload(cls, vectors, E, meta):
        return cls(vectors, meta)

    def save(self, path):
        """CodebookFile.save's fields with S behind E."""
        import json
        from .codebook import FORMAT_VERSION
        with open(path, 'wb') as f:
            np.savez(f, kind=np.array(self.kind), format_version=np.int64(FORMAT_VERSION), K=np.int64(self.K), E=np.int64(self.E),
                     S=np.int64(self.S), vectors=self.vectors, meta=np.array(json.dumps(self.meta)))

    @classmethod
    def from_fields(cls, d, path, E=None):
        where = '%s: %s field' % (path, cls.label)
        if 'kind' in d and d['kind'].shape == () and d['kind'].dtype.kind == 'U' and str(d['kind']) == cls.kind:
            if 'S' not in d:                                      # (a missing or foreign kind is refused below, in the shared words)
                raise ValueError("%s 'S' is missing" % where)
            if d['S'].shape != () or d['S'].dtype.kind not in 'iu':
                raise ValueError("%s 'S' must be one integer" % where)
        cb = super(ResidualCodebook, cls).from_fields(d, path, E)
        if cb.S != int(d['S']):
            raise ValueError('%s S is %d but vectors has %d stages' % (where, int(d['S']), cb.S))
        return cb

    @staticmethod
    def check_mode(enc_mode, who="a residual codebook serves enc_mode 'continues'"):
        """A residual codebook serves enc_mode 'continues' and no other mode; `who`: the caller's own opening of the refusal."""
        if enc_mode != 'continues':
            raise ValueError("%s: this model's enc_mode is %r" % (who, enc_mode))

    @classmethod
    def default_path(cls, ckpt_dir, K, S):
        """{ckpt_dir}/codebooks/K<K>x<S>.rvq.npz"""
        import os
        return os.path.join(ckpt_dir, 'codebooks', 'K%dx%d.%s' % (int(K), int(S), cls.suffix))

    def _upload(self, dev):
        """(vectors [S, K, E], cnorm [S, K]) on the device."""
        return torch.from_numpy(self.vectors).to(dev), torch.from_numpy(self.cnorm).to(dev)

    stages = None                                 # with_stages(): the stages conversion and synthesis use (None: their own defaults)

    def with_stages(self, stages):
        """This codebook (the same arrays, the same device copies) using its first `stages` stages wherever it is handed to a
        conversion path as `codebook` (--rvq_stages).  None: every stage for conversion, a unit file's own columns for synthesis."""
        import copy
        cb = copy.copy(self)
        cb.stages = None if stages is None else check_stages(stages, self.S, '--rvq_stages')
        return cb

    def units(self, stages=None):
        """What batched conversion and the folder drivers do with units under the first `stages` stages (convert._ResidualUnits)."""
        from .convert import _ResidualUnits
        return _ResidualUnits(self, self.stages if stages is None else stages)

    def scores_(self, rows, out):
        """Refused: --segment chooses one path among the codewords of one codebook, and the stages of a residual codebook have none."""
        from .segment import check_codebook
        check_codebook(self)

    def snap(self, x_dev, stages=None, work=None, residuals=None):
        """(idx int32 [S', n], dist fp32 [S', n]) of the rows of x_dev (fp32 / bf16 [n, >= E]) through the first S' = stages stages, on
        the device: dist[s] is the squared distance left behind stage s.  work: a zs_vq_assign workspace, or None for the row
        decomposition.  residuals: a list that receives a copy of every stage's input behind the first (tests)."""
        s_use = check_stages(stages, self.S)
        _check_x(x_dev, self.E)
        dev, n = x_dev.device, int(x_dev.shape[0])
        code, cn = self.to(dev)
        idx = torch.empty(s_use, n, dtype=torch.int32, device=dev)
        dist = torch.empty(s_use, n, dtype=torch.float32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        r = None
        for s in range(s_use):
            assign(x_dev if s == 0 else r, code[s], cn[s], idx=idx[s], dist=dist[s], work=work, E=self.E)
            if s + 1 < s_use:
                if r is None:
                    r = torch.empty(n, self.E, dtype=torch.float32, device=dev)
                    residual(x_dev, idx[s], code[s], r, bad, E=self.E)
                else:
                    residual(r, idx[s], code[s], r, bad)
                if residuals is not None:
                    residuals.append(r.clone())
        return idx, dist

    def reconstruct(self, idx, stages=None):
        """fp32 [n, E] on the host from idx [S' <= S, n] (or [n] for one stage): the codewords of the first `stages` planes (default: all
        given) added in fp32 in increasing stage, each add rounded once.  A frame with a used index outside [0, K) is a zero row."""
        idx = np.asarray(idx)
        idx = idx[None] if idx.ndim == 1 else idx
        if idx.ndim != 2 or idx.dtype.kind not in 'iu' or not 1 <= idx.shape[0] <= self.S:
            raise ValueError('reconstruct: idx must be integers [1 .. %d, n] (got %s %s)' % (self.S, idx.dtype, idx.shape))
        s_use = check_stages(stages, idx.shape[0])
        idx = idx[:s_use].astype(np.int64)
        ok = ((idx >= 0) & (idx < self.K)).all(0)
        safe = np.where(ok[None], idx, 0)
        q = self.vectors[0][safe[0]].copy()
        for s in range(1, s_use):
            q = (q + self.vectors[s][safe[s]]).astype(np.float32)
        q[~ok] = 0.0
        return q

    def rows_at(self, idx):
        """The rows fp32 [n, E] of the index rows idx (integers [n, c], c <= S: an index file's lines) on the host: the sum of the
        stages a line holds (reconstruct)."""
        return self.reconstruct(np.asarray(idx).T)

    # ---- CodebookFile.fit_dir's hooks -------------------------------------------------------------------------------------------
    _dir_rows = VectorCodebook._dir_rows

    @classmethod
    def _fit(cls, x_dev, K, iters, seed, E, enc_mode, S=None):
        return fit_residual(x_dev, K, S, iters=iters, seed=seed, enc_mode=enc_mode)

    def _usage(self, rows_dev):
        """(symbols used by the busiest stage, bits per unit summed over the stages) of the fit rows: what the fit recorded."""
        return max(st['symbols_used'] for st in self.meta['stages']), float(self.meta['bits_per_unit'])

    def _report_extra(self):
        return {'S': self.S, 'stages': self.meta['stages']}

    def _fit_summary(self, K, n_rows, n_files, n_used, entropy, out_path):
        st = self.meta['stages']
        return self._fit_line % (K, self.S, n_rows, n_files, ' + '.join('%d' % len(s['history']) for s in st),
                                 ' > '.join('%.6g' % s['summed_distance'] for s in st), n_used, entropy, out_path)


def fit_residual(x_dev, K, S, iters=40, seed=0, on_stage=None, enc_mode='continues'):
    """The greedy fit: stage 0 is vq.fit_vectors(x, K, iters, seed); the rows are assigned again under the fitted codebook (fit_vectors
    returns the codebook after its last update), zs_rvq_residual forms what is left, and stage s is fit_vectors of that with seed + s.
    The residual is one fp32 [n, E] buffer, updated in place from stage 1 on; x_dev (fp32 [n, E] contiguous) is left unchanged.  Every
    step is bitwise reproducible, so the fit is.  on_stage(s, dict(rows, code, cnorm, idx, dist, history)) -- host copies of the
    stage's input rows, its fitted codebook and the assignment under it -- is called after every stage."""
    K, S = int(K), int(S)
    if not MIN_S <= S <= MAX_S:
        raise ValueError('fit_residual: S must be in [%d, %d] (got %d)' % (MIN_S, MAX_S, S))
    r, stages, planes = None, [], []
    bad = None
    for s in range(S):
        src = x_dev if s == 0 else r
        cb = fit_vectors(src, K, iters=iters, seed=int(seed) + s, enc_mode=enc_mode)
        dev, n, E = src.device, int(src.shape[0]), int(src.shape[1])
        idx, dist = cb.snap(src, work=_stage_work(n, dev))
        total = float(dist.sum(dtype=torch.float64).item())
        n_used, entropy = usage(idx, K)
        stages.append({'history': cb.meta['history'], 'shift': cb.meta['shift'], 'summed_distance': total, 'symbols_used': n_used,
                       'bits_per_unit': entropy})
        planes.append(cb.vectors)
        if on_stage is not None:
            on_stage(s, dict(rows=src.cpu().numpy(), code=cb.vectors, cnorm=cb.cnorm, idx=idx.cpu().numpy(), dist=dist.cpu().numpy(),
                             history=cb.meta['history']))
        if s + 1 < S:
            code_d = cb.to(dev)[0]
            if bad is None:
                bad = torch.zeros(1, dtype=torch.int32, device=dev)
                r = torch.empty(n, E, dtype=torch.float32, device=dev)
            residual(src, idx, code_d, r, bad)
    if bad is not None and int(bad.item()):
        raise RuntimeError('fit_residual: zs_vq_assign gave %d indices outside [0, %d)' % (int(bad.item()), K))
    return ResidualCodebook(np.stack(planes), {'enc_mode': enc_mode, 'n_rows': int(x_dev.shape[0]), 'seed': int(seed), 'stages': stages,
                                               'history': [st['history'] for st in stages],
                                               'bits_per_unit': float(sum(st['bits_per_unit'] for st in stages))})


def fit_dir(trainer, seg_len, in_dir, K, S, out_path, iters=40, seed=0, batch=64):
    """--fit_codebook K --rvq S for a 'continues' model: a residual codebook of S stages of K codewords over the encoder rows of a folder
    (CodebookFile.fit_dir: the same plan, trimming and skip list as a vector codebook's).  Returns (ResidualCodebook, the report
    written to fit_codebook.json, which holds the per-stage figures under 'stages')."""
    S = int(S)
    if not MIN_S <= S <= MAX_S:
        raise ValueError('--rvq: S must be in [%d, %d] (got %d)' % (MIN_S, MAX_S, S))
    return ResidualCodebook.fit_dir(trainer, seg_len, in_dir, K, out_path, iters, seed, batch, S=S)
