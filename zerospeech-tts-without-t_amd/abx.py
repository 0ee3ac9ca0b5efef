"""Scoring of unit files (--score_units): the ABX phone discriminability of the units of a folder, by a dynamic time warp
over frame distances for every pair of tokens that share a context, and their bitrate.

    token      the unit rows of a file whose centre time lies in [onset, offset] of a line of the .item file
    d(p, q)    the DTW distance of two tokens over g(i, j), the Hamming (bit units) or angular (real rows) frame distance
    triplet    (A, B, X): A and X are tokens of phone a, B of phone b != a, all in one context (prev, next); within one speaker
               (`within`), or A and B of one speaker and X of another (`across`).  It scores 1 if d(A, X) < d(B, X), 1/2 if equal.
    error      100 * (1 - the mean over ordered phone pairs of the mean over cells of the mean over triplets)

include/zs_amd_abx.h defines d to the bit and tests/abx_ref.py restates everything in numpy.  The host side is two parts:

  the planner (pure numpy, no GPU): parse_items -> collect_tokens -> plan(): the tokens of a context sorted by (speaker, phone) form
  a block, so that every A set and every B set is a contiguous range of a row of the block's distance matrix D; the block's frames
  are cut into chunks of at most ZS_SEG_MAX_K frames that fit the memory budget beside D, every pair of chunks is a score tile, every
  unordered pair of tokens is one ZsAbxPair record of exactly one tile (bucketed by the group width W its columns need), and every
  (cell, X) is one ZsAbxJob.

  the driver (run): the rows of the folder go to the device once; per tile one zs_code_scores / zs_vq_scores and one zs_abx_dtw per
  bucket, per block one zs_abx_count, one host read of the counts per group of blocks, and the aggregation in double from integers.

This aggregation is this project's own definition; it has not been compared with the challenge's evaluation tool."""
import glob
import json
import math
import os

import numpy as np

MAX_LEN = 64                                                       # ZS_ABX_MAX_LEN
MAX_TILE = 4096                                                    # ZS_SEG_MAX_K: the column side of zs_vq_scores / zs_code_scores
WIDTHS = (4, 8, 16, 32, 64)
TASKS = ('within', 'across')
METRICS = ('hamming', 'angular')
BUDGET = 4 << 30                                                   # bytes of D and one score tile a block may keep
GROUP_JOBS = 1 << 20                                               # count jobs per host read
PAIR_DTYPE = np.dtype([('row0', '<i4'), ('La', '<i4'), ('col0', '<i4'), ('Lb', '<i4'), ('dst0', '<i8'), ('dst1', '<i8')])
JOB_DTYPE = np.dtype([('x', '<i4'), ('a0', '<i4'), ('a1', '<i4'), ('b0', '<i4'), ('b1', '<i4'), ('skip', '<i4')])
DROP_REASONS = ('no_rows', 'too_long', 'no_file')


def seconds_per_unit():
    from .segment import seconds_per_unit as spu
    return spu()


# ---- the item file ---------------------------------------------------------------------------------------------------------------
def parse_items(path):
    """The tokens of an ABX .item file: a header line that starts with '#', then `file onset offset phone prev next speaker` per
    line (times in seconds); blank lines are skipped.  -> a list of dicts.  ValueError naming the file and the line otherwise."""
    out, seen_header = [], False
    with open(path, 'r') as f:
        for no, line in enumerate(f, 1):
            text = line.strip()
            if not text:
                continue
            if not seen_header:
                if not text.startswith('#'):
                    raise ValueError('%s, line %d: an item file starts with a header line that begins with # (got %r)' % (path, no, text))
                seen_header = True
                continue
            w = text.split()
            try:
                if len(w) != 7:
                    raise ValueError
                onset, offset = float(w[1]), float(w[2])
                if not (math.isfinite(onset) and math.isfinite(offset)) or offset < onset:
                    raise ValueError
            except ValueError:
                raise ValueError('%s, line %d: expected `file onset offset phone prev next speaker` with onset <= offset in seconds '
                                 '(got %r)' % (path, no, text))
            out.append({'file': w[0], 'onset': onset, 'offset': offset, 'phone': w[3], 'prev': w[4], 'next': w[5], 'speaker': w[6]})
    if not seen_header:
        raise ValueError('%s: no header line (the file is empty)' % path)
    return out


def token_rows(onset, offset, n_rows, file_offset=0.0, P=None):
    """(first row, row count) of the token [onset, offset] in a file of n_rows unit rows: the rows i whose centre
    file_offset + (i + 0.5) * P lies in [onset, offset], both ends included.  A count of 0: no row."""
    P = seconds_per_unit() if P is None else float(P)
    centre = lambda i: file_offset + (i + 0.5) * P                 # THE definition; the estimates below only start the search
    lo = int(math.ceil((onset - file_offset) / P - 0.5))
    while centre(lo - 1) >= onset:
        lo -= 1
    while centre(lo) < onset:
        lo += 1
    hi = int(math.floor((offset - file_offset) / P - 0.5))
    while centre(hi + 1) <= offset:
        hi += 1
    while centre(hi) > offset:
        hi -= 1
    lo, hi = max(lo, 0), min(hi, int(n_rows) - 1)
    return (lo, hi - lo + 1) if hi >= lo else (max(lo, 0), 0)


class Tokens(object):
    """The tokens kept: parallel arrays start (first row in the concatenated row table), length, phone, ctx, speaker (integer codes
    into the name lists phones, ctxs, speakers), and `dropped`, the count per reason."""

    def __init__(self, start, length, phone, ctx, speaker, phones, ctxs, speakers, dropped):
        self.start, self.length = np.asarray(start, dtype=np.int64), np.asarray(length, dtype=np.int64)
        self.phone, self.ctx, self.speaker = (np.asarray(a, dtype=np.int64) for a in (phone, ctx, speaker))
        self.phones, self.ctxs, self.speakers, self.dropped = list(phones), list(ctxs), list(speakers), dict(dropped)

    def __len__(self):
        return int(self.start.size)


def collect_tokens(items, file_rows, offsets=None, P=None):
    """items: parse_items' list; file_rows: {file stem: (first row in the row table, row count)}; offsets: {file stem: seconds}.
    A token is dropped when its file is absent ('no_file'), it has no row ('no_rows') or more than MAX_LEN rows ('too_long')."""
    offsets = offsets or {}
    code = lambda table, name: table.setdefault(name, len(table))
    phones, ctxs, speakers = {}, {}, {}
    dropped = dict.fromkeys(DROP_REASONS, 0)
    cols = [[], [], [], [], []]
    for it in items:
        fr = file_rows.get(it['file'])
        if fr is None:
            dropped['no_file'] += 1
            continue
        first, n = token_rows(it['onset'], it['offset'], fr[1], float(offsets.get(it['file'], 0.0)), P)
        if n == 0 or n > MAX_LEN:
            dropped['no_rows' if n == 0 else 'too_long'] += 1
            continue
        for c, v in zip(cols, (fr[0] + first, n, code(phones, it['phone']), code(ctxs, (it['prev'], it['next'])), code(speakers, it['speaker']))):
            c.append(v)
    return Tokens(*cols, phones=list(phones), ctxs=list(ctxs), speakers=list(speakers), dropped=dropped)


# ---- the plan --------------------------------------------------------------------------------------------------------------------
def width_for(Lb):
    """The least group width of zs_abx_dtw that holds Lb columns."""
    for w in WIDTHS:
        if Lb <= w:
            return w
    raise ValueError('a token of %d rows exceeds ZS_ABX_MAX_LEN = %d' % (Lb, MAX_LEN))


class Block(object):
    """The tokens of one context, sorted by (speaker, phone): tok (indices into Tokens), lens, foff (the frame offset of every token
    in the block's own row table, [n + 1]), chunks [(t0, t1)] of tokens, jobs (JOB_DTYPE) and job_cell (the cell of every job)."""

    def __init__(self, ctx, tok, lens):
        self.ctx, self.tok, self.lens = ctx, tok, lens
        self.n = int(tok.size)
        self.foff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.chunks, self.jobs, self.job_cell = [], np.zeros(0, dtype=JOB_DTYPE), np.zeros(0, dtype=np.int64)

    @property
    def frames(self):
        return int(self.foff[-1])

    def tiles(self):
        """The score tiles: (row chunk, column chunk), row chunk <= column chunk."""
        return [(r, c) for r in range(len(self.chunks)) for c in range(r, len(self.chunks))]

    def tile_pairs(self, r, c):
        """The records of tile (r, c) by group width: {W: PAIR_DTYPE array}.  Offsets are relative to the tile (its rows are the
        frames of chunk r, its columns those of chunk c); dst are offsets into the block's D [n][n].  Every unordered pair of tokens
        {x, y} of the block is a record of exactly one tile; on a diagonal tile, where both orientations of S exist, the shorter
        token takes the columns."""
        (r0, r1), (c0, c1) = self.chunks[r], self.chunks[c]
        x, y = np.meshgrid(np.arange(r0, r1, dtype=np.int64), np.arange(c0, c1, dtype=np.int64), indexing='ij')
        x, y = x.reshape(-1), y.reshape(-1)
        if r == c:
            keep = x < y
            x, y = x[keep], y[keep]
            swap = self.lens[y] > self.lens[x]
            x, y = np.where(swap, y, x), np.where(swap, x, y)
        rec = np.zeros(x.size, dtype=PAIR_DTYPE)
        rec['row0'], rec['La'] = self.foff[x] - self.foff[r0], self.lens[x]
        rec['col0'], rec['Lb'] = self.foff[y] - self.foff[c0], self.lens[y]
        rec['dst0'], rec['dst1'] = x * self.n + y, y * self.n + x
        w = np.asarray(WIDTHS)[np.searchsorted(WIDTHS, rec['Lb'])] if x.size else np.zeros(0, dtype=np.int64)
        return {int(W): rec[w == W] for W in WIDTHS if (w == W).any()}


class Plan(object):
    """blocks, and the cell table: cell_task (index into TASKS), cell_a, cell_b (phone codes), cell_ctx, cell_s, cell_s2 (speaker
    codes; s2 = -1 for within) and cell_n, the triplets of the cell."""

    def __init__(self, tokens, tasks, blocks, cells):
        self.tokens, self.tasks, self.blocks = tokens, tuple(tasks), blocks
        c = np.asarray(cells, dtype=np.int64).reshape(-1, 7)
        self.cell_task, self.cell_a, self.cell_b, self.cell_ctx, self.cell_s, self.cell_s2, self.cell_n = (c[:, k] for k in range(7))

    @property
    def n_jobs(self):
        return sum(b.jobs.size for b in self.blocks)


def check_tasks(tasks):
    """'within,across' or a sequence -> a tuple of distinct task names (ValueError otherwise)."""
    names = [t.strip() for t in tasks.split(',')] if isinstance(tasks, str) else list(tasks)
    if not names or any(t not in TASKS for t in names) or len(set(names)) != len(names):
        raise ValueError('--abx_task takes within, across or within,across (got %r)' % (tasks,))
    return tuple(names)


def _chunk(lens, limit):
    """Consecutive tokens in chunks of at most `limit` frames: [(t0, t1)]."""
    out, t0, used = [], 0, 0
    for t, n in enumerate(lens):
        if used + n > limit:
            out.append((t0, t))
            t0, used = t, 0
        used += int(n)
    out.append((t0, len(lens)))
    return out


def plan(tokens, tasks=TASKS, budget=None, max_tile=MAX_TILE):
    """The Plan of `tokens` for `tasks` under `budget` bytes (None: BUDGET) per block: D fp32 [n][n] and one score tile fp32 of at
    most max_tile x max_tile frames.  ValueError naming the context and the sizes for a block that cannot be tiled inside it."""
    tasks = check_tasks(tasks)
    budget = BUDGET if budget is None else int(budget)
    blocks, cells = [], []
    order = np.lexsort((np.arange(len(tokens)), tokens.phone, tokens.speaker, tokens.ctx))
    bounds = np.flatnonzero(np.diff(tokens.ctx[order])) + 1 if len(tokens) else np.zeros(0, dtype=np.int64)
    for tok in np.split(order, bounds) if len(tokens) else []:
        ctx = int(tokens.ctx[tok[0]])
        blk = Block(ctx, tok, tokens.length[tok])
        spk, pho = tokens.speaker[tok], tokens.phone[tok]
        # the contiguous range of every (speaker, phone) of the block
        key = spk * (len(tokens.phones) + 1) + pho
        starts = np.concatenate([[0], np.flatnonzero(np.diff(key)) + 1, [blk.n]])
        sets = {}
        for k in range(starts.size - 1):
            sets.setdefault(int(spk[starts[k]]), []).append((int(pho[starts[k]]), int(starts[k]), int(starts[k + 1])))
        jobs, job_cell = [], []

        def emit(task, a, b, s, s2, xs, ar, br, skip_self):
            n_trip = (ar[1] - ar[0] - int(skip_self)) * (br[1] - br[0]) * xs.size
            if n_trip <= 0:
                return
            j = np.zeros(xs.size, dtype=JOB_DTYPE)
            j['x'], j['a0'], j['a1'], j['b0'], j['b1'] = xs, ar[0], ar[1], br[0], br[1]
            j['skip'] = xs if skip_self else -1
            jobs.append(j)
            job_cell.append(np.full(xs.size, len(cells), dtype=np.int64))
            cells.append((TASKS.index(task), a, b, ctx, s, s2, n_trip))

        for s, ps in sets.items():
            for a, a0, a1 in ps:
                for b, b0, b1 in ps:
                    if b == a:
                        continue
                    if 'within' in tasks:
                        emit('within', a, b, s, -1, np.arange(a0, a1, dtype=np.int64), (a0, a1), (b0, b1), True)
                    if 'across' in tasks:
                        for s2, ps2 in sets.items():
                            if s2 == s:
                                continue
                            for a2, x0, x1 in ps2:
                                if a2 == a:
                                    emit('across', a, b, s, s2, np.arange(x0, x1, dtype=np.int64), (a0, a1), (b0, b1), False)
        if not jobs:
            continue                                              # a context without a triplet needs no distance
        blk.jobs, blk.job_cell = np.concatenate(jobs), np.concatenate(job_cell)
        # tiles: the largest chunk F (frames) with 4 n^2 + 4 F^2 <= budget, F <= max_tile; every token must fit a chunk
        need_d = 4 * blk.n * blk.n
        limit = min(int(max_tile), int(math.isqrt(max(budget - need_d, 0) // 4)))
        if limit < int(blk.lens.max()):
            raise ValueError('--score_units: the context %s has %d tokens of %d frames (the longest %d): its distance matrix of %d '
                             'bytes and one score tile do not fit the budget of %d bytes'
                             % (' '.join(tokens.ctxs[ctx]), blk.n, blk.frames, int(blk.lens.max()), need_d, budget))
        blk.chunks = _chunk(blk.lens, limit)
        blocks.append(blk)
    return Plan(tokens, tasks, blocks, cells)


# ---- aggregation -----------------------------------------------------------------------------------------------------------------
def aggregate(plan_, wins2):
    """wins2: the integer 2 x score sum of every cell of plan_ (a sequence of Python / numpy integers).  -> {task: {error,
    ordered_pairs, cells, triplets}}: the cell's score is wins2 / (2 n), the score of an ordered pair (a, b) the unweighted mean of
    its cells, the error 100 * (1 - the unweighted mean over the ordered pairs); all in double, every sum exactly rounded (math.fsum),
    so the figures do not depend on the order the cells come in.  A task without a cell has error None."""
    out = {}
    for t, task in enumerate(TASKS):
        if task not in plan_.tasks:
            continue
        pairs = {}
        sel = np.flatnonzero(plan_.cell_task == t)
        for c in sel:
            pairs.setdefault((int(plan_.cell_a[c]), int(plan_.cell_b[c])), []).append(int(wins2[c]) / (2.0 * int(plan_.cell_n[c])))
        scores = [math.fsum(v) / len(v) for v in pairs.values()]  # (fsum: the exactly rounded sum, whatever the order of the cells)
        out[task] = {'error': (100.0 * (1.0 - math.fsum(scores) / len(scores)) if scores else None), 'ordered_pairs': len(scores),
                     'cells': int(sel.size), 'triplets': int(plan_.cell_n[sel].sum())}
    return out


def cell_wins(plan_, job_wins):
    """Per-cell sums of the per-job counts (job_wins: one array per block, in the order of plan_.blocks) as Python integers."""
    wins = [0] * int(plan_.cell_n.size)
    for blk, jw in zip(plan_.blocks, job_wins):
        for c, w in zip(blk.job_cell.tolist(), np.asarray(jw).tolist()):
            wins[c] += int(w)
    return wins


# ---- bitrate ---------------------------------------------------------------------------------------------------------------------
def bitrate(lines, P=None):
    """lines: every line of every unit file of the folder (an iterable of strings).  A symbol is a distinct line; H is the entropy of
    the symbol distribution in bits.  -> {units, symbols, bits_per_unit: H, bits_per_second: H / P}."""
    P = seconds_per_unit() if P is None else float(P)
    counts = {}
    for s in lines:
        counts[s] = counts.get(s, 0) + 1
    n = sum(counts.values())
    H = -sum(c / n * math.log2(c / n) for c in counts.values()) if n else 0.0
    return {'units': n, 'symbols': len(counts), 'bits_per_unit': H + 0.0, 'bits_per_second': H / P + 0.0}


# ---- the folder ------------------------------------------------------------------------------------------------------------------
def read_folder(in_dir, codebook=None):
    """The unit files of in_dir: without a codebook the <name>.txt bit unit files (convert.read_units; the width is that of the first
    line of the first file), with one the <name>.idx.txt through the codebook's readers.  -> (stems, rows per file: float32 [U, E]
    of 0 / 1, or what codebook.rows_at gives, the lines of every file for the bitrate, E).  ValueError for a folder without one."""
    from . import convert as cv
    stems, rows, lines, E = [], [], [], None
    if codebook is None:
        paths = [p for p in sorted(glob.glob(os.path.join(in_dir, '*.txt'))) if not p.endswith('.idx.txt') and not p.endswith('.seg.txt')]
    else:
        paths = sorted(glob.glob(os.path.join(in_dir, '*.idx.txt')))
    if not paths:
        raise ValueError('--score_units: %s holds no %s unit file' % (in_dir, '*.txt' if codebook is None else '*.idx.txt'))
    for path in paths:
        with open(path, 'r') as f:
            text = [' '.join(line.split()) for line in f]
        if codebook is None:
            if E is None:
                E = len(text[0].split()) if text else 0
                if E < 1:
                    raise ValueError('%s: no units (the first line is empty)' % path)
            rows.append(cv.read_units(path, E))
            stems.append(os.path.basename(path)[:-len('.txt')])
        else:
            S = getattr(codebook, 'S', None)
            idx = cv.read_index_rows(path, codebook.K, S) if S else cv.read_indices(path, codebook.K)
            rows.append(codebook.rows_at(idx))
            stems.append(os.path.basename(path)[:-len('.idx.txt')])
            E = codebook.E
        lines.extend(text)
    return stems, rows, lines, E


def load_codebook(path):
    """The codebook of a file by the file's own fields (vq.load_codebook without a model: scoring needs no enc_mode)."""
    from .codebook import Codebook, read_npz
    d = read_npz(path)
    kind = str(d['kind']) if 'kind' in d and d['kind'].shape == () and d['kind'].dtype.kind == 'U' else None
    if kind == 'residual':
        from .rvq import ResidualCodebook
        return ResidualCodebook.from_fields(d, path)
    if 'kind' in d or 'vectors' in d:
        from .vq import VectorCodebook
        return VectorCodebook.from_fields(d, path)
    return Codebook.from_fields(d, path)


def check_metric(metric, codebook=None):
    """The metric of a run: `hamming` by default without a codebook and under a bit codebook, `angular` under a vector or residual
    one, where `hamming` is refused."""
    real = codebook is not None and getattr(codebook, 'kind', None) in ('vector', 'residual')
    metric = ('angular' if real else 'hamming') if metric is None else metric
    if metric not in METRICS:
        raise ValueError('--abx_metric must be hamming or angular (got %r)' % (metric,))
    if metric == 'hamming' and real:
        raise ValueError('--abx_metric hamming needs bit units: the rows of a %s codebook are real' % codebook.kind)
    return metric


def read_offsets(path):
    """--abx_offsets: a json object {file stem: seconds}."""
    with open(path, 'r') as f:
        d = json.load(f)
    if not isinstance(d, dict) or not all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) for v in d.values()):
        raise ValueError('%s: --abx_offsets takes a json object of seconds per file stem' % path)
    return {str(k): float(v) for k, v in d.items()}


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def _stream(dev):
    import torch
    return torch.cuda.current_stream(dev).cuda_stream


def rownorm(x):
    """zs_abx_rownorm on the current stream: rinv fp32 [n] of the fp32 device rows x [n, E]."""
    import torch
    from . import _lib as L
    rinv = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    L.call('zs_abx_rownorm', 'ZsAbxRownorm', _stream(x.device), x=L.ptr(x), n=x.shape[0], ld_x=(x.stride(0) if x.shape[0] > 1 else x.shape[1]),
           E=x.shape[1], rinv=L.ptr(rinv))
    return rinv


def dtw(S, n_cols, pairs, out, bad, metric, E, width=0, rinv_row=None, rinv_col=None, dpp=1):
    """zs_abx_dtw on the current stream.  S fp32 [n_rows, ld >= n_cols] and out fp32 (flat) on the device; pairs: a uint8 device
    tensor holding PAIR_DTYPE records.  dpp: the lane shift of the sweep, DPP (1, the faster one on every length mix measured:
    DESIGN 41) or __shfl_up (0); the results are the same bits."""
    from . import _lib as L
    L.call('zs_abx_dtw', 'ZsAbxDtw', _stream(S.device), scores=L.ptr(S), n_rows=S.shape[0], n_cols=int(n_cols),
           ld_s=(S.stride(0) if S.shape[0] > 1 else S.shape[1]), rinv_row=L.ptr(rinv_row), rinv_col=L.ptr(rinv_col),
           metric=METRICS.index(metric), E=int(E), width=int(width), dpp=int(dpp), pairs=L.ptr(pairs),
           n_pairs=pairs.numel() // PAIR_DTYPE.itemsize, out=L.ptr(out), n_out=out.numel(), bad=L.ptr(bad))


def count(D, n_cols, jobs, wins2, bad):
    """zs_abx_count on the current stream.  D fp32 [n, ld >= n_cols]; jobs: a uint8 device tensor of JOB_DTYPE records; wins2: an int64
    device tensor [n_jobs] (the kernel's uint64, read as int64)."""
    from . import _lib as L
    L.call('zs_abx_count', 'ZsAbxCount', _stream(D.device), d=L.ptr(D), n=D.shape[0], n_cols=int(n_cols),
           ld_d=(D.stride(0) if D.shape[0] > 1 else D.shape[1]), jobs=L.ptr(jobs), n_jobs=jobs.numel() // JOB_DTYPE.itemsize,
           wins2=L.ptr(wins2), bad=L.ptr(bad))


def to_device(records, dev):
    """A numpy record array as a uint8 device tensor."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(-1).copy()).to(dev)


def scores_tile(x_rows, x_cols, out, metric, E, zero_norm=None):
    """The frame scores of a tile into out fp32 [n_rows, >= n_cols]: zs_code_scores of packed rows (hamming) or zs_vq_scores of fp32
    rows against x_cols as `code` with cnorm all zero (angular: S = -2 x.c)."""
    from . import _lib as L
    dev, K = x_rows.device, int(x_cols.shape[0])
    ld = int(out.stride(0)) if out.shape[0] > 1 else int(out.shape[1])
    if metric == 'hamming':
        L.call('zs_code_scores', 'ZsCodeScores', _stream(dev), units=L.ptr(x_rows), n=x_rows.shape[0], row_bytes=x_rows.shape[1],
               code=L.ptr(x_cols), K=K, code_bytes=x_cols.shape[1], E=int(E), scores=L.ptr(out), ld_s=ld)
    else:
        L.call('zs_vq_scores', 'ZsVqScores', _stream(dev), dtype=L.ZS_F32, src_f32=0, x=L.ptr(x_rows), n=x_rows.shape[0], ld_x=x_rows.shape[1],
               code=L.ptr(x_cols), ld_code=x_cols.shape[1], cnorm=L.ptr(zero_norm), K=K, E=int(E), scores=L.ptr(out), ld_s=ld)


def run(plan_, rows, metric, E, device='cuda:0', dpp=1, keep=None):
    """The per-job counts of plan_ over `rows` (the concatenated row table of the folder on the host: packed uint8 for hamming,
    float32 [N, E] for angular): a list of int64 arrays, one per block.  One upload of the rows; per tile the scores and one
    zs_abx_dtw per bucket; per block one zs_abx_count; one host read per group of blocks of at most GROUP_JOBS jobs.  keep: a dict
    that receives {'D': [the distance matrix of every block, on the host]} (tests)."""
    import torch
    dev = torch.device(device)
    rows_dev = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    tok = plan_.tokens
    out, group, group_jobs = [], [], 0
    if keep is not None:
        keep['D'] = []

    def flush():
        for w in group:
            out.append(w.cpu().numpy())                           # (one synchronising read per group: the copies queue behind the kernels)
        del group[:]

    for blk in plan_.blocks:
        # the block's own row table: the frames of its tokens in the block's order
        frame = np.concatenate([np.arange(s, s + n, dtype=np.int64) for s, n in zip(tok.start[blk.tok], blk.lens)])
        xb = rows_dev.index_select(0, torch.from_numpy(frame).to(dev)).contiguous()
        rinv = rownorm(xb) if metric == 'angular' else None
        D = torch.full((blk.n, blk.n), float('nan'), dtype=torch.float32, device=dev)
        for r, c in blk.tiles():
            fr0, fr1 = int(blk.foff[blk.chunks[r][0]]), int(blk.foff[blk.chunks[r][1]])
            fc0, fc1 = int(blk.foff[blk.chunks[c][0]]), int(blk.foff[blk.chunks[c][1]])
            S = torch.empty(fr1 - fr0, fc1 - fc0, dtype=torch.float32, device=dev)
            zero = torch.zeros(fc1 - fc0, dtype=torch.float32, device=dev) if metric == 'angular' else None
            scores_tile(xb[fr0:fr1], xb[fc0:fc1], S, metric, E, zero)
            for W, rec in blk.tile_pairs(r, c).items():
                dtw(S, fc1 - fc0, to_device(rec, dev), D, bad, metric, E, width=W, dpp=dpp,
                    rinv_row=(rinv[fr0:fr1] if rinv is not None else None), rinv_col=(rinv[fc0:fc1] if rinv is not None else None))
        wins2 = torch.zeros(blk.jobs.size, dtype=torch.int64, device=dev)
        count(D, blk.n, to_device(blk.jobs, dev), wins2, bad)
        if keep is not None:
            keep['D'].append(D.cpu().numpy())
        group.append(wins2)
        group_jobs += blk.jobs.size
        if group_jobs >= GROUP_JOBS:
            flush()
            group_jobs = 0
    flush()
    if int(bad.item()):
        raise RuntimeError('--score_units: %d records of the plan were refused by the kernels' % int(bad.item()))
    return out


def score_units(in_dir, item_path, tasks='within,across', metric=None, codebook=None, offsets=None, out_path=None, budget=None,
                device='cuda:0', details=None):
    """--score_units: the ABX error of the unit files of in_dir against the item file, and their bitrate.  Writes score.json (out_path,
    default in_dir/score.json), prints one [Score] line and returns the report.  details: a dict that receives the tokens, the plan and
    the integer count of every cell (tests)."""
    from . import convert as cv
    tasks = check_tasks(tasks)
    metric = check_metric(metric, codebook)
    stems, rows, lines, E = read_folder(in_dir, codebook)
    items = parse_items(item_path)
    if metric == 'hamming':
        table = [r if r.dtype == np.uint8 else cv.pack_units(r) for r in rows]
    else:
        table = [cv.unpack_units(r, E) if r.dtype == np.uint8 else np.asarray(r, dtype=np.float32) for r in rows]
    first = np.concatenate([[0], np.cumsum([t.shape[0] for t in table])])
    file_rows = {s: (int(first[k]), int(table[k].shape[0])) for k, s in enumerate(stems)}
    tokens = collect_tokens(items, file_rows, offsets)
    plan_ = plan(tokens, tasks, budget)
    job_wins = run(plan_, np.concatenate(table, axis=0), metric, E, device) if plan_.blocks else []
    wins = cell_wins(plan_, job_wins)
    if details is not None:
        details.update(tokens=tokens, plan=plan_, wins2=wins)
    report = {'in_dir': in_dir, 'item': item_path, 'metric': metric, 'E': int(E), 'tasks': aggregate(plan_, wins),
              'tokens': {'kept': len(tokens), 'dropped': tokens.dropped}, 'files': stems}
    report.update({k: v for k, v in bitrate(lines).items()})
    out_path = out_path or os.path.join(in_dir, 'score.json')
    with open(out_path, 'w') as f:
        json.dump(report, f, indent=1)
    print('[Score] - %s: %s, %d tokens kept, %d dropped, %.3f bits per unit, %.1f bits per second, %s -> %s' % (
        in_dir, ', '.join('%s error %s over %d pairs, %d cells, %d triplets' % (
            t, ('%.3f %%' % r['error'] if r['error'] is not None else 'none'), r['ordered_pairs'], r['cells'], r['triplets'])
            for t, r in report['tasks'].items()),
        len(tokens), sum(tokens.dropped.values()), report['bits_per_unit'], report['bits_per_second'], metric, out_path))
    return report
