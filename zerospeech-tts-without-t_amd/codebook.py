"""Unit codebook: K codewords of E bits fitted by k-modes over bit-packed units (convert.pack_units' rows), and the snap of every
unit to its nearest codeword in Hamming distance.  One trained model then serves any point of the bitrate / quality
trade-off: unit files become sequences over at most K symbols, and a snapped unit is still a line of 0 / 1.

The work is three HIP entry points (csrc/zs_codebook.hip): zs_code_assign (nearest codeword, the hot call), zs_code_accum and
zs_code_update (the votes and the majority rule of one k-modes iteration).  Everything is integer: a fit is bitwise reproducible and
equals tests/codebook_ref.py, the numpy definition, codeword for codeword.  Not in the reference, which changes the size of the
symbol inventory only by retraining with another enc_size."""
import json

import numpy as np
import torch

from . import _lib as L

FORMAT_VERSION = 1
MAX_K = L.ENUMS['ZS_CODE_MAX_K']
MAX_E = L.ENUMS['ZS_CODE_MAX_E']


def row_bytes(E):
    return (int(E) + 7) // 8


def assign_tile(E):
    """Codewords zs_code_assign stages in LDS per pass at width E (a K above it crosses a tile boundary)."""
    words, w = (int(E) + 31) // 32, 1
    while w < words:
        w *= 2
    return L.ENUMS['ZS_CODE_TILE_WORDS'] // w


def refuse_continues(enc_mode):
    if enc_mode == 'continues':
        raise ValueError("enc_mode 'continues' has no units to pack (its encodings are not 0 / 1): there is nothing a codebook could snap")


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _check_rows(t, E, what):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] < row_bytes(E) or not t.is_contiguous():
        raise ValueError('%s must be a contiguous uint8 device tensor [n, >= %d] for E = %d' % (what, row_bytes(E), E))


def _check_scores(out, n, K):
    if not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != n or out.shape[1] < K \
            or (out.shape[1] > 1 and out.stride(1) != 1) or (n > 1 and out.stride(0) < out.shape[1]):
        raise ValueError('scores must be an fp32 device tensor [%d, >= %d] with unit column stride' % (n, K))


def _scores_ld(out, K):
    return int(out.stride(0)) if out.shape[0] > 1 else max(int(out.shape[1]), int(K))


def assign(units, code, E, idx=None, dist=None, snapped=None, total=None):
    """zs_code_assign on the current stream.  units uint8 [n, row_bytes], code uint8 [K, code_bytes] (device); every output optional:
    idx / dist int32 [n], snapped uint8 like units (may be units itself), total int64 [1] (added to)."""
    _check_rows(units, E, 'units')
    _check_rows(code, E, 'code')
    if snapped is not None and (snapped.shape != units.shape or snapped.dtype != torch.uint8 or not snapped.is_contiguous()):
        raise ValueError('snapped must have the shape and pitch of units')
    L.call('zs_code_assign', 'ZsCodeAssign', _stream(units.device), units=L.ptr(units), n=units.shape[0], row_bytes=units.shape[1],
           code=L.ptr(code), K=code.shape[0], code_bytes=code.shape[1], E=int(E), idx=L.ptr(idx), dist=L.ptr(dist), snapped=L.ptr(snapped),
           total=L.ptr(total))


def usage(idx, K=None):
    """(symbols used, entropy of the index histogram in bits per unit), on the host in double from a bincount."""
    i = np.asarray(idx.cpu() if torch.is_tensor(idx) else idx).reshape(-1).astype(np.int64)
    if i.size == 0:
        return 0, 0.0
    if (i < 0).any() or (K is not None and (i >= K).any()):
        raise ValueError('usage: an index outside [0, K)')
    return usage_counts(np.bincount(i, minlength=(K or 0)))


def usage_counts(counts):
    """usage() from the histogram itself (counts[k] = units of codeword k)."""
    c = np.asarray(counts, dtype=np.float64).reshape(-1)
    if (c < 0).any():
        raise ValueError('usage_counts: a negative count')
    if c.sum() == 0:
        return 0, 0.0
    p = c[c > 0] / c.sum()
    return int(len(p)), float(max(0.0, -(p * np.log2(p)).sum()))


def read_npz(path):
    """The fields of a codebook file of either kind; ValueError for anything numpy cannot read as one."""
    try:
        z = np.load(path, allow_pickle=False)
        return {k: z[k] for k in z.files}
    except Exception as e:
        raise ValueError('%s is not a codebook file: %s' % (path, e))


def reseed_rows(cnt, dist):
    """(the empty k in increasing order, the rows they take): the rows of largest dist, ties to the lowest row, each row once."""
    empties = np.flatnonzero(np.asarray(cnt) == 0)
    order = np.argsort(-np.asarray(dist, dtype=np.float64), kind='stable')[:len(empties)]
    return empties, order


def first_distinct(n, K, seed, rows_at, nouns):
    """The walk of both init_rows: numpy.random.RandomState(seed).permutation(n) in growing slices, the first K indices whose rows
    are pairwise different.  rows_at(sel) -> the host rows of the indices sel, compared by their bytes; nouns: what the error calls
    the input and a row of it."""
    K = int(K)
    perm = np.random.RandomState(seed).permutation(n)
    seen, out, at, step = set(), [], 0, max(4096, 4 * K)
    while at < n:
        sel = perm[at:at + step]
        for i, r in zip(sel, rows_at(sel)):
            key = r.tobytes()
            if key not in seen:
                seen.add(key)
                out.append(int(i))
                if len(out) == K:
                    return np.asarray(out, dtype=np.int64)
        at += step
        step *= 4
    raise ValueError('init_rows: the %s hold %d distinct %s, fewer than K = %d' % (nouns[0], len(seen), nouns[1], K))


class CodebookFile(object):
    """What the kinds of codebook (bits, vectors, zs_amd.rvq's stages of vectors) share: the file (fields format_version, K, E, meta and the kind's payload; `kind` where the
    kind has one), the width check, the per-device upload and the fit over a folder.  A kind supplies `label` (what messages call
    it), `payload` (the field and attribute of its codewords), `_from_payload` (the check of that payload: its constructor) and
    what fit_dir names below."""
    kind = None

    def save(self, path):
        fields = {'kind': np.array(self.kind)} if self.kind else {}              # in the order the file lists them
        fields.update(format_version=np.int64(FORMAT_VERSION), K=np.int64(self.K), E=np.int64(self.E))
        fields[self.payload] = getattr(self, self.payload)
        fields['meta'] = np.array(json.dumps(self.meta))
        with open(path, 'wb') as f:
            np.savez(f, **fields)

    @classmethod
    def load(cls, path, E=None):
        """ValueError naming the field for a malformed file, and for a width other than E (the Decoder's c_in) when E is given."""
        return cls.from_fields(read_npz(path), path, E)

    @classmethod
    def from_fields(cls, d, path, E=None):
        """load() of fields already read (read_npz)."""
        where = '%s: %s field' % (path, cls.label)
        for k in (('kind',) if cls.kind else ()) + ('format_version', 'K', 'E', cls.payload, 'meta'):
            if k not in d:
                raise ValueError('%s %r is missing' % (where, k))
        if cls.kind and (d['kind'].shape != () or d['kind'].dtype.kind != 'U' or str(d['kind']) != cls.kind):
            raise ValueError("%s kind must be '%s'" % (where, cls.kind))
        for k in ('format_version', 'K', 'E'):
            if d[k].shape != () or d[k].dtype.kind not in 'iu':
                raise ValueError('%s %r must be one integer' % (where, k))
        if int(d['format_version']) != FORMAT_VERSION:
            raise ValueError('%s format_version is %d, this build reads %d' % (where, int(d['format_version']), FORMAT_VERSION))
        try:
            meta = json.loads(str(d['meta']))
            if not isinstance(meta, dict):
                raise ValueError('not an object')
        except ValueError as e:
            raise ValueError('%s meta is not a json object (%s)' % (where, e))
        try:
            cb = cls._from_payload(d[cls.payload], int(d['E']), meta)
        except ValueError as e:
            raise ValueError('%s %s: %s' % (where, cls._payload_error, e))
        if cb.K != int(d['K']):
            raise ValueError('%s K is %d but %s has %d rows' % (where, int(d['K']), cls.payload, cb.K))
        if cb.E != int(d['E']):
            raise ValueError('%s E is %d but %s has %d columns' % (where, int(d['E']), cls.payload, cb.E))
        if E is not None:
            cb.check_width(E, path)
        return cb

    def check_width(self, E, where='codebook'):
        if int(E) != self.E:
            raise ValueError("%s: codebook field E is %d, the Decoder's input width (c_in) is %d" % (where, self.E, int(E)))

    def to(self, dev):
        """The codewords on the device (what the kind's _upload gives), uploaded once."""
        dev = torch.device(dev)
        t = self._dev.get(dev)
        if t is None:
            t = self._dev[dev] = self._upload(dev)
        return t

    @classmethod
    def default_path(cls, ckpt_dir, K):
        import os
        return os.path.join(ckpt_dir, 'codebooks', 'K%d.%s' % (int(K), cls.suffix))

    @classmethod
    def fit_dir(cls, trainer, seg_len, in_dir, K, out_path, iters, seed=0, batch=64, **fit_kw):
        """--fit_codebook: a codebook of this kind of K codewords over a folder.  The kind's _dir_rows reads and encodes the folder
        (-> files used, files skipped, device tensors of rows), its _fit clusters them (fit_kw: what else that kind's fit takes) and
        its _indices gives the final assignment; a kind with more to say answers _usage, _report_extra and _fit_summary itself.
        Writes the codebook to out_path and fit_codebook.json beside it (files used and skipped, n_units, the history, symbols used
        and the entropy of the final assignment); returns (the codebook, that report)."""
        import os
        cls.check_mode(trainer.enc_mode)
        K = int(K)
        if not 1 <= K <= MAX_K:
            raise ValueError('--fit_codebook: K must be in [1, %d] (got %d)' % (MAX_K, K))
        E = int(trainer.Decoder.c_in)
        used, skipped, parts = cls._dir_rows(trainer, seg_len, in_dir, batch, E)
        if not parts:
            raise ValueError('--fit_codebook: %s holds no usable %s' % (in_dir, cls._dir_files))
        rows_dev = torch.cat(parts, dim=0).contiguous()
        cb = cls._fit(rows_dev, K, iters, seed, E, trainer.enc_mode, **fit_kw)
        cb.check_width(E, out_path)
        n_used, entropy = cb._usage(rows_dev)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        cb.save(out_path)
        report = {'codebook': out_path}
        if cls.kind:
            report['kind'] = cls.kind
        report.update({'K': K, 'E': E, 'in_dir': in_dir, 'files': used, 'skipped': skipped, 'n_units': int(rows_dev.shape[0]),
                       'seed': int(seed), 'history': cb.meta['history'], 'symbols_used': n_used, 'entropy_bits_per_unit': entropy})
        report.update(cb._report_extra())
        with open(os.path.join(os.path.dirname(os.path.abspath(out_path)), 'fit_codebook.json'), 'w') as f:
            json.dump(report, f, indent=1)
        print(cb._fit_summary(K, rows_dev.shape[0], len(used), n_used, entropy, out_path))
        return cb, report

    def _usage(self, rows_dev):
        """(symbols used, entropy in bits per unit) of the final assignment of the fit rows."""
        return usage(self._indices(rows_dev), self.K)

    def _report_extra(self):
        """What fit_codebook.json holds for this kind beyond the shared fields."""
        return {}

    def _fit_summary(self, K, n_rows, n_files, n_used, entropy, out_path):
        """The line fit_dir prints."""
        return self._fit_line % (K, n_rows, n_files, len(self.meta['history']), self.meta['history'][-1][0], n_used, entropy, out_path)


class Codebook(CodebookFile):
    """K codewords of E bits: `packed` uint8 [K, (E + 7) // 8] on the host (bits at columns >= E zero), and `meta`: enc_mode, n_units,
    seed and the per-iteration history [(total distance, changed, empties)] of the fit."""
    label, payload, suffix, _payload_error = 'codebook', 'packed', 'codebook.npz', 'packed / E'
    _dir_files = '*.wav or *.txt unit file'
    _fit_line = '[Codebook] - K = %d over %d units of %d files: %d iterations, total distance %d, %d symbols used, %.3f bits per unit -> %s'

    def __init__(self, packed, E, meta=None):
        E = int(E)
        if not 1 <= E <= MAX_E:
            raise ValueError('codebook: E must be in [1, %d] (got %d)' % (MAX_E, E))
        p = np.asarray(packed)
        if p.dtype != np.uint8 or p.ndim != 2 or p.shape[1] != row_bytes(E):
            raise ValueError('codebook: packed must be uint8 [K, %d] for E = %d (got %s %s)' % (row_bytes(E), E, p.dtype, p.shape))
        if not 1 <= p.shape[0] <= MAX_K:
            raise ValueError('codebook: K must be in [1, %d] (got %d)' % (MAX_K, p.shape[0]))
        if E % 8 and (p[:, -1] >> (E % 8)).any():
            raise ValueError('codebook: packed has a bit set above column %d' % E)
        self.K, self.E, self.packed, self.meta = int(p.shape[0]), E, np.ascontiguousarray(p), dict(meta or {})
        self._dev = {}

    @classmethod
    def _from_payload(cls, packed, E, meta):
        return cls(packed, E, meta)

    check_mode = staticmethod(refuse_continues)               # a bit codebook serves every enc_mode but 'continues'

    def _upload(self, dev):
        return torch.from_numpy(self.packed).to(dev)

    @classmethod
    def _dir_rows(cls, trainer, seg_len, in_dir, batch, E):
        """The *.wav of in_dir through encode_batch(packed=True) with the packed units left on the device, and the *.txt unit files
        of in_dir (read_units) behind them."""
        import glob
        import os
        from . import convert as cv
        used, skipped, parts, skip = encode_dir(trainer, seg_len, in_dir, batch,
                                                lambda specs: cv.encode_batch(specs, trainer, seg_len, packed=True, units_on_device=True)[0])
        for path in sorted(glob.glob(os.path.join(in_dir, '*.txt'))):
            if path.endswith('.idx.txt'):
                continue
            try:
                u = cv.pack_units(cv.read_units(path, E))
            except (OSError, ValueError) as e:
                skip(path, 'cannot be read: %s' % e)
                continue
            parts.append(torch.from_numpy(u).to(trainer.device))
            used.append({'input': path, 'units': int(u.shape[0])})
        return used, skipped, parts

    @classmethod
    def _fit(cls, units_dev, K, iters, seed, E, enc_mode):
        return fit(units_dev, K, iters=iters, seed=seed, E=E, enc_mode=enc_mode)

    def _indices(self, units_dev):
        return self.snap(units_dev)[0]

    def units(self):
        """What batched conversion and the folder drivers do with units under this codebook (convert._BitUnits)."""
        from .convert import _BitUnits
        return _BitUnits(self)

    def snap_(self, units_dev, idx=None, dist=None, total=None):
        """Every row of units_dev replaced by its codeword, in place (one zs_code_assign on the current stream, no synchronisation)."""
        assign(units_dev, self.to(units_dev.device), self.E, idx=idx, dist=dist, snapped=units_dev, total=total)

    def snap(self, units_dev):
        """(idx int32 [n], snapped uint8 like units_dev), both on the device."""
        _check_rows(units_dev, self.E, 'units')
        idx = torch.empty(units_dev.shape[0], dtype=torch.int32, device=units_dev.device)
        snapped = units_dev.clone()                                # the bytes of a pitch behind the columns come along
        assign(units_dev, self.to(units_dev.device), self.E, idx=idx, snapped=snapped)
        return idx, snapped

    def scores_(self, rows, out):
        """out[i][k] = the Hamming distance of packed unit i and codeword k over the columns < E, exact in fp32 (one zs_code_scores on
        the current stream, no synchronisation).  rows uint8 [n, row_bytes] and out fp32 [n, >= K] on the device; the columns of out
        at or beyond K are not written.  What --segment chooses its paths from (zs_amd.segment)."""
        from .segment import check_codebook
        check_codebook(self)
        _check_rows(rows, self.E, 'rows')
        code = self.to(rows.device)
        _check_scores(out, rows.shape[0], self.K)
        L.call('zs_code_scores', 'ZsCodeScores', _stream(rows.device), units=L.ptr(rows), n=rows.shape[0], row_bytes=rows.shape[1],
               code=L.ptr(code), K=self.K, code_bytes=code.shape[1], E=self.E, scores=L.ptr(out), ld_s=_scores_ld(out, self.K))

    def rows_at(self, idx):
        """The packed rows uint8 [n, (E + 7) // 8] of the codewords idx (integers [n] in [0, K)) on the host: what an index file
        stands for (zs_amd.abx)."""
        return self.packed[np.asarray(idx, dtype=np.int64).reshape(-1)]

    def snap_host(self, packed):
        """Host rows uint8 [n, (E + 7) // 8] -> (idx int32 [n], snapped) as numpy arrays (one round trip through the device)."""
        idx, s = self.snap(torch.from_numpy(np.ascontiguousarray(packed)).cuda())
        return idx.cpu().numpy(), s.cpu().numpy()


def _mask_rows(rows, E):
    """The columns < E of packed rows: [n, (E + 7) // 8], the bits above E zero (a numpy array or a tensor)."""
    rows = rows[:, :row_bytes(E)]
    rows = rows.clone() if torch.is_tensor(rows) else np.array(rows, dtype=np.uint8)
    if E % 8:
        rows[:, -1] &= (1 << (E % 8)) - 1
    return rows


def init_rows(packed, K, seed, E=None):
    """The indices of the K starting codewords: numpy.random.RandomState(seed).permutation(n) walked in order, the first K indices
    whose rows are pairwise different (over the columns < E; E defaults to every bit of a row).  ValueError saying how many distinct
    rows there are when they are fewer than K.  packed: host array or device tensor [n, row_bytes]; of a device tensor only the
    rows looked at come to the host."""
    E = 8 * int(packed.shape[1]) if E is None else int(E)

    def rows_at(sel):
        if torch.is_tensor(packed):
            return _mask_rows(packed[torch.from_numpy(sel).to(packed.device)], E).cpu().numpy()
        return _mask_rows(np.asarray(packed)[sel], E)
    return first_distinct(int(packed.shape[0]), K, seed, rows_at, ('units', 'rows'))


def fit(units_dev, K, iters=20, seed=0, E=None, enc_mode='multilabel_binary', on_iter=None):
    """k-modes over units_dev (uint8 [n, row_bytes] on the device, left unchanged) -> Codebook.  Per iteration zs_code_assign,
    zs_code_accum, zs_code_update and ONE small D2H copy of (total, changed, bad, cnt) -- a synchronisation; fitting is not a captured
    path.  Empty clusters, in increasing k, take the units of largest distance (ties to the lowest unit index, each unit once),
    decided on the host from one D2H of dist in the iterations that have empties.  `changed` counts the codewords that differ from
    the iteration's start, reseeds included; the fit stops at changed == 0 or after `iters`.  The total distance never rises from
    one iteration to the next (assignment minimises per unit, the vote per bit, a tie keeps the bit, a reseed zeroes one unit's
    distance): RuntimeError if it does.  on_iter(i, packed codebook on the host) is called after every iteration."""
    refuse_continues(enc_mode)
    K, iters = int(K), int(iters)
    if not 1 <= K <= MAX_K:
        raise ValueError('fit: K must be in [1, %d] (got %d)' % (MAX_K, K))
    if iters < 1:
        raise ValueError('fit: iters must be >= 1 (got %d)' % iters)
    E = 8 * int(units_dev.shape[1]) if E is None else int(E)
    if not 1 <= E <= MAX_E:
        raise ValueError('fit: E must be in [1, %d] (got %d)' % (MAX_E, E))
    _check_rows(units_dev, E, 'units')
    n, dev, nb = int(units_dev.shape[0]), units_dev.device, row_bytes(E)
    if n >= 2 ** 31:
        raise ValueError('fit: %d units, the counters are int32' % n)
    first = init_rows(units_dev, K, seed, E)
    code = _mask_rows(units_dev[torch.from_numpy(first).to(dev)], E).contiguous()
    st = _stream(dev)
    stats = torch.empty(4 + K, dtype=torch.int32, device=dev)     # total (int64) | changed | bad | cnt [K]: one copy per iteration
    ones = torch.empty(K, E, dtype=torch.int32, device=dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    dist = torch.empty(n, dtype=torch.int32, device=dev)
    history = []
    for it in range(iters):
        stats.zero_()
        ones.zero_()
        start = code.clone()
        assign(units_dev, code, E, idx=idx, dist=dist, total=stats[0:2])
        L.call('zs_code_accum', 'ZsCodeAccum', st, units=L.ptr(units_dev), idx=L.ptr(idx), n=n, row_bytes=units_dev.shape[1], K=K, E=E,
               cnt=L.ptr(stats, 4), ones=L.ptr(ones), bad=L.ptr(stats, 3))
        L.call('zs_code_update', 'ZsCodeUpdate', st, code=L.ptr(code), K=K, code_bytes=nb, E=E, cnt=L.ptr(stats, 4), ones=L.ptr(ones),
               changed=L.ptr(stats, 2))
        h = stats.cpu().numpy()                                   # the synchronisation of this iteration
        total, changed, bad, cnt = int(h[0:2].view(np.int64)[0]), int(h[2]), int(h[3]), h[4:]
        if bad:
            raise RuntimeError('fit: zs_code_assign gave %d indices outside [0, %d)' % (bad, K))
        empties, order = reseed_rows(cnt, dist.cpu().numpy()) if (cnt == 0).any() else ((), ())
        if len(empties):
            code[torch.from_numpy(empties).to(dev)] = _mask_rows(units_dev[torch.from_numpy(order).to(dev)], E)
            changed = int((code != start).any(dim=1).sum().item())
        if history and total > history[-1][0]:
            raise RuntimeError('fit: the total distance rose from %d to %d in iteration %d' % (history[-1][0], total, it))
        history.append((total, changed, int(len(empties))))
        if on_iter is not None:
            on_iter(it, code.cpu().numpy())
        if changed == 0:
            break
    return Codebook(code.cpu().numpy(), E, {'enc_mode': enc_mode, 'n_units': n, 'seed': int(seed), 'history': [list(x) for x in history]})


def default_path(ckpt_dir, K):
    """{ckpt_dir}/codebooks/K<K>.codebook.npz"""
    return Codebook.default_path(ckpt_dir, K)


def encode_dir(trainer, seg_len, in_dir, batch, encode):
    """The *.wav of in_dir read and encoded as convert_dir reads them (any rate, the same trimming, the same skip list), in the groups
    of convert_dir_plan; encode(specs) -> one device tensor of rows per utterance.  What the _dir_rows of both kinds of
    codebook read a folder with.  Returns (used [{'input', 'units'}], skipped [{'input', 'reason'}], the device tensors, skip(path, reason))."""
    from . import convert as cv
    from .preprocess import read_wav
    dev = trainer.device
    used, parts = [], []
    skipped, skip = cv._skip_log('Codebook')
    files, durations = cv._scan_wavs(in_dir, skip)
    plan = cv.convert_dir_plan(files, durations, ['-'], in_dir, batch=batch) if files else {'groups': [], 'skipped': []}
    for s in plan['skipped']:
        skip(s['file'], s['reason'])
    for group in plan['groups']:
        wavs, rates, paths = [], [], []
        for it in group:
            try:
                w, r = read_wav(it['file'])
            except Exception as e:
                skip(it['file'], 'cannot be read: %s' % e)
                continue
            wavs.append(w)
            rates.append(r)
            paths.append(it['file'])
        if not wavs:
            continue
        specs, _ = cv._wav_features(wavs, rates, dev, strict=False)
        for p, s in zip(paths, specs):
            if s is None:
                skip(p, 'utterance too short after trimming')
        live = [(p, s) for p, s in zip(paths, specs) if s is not None]
        if live:
            units = encode([s for _, s in live])
            parts += units
            used += [{'input': p, 'units': int(u.shape[0])} for (p, _), u in zip(live, units)]
    return used, skipped, parts, skip


def fit_dir(trainer, seg_len, in_dir, K, out_path, iters=20, seed=0, batch=64):
    """--fit_codebook: a codebook of K codewords over the units of a folder (CodebookFile.fit_dir).  The *.wav of in_dir are read and
    encoded as convert_dir reads them (any rate, the same trimming, the same skip list), in the groups of convert_dir_plan; the *.txt
    unit files of in_dir are added.  Returns (Codebook, the report written to fit_codebook.json)."""
    return Codebook.fit_dir(trainer, seg_len, in_dir, K, out_path, iters, seed, batch)
