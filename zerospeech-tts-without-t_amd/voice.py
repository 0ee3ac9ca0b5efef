"""Enrol a new target voice from a few utterances (main.py --adapt_voice; not in the reference).

The Decoder sees the speaker only through one row of each of its five embedding tables (emb1..emb5, c_h floats each; reference
model/model.py:310-357), so a voice that was not in the training run is 5 * c_h numbers fitted to its utterances with every other
weight frozen:

* the utterances are encoded ONCE by the frozen Encoder in eval mode (convert.encode_batch(packed=True): the fragment rule of
  conversion, so these are the units the Decoder sees when the voice is used) and lie, with their spectrograms, in device memory
  (VoiceSet);
* one iteration (VoiceStep) is zs_voice_gather (a batch of random seg_len-frame segments behind a device cursor) -> Decoder forward
  -> zs_l1_loss -> Decoder backward without parameter gradients (DecoderEngine.backward(param_grads=False): the data-gradient chain,
  which leaves the per-sample embedding sums) -> zs_voice_adam (their sum over the batch, clip_grad_norm_ and Adam over the five
  rows, one launch) -> zs_step_counters; eagerly or as one replayed hipGraph (ZS_GRAPH, as trainer.AEStep).  Nothing crosses PCIe
  per iteration and the loss is read back only where it is logged;
* the result is a voice file (save_voice / load_voice): the five rows and a sha256 of the decoder weights they were fitted to;
* add_voices(trainer, {name: path}) appends voices to the Decoder's tables for --convert_dir / --synth_dir (autoencoder only: the
  stage-2 Generator has rows for its trained target speakers alone).

Nothing here writes a checkpoint, and nothing falls back to the host: without the library or a GPU the device classes raise."""
import ctypes
import glob
import hashlib
import json
import os

import numpy as np
import torch

from . import _lib as L

VOICE_VERSION = 1
N_ROWS = 5
EMB_KEYS = ['emb%d.weight' % i for i in range(1, N_ROWS + 1)]
N_ITEMS = 4096                 # entries of a VoiceSet's item table (a batch sequence of N_ITEMS / B batches before it repeats)
ADAPT_ITERS = 500
NOISE_SEED = 20240229          # the Gumbel noise of the one encoding pass and the item table of an --adapt_voice run


# ---- the voice file --------------------------------------------------------------------------------------------------------------
def decoder_digest(state_dict):
    """sha256 (hex) over the Decoder's non-embedding tensors in key order: name, shape and fp32 bytes of each.  A voice is only
    meaningful with the weights it was fitted to."""
    h = hashlib.sha256()
    for k in sorted(state_dict):
        if k in EMB_KEYS:
            continue
        t = state_dict[k].detach().to('cpu', torch.float32).contiguous()
        h.update(('%s %s\n' % (k, tuple(t.shape))).encode())
        h.update(t.numpy().tobytes())
    return h.hexdigest()


def save_voice(path, rows, meta):
    """Write {emb1..emb5: fp32 [c_h], meta: JSON string} as an .npz at `path` (given with its .npz suffix).  meta must carry
    version, c_h and digest (load_voice checks them); adapt() adds seg_len, iterations, final loss, init, utterance and frame counts."""
    rows = [np.ascontiguousarray(np.asarray(r, dtype=np.float32).reshape(-1)) for r in rows]
    if len(rows) != N_ROWS or len({r.shape for r in rows}) != 1:
        raise ValueError('save_voice: need %d rows of one length' % N_ROWS)
    meta = dict(meta, version=VOICE_VERSION, c_h=int(rows[0].shape[0]))
    if 'digest' not in meta:
        raise ValueError('save_voice: meta has no digest')
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'wb') as f:
        np.savez(f, meta=np.array(json.dumps(meta, sort_keys=True)), **{'emb%d' % (i + 1): r for i, r in enumerate(rows)})
    return meta


def load_voice(path, c_h=None, digest=None):
    """(rows: five fp32 [c_h] arrays, meta dict) of a voice file.  ValueError naming the field for a file of another version,
    a c_h other than `c_h`, or a digest other than `digest` (each checked when given)."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in ['meta'] + ['emb%d' % i for i in range(1, N_ROWS + 1)] if k not in z.files]
        if missing:
            raise ValueError('voice file %s: no entry %r' % (path, missing[0]))
        meta = json.loads(str(z['meta']))
        rows = [np.asarray(z['emb%d' % i], dtype=np.float32) for i in range(1, N_ROWS + 1)]
    if meta.get('version') != VOICE_VERSION:
        raise ValueError('voice file %s: version is %r, this build reads %d' % (path, meta.get('version'), VOICE_VERSION))
    if any(r.shape != (int(meta['c_h']),) for r in rows):
        raise ValueError('voice file %s: c_h is %r but the rows have shapes %s' % (path, meta['c_h'], [r.shape for r in rows]))
    if c_h is not None and int(meta['c_h']) != int(c_h):
        raise ValueError('voice file %s: c_h is %d, the decoder has %d' % (path, int(meta['c_h']), int(c_h)))
    if digest is not None and meta.get('digest') != digest:
        raise ValueError('voice file %s: digest %s... does not match the decoder weights of this checkpoint (%s...): the voice '
                         'was fitted to other weights' % (path, str(meta.get('digest'))[:12], digest[:12]))
    return rows, meta


# ---- names -----------------------------------------------------------------------------------------------------------------------
def parse_voices(specs):
    """['NAME=path', ...] (the --voice flag) -> {name: path}, in order.  ValueError for a malformed entry or a name given twice."""
    out = {}
    for s in specs or []:
        name, eq, path = s.partition('=')
        name, path = name.strip(), path.strip()
        if not eq or not name or not path:
            raise ValueError('--voice takes NAME=FILE (got %r)' % s)
        if name in out:
            raise ValueError('--voice names %r twice' % name)
        out[name] = path
    return out


def resolve_speaker(name, speaker2id, voices=None):
    """The Decoder row of a --t_speaker name: speaker2id first, then the registered voices ({name: id}).  ValueError if neither."""
    if name in speaker2id:
        return int(speaker2id[name])
    if voices and name in voices:
        return int(voices[name])
    raise ValueError('target speaker %r is neither in speaker2id nor a registered voice' % name)


# ---- the Decoder's tables --------------------------------------------------------------------------------------------------------
def init_rows(state_dict, speaker=None):
    """The five initial rows (fp32 tensors [c_h], copies): row `speaker` of each table, or, for None, the mean of each table's rows."""
    rows = []
    for k in EMB_KEYS:
        t = state_dict[k].detach().to('cpu', torch.float32)
        if speaker is not None and not 0 <= int(speaker) < t.shape[0]:
            raise ValueError('init speaker %d is outside the %d rows of %s' % (int(speaker), t.shape[0], k))
        rows.append((t[int(speaker)] if speaker is not None else t.mean(dim=0)).clone())
    return rows


def extend_state_dict(state_dict, voices_rows):
    """A copy of a Decoder state dict whose five tables have one more row per voice, appended in order (voices_rows: a list of
    five-row lists): every original row keeps its index and its bits, voice j becomes row n_speakers + j."""
    out = dict(state_dict)
    for i, k in enumerate(EMB_KEYS):
        t = state_dict[k]
        add = [torch.as_tensor(np.asarray(v[i], dtype=np.float32)).reshape(1, -1).to(t.device, t.dtype) for v in voices_rows]
        if any(a.shape[1] != t.shape[1] for a in add):
            raise ValueError('a voice row of %d values for a table of c_h = %d (%s)' % (add[0].shape[1], t.shape[1], k))
        out[k] = torch.cat([t] + add, dim=0)
    return out


def replace_tables(state_dict, rows):
    """A copy of a Decoder state dict whose five tables are the single rows `rows` (a Decoder of c_a = 1: VoiceStep's)."""
    out = dict(state_dict)
    for i, k in enumerate(EMB_KEYS):
        t = state_dict[k]
        out[k] = torch.as_tensor(np.asarray(rows[i], dtype=np.float32)).reshape(1, -1).to(t.device, t.dtype).clone()
        if out[k].shape[1] != t.shape[1]:
            raise ValueError('a voice row of %d values for a table of c_h = %d (%s)' % (out[k].shape[1], t.shape[1], k))
    return out


def _clone_decoder(dec, state_dict, c_a):
    from .model import Decoder
    dev = dec.flat_params()[0].device
    new = Decoder(c_in=dec.c_in, c_out=dec.c_out, c_h=dec.c_h, c_a=c_a, ns=dec.ns, seg_len=dec.seg_len, output_mask=dec.output_mask,
                  dtype=dec._zs_dtype).to(dev)
    new.load_state_dict(state_dict)
    return new


def add_voices(trainer, voices):
    """Register voices for conversion through the autoencoder: `voices` {name: voice file}; every file is checked against the
    trainer's Decoder (c_h, digest: ValueError naming the field) before anything changes, then trainer.Decoder is rebuilt with
    c_a = n_speakers + k rows from the same state dict, the voice rows appended.  A table speaker's rows, and so its output, do not
    change.  Returns {name: row} (also kept as trainer.voices).  For inference trainers: the optimizer state of trainer.ae still
    belongs to the Decoder that was replaced."""
    dec = trainer.Decoder
    sd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    digest = decoder_digest(sd)
    taken = dict(getattr(trainer, 'voices', None) or {})
    rows, ids = [], {}
    for name, path in voices.items():
        if name in taken or name in ids:
            raise ValueError('voice %r is registered already' % name)
        r, _ = load_voice(path, c_h=dec.c_h, digest=digest)
        ids[name] = dec.c_a + len(rows)
        rows.append(r)
    if rows:
        new = _clone_decoder(dec, extend_state_dict(sd, rows), dec.c_a + len(rows))
        new.train(dec.training)
        trainer.Decoder = new
    taken.update(ids)
    trainer.voices = taken
    return ids


# ---- the planner -----------------------------------------------------------------------------------------------------------------
def plan_items(frames, units, seg_len, n_items=N_ITEMS, seed=0):
    """The seeded item table of a VoiceSet, on the host: n_items random segments (utterance, t) with t a multiple of 8, frames
    [t, t + seg_len) inside the utterance's frames and units [t / 8, (t + seg_len) / 8) inside its units (the fragment rule drops an
    utterance's last frame, so it may have fewer units than frames / 8), drawn uniformly over all such segments.  An utterance
    with fewer than seg_len frames, or fewer than seg_len / 8 units, is left out.  Returns (utt int64 [n_items], t int64 [n_items],
    kept utterance indices, left-out utterance indices); ValueError when none remain."""
    seg_len, n_items = int(seg_len), int(n_items)
    if seg_len <= 0 or seg_len % 8:
        raise ValueError('seg_len must be a positive multiple of 8 (got %d)' % seg_len)
    if n_items <= 0:
        raise ValueError('n_items must be > 0 (got %d)' % n_items)
    if len(frames) != len(units):
        raise ValueError('%d frame counts for %d unit counts' % (len(frames), len(units)))
    Lu = seg_len // 8
    kept, left, counts = [], [], []
    for i, (n, u) in enumerate(zip(frames, units)):
        last = min(int(n) - seg_len, 8 * (int(u) - Lu))            # the last admissible start, before alignment
        if last < 0:
            left.append(i)
        else:
            kept.append(i)
            counts.append(last // 8 + 1)
    if not kept:
        raise ValueError('no utterance of at least seg_len = %d frames: nothing to adapt to (%d utterances left out)' % (seg_len, len(left)))
    counts = np.asarray(counts, dtype=np.int64)
    ends = np.cumsum(counts)
    pick = np.random.RandomState(int(seed) % (1 << 32)).randint(0, int(ends[-1]), size=n_items).astype(np.int64)
    j = np.searchsorted(ends, pick, side='right')
    t = 8 * (pick - (ends[j] - counts[j]))
    return np.asarray(kept, dtype=np.int64)[j], t.astype(np.int64), kept, left


def check_items(first, ufirst, seg_len, frames_total, n_units):
    """Every range zs_voice_gather trusts, over the whole table, before it is uploaded: ValueError otherwise."""
    first, ufirst = np.asarray(first, dtype=np.int64), np.asarray(ufirst, dtype=np.int64)
    if first.shape != ufirst.shape or first.ndim != 1 or not len(first):
        raise ValueError('the item table needs first and ufirst of one length >= 1')
    if (first % 8).any():
        raise ValueError('an item starts at a frame that is no multiple of 8')
    if first.min() < 0 or (first + seg_len).max() > frames_total:
        raise ValueError('an item leaves the pool of %d frames' % frames_total)
    if ufirst.min() < 0 or (ufirst + seg_len // 8).max() > n_units:
        raise ValueError('an item leaves the %d packed units' % n_units)


def gumbel_noise_fn(encoder, seed=NOISE_SEED):
    """encode_batch's noise_fn from a fixed seed: Gumbel noise of the encoder mode's shape, drawn on the host from one generator,
    so that the same utterances in the same order are encoded to the same units (None for 'continues', which draws none)."""
    gen = torch.Generator().manual_seed(int(seed))
    dev = encoder.flat_params()[0].device

    def noise_fn(n, t, e):
        shape = encoder.noise_shape(n, t)
        if shape is None:
            return None
        U = torch.rand(shape, generator=gen)
        return (-torch.log(-torch.log(U + 1e-20) + 1e-20)).to(dev)
    return noise_fn


class VoiceSet(object):
    """The adaptation data in device memory: the utterances' spectrograms back to back as one fp32 pool [frames_total, F] (each
    utterance starts at a multiple of 8 frames), their bit-packed units [n_units, row_bytes], and the seeded item table
    (plan_items) as device tables first / ufirst, validated on the host (check_items) before the upload.
    specs: fp32 [T_i, F] arrays or tensors (host or device); units: uint8 [U_i, row_bytes] packed rows (convert.pack_units'
    layout, what encode_batch(packed=True) returns).  left_out: the utterances shorter than seg_len (indices), reported by adapt()."""

    def __init__(self, specs, units, seg_len, device, n_items=N_ITEMS, seed=0):
        if not specs or len(specs) != len(units):
            raise ValueError('VoiceSet: %d spectrograms for %d unit arrays' % (len(specs), len(units)))
        self.device, self.seg_len = torch.device(device), int(seg_len)
        frames, ucount = [int(s.shape[0]) for s in specs], [int(u.shape[0]) for u in units]
        utt, t, self.kept, self.left_out = plan_items(frames, ucount, seg_len, n_items, seed)
        self.F = int(specs[0].shape[1])
        self.row_bytes = int(units[0].shape[1])
        if any(int(s.shape[1]) != self.F for s in specs) or any(int(u.shape[1]) != self.row_bytes for u in units):
            raise ValueError('VoiceSet: every spectrogram must be [T, %d] and every unit array [U, %d]' % (self.F, self.row_bytes))
        off = np.concatenate(([0], np.cumsum([(n + 7) // 8 * 8 for n in frames]))).astype(np.int64)
        uoff = np.concatenate(([0], np.cumsum(ucount))).astype(np.int64)
        self.frames_total, self.n_units = int(off[-1]), int(uoff[-1])
        self.n_frames_kept = int(sum(frames[i] for i in self.kept))
        self.first, self.ufirst = off[utt] + t, uoff[utt] + t // 8
        check_items(self.first, self.ufirst, self.seg_len, self.frames_total, self.n_units)
        self.pool = torch.zeros(self.frames_total, self.F, dtype=torch.float32, device=self.device)
        for i, s in enumerate(specs):
            self.pool[int(off[i]):int(off[i]) + frames[i]].copy_(torch.as_tensor(s).to(torch.float32))
        self.packed = torch.from_numpy(np.ascontiguousarray(np.concatenate([np.asarray(u, dtype=np.uint8) for u in units]))).to(self.device)
        self.first_d = torch.from_numpy(self.first).to(self.device)
        self.ufirst_d = torch.from_numpy(self.ufirst).to(self.device)
        self.n = len(self.first)

    def gather(self, cursor, B, x, bits, E, dtype, stream, advance=1):
        """Launch zs_voice_gather of the cursor's batch into x fp32 [B, seg_len, F] and the operand `bits` (layers.Act)."""
        L.call('zs_voice_gather', 'ZsVoiceGather', stream, dtype=dtype, pool=L.ptr(self.pool), packed=L.ptr(self.packed),
               row_bytes=self.row_bytes, first=L.ptr(self.first_d), ufirst=L.ptr(self.ufirst_d), n=self.n, cursor=L.ptr(cursor), B=B,
               seg_len=self.seg_len, F=self.F, E=E, x=L.ptr(x), bits=bits.ptr(), ld_bits=bits.ld, advance=advance)


# ---- the step --------------------------------------------------------------------------------------------------------------------
class VoiceStep(object):
    """One adaptation iteration over a VoiceSet for the Decoder weights `decoder` (a model.Decoder; it is not touched): a Decoder of
    c_a = 1 is built from its state dict with `rows` (init_rows) as its tables, and only those five rows are ever written.
    step() enqueues gather, forward, L1, the backward without parameter gradients, zs_voice_adam and the step counter on the current
    stream and returns the device scalar of the loss; with use_graph (default: ZS_GRAPH, on) the launches are captured after
    graph_warmup eager iterations and replayed.  Everything that changes between iterations lives in device memory (the cursor,
    the Adam step count), so the eager and the replayed iteration compute the same bits."""

    def __init__(self, decoder, vset, batch_size, rows, lr=1e-4, betas=(0.5, 0.9), max_grad_norm=5.0, use_graph=None):
        sd = {k: v.detach().clone() for k, v in decoder.state_dict().items()}
        self.dec = _clone_decoder(decoder, replace_tables(sd, rows), 1)
        self.dec.train()                                              # the backward's tape (the Decoder has no dropout)
        if vset.F != self.dec.c_out or vset.row_bytes < (self.dec.c_in + 7) // 8:
            raise ValueError('VoiceStep: the set has F = %d and %d bytes per unit, the decoder c_out = %d and c_in = %d'
                             % (vset.F, vset.row_bytes, self.dec.c_out, self.dec.c_in))
        self.vset, self.B = vset, int(batch_size)
        if self.B <= 0:
            raise ValueError('VoiceStep: batch_size must be > 0')
        self.lr, self.betas, self.max_norm = float(lr), (float(betas[0]), float(betas[1])), float(max_grad_norm or 0.0)
        dev = self.device = vset.device
        C = self.C = self.dec.c_h
        self.de = self.dec._engine()                                  # built and packed here, never re-packed: the weights are frozen
        P = dict(self.dec.named_parameters())
        self.row_params = [P[k] for k in EMB_KEYS]
        self._row_ptrs = (ctypes.c_void_p * N_ROWS)(*[p.data_ptr() for p in self.row_params])
        self.m = torch.zeros(N_ROWS * C, dtype=torch.float32, device=dev)
        self.v = torch.zeros(N_ROWS * C, dtype=torch.float32, device=dev)
        self.g = torch.zeros(N_ROWS * C, dtype=torch.float32, device=dev)
        self.sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        self._step_dev = torch.ones(1, dtype=torch.int32, device=dev)  # the Adam step count t of the NEXT update (zs_step_counters)
        self._loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self._lpart = torch.zeros(1024, dtype=torch.float32, device=dev)
        self.x = torch.zeros(self.B, vset.seg_len, vset.F, dtype=torch.float32, device=dev)
        self.cidx = torch.zeros(self.B, dtype=torch.int64, device=dev)
        self.use_graph = (os.environ.get('ZS_GRAPH', '1') == '1') if use_graph is None else bool(use_graph)
        self.graph_warmup = 2
        self._graph = None
        self._eager_calls = 0
        self.iteration = 0

    def rows(self):
        """The five rows as fp32 numpy arrays [c_h] (synchronises)."""
        return [p.detach().reshape(-1).cpu().numpy().copy() for p in self.row_params]

    # ---- the launches of one iteration, in order ----
    def gather(self, advance=1):
        ctx = self.de.ctx
        bits = ctx.act('v_bits_%d_%d' % (self.de.uid, self.B), self.B, self.vset.seg_len // 8, self.dec.c_in)
        self.vset.gather(self.cursor, self.B, self.x, bits, self.dec.c_in, ctx.dt, ctx.stream, advance=advance)
        return bits

    def l1_loss(self, xdec):
        ctx = self.de.ctx
        B, T, F = self.x.shape
        dlogit = ctx.act('v_dlogit_%d_%d' % (B, T), B, xdec.T, F)
        L.call('zs_l1_loss', 'ZsL1Loss', ctx.stream, dtype=ctx.dt, x_dec=xdec.ptr(), ld_dec=xdec.ld, x=L.ptr(self.x), ldx=F,
               rows=B * xdec.T, F=F, dlogits=dlogit.ptr(), ldg=dlogit.ld, fill_cols=dlogit.ld, partial=L.ptr(self._lpart),
               loss_out=L.ptr(self._loss), grad_scale=1.0)
        return dlogit

    def forward_backward(self):
        """gather, Decoder forward, L1, backward(param_grads=False): leaves the per-sample embedding sums in self.de._embsum."""
        bits = self.gather()
        xdec = self.de.forward(bits, self.cidx, True)
        self.de.backward(self.l1_loss(xdec), need_dbits=False, param_grads=False)
        return xdec

    def adam(self):
        st = self.de.ctx.stream
        b1, b2 = self.betas
        L.call('zs_voice_adam', 'ZsVoiceAdam', st, emb_sum=L.ptr(self.de._embsum), B=self.B, C=self.C, row=self._row_ptrs,
               m=L.ptr(self.m), v=L.ptr(self.v), g=L.ptr(self.g), lr=self.lr, beta1=b1, beta2=b2, eps=1e-8, bc1=1.0, bc2=1.0,
               sumsq=L.ptr(self.sumsq), max_norm=self.max_norm, step_ptr=L.ptr(self._step_dev))

    def _launches(self):
        self.forward_backward()
        self.adam()
        L.check(L.lib().zs_step_counters(None, L.ptr(self._step_dev), self.de.ctx.stream), 'zs_step_counters')

    def step(self):
        """One iteration on the current stream; returns the device scalar that holds its loss (mean |x_dec - x| of the batch,
        before the update) until the next iteration overwrites it."""
        if not self.use_graph:
            self._launches()
        else:
            if self._graph is None and self._eager_calls < self.graph_warmup:
                self._eager_calls += 1                               # the captured launches, eagerly: every buffer allocated
                self._launches()
            else:
                if self._graph is None:
                    torch.cuda.synchronize(self.device)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, capture_error_mode='thread_local'):
                        self._launches()
                    self._graph = g
                self._graph.replay()
        self.iteration += 1
        return self._loss

    def run(self, iters, log_every=0, log=None):
        """`iters` iterations; the loss is read back (one synchronisation) after every log_every-th iteration and after the last.
        Returns [(iteration, loss)] of those."""
        out, end = [], self.iteration + int(iters)
        while self.iteration < end:
            loss = self.step()
            if self.iteration == end or (log_every and self.iteration % log_every == 0):
                out.append((self.iteration, float(loss.item())))
                if log is not None:
                    log(*out[-1])
        from . import layers
        layers.check_status(self.device)
        return out


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def voice_path(voice_dir, name):
    return os.path.join(voice_dir, name + '.voice.npz')


def adapt(trainer, seg_len, wav_dir, name, voice_dir, speaker2id=None, iters=ADAPT_ITERS, init=None, lr=None, batch_size=None,
          seed=NOISE_SEED, log_every=100, n_items=N_ITEMS, wavs=None):
    """Fit a voice called `name` to every *.wav of wav_dir (read as --convert_dir reads them: any format and rate, features and
    trim on the device; or `wavs`, a list of (samples, rate)) and write {voice_dir}/{name}.voice.npz.  init: a speaker name of
    speaker2id whose rows start the fit (default: the mean of each table's rows).  lr default hps.lr; Adam betas (0.5, 0.9) and
    clip_grad_norm_(hps.max_grad_norm) over the five rows together, as the training run.  The same call on the same files gives
    the same file contents bit for bit.  Neither the checkpoint nor any other file is written.  Returns (path, meta)."""
    from . import convert as cv
    from .preprocess import read_wav
    hps, dev = trainer.hps, trainer.device
    if trainer.enc_mode == 'continues':
        raise ValueError("enc_mode 'continues' has no units to cache: a voice cannot be adapted")
    speaker2id = speaker2id or {}
    if name in speaker2id:
        raise ValueError('%r is a speaker of the checkpoint already' % name)
    init_id = None
    if init is not None:
        if init not in speaker2id:
            raise ValueError('--adapt_init %r is not in speaker2id' % init)
        init_id = int(speaker2id[init])
    skipped = []
    if wavs is None:
        wavs = []
        for path in sorted(glob.glob(os.path.join(wav_dir, '*.wav'))):
            try:
                wavs.append(read_wav(path))
            except Exception as e:                                  # as convert_dir: an unreadable file is skipped with a reason
                print('[Adapter] - skipped %s: cannot be read: %s' % (path, e))
                skipped.append(path)
    if not wavs:
        raise ValueError('no readable *.wav in %s' % wav_dir)
    specs, _ = cv._wav_features([w for w, _ in wavs], [r for _, r in wavs], dev, strict=False)
    too_short = sum(s is None for s in specs)
    specs = [s for s in specs if s is not None]
    if not specs:
        raise ValueError('every utterance of %s is too short after trimming' % wav_dir)
    trainer.set_eval()
    units, _ = cv.encode_batch(specs, trainer, seg_len, noise_fn=gumbel_noise_fn(trainer.Encoder, seed), packed=True)
    vset = VoiceSet(specs, units, seg_len, dev, n_items=n_items, seed=seed)
    left_out = len(vset.left_out) + too_short + len(skipped)
    if left_out:
        print('[Adapter] - %d of %d utterances were left out: %d unreadable, %d too short after trimming, %d shorter than seg_len = %d frames'
              % (left_out, len(wavs) + len(skipped), len(skipped), too_short, len(vset.left_out), seg_len))
    sd = trainer.Decoder.state_dict()
    step = VoiceStep(trainer.Decoder, vset, batch_size or hps.batch_size, init_rows(sd, init_id), lr=(hps.lr if lr is None else lr),
                     betas=(0.5, 0.9), max_grad_norm=hps.max_grad_norm)
    print('[Adapter] - voice %r: %d utterances, %d frames, %d iterations of %d segments' % (name, len(vset.kept), vset.n_frames_kept, iters, step.B))
    hist = step.run(iters, log_every, log=lambda it, loss: print('[Adapter] - iteration %d: loss_rec %.6f' % (it, loss)))
    meta = {'name': name, 'seg_len': int(seg_len), 'iterations': int(iters), 'final_loss': hist[-1][1] if hist else None,
            'init': init if init is not None else 'mean', 'utterances': len(vset.kept), 'frames': vset.n_frames_kept,
            'left_out': left_out, 'lr': float(step.lr), 'digest': decoder_digest(sd)}
    path = voice_path(voice_dir, name)
    meta = save_voice(path, step.rows(), meta)
    print('[Adapter] - wrote %s' % path)
    return path, meta
