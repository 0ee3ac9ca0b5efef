"""Inference / resynthesis surface of the reference's convert.py (lines 36-265, 303-360).

convert() / encode() reproduce the reference's fragment rule exactly (MIN_LEN zero padding, `spec[idx:-1]`
tail that drops the last frame, tails shorter than seg_len skipped, RuntimeError for a too-short input),
call Trainer.test_step / encoder_test_step per fragment and concatenate.  spectrogram2wav() /
griffin_lim() run the 300-iteration Griffin-Lim on the MI355X (zs_gl_* kernels: 1024-point FFTs in LDS),
batched over utterances by griffin_lim_batch(); `momentum` (default hp.gl_momentum = 0) selects the fast Griffin-Lim of
Perraudin et al. (2013), as librosa / torchaudio name it; de-preemphasis on the device, librosa.effects.trim restated
on the host (librosa itself is not required).  synth_units_batch() / synth_dir() go the other way from the unit files alone
(bit-packed units, zs_units_unpack into the Decoder's operand; not in the reference).  Utterances are independent: multi-GPU = replicas over a
sharded utterance list (zs_amd.parallel.shard_range), no collective.
"""
import ctypes
import glob
import json
import os
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L
from . import segment as sg
from .hps import Hps, hp

MIN_LEN = 9


# ---------------------------------------------------------------------------------------------------
# vocoder (convert.py:39-62)
# ---------------------------------------------------------------------------------------------------

def _device():
    if not torch.cuda.is_available():
        raise L.ZsError('zs_amd.convert needs an MI355X; there is no CPU fallback')
    return torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0')))


def gl_momentum(momentum):
    """The fast Griffin-Lim momentum to use: hp.gl_momentum when None; ValueError unless it is a finite number in [0, 1)."""
    m = hp.gl_momentum if momentum is None else momentum
    try:
        m = float(m)
    except (TypeError, ValueError):
        raise ValueError('Griffin-Lim momentum must be a number in [0, 1) (got %r)' % (m,))
    if not (np.isfinite(m) and 0.0 <= m < 1.0):
        raise ValueError('Griffin-Lim momentum must be in [0, 1) (got %r)' % (m,))
    return m


def griffin_lim_batch(mags, n_iter=None, device=None, impl=None, tile_frames=0, mag_padded=None, momentum=None):
    """mags: list of real [513, T_i] amplitude spectrograms (or mag_padded).  Returns (wav [n, 200*(T_max-1)] on the device, lengths, lens).
    X = S (zero phase); n_iter x { x = istft(X); E = stft(x); X = S * E / max(1e-8, |E|) }; x = istft(X)  (convert.py:39-52).
    momentum alpha > 0 (None: hp.gl_momentum): fast Griffin-Lim -- X = S * A / max(1e-8, |A|) with A = E - alpha / (1 + alpha) *
    (E of the previous iteration), A = E in the first; alpha = 0 is the loop above, bit for bit.
    impl 'fused' (default): zs_griffin_lim -- one fused kernel per iteration, the whole loop issued by one C call;
    impl 'split' (ZS_GL_IMPL=split): the older per-transform kernels (zs_gl_istft + zs_gl_stft_project per iteration), kept as
    the variant the tests compare the fused kernel with (plain loop only)."""
    n_iter = hp.n_iter if n_iter is None else n_iter
    momentum = gl_momentum(momentum)
    impl = impl or os.environ.get('ZS_GL_IMPL', 'fused')
    if impl == 'split' and momentum > 0:
        raise ValueError("griffin_lim impl 'split' runs the plain loop only (momentum must be 0)")
    dev = device or _device()
    st = torch.cuda.current_stream(dev).cuda_stream
    if mag_padded is not None:                    # (amplitudes [n, T_max, 513] fp32 on the device, frame counts)
        mag, lens = mag_padded
        n, Tm = mag.shape[0], mag.shape[1]
    else:
        n = len(mags)
        lens = [int(m.shape[1]) for m in mags]
        Tm = max(lens)
    if min(lens) < 4:
        raise ValueError('griffin_lim needs at least 4 frames (reflect padding of n_fft//2 = 512 samples on 200*(T-1) samples)')
    if mag_padded is None:
        mag = torch.zeros(n, Tm, 513, dtype=torch.float32, device=dev)
        for i, m in enumerate(mags):
            t = m if torch.is_tensor(m) else torch.as_tensor(np.asarray(m, dtype=np.float32))
            mag[i, :lens[i]] = t.to(dev, torch.float32).t()
    lengths = torch.tensor(lens, dtype=torch.int32, device=dev)
    wav_ld = 200 * (Tm - 1)
    wav = torch.zeros(n, wav_ld, dtype=torch.float32, device=dev)
    if impl == 'fused':
        spec = torch.empty(n, Tm, 513, 2, dtype=torch.float32, device=dev)     # scratch: the first iteration reads X0 = S from `mag`
        spec_b = torch.empty_like(spec)
        host_lens = np.asarray(lens, dtype=np.int32)                # the chains of zs_griffin_lim are cut at equal frame counts
        prev = torch.empty_like(spec) if momentum > 0 else None     # scratch as well: the first iteration writes it
        S = L.STRUCTS['ZsGlIter'](mag=L.ptr(mag), lengths=L.ptr(lengths), n_utt=n, T_max=Tm, wav=L.ptr(wav), wav_ld=wav_ld,
                                  tile_frames=int(tile_frames), host_lengths=host_lens.ctypes.data, momentum=momentum,
                                  spec_prev=L.ptr(prev))
        L.check(L.lib().zs_griffin_lim(ctypes.addressof(S), L.ptr(spec), L.ptr(spec_b), int(n_iter), st), 'zs_griffin_lim')
        return wav, lengths, lens
    if impl != 'split':
        raise ValueError("griffin_lim impl must be 'fused' or 'split'")
    spec = torch.zeros(n, Tm, 513, 2, dtype=torch.float32, device=dev)
    spec[..., 0] = mag                            # X0 = S, zero phase; rows past an utterance's length are never read
    frames = torch.empty(n, Tm, 1024, dtype=torch.float32, device=dev)
    ist = dict(spec=L.ptr(spec), mag=L.ptr(mag), lengths=L.ptr(lengths), n_utt=n, T_max=Tm, wav=L.ptr(wav), wav_ld=wav_ld,
               frames_ws=L.ptr(frames))
    stf = dict(wav=L.ptr(wav), wav_ld=wav_ld, mag=L.ptr(mag), lengths=L.ptr(lengths), n_utt=n, T_max=Tm, spec=L.ptr(spec))
    for _ in range(n_iter):
        L.call('zs_gl_istft', 'ZsGlIstft', st, **ist)
        L.call('zs_gl_stft_project', 'ZsGlStft', st, **stf)
    L.call('zs_gl_istft', 'ZsGlIstft', st, **ist)
    return wav, lengths, lens


def griffin_lim(spectrogram, n_iter=None, impl=None, momentum=None):
    """convert.py:39-52 for one [513, T] amplitude spectrogram."""
    wav, _, lens = griffin_lim_batch([spectrogram], n_iter=n_iter, impl=impl, momentum=momentum)
    return wav[0, :200 * (lens[0] - 1)].cpu().numpy()


def trim(wav, top_db=60, frame_length=2048, hop_length=512):
    """librosa.effects.trim defaults restated (RMS of centred frames, dB relative to the max).  The frames overlap four
    times (2048 / 512): the mean squares come from sums over 512-sample blocks, one pass over the signal."""
    y = np.asarray(wav, dtype=np.float64)
    if len(y) == 0:
        return y, (0, 0)
    yp = np.pad(y, frame_length // 2, mode='reflect')
    n_frames = 1 + (len(yp) - frame_length) // hop_length
    if frame_length % hop_length == 0:
        r = frame_length // hop_length
        nb = n_frames + r - 1
        blocks = np.einsum('ij,ij->i', yp[:nb * hop_length].reshape(nb, hop_length), yp[:nb * hop_length].reshape(nb, hop_length))
        cs = np.concatenate(([0.0], np.cumsum(blocks)))
        mse = (cs[r:r + n_frames] - cs[:n_frames]) / frame_length
        mse = np.maximum(mse, 0.0)
    else:
        idx = np.arange(frame_length)[None, :] + hop_length * np.arange(n_frames)[:, None]
        mse = np.mean(yp[idx] ** 2, axis=1)
    db = 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(np.maximum(1e-10, np.max(mse)))
    nz = np.flatnonzero(db > -top_db)
    if nz.size == 0:
        return y[0:0], (0, 0)
    start, end = int(nz[0]) * hop_length, min(len(y), (int(nz[-1]) + 1) * hop_length)
    return y[start:end], (start, end)


TRIM_FRAME, TRIM_HOP = 2048, 512        # librosa.effects.trim defaults


def trim_bounds(mse, n, top_db=60, hop_length=TRIM_HOP):
    """(start, stop) of librosa.effects.trim given the frame mean squares (see trim())."""
    mse = np.asarray(mse, dtype=np.float64)
    db = 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(np.maximum(1e-10, np.max(mse)))
    nz = np.flatnonzero(db > -top_db)
    if nz.size == 0:
        return 0, 0
    return int(nz[0]) * hop_length, min(n, (int(nz[-1]) + 1) * hop_length)


def _enqueue_vocoder(t, lens, n_iter, do_trim, dev, amplitudes=False, momentum=None):
    """t: normalised magnitudes [n, T_max, 513] fp32 on the device (amplitudes=True: already de-normalised, e.g. by
    zs_gen_scatter).  Enqueues convert.py:55-62 and returns the _VocoderWait that waits for it and cuts the waveforms
    (librosa.effects.trim restated on device-computed frame statistics)."""
    st = torch.cuda.current_stream(dev).cuda_stream
    if amplitudes:
        amp = t
    else:
        amp = torch.empty_like(t)
        L.check(L.lib().zs_gl_denormalize(L.ptr(t), L.ptr(amp), t.numel(), st), 'zs_gl_denormalize')     # convert.py:56-58
    wav, lengths, lens = griffin_lim_batch(None, n_iter=n_iter, device=dev, mag_padded=(amp, lens), momentum=momentum)
    L.check(L.lib().zs_gl_deemphasis(L.ptr(wav), wav.shape[1], L.ptr(lengths), len(lens), float(hp.preemphasis), st),
            'zs_gl_deemphasis')                               # signal.lfilter([1], [1, -0.97], wav)
    mse_h = None
    if do_trim and min(lens) > 6:                            # frame statistics of librosa.effects.trim on the device (convert.py:61)
        nf = 1 + wav.shape[1] // TRIM_HOP
        mse = torch.zeros(len(lens), nf, dtype=torch.float64, device=dev)
        L.check(L.lib().zs_gl_frame_mse(L.ptr(wav), wav.shape[1], L.ptr(lengths), len(lens), TRIM_FRAME, TRIM_HOP, L.ptr(mse), nf, st),
                'zs_gl_frame_mse')
        mse_h = _to_host(mse)
    w_h = _to_host(wav)
    from . import layers
    st_h = _to_host(layers.device_status(dev))                # the sticky GRU status word as of this batch (checked by the caller)
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(dev))
    return _VocoderWait(done, st_h, w_h, mse_h, lens, do_trim)


class _VocoderWait(object):
    """What _enqueue_vocoder returns: the call waits for the batch and cuts its waveforms; `status` is then the sticky GRU status
    word as of the batch.  An object, not a closure that names itself to carry `status`: that closure is a reference cycle, and
    the pinned buffers it holds (64 MB for 64 utterances) waited for the garbage collector instead of going back to the pool with
    the result -- the next batches then paid for fresh pinned memory or not, by when a collection happened to run."""
    __slots__ = ('done', 'st_h', 'w_h', 'mse_h', 'lens', 'do_trim', 'status')

    def __init__(self, done, st_h, w_h, mse_h, lens, do_trim):
        self.done, self.st_h, self.w_h, self.mse_h, self.lens, self.do_trim, self.status = done, st_h, w_h, mse_h, lens, do_trim, None

    def __call__(self):
        self.done.synchronize()                               # this batch's copies only: later batches may already be enqueued
        self.status = int(self.st_h[0])
        w = self.w_h.numpy()
        out = []
        for i, T in enumerate(self.lens):
            y = w[i, :200 * (T - 1)]
            if self.do_trim:
                if self.mse_h is not None:
                    a, b = trim_bounds(self.mse_h[i, :1 + len(y) // TRIM_HOP].numpy(), len(y))
                    y = y[a:b]
                else:
                    y, _ = trim(y)
            out.append(np.asarray(y, dtype=np.float32))
        return out


def spectrogram2wav_batch(mags_tf, n_iter=None, do_trim=True, momentum=None):
    """Batched spectrogram2wav (convert.py:55-62): list of [T_i, 513] normalised magnitudes -> list of float32 wavs.
    One padded buffer, one H2D copy (unless the magnitudes are on the device already), one de-normalisation launch, one
    zs_griffin_lim call, one de-emphasis launch, one D2H copy; librosa.effects.trim (restated) from frame statistics computed on
    the device.  momentum: see griffin_lim_batch."""
    momentum = gl_momentum(momentum)
    dev = _device()
    lens = [int(m.shape[0]) for m in mags_tf]
    n, Tm = len(lens), max(lens)
    if all(torch.is_tensor(m) and m.is_cuda for m in mags_tf):          # decoder outputs still on the device (encode_batch(to_host=False))
        t = torch.zeros(n, Tm, 513, dtype=torch.float32, device=dev)
        for i, m in enumerate(mags_tf):
            t[i, :lens[i]] = m
    else:
        host = np.zeros((n, Tm, 513), dtype=np.float32)
        for i, m in enumerate(mags_tf):
            host[i, :lens[i]] = np.asarray(m.cpu() if torch.is_tensor(m) else m, dtype=np.float32)
        t = torch.from_numpy(host).to(dev)
    return _enqueue_vocoder(t, lens, n_iter, do_trim, dev, momentum=momentum)()


def spectrogram2wav(mag, n_iter=None, momentum=None):
    return spectrogram2wav_batch([mag], n_iter=n_iter, momentum=momentum)[0]


# ---------------------------------------------------------------------------------------------------
# fragment drivers (convert.py:70-221)
# ---------------------------------------------------------------------------------------------------

def convert_x(x, c, trainer, enc_only, verbose=False):
    c_var = torch.from_numpy(np.array([c]))
    tensor = torch.from_numpy(np.expand_dims(x, axis=0)).type(torch.FloatTensor)
    converted, enc = trainer.test_step(tensor, c_var, enc_only=enc_only, verbose=verbose)
    return converted.squeeze(axis=0).transpose((1, 0)), enc.squeeze(axis=0).transpose((1, 0))


def encode_x(x, trainer):
    tensor = torch.from_numpy(np.expand_dims(x, axis=0)).type(torch.FloatTensor)
    return trainer.encoder_test_step(tensor).squeeze(axis=0).transpose((1, 0))


def get_trainer(hps_path, model_path, g_mode, enc_mode, clf_path=None, use_ema=False):
    """use_ema: convert with the averaged weights of the checkpoint (its `<net>_ema` entries, Trainer.load_model)."""
    from .trainer import Trainer
    hps = Hps(hps_path).get_tuple()
    global MIN_LEN
    MIN_LEN = MIN_LEN if hps.enc_mode != 'gumbel_t' else hps.seg_len
    trainer = Trainer(hps, None, g_mode, enc_mode)
    trainer.load_model(model_path, load_model_list=hps.load_model_list, clf_path=clf_path, use_ema=use_ema)
    return trainer


def fragments(n_frames, seg_len):
    """(start, stop) slices the reference sends through the network for an utterance of n_frames >= MIN_LEN
    (convert.py:151-165): full seg_len pieces, then a tail `spec[idx:-1]` once idx + 2*seg_len > len; pieces
    shorter than seg_len are skipped."""
    out = []
    for idx in range(0, n_frames, seg_len):
        if idx + (seg_len * 2) > n_frames:
            start, stop = idx, n_frames - 1
        else:
            start, stop = idx, idx + seg_len
        if stop - start >= seg_len:
            out.append((start, stop))
        elif idx == 0:
            raise RuntimeError('Please check if input is too short!')
    return out


def _pad_min(spec):
    if len(spec) < MIN_LEN:
        padding = np.zeros((MIN_LEN - spec.shape[0], spec.shape[1]))
        return np.concatenate((spec, padding), axis=0), True
    return spec, False


def parse_encodings(encodings):
    return [' '.join([str(int(e)) for e in enc]) for enc in encodings]


def write_encodings(path, encodings):
    with open(path, 'w') as file:
        for enc in encodings:
            for i, e in enumerate(enc):
                file.write(str(int(e)) + (' ' if i < len(enc) - 1 else ''))
            file.write('\n')


def read_units(path, E):
    """The parser of what write_encodings writes: one line of E tokens `0` / `1` per unit -> float32 [U, E].  ValueError naming the
    file and the line for a line of another width or a token other than 0 / 1, and for a file without a line."""
    rows = []
    with open(path, 'r') as f:
        for no, line in enumerate(f, 1):
            tokens = line.split()
            if len(tokens) != E:
                raise ValueError('%s, line %d: %d values, expected %d' % (path, no, len(tokens), E))
            bad = [t for t in tokens if t not in ('0', '1')]
            if bad:
                raise ValueError('%s, line %d: %r is not 0 or 1' % (path, no, bad[0]))
            rows.append([t == '1' for t in tokens])
    if not rows:
        raise ValueError('%s: no units (the file is empty)' % path)
    return np.asarray(rows, dtype=np.float32)


def pack_units(units):
    """[U, E] of 0 / 1 -> uint8 [U, (E + 7) // 8]: bit j of byte k of a row is column 8k + j (numpy.packbits(bitorder='little')
    along the columns), the unused high bits of a row's last byte zero.  This and unpack_units are the definition zs_units_pack and
    zs_units_unpack are tested against.  ValueError on any other value."""
    u = np.asarray(units)
    if u.ndim != 2:
        raise ValueError('pack_units: units must be [U, E] (got shape %s)' % (u.shape,))
    if not np.logical_or(u == 0, u == 1).all():
        raise ValueError('pack_units: units must be 0 or 1')
    return np.packbits(u != 0, axis=1, bitorder='little').reshape(u.shape[0], (u.shape[1] + 7) // 8)


def unpack_units(packed, E):
    """uint8 [U, (E + 7) // 8] -> float32 [U, E], the inverse of pack_units."""
    p = np.asarray(packed)
    if p.dtype != np.uint8 or p.ndim != 2 or p.shape[1] != (E + 7) // 8:
        raise ValueError('unpack_units: packed must be uint8 [U, %d] for E = %d (got %s %s)' % ((E + 7) // 8, E, p.dtype, p.shape))
    return np.unpackbits(p, axis=1, count=E, bitorder='little').astype(np.float32).reshape(p.shape[0], E)


def unit_fragments(n_units, seg_len):
    """The fragment rule on unit counts: the lengths, in units, of the pieces an utterance of n_units units is decoded in.  With
    Lu = seg_len // 8: pieces of Lu while more than 2 Lu units remain, then one tail of what is left (1 .. 2 Lu units); an
    utterance of at most 2 Lu units is one fragment.
    These are the unit lengths fragments() and _t8 give an utterance of n >= MIN_LEN frames, for every n except
      n = 1 (mod seg_len) with n >= 2 seg_len + 1,   and   n = 0 (mod seg_len) with n >= 3 seg_len:
    there the reference's tail is exactly seg_len frames, Lu units, and [.., Lu, Lu] cannot be told from a tail of 2 Lu by the unit
    count alone.  Where the rule reproduces the fragmentation, synthesis from units equals convert(); in the two exceptions it is a
    decode of the same units with one boundary fewer."""
    n, Lu = int(n_units), int(seg_len) // 8
    if n < 1 or Lu < 1:
        raise ValueError('unit_fragments: need n_units >= 1 and seg_len >= 8 (got %d, %d)' % (n, seg_len))
    out = []
    while n > 2 * Lu:
        out.append(Lu)
        n -= Lu
    out.append(n)
    return out


def check_overlap_value(overlap, seg_len):
    """The overlap of two decode windows, in spectrogram frames like seg_len: 0 (none), or a multiple of 8 in [8, 8 * (Lu // 2)] with
    Lu = seg_len // 8, so that no unit lies in more than two windows.  Returns it as an int; ValueError naming the value and the
    range for anything else."""
    Lu = int(seg_len) // 8
    top = 8 * (Lu // 2)
    try:
        ok = int(overlap) == overlap and not isinstance(overlap, bool)
    except (TypeError, ValueError):
        ok = False
    if not ok or not (overlap == 0 or (overlap % 8 == 0 and 8 <= overlap <= top)):
        raise ValueError('overlap must be 0 or a multiple of 8 in [8, %d] frames for seg_len %d (got %r)' % (top, int(seg_len), overlap))
    return int(overlap)


def unit_windows(n_units, seg_len, overlap):
    """The decode windows of an utterance of n_units units, as [(a, b)] in units, for windows that share `overlap` frames
    (check_overlap_value).  With Lu = seg_len // 8, Vu = overlap // 8 and Hu = Lu - Vu: an utterance of at most 2 Lu units is one
    window (0, n); else windows (a, a + Lu) from a = 0 in steps of Hu while more than 2 Lu units lie behind a, then the tail (a, n)
    of Lu + Vu < len <= 2 Lu units.  Consecutive windows share exactly Vu units and no unit lies in more than two.  With overlap 0
    the window lengths are unit_fragments(n_units, seg_len).  The units themselves do not change: the overlap is the decode's alone."""
    overlap = check_overlap_value(overlap, seg_len)
    n, Lu = int(n_units), int(seg_len) // 8
    if n < 1 or Lu < 1:
        raise ValueError('unit_windows: need n_units >= 1 and seg_len >= 8 (got %d, %d)' % (n, seg_len))
    Hu = Lu - overlap // 8
    out, a = [], 0
    while n - a > 2 * Lu:
        out.append((a, a + Lu))
        a += Hu
    out.append((a, n))
    return out


def xfade_weights(V):
    """The cross-fade over the V frames two windows share: frame j takes w[j] of the later window and u[j] of the earlier one,
    w[j] = (2 j + 1) / (2 V) and u[j] = 1 - (2 j + 1) / (2 V), each evaluated in double and rounded once to fp32.  Returns (w, u)."""
    x = (2.0 * np.arange(int(V), dtype=np.float64) + 1.0) / (2.0 * int(V))
    return x.astype(np.float32), (1.0 - x).astype(np.float32)


def convert(trainer, seg_len, src_speaker_spec, src_speaker, tar_speaker, utt_id, speaker2id, result_dir, enc_only=True,
            save=['wav', 'enc']):
    src_speaker_spec, PADDED = _pad_min(src_speaker_spec)
    if len(src_speaker_spec) <= seg_len:
        converted_results, encodings = convert_x(src_speaker_spec, speaker2id[tar_speaker], trainer, enc_only=enc_only)
        if PADDED:
            encodings = encodings[:MIN_LEN // 8]
    else:
        converted_results, encodings = [], []
        for a, b in fragments(len(src_speaker_spec), seg_len):
            converted_x, enc = convert_x(src_speaker_spec[a:b], speaker2id[tar_speaker], trainer, enc_only=enc_only)
            converted_results.append(converted_x)
            encodings.append(enc)
        converted_results = np.concatenate(converted_results, axis=0)
        encodings = np.concatenate(encodings, axis=0)
    wav_data = spectrogram2wav(converted_results)
    if len(save) != 0:
        wav_path = None
        if 'wav' in save:
            wav_path = os.path.join(result_dir, f'{tar_speaker}_{utt_id}.wav')
            write_wav(wav_path, to_out_sr([wav_data])[0], out_rate())
        if 'enc' in save:
            write_encodings(os.path.join(result_dir, f'{src_speaker}_{utt_id}.txt'), encodings)
        return wav_path, len(converted_results)
    return wav_data, encodings


def encode(src_speaker_spec, trainer, seg_len, s_speaker=None, utt_id=None, result_dir=None, save=True):
    if save:
        assert result_dir is not None and s_speaker is not None and utt_id is not None
    src_speaker_spec, PADDED = _pad_min(src_speaker_spec)
    if len(src_speaker_spec) <= seg_len:
        encodings = encode_x(src_speaker_spec, trainer)
        if PADDED:
            encodings = encodings[:MIN_LEN // 8]
    else:
        encodings = [encode_x(src_speaker_spec[a:b], trainer) for a, b in fragments(len(src_speaker_spec), seg_len)]
        encodings = np.concatenate(encodings, axis=0)
    if save:
        write_encodings(os.path.join(result_dir, f'{s_speaker}_{utt_id}.txt'), encodings)
    else:
        return encodings


_POOL = None


_STAGE_THREADS = 4


def _pool():
    """A few host threads for the memcpy-bound staging of batches into pinned memory."""
    global _POOL
    if _POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(max_workers=_STAGE_THREADS)
    return _POOL


def _stage_rows(arrays, dev):
    """list of [T_i, C] arrays -> (device fp32 tensor [sum T_i + 1, C] whose LAST row is zeros, row offsets).
    Host arrays: one pass over the bytes into a pinned buffer (torch's caching host allocator recycles it between calls),
    several threads, then ONE asynchronous H2D copy at the link rate -- a pageable .to(device) of the same bytes is 3-4 x
    slower.  Utterances already resident in HBM (torch tensors on `dev`): one concatenation on the device, no host pass."""
    C = int(arrays[0].shape[1])
    offs = np.concatenate(([0], np.cumsum([int(a.shape[0]) for a in arrays]))).astype(np.int64)
    total = int(offs[-1])
    if all(torch.is_tensor(a) and a.is_cuda for a in arrays):
        return torch.cat([a.to(dev, torch.float32) for a in arrays] + [torch.zeros(1, C, dtype=torch.float32, device=dev)], dim=0), offs
    host = torch.empty(total + 1, C, dtype=torch.float32, pin_memory=True)
    host[total].zero_()
    hn = host.numpy()
    src = [a.detach().cpu().float().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float32) for a in arrays]
    k = max(1, min(_STAGE_THREADS, len(src)))
    cuts = [len(src) * i // k for i in range(k + 1)]

    def put(g):                                   # numpy's copy loop (GIL released); torch's copy_ of many small slices is 3 x slower
        a, b = cuts[g], cuts[g + 1]
        if b > a:
            np.concatenate(src[a:b], axis=0, out=hn[offs[a]:offs[b]])
    list(_pool().map(put, range(k)))
    return host.to(dev, non_blocking=True), offs


def _to_host(t):
    """Device tensor -> numpy array backed by pinned memory (asynchronous D2H; the caller synchronises once for all of them)."""
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t, non_blocking=True)
    return h


def _t8(n):
    return ((((n + 1) // 2 + 1) // 2) + 1) // 2


class _Enqueued(object):
    """What _enqueue_encode and synth_units_batch leave behind: nothing here has been waited for, and a slot its producer has
    nothing for is None.  With the generator (enc_only=False), `conv` holds the converted spectrograms [n_utt, T_max, 513] fp32 on
    the device (amplitudes when de-normalised) and `ulens` their frames."""
    __slots__ = ('n_utt', 'chunks', 'enc_host', 'dec_dev', 'dec_host', 'enc_done', 'dev', 'conv', 'ulens', 'units_host', 'uoffs',
                 'units_dev', 'idx_host', 'cb_total', 'cb', 'enc_dev', 'seg_scores', 'seg_row')

    def __init__(self):
        for slot in self.__slots__:
            setattr(self, slot, None)


# ---------------------------------------------------------------------------------------------------
# the plans of a batch: host code alone (numpy in, numpy out; tests/test_convert_plan_host.py), uploaded by _upload_tables
# ---------------------------------------------------------------------------------------------------

class _Item(namedtuple('_Item', 'u k a b trunc')):
    """One fragment: rows [a, b) of utterance u (frames for _enqueue_encode, units for synth_units_batch), the k-th of its
    utterance; trunc: the units returned for an input that was padded to MIN_LEN, else None."""
    __slots__ = ()

    @property
    def n(self):
        return self.b - self.a


def _frame_items(u, n_frames, seg_len, was_padded):
    """The items of utterance u of n_frames >= MIN_LEN frames (after _pad_min): one when it is at most seg_len, else fragments()."""
    if n_frames <= seg_len:
        return [_Item(u, 0, 0, n_frames, (MIN_LEN // 8) if was_padded else None)]
    return [_Item(u, k, a, b, None) for k, (a, b) in enumerate(fragments(n_frames, seg_len))]


def _unit_items(u, n_units, seg_len):
    """The items of utterance u of n_units units: the pieces of unit_fragments, back to back."""
    ends = np.cumsum(unit_fragments(n_units, seg_len)).tolist()
    return [_Item(u, k, a, b, None) for k, (a, b) in enumerate(zip([0] + ends[:-1], ends))]


def _window_items(u, n_units, seg_len, overlap):
    """The items of utterance u of n_units units decoded in overlapping windows: those of unit_windows, which share units."""
    return [_Item(u, k, a, b, None) for k, (a, b) in enumerate(unit_windows(n_units, seg_len, overlap))]


def _split_chunks(items, full_len, max_batch):
    """Two kinds of batches instead of one per distinct length (the fragment rule leaves ~60 tail lengths per 64 utterances):
    the fragments of exactly full_len as plain batches, everything else (tails of seg_len .. 2 seg_len - 2 frames, short
    utterances) as RAGGED batches padded to their longest member, with per-sample lengths: the kernels pad / normalise / run the
    reverse GRU at each sample's own end, so a fragment's result does not depend on what it is batched with.
    Returns [(items, ragged)], ragged None for a plain chunk and True for a ragged one, each of at most max_batch items."""
    full = [it for it in items if it.n == full_len]
    rest = sorted((it for it in items if it.n != full_len), key=lambda it: -it.n)                       # longest first
    chunks = [(full[lo:lo + max_batch], None) for lo in range(0, len(full), max_batch)]
    return chunks + [(rest[lo:lo + max_batch], True) for lo in range(0, len(rest), max_batch)]


def _flat(chunks):
    return [it for chunk, _ in chunks for it in chunk]


def _fragment_layout(items, counts, n_utt):
    """THE layout of every per-utterance buffer: utterance u's rows are its fragments' rows in fragment order.  counts[i]: the rows
    of items[i] (in any order).  Returns (the first row of each item within its utterance, the rows of each utterance)."""
    at, totals = [0] * len(items), [0] * n_utt
    for i in sorted(range(len(items)), key=lambda i: items[i][:2]):
        at[i] = totals[items[i].u]
        totals[items[i].u] += counts[i]
    return at, totals


def _pack_tables(chunks, n_utt):
    """Where zs_units_pack puts every fragment's units: utterance u's units are its fragments' in fragment order, the utterances back
    to back in one buffer.  Returns (row offsets of the utterances int64 [n_utt + 1], and over all fragments in chunk order: start
    int64, len int32); len is the MIN_LEN truncation where an item carries one."""
    flat = _flat(chunks)
    lens = [it.trunc if it.trunc is not None else _t8(it.n) for it in flat]
    at, counts = _fragment_layout(flat, lens, n_utt)
    uoffs = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    starts = np.array([uoffs[it.u] + s for it, s in zip(flat, at)], dtype=np.int64)
    return uoffs, starts, np.array(lens, dtype=np.int32)


def _dense_tables(chunks):
    """The tables of the chunk-local packed buffers a codebook snaps for the Decoder: fragment i of a chunk whose longest member
    encodes to Tp frames owns rows [i Tp, i Tp + _t8(n_i)) -- every encoded frame, without the MIN_LEN truncation of _pack_tables,
    because the Decoder reads both units of an input shorter than MIN_LEN.  Over all fragments in chunk order (start int64, len int32)."""
    starts, lens = [], []
    for chunk, _ in chunks:
        Tp = _t8(max(it.n for it in chunk))
        starts += [i * Tp for i in range(len(chunk))]
        lens += [_t8(it.n) for it in chunk]
    return np.array(starts, dtype=np.int64), np.array(lens, dtype=np.int32)


def _unit_tables(chunks, uoffs):
    """Where zs_units_unpack finds every fragment in synth_units_batch's one packed buffer (utterance u's units from row uoffs[u]):
    over all fragments in chunk order (start int64, len int32)."""
    flat = _flat(chunks)
    return np.array([uoffs[it.u] + it.a for it in flat], dtype=np.int64), np.array([it.n for it in flat], dtype=np.int32)


def _scatter_tables(chunks, n_utt, rows_of=None):
    """Per chunk, the destination row of each of its output rows in the converted spectrograms' buffer [n_utt, T_max, 513]
    (b*T + t -> u*T_max + frame, -1 past a fragment's own rows): utterance u's frames are its fragments' rows in fragment order.
    rows_of(n): the output rows of a fragment of n = b - a (default: n frames in, 8 * _t8(n) rows out).
    Returns (T_max, frames per utterance, the chunk tables int32 flat, the padding rows int32: frames past an utterance's length)."""
    rows_of = rows_of or (lambda n: 8 * _t8(n))
    flat = _flat(chunks)
    out_rows = [rows_of(it.n) for it in flat]
    start, ulens = _fragment_layout(flat, out_rows, n_utt)
    Tm = max(ulens)
    tables, at = [], 0
    for chunk, _ in chunks:
        T = rows_of(max(it.n for it in chunk))
        d = np.full((len(chunk), T), -1, dtype=np.int32)
        for i, it in enumerate(chunk):
            r0, n = it.u * Tm + start[at + i], out_rows[at + i]
            d[i, :n] = np.arange(r0, r0 + n, dtype=np.int32)
        at += len(chunk)
        tables.append(d.reshape(-1))
    pad = np.concatenate([np.arange(u * Tm + ulens[u], (u + 1) * Tm, dtype=np.int32) for u in range(n_utt)])
    return Tm, ulens, tables, pad


def _gather_index(chunks, out_rows, shapes, n_utt):
    """The row index of the vocoder's padded input [n_utt, T_max] into the decoded chunks laid end to end with one zero row behind
    them: utterance u's frames are its fragments' rows in fragment order, the zero row behind them.  out_rows[ci][i]: the valid
    output rows of fragment i of chunk ci; shapes[ci]: (fragments, rows per fragment) of its decoded buffer.
    Returns (index int64 [n_utt, T_max], frames per utterance, the zero row)."""
    flat, first, total = _flat(chunks), [], 0
    for (chunk, _), (n_frag, ld) in zip(chunks, shapes):
        first += [total + i * ld for i in range(len(chunk))]
        total += n_frag * ld
    counts = [n for rows in out_rows for n in rows]
    at, ulens = _fragment_layout(flat, counts, n_utt)
    idx = np.full((n_utt, max(ulens)), total, dtype=np.int64)
    for it, r0, n, s in zip(flat, first, counts, at):
        idx[it.u, s:s + n] = np.arange(r0, r0 + n)
    return idx, ulens, total


def _xfade_tables(chunks, first, n_utt):
    """The tables of zs_xfade_gather for a batch decoded in overlapping windows (_window_items): per row of the vocoder's padded
    input [n_utt, T_max], where it comes from in a source table of decoded rows.  first[j]: the source row of the first decoded
    frame of the j-th window in chunk order (_flat), whose 8 n_j rows follow it one by one.  Frame t of utterance u lies in the
    window(s) that hold unit t // 8: one window -> i0 its row, i1 = -1; the V frames windows k and k + 1 share, at j = t - 8 a_{k+1}
    -> i0 the row in window k with w0 = u[j], i1 the row in window k + 1 with w1 = w[j] (xfade_weights(V)); behind an utterance's
    end i0 = -1.  Returns (T_max, frames per utterance, i0 int32, i1 int32, w0 fp32, w1 fp32), the tables flat [n_utt * T_max]."""
    by_utt = [[] for _ in range(n_utt)]
    for it, r0 in zip(_flat(chunks), first):
        by_utt[it.u].append((it.k, it.a, it.b, int(r0)))
    ulens = []
    for u, ws in enumerate(by_utt):
        ws.sort()
        if not ws or ws[0][1] != 0:
            raise ValueError('utterance %d has no window that starts at its first unit' % u)
        ulens.append(8 * ws[-1][2])
    Tm = max(ulens)
    i0 = np.full((n_utt, Tm), -1, dtype=np.int32)
    i1 = np.full((n_utt, Tm), -1, dtype=np.int32)
    w0 = np.zeros((n_utt, Tm), dtype=np.float32)
    w1 = np.zeros((n_utt, Tm), dtype=np.float32)
    for u, ws in enumerate(by_utt):
        done = 0                                              # the frames the windows so far cover
        for _, a, b, r0 in ws:
            lo, hi = 8 * a, 8 * b
            if not lo <= done < hi:
                raise ValueError('utterance %d: the window of units [%d, %d) does not continue the %d frames before it' % (u, a, b, done))
            V = done - lo                                     # shared with the window before
            if V:
                if (i1[u, lo:done] >= 0).any():
                    raise ValueError('utterance %d: a frame of the window of units [%d, %d) lies in three windows' % (u, a, b))
                w, uw = xfade_weights(V)
                i1[u, lo:done] = np.arange(r0, r0 + V, dtype=np.int32)
                w0[u, lo:done], w1[u, lo:done] = uw, w
            i0[u, done:hi] = np.arange(r0 + V, r0 + hi - lo, dtype=np.int32)
            done = hi
    return Tm, ulens, i0.reshape(-1), i1.reshape(-1), w0.reshape(-1), w1.reshape(-1)


def _upload_tables(starts, lens, chunks, dev):
    """The (start int64, len int32) tables of a plan, over all fragments in chunk order, to the device in one copy each; returns
    per chunk its views (start, len)."""
    sizes = [len(chunk) for chunk, _ in chunks]
    st_d = torch.split(torch.from_numpy(starts).to(dev, non_blocking=True), sizes)
    ln_d = torch.split(torch.from_numpy(lens).to(dev, non_blocking=True), sizes)
    return list(zip(st_d, ln_d))


GEN_COMBINE = {'naive': 1, 'targeted': 1, 'spectrogram': 1, 'targeted_residual': 2}     # zs_gen_scatter modes (trainer.py:206-213)


def _check_speaker_range(speakers, n_spk):
    """An id outside a speaker embedding table would be read past on the GPU."""
    bad = [int(s) for s in speakers if not 0 <= int(s) < n_spk]
    if bad:
        raise ValueError('speaker id %d is outside [0, n_speakers = %d)' % (bad[0], n_spk))


def check_gen_targets(trainer, speakers):
    """test_step's target check (trainer.py:202-203) for a whole batch, on the host, before anything is enqueued: a generator other
    than 'naive' only converts to the target speakers [shift, shift + n_target_speakers); 'naive' takes any id below n_speakers
    (an id outside its embedding table would be read past on the GPU).  Returns the shift subtracted from the targets."""
    if trainer.g_mode not in GEN_COMBINE:
        raise NotImplementedError('g_mode %r has no batched conversion path' % trainer.g_mode)
    n_spk = int(trainer.hps.n_speakers)
    _check_speaker_range(speakers, n_spk)
    if trainer.g_mode == 'naive':
        return 0
    shift = n_spk - int(trainer.hps.n_target_speakers)
    if any(not shift <= int(s) < shift + int(trainer.Generator.c_a) for s in speakers):
        raise RuntimeError('This generator can only convert to target speakers!')
    return shift


def _decode_chunk(trainer, ci, utts, lens_p, decode_speakers, enc_only, gen_plan, rows):
    """The decode half of one chunk, shared by _enqueue_encode and synth_units_batch: the Decoder and, with the generator
    (enc_only=False), the generator and zs_gen_scatter into gen_plan's buffer.  utts: the utterance of each fragment; lens_p: encoded
    frames per fragment of a ragged chunk, None for a plain one; rows(ch, lens_p) -> (bits, x_dec) as Decoder.forward_rows returns
    them; gen_plan = (conv, dsts, shift, denorm).  Returns a copy of the decoded rows [n, 8 T', 513] (enc_only), else None."""
    dev = trainer.device
    ch = torch.tensor([decode_speakers[u] for u in utts], dtype=torch.int64).to(dev, non_blocking=True)
    # the engines directly (the modules would clone their outputs): x_dec and the generator's rows are read in place
    bits, xr = rows(ch, lens_p)
    if enc_only:
        return xr.valid().clone(memory_format=torch.contiguous_format)
    conv, dsts, shift, denorm = gen_plan
    gen = trainer.Generator._engine()
    cg = (ch - shift) if shift else ch                                       # trainer.py:207-213
    if trainer.g_mode == 'spectrogram':                                      # G(x_dec, c - shift), T = 8 T' frames per sample
        m = gen.forward(xr, cg, False, lengths=([8 * n for n in lens_p] if lens_p is not None else None))
    else:                                                                    # G(enc, c [- shift]) on the decoder's own input
        m = gen.forward(bits, cg, False, lengths=lens_p)
    dst = dsts[ci]
    if dst.numel() != xr.B * xr.T or m.B * m.T != xr.B * xr.T:
        raise L.ZsError('conversion chunk %d: %d destination rows for %d output rows' % (ci, dst.numel(), xr.B * xr.T))
    L.call('zs_gen_scatter', 'ZsGenScatter', torch.cuda.current_stream(dev).cuda_stream, xd=xr.ptr(), ld_xd=xr.ld, m=m.ptr(),
           ld_m=m.ld, dst=L.ptr(dst), rows=dst.numel(), amp=L.ptr(conv), amp_ld=conv.shape[2], amp_rows=conv.shape[0] * conv.shape[1],
           mode=GEN_COMBINE[trainer.g_mode], denorm=int(denorm))
    return None


def _check_codebook(codebook, trainer):
    """A codebook is refused before anything is enqueued for an enc_mode its kind does not serve (a vector codebook serves
    'continues' and no other mode) and for a width other than the Decoder's c_in."""
    codebook.check_mode(trainer.enc_mode)
    codebook.check_width(int(trainer.Decoder.c_in))


def _vq_index_map(chunks, n_utt):
    """Where the returned units of a batch lie in the chunks' index buffers laid end to end (chunk ci: len(chunk) x Tp rows, Tp the
    encoded frames of its longest member): utterance u's units are its fragments' in fragment order, under the MIN_LEN truncation of
    _pack_tables.  Returns (row offsets of the utterances int64 [n_utt + 1], the source row of every unit int64)."""
    uoffs, starts, lens = _pack_tables(chunks, n_utt)
    src = np.empty(int(uoffs[-1]), dtype=np.int64)
    j, base = 0, 0
    for chunk, _ in chunks:
        Tp = _t8(max(it.n for it in chunk))
        for i in range(len(chunk)):
            src[starts[j]:starts[j] + lens[j]] = np.arange(base + i * Tp, base + i * Tp + lens[j])
            j += 1
        base += len(chunk) * Tp
    return uoffs, src


def _launch_units_pack(enc, n_frag, tabs, packed, dev):
    """zs_units_pack of the Encoder's last chunk -- the engine's own bits buffer, read in place -- into the rows tabs = (start, len)
    give each of its n_frag fragments in `packed` (uint8 [n_units, row_bytes])."""
    bits = enc._last_bits
    L.call('zs_units_pack', 'ZsUnitsPack', torch.cuda.current_stream(dev).cuda_stream, dtype=enc._zs['ctx'].dt, src_f32=0,
           src=bits.ptr(), ld_src=bits.ld, n_frag=n_frag, T=bits.T, E=enc.enc_size, start=L.ptr(tabs[0]), len=L.ptr(tabs[1]),
           packed=L.ptr(packed), n_units=packed.shape[0], row_bytes=packed.shape[1])


def _snap_units(codebook, packed, dev, to_host):
    """Snaps the packed units of a whole batch in place, once.  Returns the pinned host copies (codeword index of every unit int32,
    summed distance int64 [1]) when to_host, else (None, None); nothing is waited for."""
    idx_dev = torch.empty(packed.shape[0], dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    codebook.snap_(packed, idx=idx_dev, total=total)
    return (_to_host(idx_dev), _to_host(total)) if to_host else (None, None)


_NO_UNITS = "enc_mode 'continues' has no units: its encodings are real-valued and cannot be synthesised from unit files"


class _Units(object):
    """What conversion does with units under a codebook of one kind (the codebook's units() hands one out per batch or folder run):
    the three points of a batch of _enqueue_encode (plan, operand, finish), the encodings _assemble returns, what _synth_batch
    speaks (check_rows, after_upload), and what the folder drivers read, speak and write.  decoder_over(dec, buf) is the one place
    where a kind builds the Decoder's operand over a batch's utterance-ordered device buffer in its own layout: it returns the
    fn(tab, B, T0, ch, lens_p) -> (bits, x_dec) that _enqueue_synth calls per chunk.  _BitUnits, _VectorUnits and _ResidualUnits
    answer the same calls."""

    keep_units = False                            # finish leaves the utterance-ordered device buffer of the units in q.units_dev
    segment = None                                # lambda of --segment: finish chooses the batch's paths (zs_amd.segment), not its argmins

    def __init__(self, codebook):
        self.cb = codebook

    def check_speakable(self, enc_mode):
        pass

    def after_upload(self, dec, rows_dev):
        """Behind the one H2D copy of check_rows' arrays: (decoder_over them, the pinned indices and distance of a snap or None, None)."""
        return self.decoder_over(dec, rows_dev), None, None

    def speak(self, units, trainer, seg_len, speakers, **kw):
        """A batch of what read_unit_file reads, spoken: _synth_batch with this kind (kw: its keywords)."""
        return _synth_batch(self, units, trainer, seg_len, speakers, **kw)

    def spoken_stem(self, stem):
        """The stem of the wav a unit file of that stem speaks as."""
        return stem

    def write_idx(self, path, idx):
        """An utterance's codeword indices as the .idx.txt beside its unit file."""
        write_indices(path, idx)

    def path_indices(self, rows_dev, segment):
        """The indices int32 (host) of the path --segment chooses for ONE utterance whose rows, in the form this kind's scores_ reads,
        are on the device."""
        scores = torch.empty(rows_dev.shape[0], self.cb.K, dtype=torch.float32, device=rows_dev.device)
        self.cb.scores_(rows_dev, scores)
        return sg.viterbi(scores, np.asarray([0, rows_dev.shape[0]]), segment)[0].cpu().numpy()


class _BitUnits(_Units):
    """Under a bit codebook (zs_amd.codebook.Codebook).  codebook None: plain unit files, which synth_dir reads and speaks as it does
    under a bit codebook."""
    packs = True                                  # the batch's units are bit-packed: a bit codebook implies pack
    unit_glob = '*.txt'
    who = 'synth_units_batch'
    packed_rows = want_idx = True                 # speak takes packed rows and returns the indices of a snap; synth_units_batch: as asked

    def check_rows(self, units, trainer):
        """The utterances as packed rows (uint8 [U_i, (E + 7) // 8]), checked on the host: ValueError for a width other than E, a value
        other than 0 / 1 (packed: a bit set above column E) and an utterance of fewer than 2 units; then the codebook's own checks."""
        E = int(trainer.Decoder.c_in)
        row_bytes = (E + 7) // 8
        out = []
        for i, u in enumerate(units):
            a = np.asarray(u.cpu() if torch.is_tensor(u) else u)
            if self.packed_rows:
                if a.dtype != np.uint8 or a.ndim != 2 or a.shape[1] != row_bytes:
                    raise ValueError("utterance %d: packed units must be uint8 [U, %d] for the Decoder's %d columns (got %s %s)" %
                                     (i, row_bytes, E, a.dtype, a.shape))
                if E % 8 and (a[:, -1] >> (E % 8)).any():
                    raise ValueError('utterance %d: packed units have a bit set above column %d' % (i, E))
            else:
                if a.ndim != 2 or a.shape[1] != E:
                    raise ValueError("utterance %d: units must be [U, %d], the Decoder's input width (got shape %s)" % (i, E, a.shape))
                try:
                    a = pack_units(a)
                except ValueError:
                    raise ValueError('utterance %d: units must be 0 or 1' % i)
            if a.shape[0] < 2:
                raise ValueError('utterance %d has fewer than 2 units (the Decoder needs two rows; the one-unit files written for inputs '
                                 'shorter than MIN_LEN frames were decoded from two units and cannot be reproduced)' % i)
            out.append(np.ascontiguousarray(a))
        if self.cb is not None:
            _check_codebook(self.cb, trainer)
        return out

    def after_upload(self, dec, packed_dev):
        """The one buffer snapped once, in place, before the first chunk."""
        idx_h = total_h = None
        if self.cb is not None:
            idx_h, total_h = _snap_units(self.cb, packed_dev, packed_dev.device, to_host=self.want_idx)
        return self.decoder_over(dec, packed_dev), idx_h, total_h

    def decoder_over(self, dec, packed_dev):
        """Over packed rows, uint8 [units, row_bytes]: zs_units_unpack writes each chunk's Decoder operand."""
        return lambda tab, B, T0, ch, lens_p: dec.forward_units(packed_dev, tab[0], tab[1], B, T0, ch, lengths=lens_p)

    def plan(self, q, chunks, decoding, want_packed):
        """Before the chunk loop: the chunk-local tables the Decoder's operands are packed by."""
        self.want_packed = want_packed
        self.dense = _upload_tables(*_dense_tables(chunks), chunks, q.dev) if decoding else None
        if self.segment is not None:
            sg.check_budget(int(q.uoffs[-1]), self.cb.K)

    def operand(self, ci, chunk, Tm, enc, act, dec, dev):
        """Behind the encoder's launches of chunk ci: the chunk's units -> chunk-local packed rows -> zs_code_assign in place.
        Returns rows(ch, lens_p) for _decode_chunk: the Decoder's operand from the snapped rows; None when nothing is decoded."""
        if self.dense is None:
            return None
        Tp = int(act.shape[2])
        if Tp != _t8(Tm):
            raise L.ZsError('conversion chunk %d: %d encoded frames where the plan has %d' % (ci, Tp, _t8(Tm)))
        st_c, ln_c = self.dense[ci]
        snapped = torch.empty(len(chunk) * Tp, (enc.enc_size + 7) // 8, dtype=torch.uint8, device=dev)
        _launch_units_pack(enc, len(chunk), (st_c, ln_c), snapped, dev)
        self.cb.snap_(snapped)                                # rows behind a fragment's len are snapped too and never read
        return lambda ch, lens_p: dec.forward_units(snapped, st_c, ln_c, len(chunk), Tp, ch, lengths=lens_p)

    def finish(self, q, units_dev):
        """Behind the last chunk: the utterance buffer snapped once, in place (the same rows, the same codewords).
        segment: zs_code_scores over that buffer, ONE zs_seg_viterbi over the batch, and the rows become the codewords of the path;
        q.cb_total is the summed distance of the path."""
        if self.segment is not None:
            scores = torch.empty(units_dev.shape[0], self.cb.K, dtype=torch.float32, device=q.dev)
            self.cb.scores_(units_dev, scores)
            idx, _, _ = sg.viterbi(scores, q.uoffs, self.segment)
            at = idx.long()
            units_dev.copy_(self.cb.to(q.dev)[at])
            q.idx_host = _to_host(idx)
            q.cb_total = _to_host(scores.gather(1, at[:, None]).sum(dtype=torch.float64).to(torch.int64).reshape(1))
            q.seg_scores, q.seg_row = scores, None
            return
        q.idx_host, q.cb_total = _snap_units(self.cb, units_dev, q.dev, to_host=True)

    def encodings(self, q, u):
        """Utterance u's snapped units, in the form the caller asked for."""
        rows = q.units_host.numpy()[q.uoffs[u]:q.uoffs[u + 1]]
        return rows.copy() if self.want_packed else unpack_units(rows, self.cb.E)

    def check_speakable(self, enc_mode):
        if enc_mode == 'continues':
            raise ValueError(_NO_UNITS)

    def read_unit_file(self, path, E):
        return pack_units(read_units(path, E))

    def spoken(self, res, units):
        """(the indices spoken per utterance, the summed distance) of a batch speak() has finished (res) from `units`."""
        return res[2], res[3]

    def write_spoken(self, base, idx, E):
        """What was spoken, beside the wav: the codewords of the file's units and their indices."""
        write_encodings(base + '.txt', unpack_units(self.cb.packed[idx], E))
        write_indices(base + '.idx.txt', idx)

    def from_indices(self, idx):
        """What speak() takes for an utterance of these codeword indices: the packed codewords."""
        return self.cb.packed[np.asarray(idx, dtype=np.int64)]

    def write_encoded(self, txt, units, dev, segment=None):
        """--test_encode: the snapped units as the .txt, their indices beside it.  segment: the codewords and indices of the path, and
        its runs as the .seg.txt."""
        if segment is not None:
            idx = self.path_indices(torch.from_numpy(pack_units(units)).to(dev), segment)
            write_encodings(txt, unpack_units(self.cb.packed[idx], self.cb.E))
            write_indices(idx_path(txt), idx)
            sg.write_segments(sg.seg_path(txt), sg.runs(idx))
            return
        idx, snapped = self.cb.snap_host(pack_units(units))
        write_encodings(txt, unpack_units(snapped, self.cb.E))
        write_indices(idx_path(txt), idx)


class _VectorUnits(_Units):
    """Under a vector codebook (zs_amd.vq.VectorCodebook, enc_mode 'continues'): nothing is packed, the units are codeword indices
    and the unit files are <name>.idx.txt."""
    packs = False
    unit_glob = '*.idx.txt'
    who = 'synth_index_batch'

    def check_rows(self, idx_lists, trainer):
        """The utterances of synth_index_batch as contiguous int32 arrays, checked on the host: ValueError for a shape or dtype other
        than the kind's, fewer than 2 rows and an index outside [0, K)."""
        rows = []
        for i, seq in enumerate(idx_lists):
            a = np.asarray(seq.cpu() if torch.is_tensor(seq) else seq)
            self._check_shape(i, a, rows)
            if a.shape[0] < 2:
                raise ValueError('utterance %d has fewer than 2 indices (the Decoder needs two rows)' % i)
            if (a < 0).any() or (a >= self.cb.K).any():
                raise ValueError('utterance %d: an index is outside [0, K = %d)' % (i, self.cb.K))
            rows.append(np.ascontiguousarray(a.astype(np.int32)))
        return rows

    def _check_shape(self, i, a, rows):
        if a.ndim != 1 or a.dtype.kind not in 'iu':
            raise ValueError('utterance %d: indices must be a 1-D integer sequence (got %s %s)' % (i, a.dtype, a.shape))

    def decoder_over(self, dec, idx_dev):
        """Over indices, int32 [units]: zs_vq_gather writes each chunk's Decoder operand from the codewords."""
        code_d, _ = self.cb.to(idx_dev.device)
        bad = torch.zeros(1, dtype=torch.int32, device=idx_dev.device)
        return lambda tab, B, T0, ch, lens_p: dec.forward_indices(idx_dev, code_d, tab[0], tab[1], B, T0, ch, bad, lengths=lens_p)

    def plan(self, q, chunks, decoding, want_packed):
        """Before the chunk loop: the codebook and the workspace on the device, and where the returned units will lie."""
        from .vq import workspace
        self.dense = _upload_tables(*_dense_tables(chunks), chunks, q.dev) if decoding else None
        self.code, self.cnorm = self.cb.to(q.dev)
        self.work, self.idx, self.dist = workspace(q.dev), [], []
        self.bad = torch.zeros(1, dtype=torch.int32, device=q.dev)
        q.uoffs, src = _vq_index_map(chunks, q.n_utt)
        self.src = torch.from_numpy(src).to(q.dev, non_blocking=True)
        if self.segment is not None:                          # the scores of every chunk row, in chunk order (what _vq_index_map indexes)
            rows = sum(len(chunk) * _t8(max(it.n for it in chunk)) for chunk, _ in chunks)
            sg.check_budget(rows, self.cb.K)
            self.scores = torch.empty(rows, self.cb.K, dtype=torch.float32, device=q.dev)
            self.base, self.xn = 0, []

    def operand(self, ci, chunk, Tm, enc, act, dec, dev):
        """Behind the encoder's launches of chunk ci: the kind's _assign over the chunk's rows, read in place from the engine's output.
        Returns rows(ch, lens_p) for _decode_chunk: the kind's gather builds the Decoder's operand from the chunk's own indices.
        segment: zs_vq_scores in its place, into the chunk's rows of the batch's score buffer (and the rows' squared norms, for the
        distance of the path); nothing is decoded."""
        bits = enc._last_bits
        Tp = int(bits.T)
        if Tp != _t8(Tm) or int(bits.B) != len(chunk):
            raise L.ZsError('conversion chunk %d: %d x %d encoded frames where the plan has %d x %d' % (ci, bits.B, Tp, len(chunk), _t8(Tm)))
        st, dt, n = torch.cuda.current_stream(dev).cuda_stream, enc._zs['ctx'].dt, len(chunk) * Tp
        if self.segment is not None:
            from .vq import launch_scores
            launch_scores(st, dt, bits.ptr(), n, bits.ld, self.code, self.cnorm, L.ptr(self.scores, self.base * self.cb.K), self.cb.K)
            self.xn.append(bits.valid().float().pow(2).sum(-1).reshape(-1))
            self.base += n
            return None
        idx_c, dist_c, forward = self._assign(st, dt, bits, n, dec, dev)
        self.idx.append(idx_c)
        self.dist.append(dist_c)
        if self.dense is None:
            return None
        st_c, ln_c = self.dense[ci]
        return lambda ch, lens_p: forward(st_c, ln_c, len(chunk), Tp, ch, self.bad, lengths=lens_p)

    def _assign(self, st, dt, bits, n, dec, dev):
        """zs_vq_assign over the n rows of `bits`.  Returns (indices, distances, the Decoder's forward over them: zs_vq_gather)."""
        from .vq import launch_assign
        idx_c = torch.empty(n, dtype=torch.int32, device=dev)
        dist_c = torch.empty(n, dtype=torch.float32, device=dev)
        launch_assign(st, dt, bits.ptr(), n, bits.ld, self.code, self.cnorm, idx=idx_c, dist=dist_c, work=self.work)
        return idx_c, dist_c, lambda *a, **kw: dec.forward_indices(idx_c, self.code, *a, **kw)

    def finish(self, q, units_dev):
        """Behind the last chunk: the chunks' indices into utterance order, then one copy.  The batch's device buffers go with it.
        segment: ONE zs_seg_viterbi over the batch's score buffer through the row table of _vq_index_map gives the indices, already
        in utterance order; q.cb_total is the summed distance of the path, max(0, |x|^2 + score) per unit."""
        if self.segment is not None:
            idx, _, _ = sg.viterbi(self.scores, q.uoffs, self.segment, row=self.src)
            q.idx_host = _to_host(idx)
            if self.keep_units:
                q.units_dev = idx
            xn = torch.cat(self.xn) if len(self.xn) > 1 else self.xn[0]
            path = self.scores[self.src, idx.long()]
            q.cb_total = _to_host((xn[self.src] + path).clamp_(min=0).sum(dtype=torch.float64).reshape(1))
            q.seg_scores, q.seg_row = self.scores, self.src
            self.scores = self.xn = self.work = self.src = self.dense = None
            return
        idx_all, dist_all = (torch.cat(self.idx), torch.cat(self.dist)) if len(self.idx) > 1 else (self.idx[0], self.dist[0])
        idx_utt = idx_all[self.src]
        q.idx_host = _to_host(idx_utt)
        if self.keep_units:                                   # spoken from behind this batch (resynth_batch(overlap=...)): int32 [units]
            q.units_dev = idx_utt
        q.cb_total = _to_host(dist_all[self.src].sum(dtype=torch.float64).reshape(1))
        self.idx = self.dist = self.work = self.src = self.dense = None

    def encodings(self, q, u):
        """Utterance u's encodings: the codewords of its indices."""
        return self.cb.vectors[q.idx_host.numpy()[q.uoffs[u]:q.uoffs[u + 1]]]

    def read_unit_file(self, path, E):
        return read_indices(path, self.cb.K)

    def spoken_stem(self, stem):
        return stem[:-len('.idx')]                            # <name>.idx.txt speaks as <name>.wav

    def spoken(self, res, units):
        return units, 0.0                                     # the file's own indices: nothing was snapped

    def write_spoken(self, base, idx, E):
        write_indices(base + '.idx.txt', idx)

    def from_indices(self, idx):
        return np.asarray(idx, dtype=np.int32)

    def write_encoded(self, txt, units, dev, segment=None):
        """--test_encode: the .txt as without a codebook, the nearest codeword of every encoded frame beside it.  segment: the
        indices of the path instead, and its runs as the .seg.txt."""
        x = torch.from_numpy(np.ascontiguousarray(units, dtype=np.float32)).to(dev)
        write_encodings(txt, units)
        if segment is not None:
            idx = self.path_indices(x, segment)
            write_indices(idx_path(txt), idx)
            sg.write_segments(sg.seg_path(txt), sg.runs(idx))
            return
        idx, _ = self.cb.snap(x)
        write_indices(idx_path(txt), idx.cpu().numpy())


class _ResidualUnits(_VectorUnits):
    """Under a residual codebook (zs_amd.rvq.ResidualCodebook, enc_mode 'continues'): the units of a frame are the indices of its
    first s' stages, one row of s' columns, and the unit files are <name>.idx.txt with that row per line.  stages: s' (None: every
    stage for conversion, a file's own columns for synthesis)."""

    def __init__(self, codebook, stages=None):
        from .rvq import check_stages
        super(_ResidualUnits, self).__init__(codebook)
        self.stages = None if stages is None else check_stages(stages, codebook.S, '--rvq_stages')
        self.s_use = codebook.S if self.stages is None else self.stages

    def _check_shape(self, i, a, rows):
        if a.ndim != 2 or a.dtype.kind not in 'iu' or not 1 <= a.shape[1] <= self.cb.S:
            raise ValueError('utterance %d: indices must be integers [U, 1 .. S = %d] (got %s %s)' % (i, self.cb.S, a.dtype, a.shape))
        if rows and a.shape[1] != rows[0].shape[1]:
            raise ValueError('utterance %d has %d indices per frame where utterance 0 has %d' % (i, a.shape[1], rows[0].shape[1]))

    def after_upload(self, dec, rows_dev):
        """The batch's rows [units, c] as c planes, every column used: decoder_over makes the transposed view contiguous."""
        return self.decoder_over(dec, rows_dev.t()), None, None

    def decoder_over(self, dec, planes):
        """Over planes, int32 [s', units] (a strided view is copied once, behind the codebook's upload and the `bad` word):
        zs_rvq_gather writes each chunk's Decoder operand as the sum of the s' stages' codewords."""
        code_d, _ = self.cb.to(planes.device)
        bad = torch.zeros(1, dtype=torch.int32, device=planes.device)
        planes = planes.contiguous()
        return lambda tab, B, T0, ch, lens_p: dec.forward_index_planes(planes, planes.shape[0], code_d, tab[0], tab[1], B, T0, ch, bad,
                                                                       lengths=lens_p)

    def plan(self, q, chunks, decoding, want_packed):
        """_VectorUnits.plan, and the one fp32 residual buffer of the batch: the rows of its largest chunk."""
        super(_ResidualUnits, self).plan(q, chunks, decoding, want_packed)
        rows = max(len(chunk) * _t8(max(it.n for it in chunk)) for chunk, _ in chunks)
        self.resid = torch.empty(rows if self.s_use > 1 else 0, self.cb.E, dtype=torch.float32, device=q.dev)

    def _assign(self, st, dt, bits, n, dec, dev):
        """Stage 0 is zs_vq_assign over the n rows of `bits`; zs_rvq_residual writes what it leaves into the fp32 buffer, and every
        further stage assigns on that buffer and subtracts in place.  Returns (the planes, the distances behind every stage, the
        Decoder's forward over the planes: zs_rvq_gather)."""
        from .rvq import launch_residual
        from .vq import launch_assign
        E, s_use = self.cb.E, self.s_use
        idx_c = torch.empty(s_use, n, dtype=torch.int32, device=dev)
        dist_c = torch.empty(s_use, n, dtype=torch.float32, device=dev)
        launch_assign(st, dt, bits.ptr(), n, bits.ld, self.code[0], self.cnorm[0], idx=idx_c[0], dist=dist_c[0], work=self.work)
        r = L.ptr(self.resid)
        for s in range(1, s_use):
            if s == 1:
                launch_residual(st, dt, 0, bits.ptr(), n, bits.ld, idx_c[0], self.code[0], r, E, self.bad)
            else:
                launch_residual(st, L.ZS_F32, 1, r, n, E, idx_c[s - 1], self.code[s - 1], r, E, self.bad)
            launch_assign(st, L.ZS_F32, r, n, E, self.code[s], self.cnorm[s], idx=idx_c[s], dist=dist_c[s], work=self.work)
        return idx_c, dist_c, lambda *a, **kw: dec.forward_index_planes(idx_c, s_use, self.code, *a, **kw)

    def finish(self, q, units_dev):
        """Behind the last chunk: the planes into utterance order (_vq_index_map), then one copy: q.idx_host int32 [units, s'], a row per
        frame, and q.cb_total double [s'], the summed squared distance left behind every stage (the last: that of the units written)."""
        idx_all, dist_all = (torch.cat(self.idx, dim=1), torch.cat(self.dist, dim=1)) if len(self.idx) > 1 else (self.idx[0], self.dist[0])
        planes = idx_all[:, self.src]
        q.idx_host = _to_host(planes.t().contiguous())
        if self.keep_units:                                   # as _VectorUnits.finish: the planes int32 [s', units]
            q.units_dev = planes
        q.cb_total = _to_host(dist_all[:, self.src].sum(dim=1, dtype=torch.float64))
        self.idx = self.dist = self.work = self.src = self.dense = self.resid = None

    def encodings(self, q, u):
        """Utterance u's encodings: the sums of the codewords of its indices (ResidualCodebook.reconstruct)."""
        return self.cb.reconstruct(q.idx_host.numpy()[q.uoffs[u]:q.uoffs[u + 1]].T)

    def read_unit_file(self, path, E):
        """int32 [U, c] of the file, cut to the first s' columns when s' is given; a file of fewer columns is refused."""
        rows = read_index_rows(path, self.cb.K, self.cb.S)
        if self.stages is not None and rows.shape[1] < self.stages:
            raise ValueError('%s holds c = %d indices per line, fewer than the s = %d stages asked for (--rvq_stages)'
                             % (path, rows.shape[1], self.stages))
        return rows if self.stages is None else np.ascontiguousarray(rows[:, :self.stages])

    def speak(self, units, trainer, seg_len, speakers, **kw):
        """Files of different widths (no s' given: each speaks with its own columns) are spoken width by width, and the results come
        back in the order given."""
        one = super(_ResidualUnits, self).speak
        widths = sorted({int(u.shape[1]) for u in units})
        if len(widths) == 1:
            return one(units, trainer, seg_len, speakers, **kw)
        parts = []
        for c in widths:
            sel = [i for i, u in enumerate(units) if u.shape[1] == c]
            parts.append((sel, one([units[i] for i in sel], trainer, seg_len, [speakers[i] for i in sel], **kw)))

        def finish():
            specs, wavs = [None] * len(units), [None] * len(units)
            for sel, res in parts:
                res = res() if callable(res) else res
                for j, i in enumerate(sel):
                    wavs[i] = res[1][j]
                    if res[0] is not None:
                        specs[i] = res[0][j]
            return (specs if any(s is not None for s in specs) else None), wavs
        return finish if kw.get('defer') else finish()

    def write_idx(self, path, idx):
        write_index_rows(path, idx)

    def write_spoken(self, base, idx, E):
        write_index_rows(base + '.idx.txt', idx)

    def write_encoded(self, txt, units, dev):
        """--test_encode: the .txt as without a codebook, the s' indices of every encoded frame beside it."""
        idx, _ = self.cb.snap(torch.from_numpy(np.ascontiguousarray(units, dtype=np.float32)).to(dev), stages=self.s_use)
        write_encodings(txt, units)
        write_index_rows(idx_path(txt), idx.t().cpu().numpy())


def _enqueue_encode(specs, trainer, seg_len, decode_speakers, noise_fn, max_batch, dec_to_host, enc_only=True, denorm=False, pack=False,
                    codebook=None, rows_on_device=False, keep_units=False, segment=None):
    """Fragment rule + every Encoder / Decoder launch of a batch of utterances, WITHOUT a host synchronisation: the caller decides
    what else to put on the stream (the vocoder) before it waits.
    enc_only=False (decode_speakers required): the stage-2 generator as well, and zs_gen_scatter writes every chunk's converted rows
    into q.conv right behind it (de-normalised when `denorm`): the engines reuse their output buffers for the next chunk of the
    same shape.
    pack: zs_units_pack writes every chunk's units, bit-packed, to their utterance's place in one device buffer, and ONE copy
    brings them to the host (q.units_host, q.uoffs) instead of a fp32 copy per chunk.
    codebook (zs_amd.codebook.Codebook; implies pack): every unit is snapped to its nearest codeword.  A chunk's units go encoder ->
    chunk-local packed rows -> zs_code_assign in place -> Decoder.forward_units, so the Decoder and the generator read the snapped
    units of every encoded frame; the utterance buffer is snapped once, in place, behind the last chunk (the same rows, the same
    codewords) with the index of every unit (q.idx_host) and the summed distance (q.cb_total).
    codebook a zs_amd.vq.VectorCodebook (enc_mode 'continues'; nothing is packed): a chunk goes encoder -> zs_vq_assign over the
    chunk's rows, read in place from the engine's output -> zs_vq_gather (Decoder.forward_indices) -> the Decoder's launches; the
    chunks' indices are brought into utterance order on the device (_vq_index_map) and copied once (q.idx_host), with the summed
    squared distance of the returned units (q.cb_total, a double), and the encodings returned are the codewords of the indices.
    rows_on_device: the fp32 encodings stay on the device (q.enc_dev, one tensor per chunk) instead of being copied to the host.
    keep_units: under a vector or residual codebook the utterance-ordered device buffer of the indices, which the copy to the host is
    made from, stays in q.units_dev (bit-packed units are there whenever they are packed), in the layout q.uoffs describes.
    segment (lambda >= 0; needs a bit or vector codebook and no decode): the units of the batch are the codewords of the paths
    zs_seg_viterbi chooses, one launch behind the last chunk, over the scores of the batch (zs_amd.segment): zs_vq_scores
    per chunk where zs_vq_assign runs without it, or zs_code_scores over the utterance-ordered packed buffer.  q.seg_scores and
    q.seg_row keep the score buffer and its row table (None: unit i is row i)."""
    if segment is not None:
        segment = sg.check_lambda(segment, 'segment')
        sg.check_codebook(codebook, 'segment')
        if decode_speakers is not None:
            raise ValueError('segment: the paths are chosen behind the last chunk, so nothing is decoded beside the encoder: '
                             'resynth_batch(segment=...) speaks the units of the paths')
    side = None                                               # what the codebook's kind does to this batch (_BitUnits, _VectorUnits)
    if codebook is not None:
        _check_codebook(codebook, trainer)
        if int(trainer.Encoder.enc_size) != codebook.E:
            raise ValueError("codebook field E is %d, the Encoder's enc_size is %d" % (codebook.E, int(trainer.Encoder.enc_size)))
        side, want_packed = codebook.units(), pack
        side.keep_units = bool(keep_units)
        side.segment = segment
        pack = pack or side.packs
    if pack and trainer.enc_mode == 'continues':
        raise ValueError("enc_mode 'continues' has no units to pack (its encodings are not 0 / 1)")
    if not enc_only:
        if decode_speakers is None:
            raise ValueError('conversion with the generator (enc_only=False) needs the target speakers')
        shift = check_gen_targets(trainer, decode_speakers)
    trainer.set_eval()
    enc, dec = trainer.Encoder, trainer.Decoder
    dev = trainer.device
    items, padded = [], []
    for u, spec in enumerate(specs):
        if torch.is_tensor(spec) and spec.is_cuda:
            was_padded = spec.shape[0] < MIN_LEN
            if was_padded:
                spec = torch.nn.functional.pad(spec, (0, 0, 0, MIN_LEN - spec.shape[0]))
        else:
            spec, was_padded = _pad_min(np.asarray(spec, dtype=np.float32))
        padded.append(spec)
        items += _frame_items(u, len(spec), seg_len, was_padded)
    chunks = _split_chunks(items, seg_len, max_batch)
    # every utterance goes to the device once, whole; the fragments are gathered there (row index tables, a few hundred KB)
    rows, offs = _stage_rows(padded, dev)
    zero_row = int(offs[-1])
    q = _Enqueued()
    q.n_utt, q.dev, q.chunks, q.enc_host, q.dec_dev, q.dec_host = len(specs), dev, [], [], [], []
    gen_plan = None
    if not enc_only:
        q.conv, q.ulens, dsts = _plan_scatter(chunks, len(specs), denorm, dev)
        gen_plan = (q.conv, dsts, shift, denorm)
    if pack:
        q.uoffs, starts, counts = _pack_tables(chunks, len(specs))
        pack_tabs = _upload_tables(starts, counts, chunks, dev)
        row_bytes = (enc.enc_size + 7) // 8
        units_dev = torch.empty(int(q.uoffs[-1]), row_bytes, dtype=torch.uint8, device=dev)
    if side is not None:
        side.plan(q, chunks, decode_speakers is not None, want_packed)
    for ci, (chunk, ragged) in enumerate(chunks):
        lens = [it.n for it in chunk]
        Tm = max(lens)
        idx = np.full((len(chunk), Tm), zero_row, dtype=np.int64)
        for i, it in enumerate(chunk):
            idx[i, :it.n] = np.arange(offs[it.u] + it.a, offs[it.u] + it.b)
        x = rows[torch.from_numpy(idx).to(dev, non_blocking=True)]                                     # [n, Tm, 513]
        G = noise_fn(len(chunk), _t8(Tm), enc.enc_size) if noise_fn is not None else None
        act, _ = enc(x.permute(0, 2, 1), G=G, lengths=(lens if ragged else None))
        xd = None
        if side is not None:                                  # the snap of the chunk, and the Decoder's operand from what it gave
            rows_fn = side.operand(ci, chunk, Tm, enc, act, dec, dev)
        else:
            rows_fn = lambda ch, lens_p: dec.forward_rows(act, ch, lengths=lens_p)
        if decode_speakers is not None:
            xd = _decode_chunk(trainer, ci, [it.u for it in chunk], ([_t8(n) for n in lens] if ragged else None), decode_speakers,
                               enc_only, gen_plan, rows_fn)
        q.chunks.append((chunk, lens))
        if pack:
            _launch_units_pack(enc, len(chunk), pack_tabs[ci], units_dev, dev)
            q.enc_host.append(None)
        elif side is not None:                                # the encodings returned come from the codebook (side.encodings)
            q.enc_host.append(None)
        elif rows_on_device:                                  # the fp32 rows stay where they are (q.enc_dev): no copy to the host
            q.enc_host.append(None)
            q.enc_dev = (q.enc_dev or []) + [act.permute(0, 2, 1).contiguous()]
        else:
            q.enc_host.append(_to_host(act.permute(0, 2, 1).contiguous()))
        q.dec_dev.append(xd)
        q.dec_host.append(_to_host(xd) if (xd is not None and dec_to_host) else None)
    if side is not None:                                      # the index of every returned unit and the summed distance
        side.finish(q, units_dev if pack else None)
        q.cb = side
    if pack:
        q.units_dev = units_dev
        q.units_host = _to_host(units_dev)
    q.enc_done = torch.cuda.Event()
    q.enc_done.record(torch.cuda.current_stream(dev))
    return q


def _plan_scatter(chunks, n_utt, denorm, dev, rows_of=None):
    """The converted spectrograms' buffer [n_utt, T_max, 513] and, per chunk, the device table of _scatter_tables (rows_of: see
    there).  The padding rows (frames past an utterance's length) are filled here, once: what the per-utterance path gives them,
    (denorm of) zero.  All destination tables go to the device in one copy.  Returns (buffer, frames per utterance, tables)."""
    Tm, ulens, tables, pad = _scatter_tables(chunks, n_utt, rows_of)
    sizes = [len(t) for t in tables] + [len(pad)]
    if n_utt * Tm >= 2 ** 31:
        raise ValueError('converted batch too large: %d rows' % (n_utt * Tm))
    dev_t = torch.from_numpy(np.concatenate(tables + [pad])).to(dev, non_blocking=True)
    parts = list(torch.split(dev_t, sizes))
    conv = torch.empty(n_utt, Tm, 513, dtype=torch.float32, device=dev)
    if len(pad):
        zero = torch.zeros(513, dtype=torch.float32, device=dev)
        L.call('zs_gen_scatter', 'ZsGenScatter', torch.cuda.current_stream(dev).cuda_stream, xd=L.ptr(zero), ld_xd=0, dst=L.ptr(parts[-1]),
               rows=len(pad), amp=L.ptr(conv), amp_ld=513, amp_rows=n_utt * Tm, mode=0, denorm=int(denorm))
    return conv, ulens, parts[:-1]


def _assemble(q, want_dec):
    """Per-utterance encodings (and decoded spectrograms: 'host', 'device' or None) from the chunk outputs, in fragment order.
    The caller has waited for the copies."""
    enc_out, dec_out = {}, {}
    units = q.units_host.numpy() if q.units_host is not None else None      # packed: one buffer, utterance by utterance
    for ci, (chunk, lens) in enumerate(q.chunks):
        e = q.enc_host[ci].numpy() if q.enc_host[ci] is not None else None
        xd = None
        if want_dec == 'host':
            xd = q.dec_host[ci].numpy()
        elif want_dec == 'device':
            xd = q.dec_dev[ci]
        for i, it in enumerate(chunk):
            tp = _t8(lens[i])
            enc_out[(it.u, it.k)] = None if e is None else (e[i][:it.trunc] if it.trunc is not None else e[i][:tp])
            if xd is not None:
                dec_out[(it.u, it.k)] = xd[i][:8 * tp]
    by_utt = {}
    for (u, k) in enc_out:
        by_utt.setdefault(u, []).append(k)
    encs, decs = [], ([] if want_dec else None)
    for u in range(q.n_utt):
        ks = sorted(by_utt[u])
        if q.cb is not None:                                  # a codebook: what its kind returns for the snapped units
            encs.append(q.cb.encodings(q, u))
        elif units is None:
            encs.append(np.concatenate([enc_out[(u, k)] for k in ks], axis=0))
        else:
            encs.append(units[q.uoffs[u]:q.uoffs[u + 1]].copy())
        if decs is not None:
            parts = [dec_out[(u, k)] for k in ks]
            decs.append(np.concatenate(parts, axis=0) if want_dec == 'host' else (parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)))
    return encs, decs


def _unit_indices(idx_host, cb_total, uoffs):
    """Per utterance the codeword index of every returned unit (int32 [U_i]) and the summed distance, from _snap_units' host copies
    (which have been waited for) and the utterances' row offsets."""
    idx, total = idx_host.numpy(), cb_total.numpy()[0]
    if cb_total.numel() > 1:                                  # a residual codebook: [U_i, s'] indices, the distance left behind every stage
        return [idx[uoffs[u]:uoffs[u + 1]].copy() for u in range(len(uoffs) - 1)], cb_total.numpy().astype(np.float64)
    return [idx[uoffs[u]:uoffs[u + 1]].copy() for u in range(len(uoffs) - 1)], (float(total) if total.dtype.kind == 'f' else int(total))


def encode_rows_on_device(specs, trainer, seg_len, noise_fn=None, max_batch=256):
    """encode_batch's encodings as fp32 device tensors [U_i, E], one per utterance, under the same fragment and truncation rules:
    the encoder's rows never visit the host (what a vector codebook is fitted to, zs_amd.vq.fit_dir)."""
    q = _enqueue_encode(specs, trainer, seg_len, None, noise_fn, max_batch, dec_to_host=False, rows_on_device=True)
    torch.cuda.current_stream(q.dev).synchronize()
    from . import layers
    layers.check_status(q.dev)
    parts = {}
    for (chunk, lens), e in zip(q.chunks, q.enc_dev):
        for i, it in enumerate(chunk):
            parts[(it.u, it.k)] = e[i][:(it.trunc if it.trunc is not None else _t8(lens[i]))]
    return [torch.cat([parts[k] for k in sorted(k for k in parts if k[0] == u)], dim=0) for u in range(q.n_utt)]


def encode_batch(specs, trainer, seg_len, decode_speakers=None, noise_fn=None, max_batch=256, to_host=True, enc_only=True, packed=False,
                 codebook=None, want_idx=False, units_on_device=False, segment=None):
    """Batched encode()/convert() for many utterances: the same fragments the reference would send through the network one by
    one (convert.py:151-165), as a few large batches on the GPU.
    specs: list of [T_i, 513] arrays (host arrays, or torch tensors already on the device).  decode_speakers: optional list of
    target speaker ids -> also returns the decoded spectrograms (enc_only path of convert()).  noise_fn(n_frag, T', E) -> Gumbel
    noise of the encoder mode's shape ([n, T', E, 2] multilabel_binary, [n, T', E] one_hot, [n, T', E, E] binary; None for
    continues, which draws none) or None makes the stochastic discretiser reproducible (called once per batch; T' = encoded frames of the
    longest member).  Returns (encodings list, decoded list or None); to_host=False leaves the decoded spectrograms on the
    device (torch tensors [T_out, 513]) for spectrogram2wav_batch.
    enc_only=False: convert() with the stage-2 generator (trainer.py:198-213) -- the decoded list holds the CONVERTED spectrograms
    (normalised, as test_step returns them), bit for bit the concatenated per-fragment test_step outputs given the same noise.
    packed=True: the encodings come back bit-packed, uint8 [U_i, (E + 7) // 8] as pack_units defines them -- zs_units_pack writes
    every fragment's units to its utterance's place in one device buffer and one D2H copy of E / 8 bytes per unit replaces the
    per-chunk fp32 copies of 4 E bytes per unit (ValueError for enc_mode 'continues', whose encodings are not units).
    units_on_device=True (with packed): the packed encodings are returned as device tensors, views of the one uint8 buffer.
    codebook: a zs_amd.codebook.Codebook -- every unit is snapped to its nearest codeword before the Decoder and the generator see
    it and before it is returned (under the same truncation rules, in the form `packed` asks for); want_idx=True appends the list
    of codeword indices, int32 [U_i] per utterance, to the result.  For enc_mode 'continues' a zs_amd.vq.VectorCodebook: every encoded
    frame is snapped to its nearest codeword in Euclidean distance and the encodings returned are those codewords, fp32 [U_i, E].
    segment (lambda >= 0, in the score's own units; needs a bit or vector codebook, and decode_speakers None): the units returned
    are the codewords of the path zs_seg_viterbi chooses for the whole utterance (zs_amd.segment), not of each frame
    alone; lambda = 0 gives the indices it gives without segment."""
    if want_idx and codebook is None:
        raise ValueError('encode_batch: want_idx needs a codebook')
    if units_on_device and not packed:
        raise ValueError('encode_batch: units_on_device needs packed=True')
    q = _enqueue_encode(specs, trainer, seg_len, decode_speakers, noise_fn, max_batch, dec_to_host=to_host, enc_only=enc_only,
                        pack=packed, codebook=codebook, segment=segment)
    out = _encode_result(q, decode_speakers, to_host, enc_only, units_on_device)
    return out + (_unit_indices(q.idx_host, q.cb_total, q.uoffs)[0],) if want_idx else out


def _encode_result(q, decode_speakers, to_host, enc_only, units_on_device):
    """encode_batch's wait and assembly: (encodings, decoded or converted spectrograms or None)."""
    conv_h = _to_host(q.conv) if (q.conv is not None and to_host) else None
    torch.cuda.current_stream(q.dev).synchronize()
    from . import layers
    layers.check_status(q.dev)                                # synchronised: a timed-out GRU pass raises here
    if units_on_device:
        encs_dev = [q.units_dev[q.uoffs[u]:q.uoffs[u + 1]] for u in range(q.n_utt)]
    if enc_only:
        encs, decs = _assemble(q, None if decode_speakers is None else ('host' if to_host else 'device'))
        return (encs_dev if units_on_device else encs), decs
    encs, _ = _assemble(q, None)
    conv = conv_h.numpy() if to_host else q.conv
    return (encs_dev if units_on_device else encs), [conv[u, :n] for u, n in enumerate(q.ulens)]


def resynth_batch(specs, trainer, seg_len, speakers, n_iter=None, do_trim=True, noise_fn=None, max_batch=256, defer=False, enc_only=True,
                  momentum=None, codebook=None, want_idx=False, overlap=0, segment=None):
    """test_encode + convert(enc_only) + spectrogram2wav for a batch of utterances as ONE enqueue (convert.py:151-165, 55-62):
    the fragments' Encoder / Decoder launches, the gather of the decoded fragments into the vocoder's padded [n, T_max, 513]
    input (one index kernel on the device), de-normalisation, the Griffin-Lim loop, de-emphasis, the trim statistics and the
    D2H copies go onto the stream back to back; the host assembles the encodings while the vocoder runs and waits ONCE.
    Returns (encodings list, wav list) -- the same values as encode_batch(...) followed by spectrogram2wav_batch(...).
    defer=True returns a function instead that waits for THIS batch (an event behind its last copy) and returns that pair: a
    serving loop enqueues batch i + 1 before it calls the function of batch i, so the host-side assembly and the D2H copies of one
    batch run under the GPU work of the next.
    enc_only=False: convert() with the stage-2 generator; zs_gen_scatter writes each chunk's de-normalised converted rows straight
    into the vocoder's input, so the gather / combine / de-normalisation passes below do not exist on that path.
    momentum: the vocoder's fast Griffin-Lim momentum (see griffin_lim_batch; None: hp.gl_momentum).
    codebook: as encode_batch's -- the Decoder, the generator and the returned encodings see the snapped units; want_idx=True
    makes the result (encodings, wavs, codeword indices int32 [U_i] per utterance, summed Hamming distance of the snap -- under a
    vector codebook, enc_mode 'continues', the summed squared Euclidean distance, a float).
    overlap > 0 (frames; check_overlap_value): encode_batch, then the matching synth_units_batch / synth_index_batch(overlap=...) of
    the units or indices it returns, as one enqueue -- the encoder runs without a decode, and the decode windows of unit_windows read
    the units where the encoder left them on the device.  The encodings returned are encode_batch's.  An input padded to MIN_LEN is
    spoken from the truncated units it returns, as --synth_dir would speak its file, so one of fewer than 2 units is refused, as is
    enc_mode 'continues' without a codebook, which has nothing to speak from; both before anything is enqueued.
    segment (lambda >= 0; encode_batch's): the same one enqueue at any overlap, 0 included -- the encoder runs without a decode,
    zs_seg_viterbi chooses the batch's paths, and the units of the paths are spoken from the device buffer by the drivers of
    synth_units_batch / synth_index_batch.  The indices and the summed distance returned are the path's."""
    momentum = gl_momentum(momentum)
    if want_idx and codebook is None:
        raise ValueError('resynth_batch: want_idx needs a codebook')
    if segment is not None:
        segment = sg.check_lambda(segment, 'resynth_batch: segment')
        sg.check_codebook(codebook, 'resynth_batch: segment')
    if check_overlap_value(overlap, seg_len) or segment is not None:
        return _resynth_overlap(specs, trainer, seg_len, speakers, n_iter, do_trim, noise_fn, max_batch, defer, enc_only, momentum, codebook,
                                want_idx, overlap, segment)
    if not enc_only:
        q = _enqueue_encode(specs, trainer, seg_len, speakers, noise_fn, max_batch, dec_to_host=False, enc_only=False, denorm=True,
                            codebook=codebook)
        fin = _enqueue_vocoder(q.conv, q.ulens, n_iter, do_trim, q.dev, amplitudes=True, momentum=momentum)
    else:
        q = _enqueue_encode(specs, trainer, seg_len, speakers, noise_fn, max_batch, dec_to_host=False, codebook=codebook)
        t, ulens = _gather_decoded(q, [[8 * _t8(n) for n in lens] for _, lens in q.chunks])
        fin = _enqueue_vocoder(t, ulens, n_iter, do_trim, q.dev, momentum=momentum)
    return _finish_resynth(q, fin, defer, want_idx)


def _unit_counts(specs, seg_len):
    """The units encode_batch returns for each utterance, from the frame counts alone (the rules of _enqueue_encode: padding to
    MIN_LEN and its truncation, _frame_items, _t8)."""
    counts = []
    for u, spec in enumerate(specs):
        n = int(spec.shape[0])
        items = _frame_items(u, max(n, MIN_LEN), seg_len, n < MIN_LEN)
        counts.append(sum(it.trunc if it.trunc is not None else _t8(it.n) for it in items))
    return counts


def _resynth_overlap(specs, trainer, seg_len, speakers, n_iter, do_trim, noise_fn, max_batch, defer, enc_only, momentum, codebook, want_idx,
                     overlap, segment=None):
    """resynth_batch with overlap > 0, as one enqueue: _enqueue_encode without a decode leaves the batch's units on the device in
    utterance order -- bit-packed (pack=True, snapped in place under a bit codebook), or the index buffer a vector or residual
    codebook's finish makes -- and _enqueue_synth decodes the windows of unit_windows over that buffer, whose layout (q.uoffs) is
    the one _unit_tables expects.  segment: the buffer holds the units of the chosen paths (_enqueue_encode), and overlap may be 0:
    the windows are then the fragments of unit_fragments."""
    def count_units():
        if codebook is None and trainer.enc_mode == 'continues':
            raise ValueError("resynth_batch: overlap = %d needs units to speak from, and enc_mode 'continues' has none without a codebook"
                             % overlap)
        if codebook is not None:
            _check_codebook(codebook, trainer)
        return _unit_counts(specs, seg_len)
    counts, shift = _speak_checks('resynth_batch', trainer, speakers, len(specs), count_units, enc_only)
    short = [u for u, n in enumerate(counts) if n < 2]
    if short:
        raise ValueError('resynth_batch: overlap = %d speaks the units an utterance returns, and utterance %d returns %d (an input '
                         'shorter than MIN_LEN = %d frames); the Decoder needs two' % (overlap, short[0], counts[short[0]], MIN_LEN))
    side = codebook.units() if codebook is not None else _BitUnits(None)      # whose layout q.units_dev has
    q = _enqueue_encode(specs, trainer, seg_len, None, noise_fn, max_batch, dec_to_host=False, pack=codebook is None, codebook=codebook,
                        keep_units=True, segment=segment)     # (a bit codebook packs by itself and returns the units unpacked)
    if [int(n) for n in np.diff(q.uoffs)] != counts:
        raise L.ZsError('resynth_batch: the encoder left %s units where the plan has %s' % (np.diff(q.uoffs).tolist(), counts))
    operand = side.decoder_over(trainer.Decoder, q.units_dev)
    chunks = _speak_chunks(counts, seg_len, overlap, max_batch)               # host work behind the encoder's enqueue, as it always was
    fin, _, _ = _enqueue_synth(trainer, seg_len, chunks, q.uoffs, speakers, enc_only, shift, n_iter, do_trim, momentum, False, operand,
                               overlap=overlap)
    return _finish_resynth(q, fin, defer, want_idx, unpack=(int(trainer.Encoder.enc_size) if codebook is None else None))


def _speak_checks(who, trainer, speakers, n_utt, count_units, enc_only):
    """The refusals of a batch spoken from units (_resynth_overlap, _synth_batch), before anything is enqueued: a speaker per
    utterance; count_units() -> the units of each, behind the caller's own refusals, which keep their place between that check and
    the speakers' (the Decoder's table, the generator's targets).  Returns (units per utterance, the shift of check_gen_targets or 0)."""
    if len(speakers) != n_utt or not n_utt:
        raise ValueError('%s: %d target speakers for %d utterances' % (who, len(speakers), n_utt))
    counts = count_units()
    _check_speaker_range(speakers, int(trainer.Decoder.c_a))
    return counts, (0 if enc_only else check_gen_targets(trainer, speakers))


def _speak_chunks(counts, seg_len, overlap, max_batch):
    """The chunks of a batch spoken from units: each utterance cut into the windows of unit_windows (overlap > 0), which share units,
    or the pieces of unit_fragments."""
    items = [it for u, n in enumerate(counts) for it in (_window_items(u, n, seg_len, overlap) if overlap else _unit_items(u, n, seg_len))]
    return _split_chunks(items, int(seg_len) // 8, max_batch)


def _gather_decoded(q, out_rows):
    """The vocoder's padded input [n_utt, T_max, 513] fp32 from the decoded chunks q.dec_dev, by one index kernel on the device:
    utterance u's frames are its fragments' rows in fragment order, zeros behind them.  out_rows[ci][i]: the valid output rows of
    fragment i of chunk ci.  Returns (t, frames per utterance)."""
    dev = q.dev
    idx, ulens, _ = _gather_index(q.chunks, out_rows, [(x.shape[0], x.shape[1]) for x in q.dec_dev], q.n_utt)
    table = torch.cat([x.reshape(-1, x.shape[2]) for x in q.dec_dev] + [torch.zeros(1, q.dec_dev[0].shape[2], dtype=q.dec_dev[0].dtype, device=dev)], dim=0)
    return table[torch.from_numpy(idx).to(dev, non_blocking=True)].float(), ulens                     # [n, Tm, 513]


def _wait_vocoder(fin, dev):
    """The wavs of a batch, waited for; a persistent GRU pass that timed out before the batch's end raises here."""
    wavs = fin()
    if fin.status:
        from . import layers
        layers.check_status(dev)                              # synchronises, clears the word and raises
    return wavs


def _finish_resynth(q, fin, defer, want_idx=False, unpack=None):
    """unpack: the width E of units that were bit-packed for the device's sake alone and are returned as [U_i, E] of 0 / 1."""
    def finish():
        q.enc_done.synchronize()                              # the encodings are on the host; the vocoder is still running
        encs, _ = _assemble(q, None)
        if unpack is not None:
            encs = [unpack_units(e, unpack) for e in encs]
        wavs = _wait_vocoder(fin, q.dev)
        return (encs, wavs) + _unit_indices(q.idx_host, q.cb_total, q.uoffs) if want_idx else (encs, wavs)
    return finish if defer else finish()


def synth_units_batch(units, trainer, seg_len, speakers, enc_only=True, n_iter=None, do_trim=True, max_batch=256, defer=False,
                      momentum=None, packed=False, want_specs=False, codebook=None, want_idx=False, overlap=0):
    """Speech from units: what resynth_batch does behind its encoder, from the units alone.  units: a list of [U_i, E] arrays of
    0 / 1 as encode_batch returns them (what read_units parses from a --test_encode file); packed=True: a list of uint8
    [U_i, (E + 7) // 8] arrays (pack_units, encode_batch(packed=True)).  speakers: the target id of each.
    Every utterance goes to the device once, bit-packed, in one buffer; unit_fragments cuts each into the pieces the Decoder runs
    on -- pieces of exactly seg_len // 8 units as plain batches, the rest as ragged batches, longest first, as _enqueue_encode
    batches them -- zs_units_unpack writes each chunk's Decoder operand, the decode half is _enqueue_encode's own (_decode_chunk:
    with enc_only=False the stage-2 generator and zs_gen_scatter), and the vocoder follows on the same stream.
    Returns (specs or None, wavs): wavs as resynth_batch returns them; specs (want_specs=True) the normalised spectrograms
    [8 U_i, 513] the vocoder was given.  defer=True returns the function that waits for this batch and returns that pair.
    Where unit_fragments reproduces the fragmentation of the frames (see there) the result is resynth_batch's / convert()'s.
    Refused before anything is enqueued: enc_mode 'continues' (its files are not units), a width other than the Decoder's c_in, a
    value other than 0 / 1, fewer than 2 units (ValueError); a speaker the Decoder or the generator cannot take
    (check_gen_targets).
    codebook: a zs_amd.codebook.Codebook -- the one device buffer is snapped once, in place, before the first chunk, so every
    fragment is decoded from snapped units; want_idx=True appends (codeword indices int32 [U_i] per utterance, summed Hamming
    distance of the snap) to the result.
    overlap (frames, like seg_len; check_overlap_value): the utterance is decoded in the windows of unit_windows, which share
    overlap // 8 units, and the frames two windows share are cross-faded (zs_xfade_gather, on the normalised rows) instead of cut:
    the spectrogram no longer jumps where a piece ends.  The units are the same; an utterance of at most 2 (seg_len // 8) units is
    one window and is spoken exactly as with overlap 0, which is today's path launch for launch."""
    momentum = gl_momentum(momentum)
    if want_idx and codebook is None:
        raise ValueError('synth_units_batch: want_idx needs a codebook')
    if trainer.enc_mode == 'continues':
        raise ValueError(_NO_UNITS)
    side = _BitUnits(codebook)                                # rows of bits whatever the codebook: check_rows refuses one of another kind
    side.packed_rows, side.want_idx = packed, want_idx
    return _synth_batch(side, units, trainer, seg_len, speakers, enc_only, n_iter, do_trim, max_batch, defer, momentum, want_specs, overlap)


def _synth_batch(side, units, trainer, seg_len, speakers, enc_only=True, n_iter=None, do_trim=True, max_batch=256, defer=False, momentum=None,
                 want_specs=False, overlap=0):
    """The one driver of synth_units_batch, synth_index_batch and the kinds' speak.  side.check_rows -> the utterances as host
    arrays of one dtype and row shape (ValueError for what cannot be spoken); they go to the device once, in one pinned buffer and
    one copy, and _speak_chunks cuts each into the row ranges the Decoder runs on.  side.after_upload -> (the function _enqueue_synth
    builds a chunk's Decoder operand with, and the pinned codeword indices and summed distance of a snap, or None, None)."""
    rows = []

    def count_units():
        check_overlap_value(overlap, seg_len)
        rows.extend(side.check_rows(units, trainer))
        return [len(r) for r in rows]
    counts, shift = _speak_checks(side.who, trainer, speakers, len(units), count_units, enc_only)
    chunks = _speak_chunks(counts, seg_len, overlap, max_batch)
    trainer.set_eval()
    dev = trainer.device
    uoffs = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    host = torch.empty((int(uoffs[-1]),) + rows[0].shape[1:], dtype=torch.from_numpy(rows[0]).dtype, pin_memory=True)
    np.concatenate(rows, axis=0, out=host.numpy())
    chunk_operand, idx_h, total_h = side.after_upload(trainer.Decoder, host.to(dev, non_blocking=True))     # the one H2D copy of the batch
    fin, spec_h, ulens = _enqueue_synth(trainer, seg_len, chunks, uoffs, speakers, enc_only, shift, n_iter, do_trim, momentum, want_specs,
                                        chunk_operand, overlap=overlap)

    def finish():
        wavs = _wait_vocoder(fin, dev)
        specs = [spec_h.numpy()[u, :n].copy() for u, n in enumerate(ulens)] if spec_h is not None else None
        # the indices were copied before the vocoder, which fin() has waited for
        return (specs, wavs) + _unit_indices(idx_h, total_h, uoffs) if idx_h is not None else (specs, wavs)
    return finish if defer else finish()


def _xfade_gather(src, chunks, first, n_utt, denorm, dev):
    """The vocoder's padded input [n_utt, T_max, 513] fp32 of a batch decoded in overlapping windows, by ONE zs_xfade_gather over the
    source table src (fp32 [rows, 513], contiguous): the plan of _xfade_tables goes to the device in one copy.  denorm: the rows are
    written de-normalised (amplitudes).  Returns (t, frames per utterance)."""
    Tm, ulens, i0, i1, w0, w1 = _xfade_tables(chunks, first, n_utt)
    rows = n_utt * Tm
    if rows >= 2 ** 31 or src.shape[0] >= 2 ** 31:
        raise ValueError('overlapped batch too large: %d rows from %d' % (rows, src.shape[0]))
    tab = torch.from_numpy(np.concatenate([i0, i1, w0.view(np.int32), w1.view(np.int32)])).to(dev, non_blocking=True)
    i0_d, i1_d, w0_d, w1_d = torch.split(tab, rows)
    t = torch.empty(n_utt, Tm, 513, dtype=torch.float32, device=dev)
    L.call('zs_xfade_gather', 'ZsXfadeGather', torch.cuda.current_stream(dev).cuda_stream, src=L.ptr(src), src_rows=src.shape[0],
           ld_src=src.stride(0), i0=L.ptr(i0_d), i1=L.ptr(i1_d), w0=L.ptr(w0_d), w1=L.ptr(w1_d), out=L.ptr(t), rows=rows, out_ld=513,
           cols=513, denorm=int(denorm))
    return t, ulens


def _enqueue_synth(trainer, seg_len, chunks, uoffs, speakers, enc_only, shift, n_iter, do_trim, momentum, want_specs, operand, overlap=0):
    """The decode half and the vocoder of a batch of unit (or index) sequences, shared by synth_units_batch and synth_index_batch:
    operand(tab, B, T0, ch, lens_p) -> (bits, x_dec) builds and decodes one chunk's operand from its (start, len) device tables over
    the batch's one buffer.  Returns (the vocoder's finish function, the pinned copy of the spectrograms or None, frames per
    utterance); nothing is waited for.
    overlap > 0: the chunks hold the windows of _window_items, which share units, and ONE zs_xfade_gather builds the vocoder's input
    from the decoded windows, cross-fading the frames two of them share (_xfade_gather) on the NORMALISED rows; the de-normalisation
    is the gather's own, under the same want_specs rule.  enc_only: the decoded chunks laid end to end are the source table, as
    _gather_decoded builds it.  With the generator, zs_gen_scatter writes each chunk's combined rows, not de-normalised, into a
    staging buffer of _plan_scatter's layout in which an utterance's windows lie back to back (the shared rows twice), and the gather
    reads that."""
    dev, n_utt = trainer.device, len(uoffs) - 1
    q = _Enqueued()
    q.n_utt, q.dev, q.chunks, q.dec_dev = n_utt, dev, [], []
    tabs = _upload_tables(*_unit_tables(chunks, uoffs), chunks, dev)
    denorm = not want_specs                               # the vocoder de-normalises (the same device function) when the rows are wanted
    gen_plan = None
    if not enc_only:                                      # zs_gen_scatter's buffer: the vocoder's input; overlap: the staging buffer
        q.conv, q.ulens, dsts = _plan_scatter(chunks, n_utt, denorm and not overlap, dev, rows_of=lambda n: 8 * n)
        gen_plan = (q.conv, dsts, shift, denorm and not overlap)
    for ci, (chunk, ragged) in enumerate(chunks):
        lens = [it.n for it in chunk]
        xd = _decode_chunk(trainer, ci, [it.u for it in chunk], (lens if ragged else None), speakers, enc_only, gen_plan,
                           lambda ch, lens_p: operand(tabs[ci], len(chunk), max(lens), ch, lens_p))
        q.chunks.append((chunk, lens))
        q.dec_dev.append(xd)
    if overlap:
        if enc_only:
            first, total = [], 0
            for (chunk, _), x in zip(chunks, q.dec_dev):
                first += [total + i * x.shape[1] for i in range(len(chunk))]
                total += x.shape[0] * x.shape[1]
            src = q.dec_dev[0].reshape(-1, 513) if len(q.dec_dev) == 1 else torch.cat([x.reshape(-1, 513) for x in q.dec_dev], dim=0)
            src = src.float()
        else:                                             # [n_utt, rows of the longest utterance's windows, 513]
            flat = _flat(chunks)
            at, _ = _fragment_layout(flat, [8 * it.n for it in flat], n_utt)
            first = [it.u * q.conv.shape[1] + s for it, s in zip(flat, at)]
            src = q.conv.reshape(-1, 513)
        t, ulens = _xfade_gather(src, chunks, first, n_utt, denorm, dev)
        amplitudes = denorm
    elif enc_only:
        t, ulens = _gather_decoded(q, [[8 * n for n in lens] for _, lens in q.chunks])
        amplitudes = False
    else:
        t, ulens, amplitudes = q.conv, q.ulens, denorm
    spec_h = _to_host(t) if want_specs else None
    return _enqueue_vocoder(t, ulens, n_iter, do_trim, dev, amplitudes=amplitudes, momentum=momentum), spec_h, ulens


def synth_index_batch(idx_lists, trainer, seg_len, speakers, codebook, enc_only=True, n_iter=None, do_trim=True, max_batch=256, defer=False,
                      momentum=None, want_specs=False, overlap=0):
    """Speech from codeword indices: synth_units_batch for enc_mode 'continues' under a vector codebook (zs_amd.vq.VectorCodebook).
    idx_lists: one integer sequence per utterance (what resynth_batch(want_idx=True) returns, what read_indices parses from an
    .idx.txt file).  Every index goes to the device once, in one int32 buffer; unit_fragments cuts each utterance as
    synth_units_batch cuts it, zs_vq_gather writes each chunk's Decoder operand from the codewords, and the decode half and the
    vocoder are synth_units_batch's own.  Returns (specs or None, wavs); defer=True returns the function that waits for them.
    Refused before anything is enqueued: a codebook that is no vector codebook (for 'continues' in synth_units_batch's words), a
    width other than the Decoder's c_in, an index outside [0, K), fewer than 2 indices (ValueError); a speaker the Decoder or the
    generator cannot take.
    Under a zs_amd.rvq.ResidualCodebook an utterance is integers [U_i, c], a row of c <= S indices per frame and the same c for the
    whole batch (what read_index_rows parses): the rows go to the device once, are transposed there into c planes, and zs_rvq_gather
    (Decoder.forward_index_planes) writes each chunk's operand as the sum of the c stages' codewords.  The driver is the same.
    overlap: as synth_units_batch's -- overlapping decode windows over the same indices, cross-faded."""
    momentum = gl_momentum(momentum)
    side = codebook.units() if codebook is not None else _BitUnits(None)
    if not isinstance(side, _VectorUnits):                    # (a zs_amd.rvq.ResidualCodebook's kind is a _VectorUnits)
        side.check_speakable(trainer.enc_mode)
        raise ValueError('synth_index_batch: the codebook must be a vector codebook (zs_amd.vq.VectorCodebook)')
    _check_codebook(codebook, trainer)
    return _synth_batch(side, idx_lists, trainer, seg_len, speakers, enc_only, n_iter, do_trim, max_batch, defer, momentum, want_specs, overlap)


def out_rate():
    """The sample rate of the wavs convert(), cross_test and test_single write: hp.out_sr (--out_sr), or hp.sr when it is None."""
    return hp.sr if hp.out_sr is None else int(hp.out_sr)


def to_out_sr(wavs):
    """A list of hp.sr waveforms at the output rate: the very list when hp.out_sr is None or hp.sr, else resampled in one
    zs_resample launch (zs_amd.resample)."""
    if out_rate() == hp.sr:
        return wavs
    from .resample import resample_batch
    return resample_batch(wavs, hp.sr, out_rate())


def write_wav(path, wav, sr):
    """16-bit PCM mono wav (the reference uses soundfile.write(..., 'PCM_16'), convert.py:174)."""
    import wave
    pcm = np.clip(np.round(np.asarray(wav, dtype=np.float64) * 32767.0), -32768, 32767).astype('<i2')
    with wave.open(path, 'wb') as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(pcm.tobytes())


def _open_h5(path):
    """The preprocessed dataset: HDF5 when h5py is importable, else the .npz container zs_amd.preprocess writes."""
    from .dataloader import open_store
    return open_store(path, 'r')


def test_from_list(trainer, seg_len, synthesis_list, data_path, speaker2id_path, result_dir, enc_only, flag='test', run_asr=False):
    """convert.py:224-265 (the ASR scoring branch needs the network and is not reproduced)."""
    with open(speaker2id_path, 'r') as f_json:
        speaker2id = json.load(f_json)
    feeds = []
    with open(synthesis_list, 'r') as f:
        for line in f.readlines():
            line = line.split('\n')[0].split(' ')
            feeds.append({'s_id': line[0].split('/')[1].split('_')[0], 'utt_id': line[0].split('/')[1].split('_')[1], 't_id': line[1]})
    print('[Tester] - Number of files to be resynthesize: ', len(feeds))
    dir_path = os.path.join(result_dir, f'{flag}/')
    os.makedirs(dir_path, exist_ok=True)
    with _open_h5(data_path) as f_h5:
        for feed in feeds:
            convert(trainer, seg_len, src_speaker_spec=f_h5[f"test/{feed['s_id']}/{feed['utt_id']}/lin"][()], src_speaker=feed['s_id'],
                    tar_speaker=feed['t_id'], utt_id=feed['utt_id'], speaker2id=speaker2id, result_dir=dir_path, enc_only=enc_only,
                    save=['wav'])


def store_keys(store, prefix):
    """Names directly under `prefix` of the dataset container: list(f[prefix].keys()) for HDF5, NpzStore.keys(prefix) for .npz."""
    from .dataloader import NpzStore
    if isinstance(store, NpzStore):
        return store.keys(prefix)
    return sorted(store[prefix].keys())


def _run_deferred(groups, enqueue, write):
    """The serving loop of every driver: group i + 1 is enqueued before group i is written, so the host's share of one group (the
    wait, the assembly, the files) runs under the GPU work of the next.  enqueue(group) puts a group on the stream and returns
    the arguments of write for it, or None for a group with nothing to write."""
    pending = None
    for group in groups:
        enqueued = enqueue(group)
        if pending is not None:
            write(*pending)
        pending = enqueued
    if pending is not None:
        write(*pending)


def cross_test_plan(keys, flag, result_dir):
    """The work list of cross_test (convert.py:268-300): every utterance of every source speaker to every target speaker.
    keys(prefix) lists the names under a container prefix (store_keys).  Sources: the speakers under test/ (flag 'test') or the
    S* speakers under train/ (flag 'train'); targets: the V* speakers under train/.  Returns one dict per (source utterance,
    target) pair, in the reference's loop order, with the spectrogram's key and the two files convert() would write:
    {result_dir}/{src}_to_{tar}/{tar}_{utt}.wav and .../{src}_{utt}.txt."""
    if flag == 'test':
        sources = sorted(keys('test'))
    elif flag == 'train':
        sources = [s for s in sorted(keys('train')) if s[0] == 'S']
    else:
        raise ValueError("cross_test flag must be 'test' or 'train' (got %r)" % (flag,))
    targets = [s for s in sorted(keys('train')) if s[0] == 'V']
    plan = []
    for src in sources:
        utts = sorted(keys('%s/%s' % (flag, src)))
        for tar in targets:
            if src == tar:
                raise ValueError('cross_test: speaker %s is both a source and a target' % src)
            d = os.path.join(result_dir, '%s_to_%s' % (src, tar))
            for utt in utts:
                plan.append({'src': src, 'tar': tar, 'utt': utt, 'key': '%s/%s/%s/lin' % (flag, src, utt), 'dir': d,
                             'wav': os.path.join(d, '%s_%s.wav' % (tar, utt)), 'txt': os.path.join(d, '%s_%s.txt' % (src, utt))})
    return plan


def cross_test(trainer, seg_len, data_path, speaker2id_path, result_dir, enc_only, flag='test', batch=64, n_iter=None, momentum=None):
    """convert.py:268-300, as the reference means it (its call passes the target in the source speaker's slot and raises
    TypeError): convert() of every source utterance to every target speaker, with convert()'s default outputs.  Every (utterance,
    target) pair is an item of its own with its own Gumbel noise; items go through resynth_batch in groups of `batch`, and group
    i + 1 is enqueued before group i is written (defer=True).  n_iter / momentum: the vocoder's (None: hp.n_iter / hp.gl_momentum)."""
    momentum = gl_momentum(momentum)
    with open(speaker2id_path, 'r') as f_json:
        speaker2id = json.load(f_json)
    with _open_h5(data_path) as f_h5:
        plan = cross_test_plan(lambda prefix: store_keys(f_h5, prefix), flag, result_dir)
        n_src = len({it['src'] for it in plan})
        n_tar = len({it['tar'] for it in plan})
        print('[Tester] - Testing on the {}ing set...'.format(flag))
        print('[Tester] - Source speakers: %i, Target speakers: %i, conversions: %i' % (n_src, n_tar, len(plan)))
        groups = [plan[lo:lo + batch] for lo in range(0, len(plan), batch)]
        check = [speaker2id[it['tar']] for it in plan]
        if not enc_only and check:
            check_gen_targets(trainer, check)                 # before the first group is enqueued

        def write(group, fin):
            encs, wavs = fin()
            for it, e, w in zip(group, encs, to_out_sr(wavs)):
                os.makedirs(it['dir'], exist_ok=True)
                write_wav(it['wav'], w, out_rate())
                write_encodings(it['txt'], e)

        def enqueue(group):
            specs = [np.asarray(f_h5[it['key']][()], dtype=np.float32) for it in group]
            return group, resynth_batch(specs, trainer, seg_len, [speaker2id[it['tar']] for it in group], n_iter=n_iter, defer=True,
                                        enc_only=enc_only, momentum=momentum)

        _run_deferred(groups, enqueue, write)
    return plan


# ---------------------------------------------------------------------------------------------------
# a folder of sound files, end to end on the device (not in the reference: its drivers read a preprocessed container)
# ---------------------------------------------------------------------------------------------------

def _wav_features(wavs, rates, dev, do_trim=True, strict=True):
    """Sound -> spectrograms that never leave the device (preprocess.get_spectrograms_device(trim_on='device')): the list of
    mag[i, :frames[i]] views and, per input, {'bounds': (start, stop) of the trim at hp.sr, 'frames'}.  strict=False: an input of
    fewer than 2 samples after trimming gets None and frames 0 instead of the ValueError."""
    from .preprocess import _spectrograms_on_device
    mag, frames, bounds = _spectrograms_on_device(wavs, do_trim, dev, rates, strict=strict)
    specs = [mag[i, :int(frames[i])] if frames[i] > 0 else None for i in range(len(wavs))]
    info = [{'bounds': (int(bounds[i, 0]), int(bounds[i, 1])), 'frames': int(frames[i])} for i in range(len(wavs))]
    return specs, info


def convert_wavs(wavs, rates, trainer, seg_len, speakers, enc_only=True, n_iter=None, momentum=None, noise_fn=None, do_trim=True,
                 defer=False, codebook=None, overlap=0, segment=None):
    """Waveforms in, converted waveforms out, as one enqueue: wavs is a list of 1-D float arrays at `rates` (None: hp.sr; one int,
    or one per wav), speakers the target id of each.  Inputs not at hp.sr are resampled on the device, zs_trim finds the trim
    bounds there, zs_pre_spectrogram reads the trimmed windows in place and resynth_batch runs on the device-resident
    mag[i, :frames[i]]: neither the audio nor the spectrograms visit the host (one synchronisation: the n x 2 bounds).  The values
    are those of preprocess.get_spectrograms_batch(wavs, sr=rates) followed by resynth_batch(specs, ...), bit for bit.
    Returns (encodings, wavs, info); info[i] = {'bounds': (start, stop) of the input's trim at hp.sr, 'frames'}.  do_trim is
    get_spectrograms' trim of the input and the vocoder's trim of the output together; defer, enc_only, n_iter, momentum and
    noise_fn, codebook, overlap and segment are resynth_batch's.  An input of fewer than 2 samples after trimming raises ValueError before the
    network is enqueued."""
    momentum = gl_momentum(momentum)
    overlap = check_overlap_value(overlap, seg_len)
    if overlap and codebook is None and trainer.enc_mode == 'continues':
        raise ValueError("convert_wavs: overlap = %d needs units to speak from, and enc_mode 'continues' has none without a codebook"
                         % overlap)
    if len(speakers) != len(wavs):
        raise ValueError('convert_wavs: %d target speakers for %d wavs' % (len(speakers), len(wavs)))
    if segment is not None:
        segment = sg.check_lambda(segment, 'convert_wavs: segment')
        sg.check_codebook(codebook, 'convert_wavs: segment')
    if codebook is not None:
        _check_codebook(codebook, trainer)
    if not enc_only:
        check_gen_targets(trainer, speakers)
    specs, info = _wav_features(wavs, rates, trainer.device, do_trim=do_trim)
    fin = resynth_batch(specs, trainer, seg_len, speakers, n_iter=n_iter, do_trim=do_trim, noise_fn=noise_fn, defer=True, enc_only=enc_only,
                        momentum=momentum, codebook=codebook, **({'overlap': overlap} if overlap else {}),
                        **({'segment': segment} if segment is not None else {}))

    def finish():
        encs, out = fin()
        return encs, out, info
    return finish if defer else finish()


def _dir_plan(who, files, sizes, sizes_name, targets, batch, cap, reject, item):
    """The grouping convert_dir_plan and synth_dir_plan share: files sorted by (size, path), reject(size) -> the reason a file is
    skipped for or None, item(file, stem, target, size) for every target of a file that stays, then greedily groups of at most
    `batch` items and at most `cap` of padded size, items x the longest."""
    if len(files) != len(sizes):
        raise ValueError('%s: %d %s for %d files' % (who, len(sizes), sizes_name, len(files)))
    if batch < 1:
        raise ValueError('%s: batch must be >= 1' % who)
    targets = list(targets)
    if not targets or len(set(targets)) != len(targets):
        raise ValueError('%s: the targets must be a non-empty list of distinct speakers (got %r)' % (who, targets))
    stems = {}
    for f in files:
        stem = os.path.splitext(os.path.basename(f))[0]
        if stem in stems:
            raise ValueError('%s: %s and %s would write the same outputs (stem %r)' % (who, stems[stem], f, stem))
        stems[stem] = f
    skipped, groups = [], []
    for size, f in sorted(zip(sizes, files)):
        reason = reject(size)
        if reason is not None:
            skipped.append({'file': f, 'reason': reason})
            continue
        stem = os.path.splitext(os.path.basename(f))[0]
        for t in targets:                                     # ascending sizes: the newest item is a group's longest
            if groups and len(groups[-1]) < batch and (len(groups[-1]) + 1) * size <= cap:
                groups[-1].append(item(f, stem, t, size))
            else:
                groups.append([item(f, stem, t, size)])
    return {'groups': groups, 'skipped': skipped}


def convert_dir_plan(files, durations, targets, out_dir, batch=64, max_batch_seconds=600, max_seconds=1800):
    """The work list of convert_dir, on the host alone: every (file, target) pair is an item.  durations[i]: seconds of files[i]
    from its header.  Files are sorted by (duration, path) so that a group pads little and the plan does not depend on the order
    they are listed in; a file's items are adjacent, in the order of `targets`.  A group takes items in that order while it holds
    at most `batch` of them and at most max_batch_seconds of padded audio, counted as items x the longest (a single item above the
    cap is a group of its own).  A file longer than max_seconds, or whose header gives no samples, goes to 'skipped' with a reason;
    two inputs with the same stem would write the same outputs: ValueError.
    Returns {'groups': [[item]], 'skipped': [{'file', 'reason'}]}, item = {'file', 'stem', 'target', 'duration', 'wav', 'txt'} with
    the outputs {out_dir}/{target}/{stem}.wav and .txt."""
    def reject(dur):
        if not dur > 0.0:
            return 'the header gives no samples'
        if dur > max_seconds:
            return '%.1f s is longer than max_seconds = %g' % (dur, max_seconds)

    def item(f, stem, t, dur):
        return {'file': f, 'stem': stem, 'target': t, 'duration': dur, 'wav': os.path.join(out_dir, t, stem + '.wav'),
                'txt': os.path.join(out_dir, t, stem + '.txt')}
    return _dir_plan('convert_dir_plan', files, [float(d) for d in durations], 'durations', targets, batch, max_batch_seconds, reject, item)


def _write_index_lines(path, rows):
    """The one writer of index files: a line per row, its integers separated by one blank."""
    with open(path, 'w') as f:
        for r in rows:
            f.write(' '.join('%d' % int(k) for k in r) + '\n')


def write_indices(path, idx):
    """The sibling of a unit file under a codebook: one codeword index per line, one line per unit."""
    _write_index_lines(path, ([i] for i in idx))


def write_index_rows(path, rows):
    """The unit file under a residual codebook: one line per frame, its c indices separated by one blank (rows: integers [U, c])."""
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] < 1 or rows.dtype.kind not in 'iu':
        raise ValueError('write_index_rows: rows must be integers [U, c >= 1] (got %s %s)' % (rows.dtype, rows.shape))
    _write_index_lines(path, rows)


def read_index_rows(path, K, S):
    """The parser of what write_index_rows writes: c integers in [0, K) per line, 1 <= c <= S, the same c on every line -> int32
    [U, c].  ValueError naming the file and the line for anything else, and for a file without a line.  S None: read_indices' file,
    one integer per line, refused in its words."""
    out, c = [], None
    with open(path, 'r') as f:
        for no, line in enumerate(f, 1):
            tokens = line.split()
            if S is None:
                if len(tokens) != 1:
                    raise ValueError('%s, line %d: %d values, expected one index' % (path, no, len(tokens)))
            elif c is None:
                if not 1 <= len(tokens) <= S:
                    raise ValueError('%s, line %d: %d values, expected 1 to S = %d indices' % (path, no, len(tokens), S))
                c = len(tokens)
            elif len(tokens) != c:
                raise ValueError('%s, line %d: %d values where line 1 has %d' % (path, no, len(tokens), c))
            row = []
            for tok in tokens:
                try:
                    k = int(tok, 10)
                except ValueError:
                    raise ValueError('%s, line %d: %r is not an integer' % (path, no, tok))
                if not 0 <= k < K:
                    raise ValueError('%s, line %d: index %d is outside [0, K = %d)' % (path, no, k, K))
                row.append(k)
            out.append(row)
    if not out:
        raise ValueError('%s: no indices (the file is empty)' % path)
    return np.asarray(out, dtype=np.int32)


def read_indices(path, K):
    """The parser of what write_indices writes: one integer in [0, K) per line -> int32 [U].  ValueError naming the file and the line
    for anything else, and for a file without a line."""
    return read_index_rows(path, K, None).reshape(-1)


def idx_path(txt):
    """<name>.txt -> <name>.idx.txt"""
    return os.path.splitext(txt)[0] + '.idx.txt'


class _CodebookStats(object):
    """What a folder driver reports about a codebook run: the histogram of the indices written and the summed distance.  Under a
    residual codebook a histogram and a distance per stage."""

    def __init__(self, codebook, file):
        self.cb, self.file, self.total = codebook, file, 0
        self.hist = np.zeros((getattr(codebook, 'S', 1), codebook.K), dtype=np.int64)

    def add(self, idxs, total):
        for i in idxs:
            i = np.asarray(i)
            planes = i[:, None] if i.ndim == 1 else i         # [U] or, under a residual codebook, [U, s']
            for s in range(planes.shape[1]):
                self.hist[s] += np.bincount(planes[:, s], minlength=self.cb.K)
        self.total = self.total + total                       # int (Hamming), float (squared Euclidean) or, residual, a float per stage

    def manifest(self):
        from .codebook import usage_counts
        n = int(self.hist[0].sum())
        used, ent = usage_counts(self.hist[0])
        out = {'file': self.file, 'K': self.cb.K, 'symbols_used': used, 'entropy_bits_per_unit': ent}
        if getattr(self.cb, 'kind', None) != 'residual':
            out['mean_distance'] = (self.total / float(n)) if n else 0.0
            return out
        live = [s for s in range(self.hist.shape[0]) if self.hist[s].sum()]
        totals = np.broadcast_to(np.asarray(self.total, dtype=np.float64).reshape(-1), (len(live),)) if live else np.zeros(0)
        stages = []
        for s, t in zip(live, totals):
            u, e = usage_counts(self.hist[s])
            stages.append({'symbols_used': u, 'entropy_bits_per_unit': e, 'mean_distance': float(t) / float(self.hist[s].sum())})
        out.update({'S': self.cb.S, 'stages': stages, 'symbols_used': max([st['symbols_used'] for st in stages] or [0]),
                    'entropy_bits_per_unit': float(sum(st['entropy_bits_per_unit'] for st in stages)),
                    'mean_distance': stages[-1]['mean_distance'] if stages else 0.0})
        return out


def _target_table(who, trainer, speaker2id_path, voices, t_speakers, enc_only):
    """The name -> Decoder row table of a folder driver: the speaker2id file, then the registered voices (zs_amd.voice.add_voices:
    {name: row}; a name in both keeps its speaker2id row).  ValueError for a target in neither, and for voices with the generator."""
    with open(speaker2id_path, 'r') as f_json:
        speaker2id = json.load(f_json)
    if voices:
        if not enc_only:
            raise ValueError('%s: voices convert through the autoencoder alone (enc_only): the stage-2 generator has rows for its '
                             'trained target speakers only' % who)
    missing = [t for t in t_speakers if t not in speaker2id and t not in (voices or {})]
    if missing:
        raise ValueError('%s: target speaker %r is not in %s%s' % (who, missing[0], speaker2id_path,
                                                                   ' nor a registered voice' if voices else ''))
    if voices:
        from .voice import resolve_speaker
        speaker2id = dict(speaker2id, **{t: resolve_speaker(t, speaker2id, voices) for t in t_speakers})
    n_rows = int(trainer.Decoder.c_a)
    bad = [t for t in t_speakers if not 0 <= int(speaker2id[t]) < n_rows] if voices else []
    if bad:
        raise ValueError('%s: target %r is row %d of a Decoder with %d rows' % (who, bad[0], int(speaker2id[bad[0]]), n_rows))
    return speaker2id


def _codebook_stats(codebook, trainer, file):
    """A folder driver's codebook, checked before anything is read: its _CodebookStats, or None without a codebook."""
    if codebook is None:
        return None
    _check_codebook(codebook, trainer)
    return _CodebookStats(codebook, file)


def _skip_log(tag):
    """(the manifest's 'skipped' list, skip(path, reason): prints the reason under [tag] and lists the input there)."""
    skipped = []

    def skip(path, reason):
        print('[%s] - skipped %s: %s' % (tag, path, reason))
        skipped.append({'input': path, 'reason': reason})
    return skipped, skip


def _scan_wavs(in_dir, skip):
    """(the *.wav of in_dir whose header can be read, sorted; their durations in seconds); skip(path, reason) takes the others."""
    from .preprocess import wav_info
    files, durations = [], []
    for path in sorted(glob.glob(os.path.join(in_dir, '*.wav'))):
        try:
            sr, n = wav_info(path)
            if sr <= 0:
                raise ValueError('sample rate %d' % sr)
        except (OSError, ValueError) as e:
            skip(path, 'cannot be read: %s' % e)
            continue
        files.append(path)
        durations.append(n / float(sr))
    return files, durations


def _write_manifest(path, in_dir, out_dir, t_speakers, enc_only, items, skipped, stats, voices, speaker2id, overlap=None, segment=None):
    """The manifest of a folder driver, written to `path` and returned: the run's fields, the driver's own `items`, what was
    skipped, and 'codebook' / 'voices' / 'overlap' / 'segment' (a zs_amd.segment.SegmentStats) when the run had them."""
    manifest = {'in_dir': in_dir, 'out_dir': out_dir, 'targets': t_speakers, 'sr': out_rate(), 'enc_only': bool(enc_only),
                'items': items, 'skipped': skipped}
    if overlap is not None:
        manifest['overlap'] = int(overlap)
    if stats is not None:
        manifest['codebook'] = stats.manifest()
    if voices:
        manifest['voices'] = {t: int(voices[t]) for t in t_speakers if t in voices and speaker2id[t] == voices[t]}
    if segment is not None:
        manifest['segment'] = segment.manifest()
    with open(path, 'w') as f:
        json.dump(manifest, f, indent=1)
    return manifest


def convert_dir(trainer, seg_len, in_dir, speaker2id_path, out_dir, t_speakers, enc_only, batch=64, n_iter=None, momentum=None,
                voices=None, codebook=None, codebook_file=None, overlap=None, segment=None):
    """Every *.wav of in_dir (any PCM / float format, any rate, channels averaged: preprocess.read_wav) to every target speaker of
    t_speakers, on the device from the samples to the waveform: {out_dir}/{target}/{stem}.wav (PCM16 at out_rate()) and .txt (the
    units), plus the manifest {out_dir}/convert_dir.json, which is returned.
    The items of convert_dir_plan go through the network and the vocoder in groups; a file's features (resampling, zs_trim,
    zs_pre_spectrogram) are computed once and shared by its targets, every item draws its own Gumbel noise as in cross_test, group
    i + 1 is enqueued before group i is written (defer=True), and one reader thread reads the files of the next group meanwhile.
    The targets are checked before anything is read or enqueued.  A file that cannot be read, or is too short after trimming, is
    skipped with a printed reason and listed in the manifest; the run goes on.
    voices: {name: Decoder row} of voices registered with zs_amd.voice.add_voices (enc_only alone): t_speakers may name them, and
    the manifest then lists them under 'voices'.
    codebook: a zs_amd.codebook.Codebook (codebook_file: where it came from) -- the units are snapped as resynth_batch snaps them,
    every .txt gets a sibling .idx.txt (one codeword index per line) and the manifest the entry 'codebook': {file, K, symbols_used,
    entropy_bits_per_unit, mean_distance} over the units written.  A zs_amd.vq.VectorCodebook for enc_mode 'continues': the same
    outputs, the .idx.txt being the unit file (the .txt holds what write_encodings writes for real-valued rows).  A
    zs_amd.rvq.ResidualCodebook: the .idx.txt holds one line of s' indices per frame (write_index_rows), s' the stages the codebook
    was told to use (with_stages; default all), and the manifest's 'codebook' entry gains 'S' and per-stage figures under 'stages'.
    overlap (frames; None: not asked for): resynth_batch's -- the units written are the same, the wavs are spoken from them in
    overlapping, cross-faded decode windows -- and the manifest gains 'overlap'.  A file of fewer than MIN_LEN frames, whose one unit
    cannot be spoken, is then skipped with a reason; enc_mode 'continues' needs a codebook (ValueError before anything is read).
    segment (lambda; None: not asked for; needs a bit or vector codebook): resynth_batch's -- the units written and spoken are the
    codewords of the path chosen for the whole utterance.  <name>.txt and <name>.idx.txt stay per-frame files, <name>.seg.txt beside
    them holds the runs `codeword duration` (zs_amd.segment.write_segments), and the manifest gains 'segment': {lambda, units,
    segments, mean_run_units, entropy_bits_per_segment, bits_per_second}.  A file of fewer than 2 units is skipped as with overlap."""
    from concurrent.futures import ThreadPoolExecutor
    from .preprocess import read_wav
    momentum = gl_momentum(momentum)
    seg_stats = None
    if segment is not None:
        segment = sg.check_lambda(segment, 'convert_dir: segment')
        sg.check_codebook(codebook, 'convert_dir: segment')
        seg_stats = sg.SegmentStats(segment, codebook.K)
    if overlap is not None:
        overlap = check_overlap_value(overlap, seg_len)
        if overlap and codebook is None and trainer.enc_mode == 'continues':
            raise ValueError("convert_dir: overlap = %d needs units to speak from, and enc_mode 'continues' has none without a codebook"
                             % overlap)
    stats = _codebook_stats(codebook, trainer, codebook_file)
    side = codebook.units() if codebook is not None else None    # how this kind of codebook writes an utterance's indices
    t_speakers = list(t_speakers)
    speaker2id = _target_table('convert_dir', trainer, speaker2id_path, voices, t_speakers, enc_only)
    if not enc_only:
        check_gen_targets(trainer, [speaker2id[t] for t in t_speakers])
    skipped, skip = _skip_log('Converter')
    files, durations = _scan_wavs(in_dir, skip)
    plan = convert_dir_plan(files, durations, t_speakers, out_dir, batch=batch)
    for s in plan['skipped']:
        skip(s['file'], s['reason'])
    groups = plan['groups']
    print('[Converter] - %d files, %d target speakers, %d conversions in %d groups' %
          (len(files) - len(plan['skipped']), len(t_speakers), sum(len(g) for g in groups), len(groups)))
    os.makedirs(out_dir, exist_ok=True)
    dev = trainer.device
    feats = {}                                # file -> (spec on the device, rate, samples, info), None for a skipped one
    done = []

    def read(group, have):
        out = {}
        for path in dict.fromkeys(it['file'] for it in group):
            if path not in have:
                try:
                    out[path] = read_wav(path)
                except Exception as e:                        # scipy raises ValueError and its own warnings-as-errors for bad files
                    out[path] = e
        return out

    def write(group, fin):
        res = fin()
        encs, wavs = res[0], res[1]
        if stats is not None:
            stats.add(res[2], res[3])
        for i, (it, e, w) in enumerate(zip(group, encs, to_out_sr(wavs))):
            os.makedirs(os.path.dirname(it['wav']), exist_ok=True)
            write_wav(it['wav'], w, out_rate())
            write_encodings(it['txt'], e)
            if stats is not None:
                side.write_idx(idx_path(it['txt']), res[2][i])
            if seg_stats is not None:
                r = sg.runs(res[2][i])
                sg.write_segments(sg.seg_path(it['txt']), r)
                seg_stats.add(r)
            done.append(it)

    with ThreadPoolExecutor(max_workers=1) as reader:
        fut = reader.submit(read, groups[0], ()) if groups else None

        def enqueue(numbered):
            nonlocal fut
            gi, group = numbered
            data = fut.result()
            if gi + 1 < len(groups):                          # the next group's files are read under this group's GPU work
                fut = reader.submit(read, groups[gi + 1], set(feats) | set(data))
            new = [p for p, d in data.items() if not isinstance(d, Exception)]
            for p, d in data.items():
                if isinstance(d, Exception):
                    skip(p, 'cannot be read: %s' % d)
                    feats[p] = None
            if new:
                specs, info = _wav_features([data[p][0] for p in new], [data[p][1] for p in new], dev, strict=False)
                for p, spec, inf in zip(new, specs, info):
                    if spec is None:
                        skip(p, 'utterance too short after trimming')
                        feats[p] = None
                    elif (overlap or segment is not None) and _unit_counts([spec], seg_len)[0] < 2:
                        skip(p, '%d frames give fewer than 2 units: nothing to speak from with %s' %
                             (inf['frames'], 'overlap' if overlap else 'segment'))
                        feats[p] = None
                    else:
                        feats[p] = (spec, data[p][1], len(data[p][0]), inf)
            live = [it for it in group if feats[it['file']] is not None]
            for it in live:
                _, it['rate'], it['samples'], inf = feats[it['file']]
                it['bounds'], it['frames'] = list(inf['bounds']), inf['frames']
            fin = None
            if live:
                fin = resynth_batch([feats[it['file']][0] for it in live], trainer, seg_len, [speaker2id[it['target']] for it in live],
                                    n_iter=n_iter, defer=True, enc_only=enc_only, momentum=momentum, codebook=codebook,
                                    want_idx=codebook is not None, **({'overlap': overlap} if overlap else {}),
                                    **({'segment': segment} if segment is not None else {}))
            later = {it['file'] for g in groups[gi + 1:gi + 2] for it in g}
            for p in [p for p in feats if p not in later]:    # a file's items are adjacent: done with, drop its device rows
                del feats[p]
            return (live, fin) if live else None

        _run_deferred(enumerate(groups), enqueue, write)
    items = [{'input': it['file'], 'rate': it['rate'], 'samples': it['samples'], 'target': it['target'], 'bounds': it['bounds'],
              'frames': it['frames'], 'wav': it['wav'], 'txt': it['txt']} for it in done]
    return _write_manifest(os.path.join(out_dir, 'convert_dir.json'), in_dir, out_dir, t_speakers, enc_only, items, skipped, stats,
                           voices, speaker2id, overlap=overlap, segment=seg_stats)


# ---------------------------------------------------------------------------------------------------
# a folder of unit files to speech (not in the reference, whose drivers always start from the spectrogram)
# ---------------------------------------------------------------------------------------------------

def synth_dir_plan(files, n_units, targets, out_dir, batch=64, max_batch_units=6000):
    """The work list of synth_dir, on the host alone: every (file, target) pair is an item.  n_units[i]: the units of files[i].
    Files are sorted by (units, path) so that a group pads little and the plan does not depend on the order they are listed in; a
    file's items are adjacent, in the order of `targets`.  A group takes items in that order while it holds at most `batch` of them
    and at most max_batch_units of padded length, counted as items x the longest (a single item above the cap is a group of its
    own; 6000 units are the 600 s of convert_dir_plan).  A file of fewer than 2 units goes to 'skipped' with a reason; two inputs
    with the same stem would write the same outputs: ValueError.
    Returns {'groups': [[item]], 'skipped': [{'file', 'reason'}]}, item = {'file', 'stem', 'target', 'units', 'wav'} with the output
    {out_dir}/{target}/{stem}.wav."""
    def reject(n):
        if n < 2:
            return '%d unit%s: fewer than 2 units' % (n, '' if n == 1 else 's')

    def item(f, stem, t, n):
        return {'file': f, 'stem': stem, 'target': t, 'units': n, 'wav': os.path.join(out_dir, t, stem + '.wav')}
    return _dir_plan('synth_dir_plan', files, [int(n) for n in n_units], 'unit counts', targets, batch, max_batch_units, reject, item)


def synth_dir(trainer, seg_len, in_dir, speaker2id_path, out_dir, t_speakers, enc_only, batch=64, n_iter=None, momentum=None, voices=None,
              codebook=None, codebook_file=None, overlap=None, segments=False):
    """Every *.txt of in_dir -- unit files as write_encodings writes them (--test_encode, --test, --convert_dir, encode_batch), one
    line of 0 / 1 per unit -- spoken in the voice of every target speaker of t_speakers: {out_dir}/{target}/{stem}.wav (PCM16 at
    out_rate()), plus the manifest {out_dir}/synth_dir.json, which is returned.
    The files are parsed and bit-packed on the host (E / 8 bytes per unit), the items of synth_dir_plan go through
    synth_units_batch in groups, and group i + 1 is enqueued before group i is written (defer=True).  The targets are checked
    before anything is read or enqueued.  A file that cannot be read as units of the Decoder's width, or holds fewer than 2
    units, is skipped with a printed reason and listed in the manifest; the run goes on.
    voices: as convert_dir's.
    codebook: as convert_dir's -- the units of every file are snapped before they are spoken, and what was spoken is written beside
    each wav: {stem}.txt (the snapped units) and {stem}.idx.txt (one codeword index per line); the manifest gains 'codebook'.
    A zs_amd.vq.VectorCodebook (enc_mode 'continues', refused without one): the *.idx.txt of in_dir are read instead (read_indices:
    one integer in [0, K) per line), <name>.idx.txt is spoken as {stem}.wav through synth_index_batch, and the indices spoken are
    written beside each wav as {stem}.idx.txt.
    overlap (frames; None: not asked for): synth_units_batch's / synth_index_batch's -- overlapping, cross-faded decode windows --
    and the manifest gains 'overlap', each item's 'fragments' holding the lengths of its windows.
    segments (needs a bit or vector codebook): the *.seg.txt of in_dir are read instead (zs_amd.segment.read_segments: one run
    `codeword duration` per line), <name>.seg.txt is spoken as {stem}.wav -- the runs are expanded to one codeword per unit and go
    through the same drivers -- and what was spoken is written beside each wav with its {stem}.seg.txt; the manifest gains 'segment'
    (lambda null: the files do not say what they were made with)."""
    momentum = gl_momentum(momentum)
    if segments:
        sg.check_codebook(codebook, 'synth_dir: segments')
    if overlap is not None:
        overlap = check_overlap_value(overlap, seg_len)
    t_speakers = list(t_speakers)
    speaker2id = _target_table('synth_dir', trainer, speaker2id_path, voices, t_speakers, enc_only)
    side = codebook.units() if codebook is not None else _BitUnits(None)      # which files are read, and how they are spoken and written
    side.check_speakable(trainer.enc_mode)                    # 'continues' speaks from the index files of a vector codebook alone
    if not enc_only:
        check_gen_targets(trainer, [speaker2id[t] for t in t_speakers])
    E = int(trainer.Decoder.c_in)
    stats = _codebook_stats(codebook, trainer, codebook_file)
    seg_stats = sg.SegmentStats(None, codebook.K) if segments else None
    skipped, skip = _skip_log('Synthesiser')
    units = {}
    for path in sorted(glob.glob(os.path.join(in_dir, '*.seg.txt' if segments else side.unit_glob))):
        try:
            units[path] = side.from_indices(sg.expand(sg.read_segments(path, codebook.K))) if segments else side.read_unit_file(path, E)
        except (OSError, ValueError) as e:
            skip(path, 'cannot be read: %s' % e)
    files = sorted(units)
    plan = synth_dir_plan(files, [len(units[f]) for f in files], t_speakers, out_dir, batch=batch)
    for s in plan['skipped']:
        skip(s['file'], s['reason'])
    groups = plan['groups']
    for it in (it for g in groups for it in g):
        it['stem'] = it['stem'][:-len('.seg')] if segments else side.spoken_stem(it['stem'])
        it['wav'] = os.path.join(out_dir, it['target'], it['stem'] + '.wav')
    print('[Synthesiser] - %d unit files, %d target speakers, %d syntheses in %d groups' %
          (len(files) - len(plan['skipped']), len(t_speakers), sum(len(g) for g in groups), len(groups)))
    os.makedirs(out_dir, exist_ok=True)
    done = []

    def write(group, fin):
        res = fin()
        if stats is not None:
            idxs, total = side.spoken(res, [units[it['file']] for it in group])
            stats.add(idxs, total)
        for i, (it, w) in enumerate(zip(group, to_out_sr(res[1]))):
            os.makedirs(os.path.dirname(it['wav']), exist_ok=True)
            write_wav(it['wav'], w, out_rate())
            if stats is not None:                             # what was spoken, beside the wav
                side.write_spoken(os.path.splitext(it['wav'])[0], idxs[i], E)
            if seg_stats is not None:
                r = sg.runs(idxs[i])
                sg.write_segments(os.path.splitext(it['wav'])[0] + '.seg.txt', r)
                seg_stats.add(r)
            done.append(it)

    def enqueue(group):
        return group, side.speak([units[it['file']] for it in group], trainer, seg_len, [speaker2id[it['target']] for it in group],
                                 enc_only=enc_only, n_iter=n_iter, defer=True, momentum=momentum, **({'overlap': overlap} if overlap else {}))

    def pieces(n):                                            # the lengths, in units, of what an utterance of n units is decoded in
        return [b - a for a, b in unit_windows(n, seg_len, overlap)] if overlap else unit_fragments(n, seg_len)

    _run_deferred(groups, enqueue, write)
    items = [{'input': it['file'], 'units': it['units'], 'fragments': pieces(it['units']), 'target': it['target'],
              'wav': it['wav']} for it in done]
    return _write_manifest(os.path.join(out_dir, 'synth_dir.json'), in_dir, out_dir, t_speakers, enc_only, items, skipped, stats, voices,
                           speaker2id, overlap=overlap, segment=seg_stats)


SINGLE_FILES = {            # convert.py:308-317: the utterances --test_single knows per source speaker
    'S015': './data/english/train/unit/S015_0361841101.wav',
    'S119': './data/english/train/unit/S119_1561145062.wav',
    'S130': './data/english/test/S130_3516588097.wav',
    'S089': './data/english/test/S089_1810826781.wav',
    'S378': './data/surprise/test/S378_117437.wav',
}


def test_single(trainer, seg_len, speaker2id_path, result_dir, enc_only, s_speaker, t_speaker, filename=None):
    """convert.py:303-340: one wav -> spectrogram (zs_amd.preprocess, STFT on the GPU) -> convert() -> result.wav (PCM16) +
    result.txt.  The reference then scores both files with the Google Web Speech API (convert.py:96-113); that needs the
    network and is not reproduced.  `filename` overrides the per-speaker table (not in the reference signature)."""
    from .preprocess import get_spectrograms
    with open(speaker2id_path, 'r') as f_json:
        speaker2id = json.load(f_json)
    if filename is None:
        if s_speaker not in SINGLE_FILES:
            raise NotImplementedError('Please modify path manually!')
        filename = SINGLE_FILES[s_speaker]
    _, spec = get_spectrograms(filename)
    wav_data, encodings = convert(trainer, seg_len, src_speaker_spec=spec, src_speaker=s_speaker, tar_speaker=t_speaker, utt_id='',
                                  speaker2id=speaker2id, result_dir=result_dir, enc_only=enc_only, save=[])
    write_wav(os.path.join(result_dir, 'result.wav'), to_out_sr([wav_data])[0], out_rate())
    write_encodings(os.path.join(result_dir, 'result.txt'), encodings)
    print('Testing on source speaker {} and target speaker {}, output shape: {}'.format(s_speaker, t_speaker, wav_data.shape))
    print('Comparing ASR result - skipped (the reference calls the Google Web Speech API here; no network)')
    return wav_data, encodings


def test_encode(trainer, seg_len, test_path, data_path, result_dir, flag='test', codebook=None, segment=None):
    """convert.py:342-360.  codebook (not in the reference): every file's units are snapped to their codewords before they are
    written, and each .txt gets a sibling .idx.txt with one codeword index per line.  Under a zs_amd.vq.VectorCodebook ('continues')
    the .txt is written as without a codebook and the .idx.txt holds the nearest codeword of every encoded frame.
    segment (lambda; needs a bit or vector codebook): the codewords and indices written are those of the path chosen for the whole
    file (zs_amd.segment), and its runs go to a sibling .seg.txt."""
    if segment is not None:
        segment = sg.check_lambda(segment, 'test_encode: segment')
        sg.check_codebook(codebook, 'test_encode: segment')
    if codebook is not None:
        _check_codebook(codebook, trainer)
    files = sorted(glob.glob(os.path.join(test_path, '*.wav')))
    feeds = [{'s_id': f.split('/')[-1].split('_')[0], 'utt_id': f.split('/')[-1].split('_')[1].split('.')[0]} for f in files]
    print('[Tester] - Number of files to encoded: ', len(feeds))
    dir_path = os.path.join(result_dir, f'{flag}/')
    os.makedirs(dir_path, exist_ok=True)
    with _open_h5(data_path) as f_h5:
        for feed in feeds:
            if codebook is None:
                encode(f_h5[f"test/{feed['s_id']}/{feed['utt_id']}/lin"][()], trainer, seg_len, s_speaker=feed['s_id'],
                       utt_id=feed['utt_id'], result_dir=dir_path)
                continue
            units = encode(f_h5[f"test/{feed['s_id']}/{feed['utt_id']}/lin"][()], trainer, seg_len, save=False)
            txt = os.path.join(dir_path, f"{feed['s_id']}_{feed['utt_id']}.txt")
            codebook.units().write_encoded(txt, units, trainer.device, **({'segment': segment} if segment is not None else {}))


# ---------------------------------------------------------------------------------------------------
# target speaker classification (convert.py:364-414), batched
# ---------------------------------------------------------------------------------------------------

TCLF_SPEAKERS = ('V001', 'V002', 'None')           # the TargetClassifier's argmax 0 / 1 / 2 (convert.py:401-407)


def tclf_plan(frames, seg_len):
    """The fragments target_classify scores, as [(utterance, start)]: each is spec[start:start + seg_len] (convert.py:379-395).
    An utterance shorter than seg_len is zero-padded to seg_len first, so, by the `spec[idx:-1]` tail rule, any utterance of
    seg_len frames or fewer raises RuntimeError (as in the reference); the rows a fragment reads are all real frames."""
    plan = []
    for u, n in enumerate(frames):
        for start, _ in fragments(max(int(n), seg_len), seg_len):
            plan.append((u, start))
    return plan


def tclf_targets(speakers):
    """Target class per speaker name for zs_tclf_score: V001 0, V002 1, 'None' 2 (the name the reference compares its third class
    with), anything else -1 (never correct)."""
    return np.array([TCLF_SPEAKERS.index(s) if s in TCLF_SPEAKERS else -1 for s in speakers], dtype=np.int32)


def tclf_predict(logits):
    """The reference's per-fragment decision on host logits [n, 3]: numpy argmax (ties to the first index) -> speaker name."""
    return [TCLF_SPEAKERS[int(np.argmax(l))] for l in np.asarray(logits)]


def classify_batch(specs, trainer, seg_len, max_batch=256):
    """TargetClassifier eval-mode logits of every fragment of a batch of utterances, on the device, with no host synchronisation.
    specs: a list of normalised magnitude spectrograms [T_i, 513] (host arrays or torch tensors), or the pair (mag [n, T_max, 513]
    on the trainer's device, frames [n]) that preprocess.get_spectrograms_device returns.  One zs_frag_gather launch copies every
    fragment of tclf_plan into a contiguous [n_frag, seg_len, 513] batch, then the classifier runs on chunks of at most max_batch.
    Returns (logits fp32 [n_frag, 3] on the device, plan [(utterance, start)])."""
    dev = trainer.device
    if isinstance(specs, tuple):
        mag, frames = specs
        frames = [int(t) for t in frames]
        if not (torch.is_tensor(mag) and mag.device == dev and mag.dtype == torch.float32 and mag.dim() == 3 and mag.shape[2] == 513):
            raise ValueError('classify_batch: (mag, frames) needs mag fp32 [n, T_max, 513] on %s' % dev)
        if len(frames) != mag.shape[0] or max(frames) > mag.shape[1]:
            raise ValueError('classify_batch: frames do not fit mag %s' % (tuple(mag.shape),))
        src, n_utt, T_max = mag.contiguous(), int(mag.shape[0]), int(mag.shape[1])
        plan = tclf_plan(frames, seg_len)
        table = [(u, s) for u, s in plan]
    else:
        frames = [int(s.shape[0]) for s in specs]
        if any(int(s.shape[1]) != 513 for s in specs):
            raise ValueError('classify_batch: spectrograms must have 513 bins')
        plan = tclf_plan(frames, seg_len)
        src, offs = _stage_rows(specs, dev)            # every utterance back to back: one 'utterance' of sum(T_i) + 1 rows
        n_utt, T_max = 1, int(src.shape[0])
        table = [(0, int(offs[u]) + s) for u, s in plan]
    n_frag = len(plan)
    clf = trainer.TargetClassifier
    clf.eval()
    eng = clf._engine()
    st = torch.cuda.current_stream(dev).cuda_stream
    tab = torch.tensor(table, dtype=torch.int32).reshape(n_frag, 2).pin_memory().to(dev, non_blocking=True)
    frags = torch.empty(n_frag, seg_len, 513, dtype=torch.float32, device=dev)
    L.call('zs_frag_gather', 'ZsFragGather', st, src=L.ptr(src), utt_stride=T_max * 513, n_utt=n_utt, T_max=T_max, table=L.ptr(tab),
           n_frag=n_frag, seg_len=seg_len, dst=L.ptr(frags))
    out = torch.empty(n_frag, clf.n_class, dtype=torch.float32, device=dev)
    for lo in range(0, n_frag, max_batch):
        hi = min(n_frag, lo + max_batch)
        _, logits = eng.forward(frags[lo:hi], 'tclf_eval', False, classify=True, need_val=False)
        out[lo:hi].copy_(logits)
    return out, plan


def target_classify(trainer, seg_len, synthesis_list, result_dir, flag='test', max_batch=256):
    """convert.py:364-414: the accuracy of the TargetClassifier on the wavs --test wrote, {result_dir}/{flag}/{tar}_{utt}.wav for
    each line of the synthesis list, over every fragment of every utterance (V001 / V002 / 'None' against the target speaker).
    All wavs go through one zs_pre_spectrogram batch, the fragments through classify_batch, the scoring through zs_tclf_score;
    the only host synchronisation is the read of the two counts at the end (wavs that are not at hp.sr, written by another tool
    or with --out_sr, are resampled first, which brings them back to the host once).  Prints and returns the accuracy."""
    from .preprocess import get_spectrograms_device, read_wav
    dir_path = os.path.join(result_dir, f'{flag}/')
    with open(synthesis_list, 'r') as f:
        lines = [l for l in f.readlines() if l.strip()]
    wavs, rates, tars = [], [], []
    for line in lines:
        line = line.split('\n')[0].split(' ')
        utt_id = line[0].split('/')[1].split('_')[1]
        tar_speaker = line[1]
        wav, sr = read_wav(os.path.join(dir_path, f'{tar_speaker}_{utt_id}.wav'))
        wavs.append(wav)
        rates.append(sr)
        tars.append(tar_speaker)
    if not getattr(trainer, 'tclf_loaded', False):
        print('[Converter] - warning: no target_classifier was loaded (hps load_model_list does not name it, or loading failed): '
              'scoring with untrained weights')
    if not wavs:
        print('Classification Acc: {:.3f}'.format(float('nan')))
        return float('nan')
    dev = trainer.device
    mag, frames = get_spectrograms_device(wavs, device=dev, sr=rates)      # files not at hp.sr: one resampling launch per rate
    logits, plan = classify_batch((mag, frames), trainer, seg_len, max_batch=max_batch)
    target = torch.from_numpy(tclf_targets([tars[u] for u, _ in plan])).pin_memory().to(dev, non_blocking=True)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    L.call('zs_tclf_score', 'ZsTclfScore', torch.cuda.current_stream(dev).cuda_stream, logits=L.ptr(logits), ld=logits.stride(0),
           target=L.ptr(target), n_frag=len(plan), correct=L.ptr(counts), count=L.ptr(counts, 1))
    correct, count = counts.cpu().tolist()                    # the one synchronisation
    acc = correct / float(count)
    print('Classification Acc: {:.3f}'.format(acc))
    return acc
