"""Feature extraction and dataset files feeding the --train_ae path (reference preprocess.py).

* `get_spectrograms(sound_file)` / `get_spectrograms_batch(wavs)` -- preprocess.py:227-258: trim -> pre-emphasis -> STFT ->
  |.| -> mel(80) -> dB -> normalise, with the STFT / dB / mel product on the GPU (`zs_pre_spectrogram`, `zs_pre_mel`); the trim
  (librosa.effects.trim defaults) is host NumPy, or, with get_spectrograms_device(trim_on='device'), `zs_trim` on audio that
  stays in HBM (`trim_device`; the spectrogram kernel reads the trimmed window in place).  Sound files are read with scipy (`read_wav`: 8 / 16 / 32-bit PCM or float wav
  at any rate); a file that is not at hp.sr is resampled to it on the GPU as the reference's librosa.load does (`zs_resample`,
  zs_amd.resample: a restatement of resampy's kaiser_best, sample-level parity unpinned), a file at hp.sr is used as it is.
* `make_dataset`, `Sampler`, `make_samples`, `preprocess` -- preprocess.py:26-225: the `{train,test}/<speaker>/<utt>/{lin,mel}`
  float32 layout and the `[{speaker, i, t}]` index JSON.  The container is HDF5 when h5py is importable (the reference's
  format); otherwise the same keys go into an .npz archive (`NpzStore`), which `dataloader.Dataset` also reads.
"""
import glob
import json
import os
import random
from collections import defaultdict, namedtuple

import numpy as np
import torch

from . import _lib as L
from .convert import TRIM_FRAME, TRIM_HOP, trim
from .dataloader import NpzStore, open_store
from .hps import hp


def mel_basis(sr=None, n_fft=None, n_mels=None):
    """librosa.filters.mel(sr, n_fft, n_mels) defaults (Slaney scale, area-normalised triangles), float32 [n_mels, 1+n_fft//2]."""
    sr, n_fft, n_mels = sr or hp.sr, n_fft or hp.n_fft, n_mels or hp.n_mels
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp

    def hz_to_mel(f):
        f = np.asarray(f, dtype=np.float64)
        return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-12) / min_log_hz) / logstep, f / f_sp)

    def mel_to_hz(m):
        m = np.asarray(m, dtype=np.float64)
        return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)

    fft_f = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(sr / 2.0), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    w = np.maximum(0, np.minimum(-ramps[:-2] / fdiff[:-1, None], ramps[2:] / fdiff[1:, None]))
    w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w.astype(np.float32)


_BASIS = {}


def _device_of(device):
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if dev.type != 'cuda':
        raise L.ZsError('zs_amd.preprocess runs on an MI355X only (there is no CPU path)')
    return dev


def _pinned(a, dev):
    """Host array -> device tensor through a pinned staging buffer, asynchronously (a pageable .to() waits for the stream)."""
    return torch.from_numpy(a).pin_memory().to(dev, non_blocking=True)


def _enqueue_spectrograms(wavs, do_trim, dev, with_amp):
    """Trim on the host (preprocess.py:238), then ONE zs_pre_spectrogram launch over the zero-padded batch, enqueued without a
    host synchronisation.  Returns (mag fp32 [n, T_max, 513], amp (the same shape) or None, samples int32 [n] host array)."""
    ys = []
    for w in wavs:
        y = np.asarray(w, dtype=np.float32)
        if do_trim:
            y = trim(y)[0].astype(np.float32)                        # librosa.effects.trim(y)   preprocess.py:238
        if len(y) < 2:
            raise ValueError('utterance too short after trimming')
        ys.append(y)
    n = len(ys)
    lens = np.array([len(y) for y in ys], dtype=np.int32)
    ld = int(lens.max())
    T_max = 1 + ld // hp.hop_length
    host = np.zeros((n, ld), dtype=np.float32)
    for i, y in enumerate(ys):
        host[i, :len(y)] = y
    wav = _pinned(host, dev)
    ns = _pinned(lens, dev)
    mag = torch.zeros(n, T_max, 513, dtype=torch.float32, device=dev)
    amp = torch.zeros(n, T_max, 513, dtype=torch.float32, device=dev) if with_amp else None
    st = torch.cuda.current_stream(dev).cuda_stream
    L.call('zs_pre_spectrogram', 'ZsPreSpec', st, wav=L.ptr(wav), wav_ld=ld, n_samples=L.ptr(ns), n_utt=n, T_max=T_max,
           preemph=hp.preemphasis, ref_db=float(hp.ref_db), max_db=float(hp.max_db), mag=L.ptr(mag), mag_ld=513, amp=L.ptr(amp))
    return mag, amp, lens


def _to_hp_sr(wavs, sr, dev):
    """The wavs at hp.sr, in their order.  sr: None, one rate for all, or one per wav.  Entries already at hp.sr are passed through
    untouched (None / hp.sr for all: the very list comes back); the others are grouped by rate, one zs_resample launch per distinct
    rate, every launch enqueued before the first result is fetched, and come back to the host as float32 arrays."""
    if sr is None:
        return wavs
    rates = [int(sr)] * len(wavs) if np.ndim(sr) == 0 else [int(r) for r in sr]
    if len(rates) != len(wavs):
        raise ValueError('sr must be one rate or one rate per wav (%d rates for %d wavs)' % (len(rates), len(wavs)))
    if all(r == hp.sr for r in rates):
        return wavs
    from .resample import resample_batch
    out = list(wavs)
    pending = []
    for rate in sorted({r for r in rates if r != hp.sr}):
        idx = [i for i, r in enumerate(rates) if r == rate]
        pending.append((idx,) + resample_batch([wavs[i] for i in idx], rate, hp.sr, device=dev, to_host=False))
    for idx, dst, lens in pending:
        dst_h = dst.cpu().numpy()
        for k, i in enumerate(idx):
            out[i] = dst_h[k, :lens[k]].copy()
    return out


def get_spectrograms_batch(wavs, do_trim=True, device=None, sr=None):
    """wavs: list of 1-D float arrays at hp.sr, or at the rate(s) `sr` (an int, or one int per wav): those not at hp.sr are resampled
    first (_to_hp_sr).  Returns a list of (mel [T, 80], mag [T, 513]) float32 NumPy pairs."""
    dev = _device_of(device)
    wavs = _to_hp_sr(wavs, sr, dev)
    mag, amp, lens = _enqueue_spectrograms(wavs, do_trim, dev, True)
    n, T_max = mag.shape[0], mag.shape[1]
    mel = torch.zeros(n, T_max, hp.n_mels, dtype=torch.float32, device=dev)
    key = (dev.index, hp.sr, hp.n_fft, hp.n_mels)
    if key not in _BASIS:
        _BASIS[key] = torch.from_numpy(mel_basis()).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    fn = L.lib().zs_pre_mel
    L.check(fn(L.ptr(amp), L.ptr(_BASIS[key]), L.ptr(mel), n * T_max, hp.n_mels, float(hp.ref_db), float(hp.max_db), st), 'zs_pre_mel')
    mag_h, mel_h = mag.cpu().numpy(), mel.cpu().numpy()
    out = []
    for i in range(n):
        T = 1 + int(lens[i]) // hp.hop_length
        out.append((mel_h[i, :T].copy(), mag_h[i, :T].copy()))
    return out


def trim_device(wav, n_samples, top_db=60):
    """librosa.effects.trim (convert.trim is the definition) of a ragged batch on the device: ONE zs_trim call on the current
    stream, no synchronisation.  wav fp32 [n, ld] and n_samples int32 [n] are tensors on the GPU (row u holds n_samples[u] samples;
    the slack behind them is never read).  Returns bounds int32 [n, 2] = (start, stop) on the device."""
    if not (torch.is_tensor(wav) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() == 2 and wav.is_contiguous()):
        raise ValueError('trim_device: wav must be a contiguous fp32 [n, ld] tensor on the GPU')
    dev = wav.device
    n, ld = int(wav.shape[0]), int(wav.shape[1])
    if not (torch.is_tensor(n_samples) and n_samples.device == dev and n_samples.dtype == torch.int32 and n_samples.is_contiguous()
            and n_samples.numel() == n):
        raise ValueError('trim_device: n_samples must be a contiguous int32 [n] tensor on the device of wav')
    bounds = torch.empty(n, 2, dtype=torch.int32, device=dev)
    work = torch.empty(max(1, L.lib().zs_trim_workspace_bytes(n, ld, TRIM_FRAME, TRIM_HOP) // 8), dtype=torch.float64, device=dev)
    L.call('zs_trim', 'ZsTrim', torch.cuda.current_stream(dev).cuda_stream, wav=L.ptr(wav), wav_ld=ld, n_samples=L.ptr(n_samples), n_utt=n,
           frame_length=TRIM_FRAME, hop=TRIM_HOP, top_db=float(top_db), bounds=L.ptr(bounds), work=L.ptr(work), work_bytes=work.numel() * 8)
    return bounds


def _device_audio(wavs, sr, dev):
    """The wavs at hp.sr as ONE padded buffer on the device, none of them coming back to the host: (wav fp32 [n, ld], lens int32 [n]
    host array).  Entries at hp.sr go up through pinned staging; the others are resampled there, one zs_resample launch per distinct
    rate (their lengths are resample.out_length, known on the host), and every group is copied into its rows on the device."""
    n = len(wavs)
    rates = [hp.sr] * n if sr is None else ([int(sr)] * n if np.ndim(sr) == 0 else [int(r) for r in sr])
    if len(rates) != n:
        raise ValueError('sr must be one rate or one rate per wav (%d rates for %d wavs)' % (len(rates), n))
    ys = [np.asarray(w, dtype=np.float32) for w in wavs]
    if any(y.ndim != 1 for y in ys):
        raise ValueError('the wavs must be 1-D arrays')
    lens = np.zeros(n, dtype=np.int32)
    groups = []                                                              # (rows, device tensor [len(rows), ld_g])
    for rate in sorted(set(rates)):
        idx = [i for i, r in enumerate(rates) if r == rate and len(ys[i]) > 0]
        if not idx:
            continue
        if rate == hp.sr:
            glens = [len(ys[i]) for i in idx]
            host = np.zeros((len(idx), max(glens)), dtype=np.float32)
            for k, i in enumerate(idx):
                host[k, :glens[k]] = ys[i]
            part = _pinned(host, dev)
        else:
            from .resample import resample_batch
            part, glens = resample_batch([ys[i] for i in idx], rate, hp.sr, device=dev, to_host=False)
        lens[idx] = glens
        groups.append((idx, part))
    ld = max(1, int(lens.max()) if n else 1)
    if len(groups) == 1 and groups[0][0] == list(range(n)):
        return groups[0][1], lens                                           # one rate, no empty row: the buffer as it is
    wav = torch.zeros(n, ld, dtype=torch.float32, device=dev)
    for idx, part in groups:
        rows = _pinned(np.asarray(idx, dtype=np.int64), dev)
        wav[:, :part.shape[1]].index_copy_(0, rows, part)
    return wav, lens


def _spectrograms_on_device(wavs, do_trim, dev, sr, strict=True):
    """get_spectrograms_device(trim_on='device'): (mag, frames int64 [n], bounds int64 [n, 2]) with the audio never back on the
    host.  The one synchronisation is the copy of the n x 2 bounds, which sizes T_max (none at all without the trim).
    strict=False: an utterance of fewer than 2 samples after trimming gets frames 0 and a zero row instead of the ValueError."""
    wav, lens = _device_audio(wavs, sr, dev)
    n, ld = int(wav.shape[0]), int(wav.shape[1])
    ns = _pinned(lens, dev)
    start = None
    if do_trim:
        bounds_d = trim_device(wav, ns)
        bounds = bounds_d.cpu().numpy().astype(np.int64)                     # the synchronisation
        start = bounds_d[:, 0].contiguous()
        ns = (bounds_d[:, 1] - bounds_d[:, 0]).contiguous()
    else:
        bounds = np.stack([np.zeros(n, dtype=np.int64), lens.astype(np.int64)], axis=1)
    kept = bounds[:, 1] - bounds[:, 0]
    if strict and (kept < 2).any():
        raise ValueError('utterance too short after trimming')
    frames = np.where(kept < 2, 0, 1 + kept // hp.hop_length)
    T_max = max(1, int(frames.max()))
    mag = torch.zeros(n, T_max, 513, dtype=torch.float32, device=dev)
    if (kept >= 2).any():
        L.call('zs_pre_spectrogram', 'ZsPreSpec', torch.cuda.current_stream(dev).cuda_stream, wav=L.ptr(wav), wav_ld=ld,
               n_samples=L.ptr(ns), n_utt=n, T_max=T_max, preemph=hp.preemphasis, ref_db=float(hp.ref_db), max_db=float(hp.max_db),
               mag=L.ptr(mag), mag_ld=513, start=L.ptr(start))
    return mag, frames, bounds


def get_spectrograms_device(wavs, do_trim=True, device=None, sr=None, trim_on='host'):
    """The magnitudes of get_spectrograms_batch left on the device: (mag fp32 [n, T_max, 513] on `device`, frames int64 [n] host
    array).  Utterance i is mag[i, :frames[i]]; the rows behind it are zeros.  No mel, no host copy.
    trim_on='host' (default): the trim is host NumPy.  No synchronisation, unless an input needs resampling (`sr` names a rate
    other than hp.sr): the resampled audio comes back to the host for the trim, which synchronises once.
    trim_on='device': the same values, bit for bit, with the audio never back on the host -- resampled inputs stay in HBM, zs_trim
    finds the bounds there, their n x 2 copy to the host (to size T_max) is the only synchronisation, and zs_pre_spectrogram reads
    each trimmed window in place (ZsPreSpec.start)."""
    dev = _device_of(device)
    if trim_on == 'device':
        return _spectrograms_on_device(wavs, do_trim, dev, sr)[:2]
    if trim_on != 'host':
        raise ValueError("trim_on must be 'host' or 'device' (got %r)" % (trim_on,))
    mag, _, lens = _enqueue_spectrograms(_to_hp_sr(wavs, sr, dev), do_trim, dev, False)
    return mag, 1 + lens.astype(np.int64) // hp.hop_length


def wav_info(sound_file):
    """(sample rate, samples per channel) from the header of a RIFF wav file, without reading the audio.  ValueError for a file
    that is not one."""
    import struct
    with open(sound_file, 'rb') as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b'RIFF' or head[8:12] != b'WAVE':
            raise ValueError('%s is not a RIFF/WAVE file' % sound_file)
        fmt = None
        while True:
            ck = f.read(8)
            if len(ck) < 8:
                raise ValueError('%s has no data chunk' % sound_file)
            tag, size = ck[:4], struct.unpack('<I', ck[4:])[0]
            if tag == b'fmt ':
                body = f.read(size + (size & 1))
                if len(body) < 16:
                    raise ValueError('%s has a truncated fmt chunk' % sound_file)
                fmt = struct.unpack('<HHIIHH', body[:16])
            elif tag == b'data':
                if fmt is None or fmt[3] == 0 and fmt[4] == 0:
                    raise ValueError('%s has no usable fmt chunk before its data' % sound_file)
                block = fmt[4] if fmt[4] else max(1, fmt[1] * fmt[5] // 8)
                return int(fmt[2]), int(size // block)
            else:
                f.seek(size + (size & 1), 1)


def read_wav(sound_file):
    """(mono float32 waveform in [-1, 1], sample rate) of a wav file, as stored: 8-bit (unsigned), 16- and 32-bit PCM are scaled
    by their full range, float32 / float64 are taken as they are; channels are averaged after the scaling (so an integer stereo
    file is scaled too).  No GPU."""
    from scipy.io import wavfile
    sr, data = wavfile.read(sound_file)
    if data.dtype == np.int16:
        data = data.astype(np.float32) / 32768.0
    elif data.dtype == np.int32:
        data = data.astype(np.float32) / 2147483648.0
    elif data.dtype == np.uint8:
        data = (data.astype(np.float32) - 128.0) / 128.0
    if data.ndim > 1:
        data = data.mean(axis=1)
    return data.astype(np.float32), int(sr)


def load_wav(sound_file):
    """hp.sr (16 kHz) mono waveform in [-1, 1]: librosa.load(sound_file, sr=hp.sr).  A file at hp.sr is returned as read; any other
    rate is resampled on the GPU (zs_amd.resample)."""
    data, sr = read_wav(sound_file)
    if sr == hp.sr:
        return data
    from .resample import resample_batch
    return resample_batch([data], sr, hp.sr)[0]


def get_spectrograms(sound_file):
    """preprocess.py:227-258: (mel [T, n_mels], mag [T, 1+n_fft/2]) normalised log spectrograms of a sound file."""
    data, sr = read_wav(sound_file)
    return get_spectrograms_batch([data], sr=sr)[0]


def make_dataset(grps, seg_len, root_dir, make_test=False, pad=True, batch=32):
    """preprocess.py:77-107: every `<speaker>_<segment>.wav` under root_dir -> `<speaker>/<segment>/{mel,lin}`."""
    filenames = sorted(glob.glob(os.path.join(root_dir, '*_*.wav')))
    grp = grps[1] if make_test else grps[0]
    print('Number of speakers: ', len({os.path.basename(f).split('_')[0] for f in filenames}))
    for lo in range(0, len(filenames), batch):
        chunk = filenames[lo:lo + batch]
        read = [read_wav(f) for f in chunk]
        feats = get_spectrograms_batch([w for w, _ in read], sr=[r for _, r in read])     # one resampling launch per distinct rate
        for filename, (mel_spec, lin_spec) in zip(chunk, feats):
            speaker_id, segment_id = os.path.basename(filename)[:-len('.wav')].split('_')
            if pad and len(lin_spec) <= seg_len:                                       # preprocess.py:95-100
                mel_spec = np.concatenate((mel_spec, np.zeros((seg_len - mel_spec.shape[0] + 1, mel_spec.shape[1]))), axis=0)
                lin_spec = np.concatenate((lin_spec, np.zeros((seg_len - lin_spec.shape[0] + 1, lin_spec.shape[1]))), axis=0)
            grp.create_dataset('{}/{}/mel'.format(speaker_id, segment_id), data=mel_spec, dtype=np.float32)
            grp.create_dataset('{}/{}/lin'.format(speaker_id, segment_id), data=lin_spec, dtype=np.float32)


class Sampler(object):
    """preprocess.py:124-214: draws `index(speaker, i, t)` training segments, speakers weighted by their utterance counts."""

    def __init__(self, h5_path, dset='train', seg_len=64, speaker2id_path='', make_object='all'):
        self.dset, self.seg_len, self.speaker2id_path = dset, seg_len, speaker2id_path
        self.f = open_store(h5_path, 'r')
        if 'english' in h5_path:
            self.target_speakers = ['V001', 'V002']
        elif 'surprise' in h5_path:
            self.target_speakers = ['V001']
        else:
            raise NotImplementedError('Invalid dataset.hdf5 name!')
        speakers = self._keys(dset)
        if make_object == 'all':
            self.speaker_used = speakers
            self.save_speaker2id()
        elif make_object == 'source':
            self.get_speaker2id()
            self.speaker_used = [s for s in speakers if s not in self.target_speakers]
        elif make_object == 'target':
            self.get_speaker2id()
            self.speaker_used = self.target_speakers
        else:
            raise NotImplementedError('Invalid make object!')
        self.speaker2utts = {s: self._keys('%s/%s' % (dset, s)) for s in self.speaker_used}
        self.rm_too_short_utt()
        self.speaker_weight = [len(self.speaker2utts[s]) / self.total_utt for s in self.speaker_used]
        self.indexer = namedtuple('index', ['speaker', 'i', 't'])

    def _keys(self, prefix):
        return self.f.keys(prefix) if isinstance(self.f, NpzStore) else sorted(list(self.f[prefix].keys()))

    def _len(self, speaker, utt):
        return self.f['%s/%s/%s/lin' % (self.dset, speaker, utt)].shape[0]

    def get_num_utts(self):
        return sum(len(self.speaker2utts[s]) for s in self.speaker_used)

    def rm_too_short_utt(self, limit=None):
        self.total_utt = self.get_num_utts()
        limit = self.seg_len if limit is None else limit
        for s in self.speaker_used:
            self.speaker2utts[s] = [u for u in self.speaker2utts[s] if self._len(s, u) > limit]
        print('[Sampler] - %i too short utterences out of a total of %i are removed.' % (self.total_utt - self.get_num_utts(), self.total_utt))

    def sample(self):
        speaker = np.random.choice(self.speaker_used, p=self.speaker_weight)
        utt_id = random.sample(self.speaker2utts[speaker], 1)[0]
        t = random.randint(0, self._len(speaker, utt_id) - self.seg_len)
        return self.indexer(speaker=self.speaker2id[speaker], i='%s/%s' % (speaker, utt_id), t=t)

    def save_speaker2id(self):
        self.speaker2id = {s: i for i, s in enumerate(self.speaker_used)}
        with open(self.speaker2id_path, 'w') as f:
            f.write(json.dumps(self.speaker2id))

    def get_speaker2id(self):
        with open(self.speaker2id_path, 'r') as f:
            self.speaker2id = json.load(f)


def make_samples(h5py_path, json_path, speaker2id_path, make_object, seg_len=64, n_samples=200000, dset='train'):
    """preprocess.py:110-121."""
    sampler = Sampler(h5py_path, dset, seg_len, speaker2id_path, make_object)
    samples = [sampler.sample()._asdict() for _ in range(n_samples)]
    with open(json_path, 'w') as f_json:
        json.dump(samples, f_json, indent=4, separators=(',', ': '))


def preprocess(source_path, target_path, test_path, dataset_path, index_path, index_source_path, index_target_path, speaker2id_path,
               seg_len=128, n_samples=200000, dset='train', remake=True):
    """preprocess.py:26-74."""
    if remake or not (os.path.isfile(dataset_path) or os.path.isfile(dataset_path + '.npz')):
        with open_store(dataset_path, 'w') as f:
            grps = [f.create_group('train'), f.create_group('test')]
            make_dataset(grps, seg_len, root_dir=source_path)
            make_dataset(grps, seg_len, root_dir=target_path)
            make_dataset(grps, seg_len, root_dir=test_path, make_test=True, pad=False)
    for path, obj in ((index_path, 'all'), (index_source_path, 'source'), (index_target_path, 'target')):
        make_samples(dataset_path, path, speaker2id_path, make_object=obj, seg_len=seg_len, n_samples=n_samples, dset=dset)
