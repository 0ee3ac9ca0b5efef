"""Generate tests/golden/fgla_speech.npz: three of the reference's demo outputs (docs/exp/*/N.wav, audio its convert program
wrote) as int16 samples, the real speech the fast Griffin-Lim tests measure spectral convergence on.  Only data is written:
  - 'wav.<i>': int16 samples of utterance i, as stored in the file (16 kHz mono PCM16);
  - 'names': the files' paths under docs/exp/, in the order of i.
The archive is written with fixed zip metadata and key order, so a re-run reproduces it byte for byte.  Run (on a machine with
the reference checked out; nothing else reads the reference tree):
    python tools/make_golden_fgla.py REFERENCE_ROOT
"""
import io
import os
import sys
import wave
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'fgla_speech.npz')
FILES = ['128-m-1024/2.wav', '128-c-1024/4.wav', 's2-128-m-1024/1.wav']     # 432, 336 and 259 frames


def read_pcm16(path):
    with wave.open(path, 'rb') as f:
        if f.getnchannels() != 1 or f.getsampwidth() != 2 or f.getframerate() != 16000:
            raise ValueError('%s: expected 16 kHz mono PCM16' % path)
        return np.frombuffer(f.readframes(f.getnframes()), dtype='<i2').astype(np.int16)


def write_npz(path, arrays):
    """np.savez_compressed layout, with fixed zip dates and key order (np.savez stamps the current time)."""
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue())


def main(ref_root):
    out = {'names': np.array(FILES)}
    for i, name in enumerate(FILES):
        out['wav.%d' % i] = read_pcm16(os.path.join(ref_root, 'docs', 'exp', name))
        print('[golden] %s: %d samples' % (name, len(out['wav.%d' % i])))
    write_npz(OUT, out)
    print('[golden] wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
