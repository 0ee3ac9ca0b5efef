"""Held-out validation of the stage-1 autoencoder during training (no counterpart in the reference, whose --train_ae loop reports
the L1 loss of the batch it just trained on and nothing else).

This module is the host side: where the validation set comes from (ValidSet), the flag checks of main.py (check_flags), the
arithmetic that turns the device tables of zs_eval_accum into a record (finish), the record file `<ckpt_dir>/valid.jsonl` and what
a train-state file says about validation (describe / validate).  The device side -- a forward-only plan beside the training step,
with inputs, scalars and a noise stream of its own -- is trainer.ValidStep.

Noise: an eval-mode encoder draws Gumbel noise (reference behaviour).  Validation batch m draws it from the counter-hash stream
seeded VALID_SEED + m, never from torch's generators, so every validation sees the same data with the same noise and a training
run with validation computes, bit for bit, what it computes without."""
import hashlib
import json
import math
import os
from collections import namedtuple

import numpy as np

VALID_SEED = 0x56414C4944000000                    # 'VALID' in the high bytes; batch m draws from VALID_SEED + m
RECORD_FILE = 'valid.jsonl'
BEST_NAME = 'ae-best'                              # <model_path>-ae-best: outside the rolling window (no trailing iteration)
STATE_FIELDS = ('every', 'batches', 'digest', 'holdout')
UNIT_KEYS = ('valid_bit_entropy', 'valid_dead_bits', 'valid_flip_rate')

ValidConfig = namedtuple('ValidConfig', ['every', 'batches', 'set', 'holdout'])
ValidConfig.__new__.__defaults__ = (None,)
ValidConfig.__doc__ = """every: validate after every `every`-th iteration (and after the last); batches: M, the batches of a validation;
set: the ValidSet; holdout: the K of --valid_holdout, or None."""


# ---- flags ---------------------------------------------------------------------------------------------------------------------
def check_flags(args):
    """--valid_every is refused, before anything is built, where it would have no effect (without --train_ae or --train); the
    other --valid_* flags without --valid_every; --valid_index_path together with --valid_holdout; a real data set without either."""
    given = [f for f in ('valid_batches', 'valid_index_path', 'valid_holdout', 'valid_flag') if getattr(args, f, None) is not None]
    if getattr(args, 'valid_every', None) is None:
        if given:
            raise ValueError('--%s needs --valid_every' % given[0])
        return
    if not (args.train_ae or args.train):
        raise ValueError('--valid_every needs --train_ae or --train (only the pretrain_AE stage validates)')
    if args.valid_every < 1:
        raise ValueError('--valid_every must be >= 1 (got %d)' % args.valid_every)
    if args.valid_batches is not None and args.valid_batches < 1:
        raise ValueError('--valid_batches must be >= 1 (got %d)' % args.valid_batches)
    if args.valid_index_path is not None and args.valid_holdout is not None:
        raise ValueError('--valid_index_path and --valid_holdout are two sources of one validation set: give one')
    if args.valid_holdout is not None and args.valid_holdout < 2:
        raise ValueError('--valid_holdout must be >= 2 (got %d)' % args.valid_holdout)
    if args.valid_holdout is not None and args.synthetic:
        raise ValueError('--valid_holdout splits an index file: it cannot be combined with --synthetic')
    if not args.synthetic and args.valid_index_path is None and args.valid_holdout is None:
        raise ValueError('--valid_every needs a validation set: --valid_index_path, --valid_holdout, or --synthetic')


# ---- the validation set --------------------------------------------------------------------------------------------------------
def load_index(path):
    with open(path) as f:
        return json.load(f)


def holdout_split(indexes, K):
    """(training entries, validation entries) of an index (a list of {'speaker', 'i', 't'}): the distinct (speaker, i) utterances,
    sorted, every K-th of them (positions K-1, 2K-1, ...) held out.  Both lists keep the order of `indexes`; no utterance is in both."""
    K = int(K)
    if K < 2:
        raise ValueError('valid_holdout must be >= 2 (got %d)' % K)
    utts = sorted({(e['speaker'], e['i']) for e in indexes})
    held = set(utts[K - 1::K])
    train = [e for e in indexes if (e['speaker'], e['i']) not in held]
    valid = [e for e in indexes if (e['speaker'], e['i']) in held]
    return train, valid


def items_digest(items):
    """A digest of a validation item list (any JSON-serialisable description of the items, in order)."""
    return hashlib.sha1(json.dumps(items, sort_keys=True).encode()).hexdigest()


class ValidSet(object):
    """M batches of B segments in host memory: x fp32 [M, B, seg_len, F], c int64 [M, B], and the digest of what they were cut from."""

    def __init__(self, x, c, digest):
        self.x, self.c, self.digest = x, c, str(digest)

    @classmethod
    def from_dataset(cls, dataset, batches, batch_size, n_speakers, items=None):
        """The first batches * batch_size items of `dataset` (dataloader.Dataset / SyntheticDataset item contract), in order.
        ValueError, before an item is read, when there are fewer; while reading, for a speaker id outside [0, n_speakers).
        items: what the digest is taken of (default: the dataset's index entries, or its speaker ids)."""
        import torch
        n = int(batches) * int(batch_size)
        if len(dataset) < n:
            raise ValueError('the validation set has %d items, valid_batches * batch_size = %d are needed' % (len(dataset), n))
        entries = getattr(dataset, 'indexes', None)
        if entries is not None:
            bad = [e['speaker'] for e in entries[:n] if not 0 <= int(e['speaker']) < n_speakers]
            if bad:
                raise ValueError('the validation index names speaker id %d outside [0, %d)' % (bad[0], n_speakers))
        spk, lin = zip(*(dataset[i][:2] for i in range(n)))
        c = np.asarray(spk, dtype=np.int64)
        if c.min() < 0 or c.max() >= n_speakers:
            raise ValueError('the validation set has a speaker id outside [0, %d)' % n_speakers)
        x = np.stack([np.asarray(l, dtype=np.float32) for l in lin])
        if items is None:
            items = entries[:n] if entries is not None else [int(v) for v in c]
        return cls(torch.from_numpy(x).view(batches, batch_size, x.shape[1], x.shape[2]),
                   torch.from_numpy(c).view(batches, batch_size), items_digest([list(x.shape), items]))


def check_config(cfg, hps):
    """ValueError unless the ValidConfig fits the run: every >= 1, 1 <= batches <= the set's, the set's batch size the run's."""
    if int(cfg.every) < 1 or int(cfg.batches) < 1:
        raise ValueError('valid: every and batches must be >= 1 (got %r, %r)' % (cfg.every, cfg.batches))
    M, B = cfg.set.c.shape
    if M < cfg.batches or B != hps.batch_size or tuple(cfg.set.x.shape[:2]) != (M, B) or cfg.set.x.shape[2] % 8:
        raise ValueError('valid: the set holds %d batches of %d segments of %d frames; %d batches of batch_size %d (frames a multiple '
                         'of 8) are needed' % (M, B, cfg.set.x.shape[2], cfg.batches, hps.batch_size))
    return cfg


# ---- from the device tables to a record ----------------------------------------------------------------------------------------
def table_layout(n_speakers, E):
    """{name: (offset, length)} of the one device table (8-byte words) a validation accumulates into and copies to the host once:
    spk_sum (double bits), spk_cnt, ones, flips (E = 0: no unit statistics), rows, pairs, bad; and the total length."""
    lay, off = {}, 0
    for name, n in (('spk_sum', n_speakers), ('spk_cnt', n_speakers), ('ones', E), ('flips', E), ('rows', 1), ('pairs', 1), ('bad', 1)):
        lay[name] = (off, n)
        off += n
    return lay, off


def split_table(words, n_speakers, E):
    """The host copy of that table (int64 numpy [total]) as named arrays; spk_sum as float64."""
    lay, total = table_layout(n_speakers, E)
    words = np.ascontiguousarray(words, dtype=np.int64)
    assert words.shape == (total,)
    out = {k: words[o:o + n] for k, (o, n) in lay.items()}
    out['spk_sum'] = out['spk_sum'].view(np.float64)
    return out


def _h2(p):
    return 0.0 if p <= 0.0 or p >= 1.0 else -(p * math.log2(p) + (1.0 - p) * math.log2(1.0 - p))


def finish(tab, T, F, target_ids=(), units=True):
    """The record of one validation from the accumulated tables (split_table's dict, or the same names by hand), in double:
      valid_loss_rec         sum spk_sum / (sum spk_cnt * T * F)
      per_speaker            {id: {'loss': spk_sum / (spk_cnt * T * F), 'count': spk_cnt}} over the speakers with samples
      valid_loss_rec_target  mean of those losses over target_ids (None when none of them has samples), valid_loss_rec_worst their max
      valid_bit_entropy      sum_j h2(ones_j / rows), bits per frame (an upper bound: as if the units were independent)
      valid_dead_bits        #{j : ones_j in {0, rows}};   valid_flip_rate   sum flips / (pairs * E) (None without a frame pair)
    units=False (enc_mode 'continues') leaves the three unit statistics out.  ValueError when bad != 0 (a speaker id outside the
    tables was skipped on the device) or no sample was counted."""
    if int(np.asarray(tab['bad']).reshape(-1)[0]) != 0:
        raise ValueError('validation: %d samples carry a speaker id outside the tables' % int(np.asarray(tab['bad']).reshape(-1)[0]))
    s, n = np.asarray(tab['spk_sum'], dtype=np.float64), np.asarray(tab['spk_cnt'], dtype=np.int64)
    if int(n.sum()) <= 0:
        raise ValueError('validation: no sample was counted')
    per = float(T) * float(F)
    have = np.nonzero(n > 0)[0]
    loss = {int(i): float(s[i]) / (float(n[i]) * per) for i in have}
    tgt = [loss[int(i)] for i in target_ids if int(i) in loss]
    rec = {'valid_loss_rec': float(s.sum()) / (float(n.sum()) * per),
           'valid_loss_rec_target': (sum(tgt) / len(tgt)) if tgt else None,
           'valid_loss_rec_worst': max(loss.values()),
           'per_speaker': {str(i): {'loss': loss[i], 'count': int(n[i])} for i in sorted(loss)}}
    if units:
        ones, flips = np.asarray(tab['ones'], dtype=np.uint64), np.asarray(tab['flips'], dtype=np.uint64)
        rows, pairs = int(np.asarray(tab['rows']).reshape(-1)[0]), int(np.asarray(tab['pairs']).reshape(-1)[0])
        E = ones.shape[0]
        rec['valid_bit_entropy'] = float(sum(_h2(int(o) / float(rows)) for o in ones))
        rec['valid_dead_bits'] = int(sum(1 for o in ones if int(o) in (0, rows)))
        rec['valid_flip_rate'] = (float(sum(int(f) for f in flips)) / (float(pairs) * E)) if pairs > 0 else None
    return rec


SCALARS = ('valid_loss_rec', 'valid_loss_rec_target', 'valid_loss_rec_worst') + UNIT_KEYS


def line(iteration, rec):
    """The printed line of a record."""
    parts = ['%s=%s' % (k[6:], ('%d' % rec[k]) if k == 'valid_dead_bits' else ('%.5f' % rec[k]))
             for k in SCALARS if rec.get(k) is not None]
    return 'valid:[%06d], %s' % (iteration, ', '.join(parts))


# ---- the record file -----------------------------------------------------------------------------------------------------------
def record_path(model_path):
    return os.path.join(os.path.dirname(model_path), RECORD_FILE)


def best_path(model_path):
    return '%s-%s' % (model_path, BEST_NAME)


def append_record(path, iteration, rec):
    with open(path, 'a') as f:
        f.write(json.dumps(dict(rec, iteration=int(iteration)), sort_keys=True) + '\n')


def read_records(path):
    if not os.path.exists(path):
        return []
    with open(path) as f:
        return [json.loads(l) for l in f if l.strip()]


def truncate_records(path, iteration):
    """Keep the records up to `iteration`: a run that starts (0) or resumes there writes the later ones again."""
    keep = [r for r in read_records(path) if r['iteration'] <= iteration]
    if os.path.exists(path):
        tmp = path + '.tmp'
        with open(tmp, 'w') as f:
            for r in keep:
                f.write(json.dumps(r, sort_keys=True) + '\n')
        os.replace(tmp, path)


# ---- train state ---------------------------------------------------------------------------------------------------------------
def describe(cfg):
    """The `valid` entry of a train-state file: what a file and the run that loads it must agree on."""
    return {'every': int(cfg.every), 'batches': int(cfg.batches), 'digest': cfg.set.digest,
            'holdout': None if cfg.holdout is None else int(cfg.holdout)}


def validate(have, expect):
    """Raise ValueError naming what differs between a state file's `valid` entry and this run's (either may be None: off)."""
    if (have is None) != (expect is None):
        raise ValueError('train state: valid is %s in the file, %s in this run' % ('off' if have is None else 'on', 'off' if expect is None else 'on'))
    if have is None:
        return
    for f in STATE_FIELDS:
        if have.get(f) != expect.get(f):
            raise ValueError('train state: valid_%s is %r in the file, %r in this run' % (f, have.get(f), expect.get(f)))
