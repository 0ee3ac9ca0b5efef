"""Train-state files: what a checkpoint needs beside the weights to continue a run bit for bit (opt-in: Trainer.train(resume=True),
main.py --resume).  The reference saves the weights of the six nets and nothing else; it has no counterpart of this module.

A checkpoint `<dir>/<model_name>-<tag>-<iteration>` (the reference's dict, unchanged) gets a sidecar
`<dir>/train_state/<model_name>-<tag>-<iteration>.pt`: a torch.save'd dict of CPU tensors and plain Python values (loads with
weights_only=True) that holds no weights.  Its keys:

  version, tag, iteration, target_guided, autolocker, world, batch_size, dtype, g_mode, enc_mode, use_graph     what it belongs to
  ema           the decay of the weight averages (Trainer(ema=...)); the key is absent when the run keeps none.  The averages
                themselves travel in `steps`, one 'ema' buffer beside each optimizer's m and v
  flat_len      {net: length of its flat parameter buffer}
  steps         {'ae' | 'clf' | 's2' | 'tclf': that step object's state_dict()}: Adam m / v / t per stepped net and the counters
  consumed      {'data' | 'source' | 'target': batches the steps have taken from that loader}
  rng           {'cpu': torch.get_rng_state(), 'cuda': torch.cuda.get_rng_state(device)}
  valid         {'every', 'batches', 'digest', 'holdout'} of the held-out validation (validation.py) of a pretrain_AE run; the key, and
                best_loss / best_iteration (the lowest validation loss so far and its iteration) beside it, are absent when the run
                does not validate
  model_kept    the rolling window of checkpoints (Trainer.model_kept) after this checkpoint, as file names in the checkpoint's
                directory: a copied or moved directory resumes

This module is host code only: paths, the search for the newest resumable checkpoint, validation, the rolling window and the
writer thread.  What is copied from the device, and when, is trainer.Trainer's business."""
import os
import re
import threading

import torch

FORMAT_VERSION = 1
TAGS = {'pretrain_AE': 'ae', 'pretrain_C': 'c', 'train': 's1', 'patchGAN': 's2', 'autolocker': 's2', 't_classify': 'tclf'}
STATE_DIR = 'train_state'
# the fields a state file must share with the run that loads it, in the order they are compared
FIELDS = ('version', 'tag', 'target_guided', 'autolocker', 'world', 'batch_size', 'dtype', 'g_mode', 'enc_mode', 'use_graph')
NET_NAMES = ('encoder', 'decoder', 'generator', 'classifier', 'patch_discriminator', 'target_classifier')


def state_path(ckpt_path):
    """The sidecar of the checkpoint file `ckpt_path`."""
    d, base = os.path.split(ckpt_path)
    return os.path.join(d, STATE_DIR, base + '.pt')


def find_resumable(model_path, tag):
    """(checkpoint path, state path, iteration) of the newest checkpoint `<model_path>-<tag>-<iteration>` that has a state file, or
    None.  Other tags, checkpoints without a sidecar and *.tmp leftovers of a killed writer are ignored."""
    d, base = os.path.split(model_path)
    pat = re.compile(re.escape('%s-%s-' % (base, tag)) + r'(\d+)$')
    try:
        names = os.listdir(d or '.')
    except OSError:
        return None
    best = None
    for name in names:
        m = pat.match(name)
        if m is None:
            continue
        ckpt = os.path.join(d, name)
        if not os.path.isfile(ckpt) or not os.path.isfile(state_path(ckpt)):
            continue
        it = int(m.group(1))
        if best is None or it > best[2]:
            best = (ckpt, state_path(ckpt), it)
    return best


def describe(trainer, tag, target_guided=False, autolocker=False):
    """The fields of FIELDS plus flat_len for `trainer` as it stands: what a state file written now records, and what one loaded
    now must match.  Reads attributes and buffer lengths only."""
    from . import parallel
    d = {'version': FORMAT_VERSION, 'tag': tag, 'target_guided': bool(target_guided), 'autolocker': bool(autolocker),
         'world': int(parallel.world_size()), 'batch_size': int(trainer.hps.batch_size), 'dtype': str(trainer.dtype),
         'g_mode': str(trainer.g_mode), 'enc_mode': str(trainer.enc_mode), 'use_graph': bool(trainer.ae.use_graph),
         'flat_len': {name: int(net.flat_params()[0].numel()) for name, net in zip(NET_NAMES, trainer.nets())}}
    if getattr(trainer, 'ema', None) is not None:                          # recorded only when on: an EMA-off file is today's
        d['ema'] = float(trainer.ema)
    if tag == 'ae' and getattr(trainer, 'valid', None) is not None:        # recorded only when on, as ema
        from . import validation
        d['valid'] = validation.describe(trainer.valid)
    return d


def validate(state, expect):
    """Raise ValueError naming the first field of `state` (a loaded state file) that differs from `expect` (describe())."""
    for f in FIELDS:
        if f not in state:
            raise ValueError('train state: field %r is missing' % f)
        if state[f] != expect[f]:
            raise ValueError('train state: %s is %r in the file, %r in this run' % (f, state[f], expect[f]))
    if state.get('ema') != expect.get('ema'):                             # the decay, or None: on / off and the value must agree
        raise ValueError('train state: ema is %r in the file, %r in this run' % (state.get('ema'), expect.get('ema')))
    from . import validation
    validation.validate(state.get('valid'), expect.get('valid'))         # on / off, every, batches, the set's digest, the holdout K
    have = state.get('flat_len')
    if not isinstance(have, dict):
        raise ValueError("train state: field 'flat_len' is missing")
    for name, n in expect['flat_len'].items():
        if have.get(name) != n:
            raise ValueError('train state: flat_len[%s] is %r in the file, %r in this run' % (name, have.get(name), n))


def ema_keys(file_keys, wanted, path='checkpoint'):
    """Which entry of a checkpoint each net is loaded from when the averaged weights are asked for (load_model(use_ema=True)):
    {net: '<net>_ema' where the file has it, else '<net>'} for the nets `wanted`.  file_keys: the checkpoint's top-level keys.
    ValueError naming `path` when the file has no `*_ema` entry at all: it was written without --ema."""
    file_keys = set(file_keys)
    if not any(k.endswith('_ema') for k in file_keys):
        raise ValueError('use_ema: %s has no *_ema entry (it was written by a run without --ema)' % path)
    return {net: (net + '_ema' if net + '_ema' in file_keys else net) for net in wanted}


def roll_window(model_kept, new_path, max_keep):
    """Trainer.save_model's rolling window (trainer.py:118-125): append new_path; once the list is max_keep long its oldest entry
    leaves it.  Returns the checkpoint paths to remove (remove_checkpoint)."""
    model_kept.append(new_path)
    if len(model_kept) >= max_keep:
        return [model_kept.pop(0)]
    return []


def remove_checkpoint(path):
    """Remove a checkpoint file and, where there is one, its state file and the codebook --vq_train or --rvq_train wrote beside it."""
    os.remove(path)
    for side in (state_path(path), path + '.vq.npz', path + '.rvq.npz'):
        if os.path.exists(side):
            os.remove(side)


def map_tensors(tree, fn):
    """A copy of a tree of dicts / lists / tuples with fn applied to every tensor leaf."""
    if isinstance(tree, torch.Tensor):
        return fn(tree)
    if isinstance(tree, dict):
        return {k: map_tensors(v, fn) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return [map_tensors(v, fn) for v in tree]
    return tree


def atomic_save(obj, path):
    """torch.save under a temporary name in the target's directory, then os.replace: a killed process never leaves a half-written
    file under a real name."""
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    tmp = path + '.tmp'
    torch.save(obj, tmp)
    os.replace(tmp, path)


class Writer(object):
    """One worker thread, at most one job in flight.  submit(fn) waits for the previous job, then starts fn on the worker;
    wait() blocks until the worker is idle and re-raises, on the caller's thread, what the last job raised."""

    def __init__(self):
        self._thread = None
        self._error = None

    def _run(self, fn):
        try:
            fn()
        except BaseException as e:                                            # handed to the training thread by wait()
            self._error = e

    def submit(self, fn):
        self.wait()
        self._thread = threading.Thread(target=self._run, args=(fn,), name='zs-ckpt-writer', daemon=True)
        self._thread.start()

    def poll(self):
        """Raise what the job raised if it has failed; never blocks on a job that is still running."""
        if self._error is not None:
            self.wait()

    def wait(self):
        t, self._thread = self._thread, None
        if t is not None:
            t.join()
        e, self._error = self._error, None
        if e is not None:
            raise e
