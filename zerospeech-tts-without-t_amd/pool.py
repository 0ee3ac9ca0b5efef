"""Training from a dataset held in device memory (opt-in: main.py --device_data).

The reference's loader has no shuffling: preprocess.Sampler draws the (speaker, utterance, t) items once and DataLoader walks them
in order with a fixed wrap rule (dataloader.py:34-52), so the batch sequence is a pure function of the batch number and a batch is
a gather of B contiguous segments out of the utterances.  `DevicePool` uploads every utterance an index refers to once, back to
back; `PoolLoader` validates an index against it on the host, once, and serves the batches with the zs_pool_gather kernel: nothing
crosses PCIe per step and the host does no work per batch.  `batch_items` is the loader's order in closed form.  The --train_ae
step that begins with the gather is trainer.PoolFedStep.

Nothing here falls back to the host loader: a pool that does not fit is an error."""
import os

import numpy as np
import torch

from . import _lib as L

HEADROOM_BYTES = 4 << 30          # device memory left free beside the pool (the training step's own buffers grow after it)
STAGE_BYTES = 64 << 20            # each of the two pinned staging buffers of an upload


def batch_items(n, B, rank=0, world=1, k=0):
    """Items of batch k, in order, as DataLoader(dataset of n items, B, rank, world) serves them at its k-th `next()`:
    (k mod P) * S + rank * B + i for i < B, taken modulo n when world > 1, with S = world * B and P = max(1, ceil(n / S) - 1).
    DataLoader's index visits 0, S, 2S, ... while index + 2S < n and then wraps to 0: P positions, the last of them
    (P - 1) * S with P * S < n, so a tail of n - P * S items (a whole global batch when S divides n) is never served."""
    n, B, rank, world, k = int(n), int(B), int(rank), max(1, int(world)), int(k)
    S = world * B
    if B <= 0 or not 0 <= rank < world or k < 0:
        raise ValueError('batch_items: need B > 0, 0 <= rank < world and k >= 0 (got B=%d rank=%d world=%d k=%d)' % (B, rank, world, k))
    if n < S:
        raise ValueError('%d items are fewer than one global batch of world * batch_size = %d' % (n, S))
    P = max(1, -(-n // S) - 1)
    base = (k % P) * S + rank * B
    return [(base + i) % n if world > 1 else base + i for i in range(B)]


class PoolPlan(object):
    """Host-side layout of a pool: which utterances it holds, in which order, and where each starts (in frames).  An utterance is
    one contiguous fp32 [frames, F] array: `{dset}/{utt}/lin` of a Dataset's store (HDF5 or NpzStore; keyed by the store's path, so
    several index files over one store share their utterances) or the whole `lin` array of a SyntheticDataset, whose item i starts
    at frame i * seg_len.  No device is touched."""

    def __init__(self, datasets):
        if not isinstance(datasets, (list, tuple)):
            datasets = [datasets]
        self.offsets, self.lengths, self._source = {}, {}, {}
        self.order = []
        self.F = None
        self.frames_total = 0
        for ds in datasets:
            self.add(ds)

    @staticmethod
    def _store_id(ds):
        st = ds.dataset
        return getattr(st, 'path', None) or getattr(st, 'filename', None) or id(st)

    def _utterance(self, key, shape, read):
        if key in self.offsets:
            return
        if len(shape) != 2 or (self.F is not None and shape[1] != self.F):
            raise ValueError('pool utterance %r has shape %r: every utterance must be [frames, %s]' % (key, tuple(shape), self.F or 'F'))
        self.F = int(shape[1])
        self.offsets[key], self.lengths[key], self._source[key] = self.frames_total, int(shape[0]), read
        self.order.append(key)
        self.frames_total += int(shape[0])

    def add(self, ds):
        """Plan every utterance the items of `ds` refer to (once each, in first-use order)."""
        if hasattr(ds, 'lin') and hasattr(ds, 'spk'):                          # SyntheticDataset: the lin array is the utterance
            lin = ds.lin                                                       # (the reader keeps ds alive: its id is the key)
            self._utterance(('synthetic', id(ds)), (lin.shape[0] * lin.shape[1], lin.shape[2]),
                            lambda ds=ds: ds.lin.reshape(-1, ds.lin.shape[2]))
        elif hasattr(ds, 'indexes') and hasattr(ds, 'dataset'):
            if getattr(ds, 'load_mel', False):
                raise NotImplementedError('a pool holds lin spectrograms only (load_mel is the Tacotron path)')
            sid, store = self._store_id(ds), ds.dataset
            for it in ds.indexes:
                name = '%s/%s/lin' % (ds.dset, it['i'])
                key = (sid, name)
                if key not in self.offsets:
                    self._utterance(key, store[name].shape, lambda store=store, name=name: store[name][...])
        else:
            raise TypeError('a pool is built from Dataset or SyntheticDataset objects (got %s)' % type(ds).__name__)

    @property
    def nbytes(self):
        return self.frames_total * (self.F or 0) * 4

    def read(self, key):
        """The utterance as a C-contiguous fp32 [frames, F] host array."""
        return np.ascontiguousarray(self._source[key](), dtype=np.float32)

    def items(self, ds):
        """(speaker int64 [n], first frame in the pool int64 [n], t int64 [n], utterance length int64 [n], seg_len) of the items of
        `ds`, unvalidated.  Raises KeyError for an utterance the plan does not hold."""
        if hasattr(ds, 'lin') and hasattr(ds, 'spk'):
            n, seg = ds.lin.shape[0], ds.lin.shape[1]
            off = self.offsets[('synthetic', id(ds))]
            t = np.zeros(n, dtype=np.int64)
            return np.asarray(ds.spk, dtype=np.int64), off + np.arange(n, dtype=np.int64) * seg, t, np.full(n, seg, dtype=np.int64), seg
        sid = self._store_id(ds)
        keys = [(sid, '%s/%s/lin' % (ds.dset, it['i'])) for it in ds.indexes]
        spk = np.array([int(it['speaker']) for it in ds.indexes], dtype=np.int64)
        t = np.array([int(it['t']) for it in ds.indexes], dtype=np.int64)
        off = np.array([self.offsets[k] for k in keys], dtype=np.int64)
        ulen = np.array([self.lengths[k] for k in keys], dtype=np.int64)
        return spk, off + t, t, ulen, int(ds.seg_len)


def check_speakers(spk, n_speakers=None, check=None):
    """The checks DevicePrefetcher applies to the speaker ids of every host batch, applied to a whole speaker column: the range
    [0, n_speakers) (ValueError, the host path's message) and the caller's hook (PatchGANStep.check_targets, Trainer.tclf_labels)."""
    c = torch.as_tensor(np.asarray(spk, dtype=np.int64))
    if n_speakers is not None and c.numel() and (int(c.min()) < 0 or int(c.max()) >= n_speakers):
        raise ValueError('speaker index outside [0, %d) in the batch' % n_speakers)   # would fault the GPU in the embedding lookups
    if check is not None:
        check(c)


def item_table(plan, ds, batch_size, world=1, n_speakers=None, check=None):
    """The validated item table of `ds` over `plan`: (speaker int32 [n], first int64 [n], seg_len).  Every range the kernel trusts
    is checked here, over all n items: 0 <= t, t + seg_len <= len(utterance) (so first + seg_len never leaves the utterance, let
    alone the pool), the speakers (check_speakers) and n >= world * batch_size.  Raises ValueError (RuntimeError from a hook)."""
    spk, first, t, ulen, seg = plan.items(ds)
    n, S = len(spk), max(1, int(world)) * int(batch_size)
    if n < S:
        raise ValueError('%d items are fewer than one global batch of world * batch_size = %d' % (n, S))
    bad = np.nonzero((t < 0) | (t + seg > ulen))[0]
    if len(bad):
        i = int(bad[0])
        raise ValueError('item %d: frames [%d, %d) leave its utterance of %d frames (%d such items)' % (i, t[i], t[i] + seg, ulen[i], len(bad)))
    if spk.min() < -2 ** 31 or spk.max() >= 2 ** 31:
        raise ValueError('speaker index does not fit int32')
    check_speakers(spk, n_speakers, check)
    if first.min() < 0 or (first + seg).max() > plan.frames_total:            # cannot happen once the checks above passed
        raise ValueError('an item leaves the pool')
    return spk.astype(np.int32), first.astype(np.int64), seg


def pool_limit_bytes(max_bytes=None):
    """The configured size limit of a pool: max_bytes, else ZS_POOL_MAX_GB (GiB, may be fractional), else None."""
    if max_bytes is not None:
        return int(max_bytes)
    gb = os.environ.get('ZS_POOL_MAX_GB', '').strip()
    return int(float(gb) * (1 << 30)) if gb else None


class DevicePool(object):
    """The utterances of one or several datasets as one fp32 [frames_total, F] device tensor (see PoolPlan for the layout).
    Uploaded utterance by utterance through two pinned staging buffers of STAGE_BYTES: host memory never holds a second copy of
    the set.  The size is compared with max_bytes / ZS_POOL_MAX_GB and with the device's free memory less HEADROOM_BYTES before
    anything is allocated; a pool that does not fit raises MemoryError naming both numbers."""

    def __init__(self, dataset_like, device, max_bytes=None, headroom_bytes=HEADROOM_BYTES):
        self.plan = dataset_like if isinstance(dataset_like, PoolPlan) else PoolPlan(dataset_like)
        need, limit = self.plan.nbytes, pool_limit_bytes(max_bytes)
        if need <= 0:
            raise ValueError('an empty pool: the datasets refer to no utterance')
        if limit is not None and need > limit:
            raise MemoryError('the pool needs %d bytes, more than the %d bytes allowed (max_bytes / ZS_POOL_MAX_GB)' % (need, limit))
        self.device = torch.device(device)
        free, _ = torch.cuda.mem_get_info(self.device)
        if need > free - headroom_bytes:
            raise MemoryError('the pool needs %d bytes, the device has %d bytes free less a headroom of %d' % (need, free, headroom_bytes))
        self.F, self.frames_total = self.plan.F, self.plan.frames_total
        self.data = torch.empty(self.frames_total, self.F, dtype=torch.float32, device=self.device)
        self._upload()

    def _upload(self):
        flat = self.data.view(-1)
        cap = STAGE_BYTES // 4
        stage = [torch.empty(cap, dtype=torch.float32).pin_memory() for _ in range(2)]
        free = [torch.cuda.Event(), torch.cuda.Event()]
        turn = 0
        stream = torch.cuda.current_stream(self.device)
        for key in self.plan.order:
            src = torch.from_numpy(self.plan.read(key)).view(-1)
            at = self.plan.offsets[key] * self.F
            for lo in range(0, src.numel(), cap):
                m = min(cap, src.numel() - lo)
                free[turn].synchronize()                                       # the copy that last read this buffer is done
                stage[turn][:m].copy_(src[lo:lo + m])
                flat[at + lo:at + lo + m].copy_(stage[turn][:m], non_blocking=True)
                free[turn].record(stream)
                turn = 1 - turn
        torch.cuda.synchronize(self.device)


class PoolLoader(object):
    """DataLoader + DevicePrefetcher over a DevicePool: `next(loader)` launches zs_pool_gather on the current stream into one of two
    device slots and returns `(c int64 [B], x fp32 [B, seg_len, F])`, valid until the call after next (DevicePrefetcher's
    contract), batch for batch what `DataLoader(index, batch_size, rank, world)` serves.  The item table is validated on the host
    over all items at construction (item_table), before anything is uploaded or launched.  The batch number lives in device memory
    (`cursor`) and advances behind every gather; `set_cursor(k)` makes the next batch number k."""

    def __init__(self, pool, index, batch_size, rank=0, world=1, n_speakers=None, check=None):
        self.pool = pool
        self.batch_size, self.rank, self.world = int(batch_size), int(rank), max(1, int(world))
        if not 0 <= self.rank < self.world:
            raise ValueError('rank %d outside [0, %d)' % (self.rank, self.world))
        spk, first, self.seg_len = item_table(pool.plan, index, self.batch_size, self.world, n_speakers, check)
        self.speakers = torch.from_numpy(spk.astype(np.int64))                 # host copy of the speaker column (require())
        self.n, self.F, self.device = len(spk), pool.F, pool.device
        self._checked = {(n_speakers, check)}
        self._spk = torch.from_numpy(spk).to(self.device)
        self._first = torch.from_numpy(first).to(self.device)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.slots = [None, None]
        self.turn = 0

    def require(self, n_speakers=None, check=None):
        """Apply a consumer's speaker checks to the whole speaker column, once per (n_speakers, check) (host memory only).
        Returns the loader."""
        key = (n_speakers, check)
        if key not in self._checked:
            check_speakers(self.speakers, n_speakers, check)
            self._checked.add(key)
        return self

    def set_cursor(self, k):
        """The next batch served is batch k (resume)."""
        if int(k) < 0:
            raise ValueError('the batch number must be >= 0')
        self.cursor.fill_(int(k))

    def gather_into(self, x, c):
        """Launch the gather of the cursor's batch into x fp32 [B, seg_len, F] and c int64 [B], and the cursor's advance, on the
        current stream."""
        if x.dtype != torch.float32 or c.dtype != torch.int64 or not x.is_contiguous() or not c.is_contiguous() or \
                tuple(x.shape) != (self.batch_size, self.seg_len, self.F) or tuple(c.shape) != (self.batch_size,):
            raise ValueError('gather_into: x must be contiguous fp32 [%d, %d, %d] and c contiguous int64 [%d]'
                             % (self.batch_size, self.seg_len, self.F, self.batch_size))
        L.call('zs_pool_gather', 'ZsPoolGather', torch.cuda.current_stream(self.device).cuda_stream, pool=L.ptr(self.pool.data),
               speaker=L.ptr(self._spk), first=L.ptr(self._first), cursor=L.ptr(self.cursor), n=self.n, B=self.batch_size,
               seg_len=self.seg_len, F=self.F, rank=self.rank, world=self.world, x=L.ptr(x), c=L.ptr(c), advance=1)

    def __iter__(self):
        return self

    def __next__(self):
        i = self.turn
        if self.slots[i] is None:
            self.slots[i] = (torch.empty(self.batch_size, dtype=torch.int64, device=self.device),
                             torch.empty(self.batch_size, self.seg_len, self.F, dtype=torch.float32, device=self.device))
        c, x = self.slots[i]
        self.gather_into(x, c)
        self.turn = 1 - i
        return c, x
