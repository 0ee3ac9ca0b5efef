"""Training a 'continues' model through its vector codebook: `--vq_train FILE.vq.npz` puts a quantiser between the Encoder
and the Decoder of the --train_ae step.  Each encoder row is snapped to its nearest codeword (zs_vq_assign), the Decoder reads the
codewords and hands its input gradient straight through to the encoder (zs_vq_commit, zs_vq_st_bwd), a commitment term
beta * mean (z - code[idx])^2 keeps the encoder near its codewords, and the codebook follows the encoder by an exponential moving
average of the counts and sums of the rows each codeword took (zs_vq_accum, zs_vq_ema; van den Oord et al. 2017, the EMA variant).
The codebook receives no gradient.  Step t quantises, and takes its gradient, against the codebook step t - 1 left: the average is
written to the `next` copy and becomes the live one at the head of the next forward.  Everything is enqueued on the current stream
with launch arguments that do not change between iterations, so the captured step replays it; nothing adds floats atomically, so a
run is bitwise reproducible.  tests/vq_train_ref.py is the numpy definition.  Not in the reference, which has no codebook.
`--vq_restart T`: a codeword that took no row of the step and whose averaged count fell below T is put back onto one of
the step's encoder rows by zs_vq_restart, behind the average; tests/vq_restart_ref.py is its definition.
Bottleneck is what this quantiser and the residual one (rvq_train.RvqBottleneck) share: the plan's host constants, the state and
its per-stage layout, a stage's average, the checkpoint side."""
import os

import numpy as np
import torch

from . import _lib as L
from . import vq

BETA = 0.25            # the commitment weight and the decay of the paper
DECAY = 0.99
MAX_ABS = float(L.ENUMS['ZS_VQ_MAX_ABS'])
PARTS = L.ENUMS['ZS_VQ_COMMIT_PARTS']
MIN_COUNT = 1e-3       # a codeword whose averaged count is below this keeps its row (zs_vq_ema)
GOLDEN = 0x9E3779B97F4A7C15        # stage s restarts with the seed (seed + s GOLDEN) mod 2^64


def check_beta(beta):
    b = float(beta)
    if not (0.0 < b <= 10.0):                  # NaN fails too
        raise ValueError('--vq_beta must be in (0, 10] (got %r)' % (beta,))
    return b


def check_decay(decay):
    d = float(decay)
    if not (0.0 <= d < 1.0):
        raise ValueError('--vq_decay must be in [0, 1) (got %r)' % (decay,))
    return d


def check_restart(v):
    t = float(v)
    if not (0.0 < t < 1.0):                    # NaN fails too
        raise ValueError('--vq_restart must be in (0, 1) (got %r)' % (v,))
    return t


def restart_stride(n):
    """The step between the rows that consecutive dead codewords take (zs_vq_restart): the largest s with
    1 <= s <= max(1, floor(0.6180339887 n)) and gcd(s, n) == 1, so that up to n dead codewords take n distinct rows spread over
    the batch."""
    from math import gcd
    n = int(n)
    if n < 1:
        raise ValueError('restart_stride: n must be at least 1 (got %d)' % n)
    s = max(1, int(0.6180339887 * n))
    while gcd(s, n) != 1:
        s -= 1
    return s


def encoded_rows(batch_size, seg_len):
    """Rows of the encoder's output for a batch of seg_len-frame segments: three stride-2 convs, each rounding up."""
    t = int(seg_len)
    for _ in range(3):
        t = (t + 1) // 2
    return int(batch_size) * t


def perplexity(cnt):
    """exp of the entropy (nats) of the counts' distribution; 0.0 when nothing was counted."""
    c = np.asarray(cnt, dtype=np.float64)
    tot = c.sum()
    if tot <= 0:
        return 0.0
    p = c[c > 0] / tot
    return float(np.exp(-(p * np.log(p)).sum()))


class Bottleneck(object):
    """What VqBottleneck and rvq_train.RvqBottleneck share.  A subclass names its flag, its codebook's kind and file suffix and the
    words of its messages, builds what its own commit needs, and writes forward, backward and the figures of stats()."""
    kind = flag = ckpt_suffix = None
    over_text = None                                             # stats(): the rows left out for their magnitude, in the class's words

    @classmethod
    def of_kind(cls, kind):
        """The bottleneck that trains through a codebook of this kind: the trainer's one switch."""
        if kind == 'residual':
            from .rvq_train import RvqBottleneck
            return RvqBottleneck
        return VqBottleneck

    def __init__(self, codebook, beta, decay, rows, ctx, restart, stages=None):
        """stages: None for the one codebook of a vector quantiser, whose state has no stage dimension, or S: every per-stage tensor
        then leads with it."""
        self.beta, self.decay = check_beta(beta), check_decay(decay)
        self.rows = int(rows)
        if not 1 <= self.rows < 2 ** 31:
            raise ValueError('%s: rows must be in [1, 2^31) (got %d)' % (type(self).__name__, self.rows))
        self.ctx, self.base = ctx, codebook
        self.K, self.E = codebook.K, codebook.E
        dev = self.device = ctx.device
        K, E, n = self.K, self.E, self.rows
        lead = () if stages is None else (stages,)
        self.shift = vq.vq_shift(n, MAX_ABS)                     # a host constant of the plan: a row above MAX_ABS is left out
        self.scale = self.beta / (float(n) * E)                  # loss_vq = scale * sum (over the stages) of the squared residuals
        self.g = float(np.float32(2.0 * self.beta / (float(n) * E)))
        # the state: what the last step left (`code`, `cnorm` are the `next` copies the averages write)
        self.code = torch.from_numpy(codebook.vectors).to(dev).contiguous()          # [K, E] or [S, K, E]
        self.cnorm = torch.from_numpy(codebook.cnorm).to(dev).contiguous()
        self.N = torch.ones(*lead, K, dtype=torch.float32, device=dev)
        self.m = self.code.clone()
        # the live copies: what this step's assigns, commits and backward (gather) read
        self.code_live, self.cnorm_live = self.code.clone(), self.cnorm.clone()
        self.idx = torch.zeros(*lead, n, dtype=torch.int32, device=dev)              # (the planes zs_rvq_gather reads)
        self.idx_acc = torch.zeros(*lead, n, dtype=torch.int32, device=dev)
        # zeroed at the head of every step, per stage: (used | accum's own bad count) | cnt int32 [K] | sum int64 [K][E]
        self._cnt_at = 1
        self._sum_at = 1 + (K + 1) // 2
        self.acc = torch.zeros(*lead, self._sum_at + K * E, dtype=torch.int64, device=dev)
        cnt = [a[self._cnt_at:self._sum_at].view(torch.int32)[:K] for a in self.acc.view(-1, self.acc.shape[-1])]
        sums = [a[self._sum_at:].view(K, E) for a in self.acc.view(-1, self.acc.shape[-1])]
        self.cnt, self.sums = (cnt[0], sums[0]) if stages is None else (cnt, sums)
        self.partial = torch.zeros(*lead, PARTS, dtype=torch.float64, device=dev)
        self.work = vq.workspace(dev) if n < vq.SPLIT_N else None
        self.restart = None if restart is None else check_restart(restart)
        if self.restart is not None:
            self.stride = restart_stride(n)                      # a host constant of the plan
            self.rwork = torch.zeros(K + 2, dtype=torch.int32, device=dev)
        self.steps = 0
        self._bits = None

    def _stage(self, t, s):
        """Stage s of a per-stage tensor or list; a vector codebook is its one stage."""
        return t if self.kind == 'vector' else t[s]

    def _check_forward(self, bits):
        if bits.rows != self.rows or bits.C != self.E or bits.t.dtype != self.ctx.tdt:
            raise ValueError('%s: built for %d rows of %d columns of %s, got %d rows of %d of %s' %
                             (type(self).__name__, self.rows, self.E, self.ctx.tdt, bits.rows, bits.C, bits.t.dtype))

    def _check_backward(self, dbits):
        if self._bits is None or dbits.rows != self.rows or dbits.C != self.E:
            raise ValueError('%s.backward: no forward of %d rows before it' % (type(self).__name__, dbits.rows))

    def _average(self, s, rows32, ld32, seed, seed_ptr):
        """Enqueues stage s's zs_vq_accum, zs_vq_ema and, with restart on, zs_vq_restart over the fp32 rows (rows32, ld32) that stage
        quantised, behind its commit.  Stage s restarts with (seed + s GOLDEN) mod 2^64: at s = 0 the step's own seed."""
        st, K, E, n = self.ctx.stream, self.K, self.E, self.rows
        idx_acc, cnt, sums, N, m, code, cnorm = (L.ptr(self._stage(t, s)) for t in
                                                 (self.idx_acc, self.cnt, self.sums, self.N, self.m, self.code, self.cnorm))
        acc32 = self.acc.view(torch.int32)
        head = s * self.acc.shape[-1] * 2                        # this stage's (used | bad) words, in int32 elements
        L.call('zs_vq_accum', 'ZsVqAccum', st, x=rows32, idx=idx_acc, n=n, ld_x=ld32, K=K, E=E, shift=self.shift, cnt=cnt, sum=sums,
               bad=L.ptr(acc32, head + 1))
        L.call('zs_vq_ema', 'ZsVqEma', st, cnt=cnt, sum=sums, K=K, E=E, shift=self.shift, decay=self.decay, N=N, m=m, code=code,
               ld_code=E, cnorm=cnorm, used=L.ptr(acc32, head))
        if self.restart is not None:
            L.call('zs_vq_restart', 'ZsVqRestart', st, thresh=self.restart, x=rows32, n=n, ld_x=ld32, idx_acc=idx_acc, cnt=cnt, K=K, E=E,
                   N=N, m=m, code=code, ld_code=E, cnorm=cnorm, seed=(int(seed or 0) + s * GOLDEN) % (1 << 64), seed_ptr=seed_ptr,
                   stride=self.stride, work=L.ptr(self.rwork), restarted=L.ptr(self.stat, 3), skipped=L.ptr(self.stat, 4))

    # ---- host side ---------------------------------------------------------------------------------------------------------------------
    def _checked_stat(self):
        """The sticky counters, read from the device.  RuntimeError when a row was left out of an average because an element reached
        ZS_VQ_MAX_ABS, or an index was outside [0, K)."""
        stat = self.stat.cpu().numpy()
        if stat[1]:
            raise RuntimeError(self.over_text % (self.flag, int(stat[1]), MAX_ABS))
        if stat[0] or stat[2]:
            raise RuntimeError('%s: zs_vq_assign gave %d indices outside [0, %d)' % (self.flag, int(stat[0]) + int(stat[2]), self.K))
        return stat

    def state_dict(self):
        return {'code': self.code, 'cnorm': self.cnorm, 'N': self.N, 'm': self.m}

    def load_state_dict(self, sd):
        for k in ('code', 'cnorm', 'N', 'm'):
            dst, src = getattr(self, k), torch.as_tensor(sd[k])
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError('%s: state %r has shape %s, this bottleneck %s' %
                                 (type(self).__name__, k, tuple(src.shape), tuple(dst.shape)))
        for k in ('code', 'cnorm', 'N', 'm'):
            getattr(self, k).copy_(torch.as_tensor(sd[k]).to(torch.float32))

    def ckpt_meta(self, iteration, s):
        """The meta fields of <checkpoint><ckpt_suffix> after `iteration` iterations; s: stats()."""
        meta = {'trained_iterations': int(iteration), 'beta': self.beta, 'decay': self.decay, 'used': s['used']}
        if self.restart is not None:
            meta.update(restart=self.restart, restarts=s['restarts'])
        return meta

    def to_codebook(self, meta=None):
        """The codebook as the last step left it: one of the starting file's class whose meta is that file's plus `meta`."""
        out = dict(self.base.meta)
        out.update(meta or {})
        return type(self.base)(self.code.cpu().numpy(), out)


class VqBottleneck(Bottleneck):
    """The device state (code, cnorm, N, m) and the plan's buffers of the quantiser for `rows` encoder rows per step.
    codebook: the vq.VectorCodebook the run starts from (code = vectors, N = 1, m = code); ctx: a layers.Ctx (device, compute dtype
    and the buffer of q)."""
    kind, flag, ckpt_suffix = 'vector', '--vq_train', '.vq.npz'  # (rvq_train.RvqBottleneck: 'residual')
    over_text = "%s: %d encoder rows held a value of magnitude >= %g (or not finite) and were left out of the codebook's average"

    def __init__(self, codebook, beta=BETA, decay=DECAY, rows=0, ctx=None, restart=None):
        """restart: None, or the threshold in (0, 1) below which a codeword that took no row this step is put back onto one of the
        step's encoder rows (zs_vq_restart)."""
        if not isinstance(codebook, vq.VectorCodebook):
            raise ValueError('VqBottleneck: a vector codebook (vq.VectorCodebook) is needed')
        super(VqBottleneck, self).__init__(codebook, beta, decay, rows, ctx, restart)
        dev, f32 = self.device, torch.float32
        self.loss = torch.zeros(1, dtype=f32, device=dev)        # loss_vq of the last step
        # sticky: bad idx (commit) | rows above MAX_ABS | bad idx (backward) | with restart: codewords restarted so far | restarts skipped
        self.stat = torch.zeros(4 if restart is None else 5, dtype=torch.int32, device=dev)
        self.z_f32 = torch.zeros(self.rows, self.E, dtype=f32, device=dev) if ctx.tdt != f32 else None

    # ---- the step ----------------------------------------------------------------------------------------------------------------------
    def forward(self, bits, seed=0, seed_ptr=None):
        """bits: the Act [B, T', E] EncoderEngine.forward returns.  Enqueues assign, commit, accum and the codebook's average;
        returns q, an Act the DecoderEngine takes as it takes bits.  (seed, seed_ptr): the pair the encoder's forward of this step
        was given; with restart on, the rows that dead codewords take follow it."""
        ctx, K, E, n = self.ctx, self.K, self.E, self.rows
        self._check_forward(bits)
        st = ctx.stream
        self.code_live.copy_(self.code)                          # the codebook the step before left
        self.cnorm_live.copy_(self.cnorm)
        self.acc.zero_()
        vq.launch_assign(st, ctx.dt, bits.ptr(), n, bits.ld, self.code_live, self.cnorm_live, idx=self.idx, work=self.work)
        q = ctx.act('vq_q_%d_%d' % (bits.B, bits.T), bits.B, bits.T, E)
        zf = self.z_f32
        L.call('zs_vq_commit', 'ZsVqCommit', st, dtype=ctx.dt, z=bits.ptr(), n=n, ld_z=bits.ld, idx=L.ptr(self.idx),
               code=L.ptr(self.code_live), ld_code=E, K=K, E=E, q=q.ptr(), ld_q=q.ld, z_f32=L.ptr(zf), ld_zf=(E if zf is not None else 0),
               idx_acc=L.ptr(self.idx_acc), scale=self.scale, partial=L.ptr(self.partial), loss=L.ptr(self.loss),
               bad=L.ptr(self.stat), over=L.ptr(self.stat, 1))
        rows32, ld32 = (L.ptr(zf), E) if zf is not None else (bits.ptr(), bits.ld)
        self._average(0, rows32, ld32, seed, seed_ptr)
        self._bits = bits
        self.steps += 1
        return q

    def backward(self, dbits):
        """dbits: the Act [B, T', E] the Decoder's backward returns (d loss / d q).  Returns d loss / d z, written in place."""
        self._check_backward(dbits)
        bits = self._bits
        L.call('zs_vq_st_bwd', 'ZsVqStBwd', self.ctx.stream, dtype=self.ctx.dt, dq=dbits.ptr(), n=self.rows, ld_dq=dbits.ld, z=bits.ptr(),
               ld_z=bits.ld, idx=L.ptr(self.idx), code=L.ptr(self.code_live), ld_code=self.E, K=self.K, E=self.E, g=self.g,
               dz=dbits.ptr(), ld_dz=dbits.ld, bad=L.ptr(self.stat, 2))
        return dbits

    def stats(self):
        """The last step's figures, read from the device (a synchronisation: call where the host syncs anyway).  RuntimeError when a
        row was left out of the average because an element reached ZS_VQ_MAX_ABS, or an index was outside [0, K)."""
        stat = self._checked_stat()
        head = self.acc[:self._sum_at].cpu().numpy()
        cnt = head[self._cnt_at:].view(np.int32)[:self.K]
        used = int(head[:1].view(np.int32)[0])
        out = {'loss_vq': float(self.loss.item()), 'used': used, 'K': self.K, 'perplexity': perplexity(cnt)}
        if self.restart is not None:
            out.update(restarts=int(stat[3]), skipped=int(stat[4]), dead=int((self.N < self.restart).sum().item()))
        return out


def check_train_flags(args, flag, book, whose, carried):
    """The refusals --vq_train and --rvq_train share, in the order both make them: `flag` without --train_ae or beside another
    --train* mode, under a multi-rank launch, with --resume, with --valid_every, and --vq_beta, --vq_decay or --vq_restart out of
    range.  book, whose, carried: the words in which the two messages differ."""
    others = [f for f in ('train', 'train_p', 'train_tgat', 'train_c') if getattr(args, f, False)]
    if others or not getattr(args, 'train_ae', False):
        raise ValueError('%s trains the autoencoder through its %s: it needs --train_ae and no other --train* mode' % (flag, book)
                         + (' (got --%s)' % others[0] if others else ''))
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise ValueError('%s runs on one GPU: %s counts and sums would need an all-reduce (WORLD_SIZE = %s)'
                         % (flag, whose, os.environ['WORLD_SIZE']))
    if getattr(args, 'resume', False):
        raise ValueError('%s cannot be combined with --resume: the train-state file does not carry the %s' % (flag, carried))
    if getattr(args, 'valid_every', None) is not None:
        raise ValueError('%s cannot be combined with --valid_every: the validation step does not quantise' % flag)
    for name, check in (('vq_beta', check_beta), ('vq_decay', check_decay), ('vq_restart', check_restart)):
        if getattr(args, name, None) is not None:
            check(getattr(args, name))


def load_for(flag, path, enc_mode, c_in):
    """The codebook file of `flag`, read; what the reader refuses is refused in the flag's name."""
    try:
        return vq.load_codebook(path, enc_mode, E=c_in)
    except ValueError as e:
        raise ValueError('%s: %s' % (flag, e))


def check_vq_train(args, enc_mode=None, c_in=None):
    """--vq_train, --vq_beta and --vq_decay are refused, before anything is built, where they cannot do what they say.  Called
    before hps is read (enc_mode None: the flag combinations) and again once enc_mode and the Decoder's width are known: then the
    file is read, and the loaded VectorCodebook returned (None without --vq_train)."""
    path = getattr(args, 'vq_train', None)
    if path is None:
        if getattr(args, 'rvq_train', None) is not None:       # the three options serve it too (rvq_train.check_rvq_train)
            return None
        for flag in ('vq_beta', 'vq_decay', 'vq_restart'):
            if getattr(args, flag, None) is not None:
                raise ValueError('--%s needs --vq_train or --rvq_train' % flag)
        return None
    check_train_flags(args, '--vq_train', 'codebook', "the codebook's", 'codebook')
    if enc_mode is None:
        return None
    vq.VectorCodebook.check_mode(enc_mode, "--vq_train needs enc_mode 'continues'")
    cb = load_for('--vq_train', path, enc_mode, c_in)
    if cb.kind == 'residual':
        raise ValueError("--vq_train: %s is a residual codebook (kind 'residual'): training through a residual codebook is not "
                         'supported, --vq_train takes a vector codebook (FILE.vq.npz)' % path)
    return cb


def ckpt_path(checkpoint):
    """<checkpoint name>.vq.npz: the codebook beside a checkpoint."""
    return checkpoint + VqBottleneck.ckpt_suffix
