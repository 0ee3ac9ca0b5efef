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
the step's encoder rows by zs_vq_restart, behind the average; tests/vq_restart_ref.py is its definition."""
import numpy as np
import torch

from . import _lib as L
from . import vq

BETA = 0.25            # the commitment weight and the decay of the paper
DECAY = 0.99
MAX_ABS = float(L.ENUMS['ZS_VQ_MAX_ABS'])
PARTS = L.ENUMS['ZS_VQ_COMMIT_PARTS']
MIN_COUNT = 1e-3       # a codeword whose averaged count is below this keeps its row (zs_vq_ema)


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


class VqBottleneck(object):
    """The device state (code, cnorm, N, m) and the plan's buffers of the quantiser for `rows` encoder rows per step.
    codebook: the vq.VectorCodebook the run starts from (code = vectors, N = 1, m = code); ctx: a layers.Ctx (device, compute dtype
    and the buffer of q)."""
    kind = 'vector'                                              # its codebook's (rvq_train.RvqBottleneck: 'residual')

    def __init__(self, codebook, beta=BETA, decay=DECAY, rows=0, ctx=None, restart=None):
        """restart: None, or the threshold in (0, 1) below which a codeword that took no row this step is put back onto one of the
        step's encoder rows (zs_vq_restart)."""
        if not isinstance(codebook, vq.VectorCodebook):
            raise ValueError('VqBottleneck: a vector codebook (vq.VectorCodebook) is needed')
        self.beta, self.decay = check_beta(beta), check_decay(decay)
        self.rows = int(rows)
        if not 1 <= self.rows < 2 ** 31:
            raise ValueError('VqBottleneck: rows must be in [1, 2^31) (got %d)' % self.rows)
        self.ctx, self.base = ctx, codebook
        self.K, self.E = codebook.K, codebook.E
        dev = self.device = ctx.device
        K, E, n = self.K, self.E, self.rows
        self.shift = vq.vq_shift(n, MAX_ABS)                     # a host constant of the plan: a row above MAX_ABS is left out
        self.scale = self.beta / (float(n) * E)                  # loss_vq = scale * sum (z - code[idx])^2
        self.g = float(np.float32(2.0 * self.beta / (float(n) * E)))
        f32 = dict(dtype=torch.float32, device=dev)
        # the state: what the last step left (`code`, `cnorm` are the `next` copies the average writes)
        self.code = torch.from_numpy(codebook.vectors).to(dev).contiguous()
        self.cnorm = torch.from_numpy(codebook.cnorm).to(dev).contiguous()
        self.N = torch.ones(K, **f32)
        self.m = self.code.clone()
        # the live copies: what this step's assign, commit and backward read
        self.code_live, self.cnorm_live = self.code.clone(), self.cnorm.clone()
        self.idx = torch.zeros(n, dtype=torch.int32, device=dev)
        self.idx_acc = torch.zeros(n, dtype=torch.int32, device=dev)
        # zeroed at the head of every step: (used | accum's own bad count) | cnt int32 [K] | sum int64 [K][E]
        self._cnt_at = 1
        self._sum_at = 1 + (K + 1) // 2
        self.acc = torch.zeros(self._sum_at + K * E, dtype=torch.int64, device=dev)
        self.cnt = self.acc[self._cnt_at:self._sum_at].view(torch.int32)[:K]
        self.sums = self.acc[self._sum_at:].view(K, E)
        self.partial = torch.zeros(PARTS, dtype=torch.float64, device=dev)
        self.loss = torch.zeros(1, **f32)                        # loss_vq of the last step
        # sticky: bad idx (commit) | rows above MAX_ABS | bad idx (backward) | with restart: codewords restarted so far | restarts skipped
        self.stat = torch.zeros(4 if restart is None else 5, dtype=torch.int32, device=dev)
        self.work = vq.workspace(dev) if n < vq.SPLIT_N else None
        self.z_f32 = torch.zeros(n, E, **f32) if ctx.tdt != torch.float32 else None
        self.restart = None if restart is None else check_restart(restart)
        if self.restart is not None:
            self.stride = restart_stride(n)                      # a host constant of the plan
            self.rwork = torch.zeros(K + 2, dtype=torch.int32, device=dev)
        self.steps = 0
        self._bits = None

    # ---- the step ----------------------------------------------------------------------------------------------------------------------
    def forward(self, bits, seed=0, seed_ptr=None):
        """bits: the Act [B, T', E] EncoderEngine.forward returns.  Enqueues assign, commit, accum and the codebook's average;
        returns q, an Act the DecoderEngine takes as it takes bits.  (seed, seed_ptr): the pair the encoder's forward of this step
        was given; with restart on, the rows that dead codewords take follow it."""
        ctx, K, E, n = self.ctx, self.K, self.E, self.rows
        if bits.rows != n or bits.C != E or bits.t.dtype != ctx.tdt:
            raise ValueError('VqBottleneck: built for %d rows of %d columns of %s, got %d rows of %d of %s' %
                             (n, E, ctx.tdt, bits.rows, bits.C, bits.t.dtype))
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
        L.call('zs_vq_accum', 'ZsVqAccum', st, x=(L.ptr(zf) if zf is not None else bits.ptr()), idx=L.ptr(self.idx_acc), n=n,
               ld_x=(E if zf is not None else bits.ld), K=K, E=E, shift=self.shift, cnt=L.ptr(self.cnt), sum=L.ptr(self.sums),
               bad=L.ptr(self.acc.view(torch.int32), 1))
        L.call('zs_vq_ema', 'ZsVqEma', st, cnt=L.ptr(self.cnt), sum=L.ptr(self.sums), K=K, E=E, shift=self.shift, decay=self.decay,
               N=L.ptr(self.N), m=L.ptr(self.m), code=L.ptr(self.code), ld_code=E, cnorm=L.ptr(self.cnorm),
               used=L.ptr(self.acc.view(torch.int32)))
        if self.restart is not None:
            L.call('zs_vq_restart', 'ZsVqRestart', st, thresh=self.restart, x=(L.ptr(zf) if zf is not None else bits.ptr()), n=n,
                   ld_x=(E if zf is not None else bits.ld), idx_acc=L.ptr(self.idx_acc), cnt=L.ptr(self.cnt), K=K, E=E, N=L.ptr(self.N),
                   m=L.ptr(self.m), code=L.ptr(self.code), ld_code=E, cnorm=L.ptr(self.cnorm), seed=int(seed or 0) % (1 << 64),
                   seed_ptr=seed_ptr, stride=self.stride, work=L.ptr(self.rwork), restarted=L.ptr(self.stat, 3),
                   skipped=L.ptr(self.stat, 4))
        self._bits = bits
        self.steps += 1
        return q

    def backward(self, dbits):
        """dbits: the Act [B, T', E] the Decoder's backward returns (d loss / d q).  Returns d loss / d z, written in place."""
        bits = self._bits
        if bits is None or dbits.rows != self.rows or dbits.C != self.E:
            raise ValueError('VqBottleneck.backward: no forward of %d rows before it' % dbits.rows)
        L.call('zs_vq_st_bwd', 'ZsVqStBwd', self.ctx.stream, dtype=self.ctx.dt, dq=dbits.ptr(), n=self.rows, ld_dq=dbits.ld, z=bits.ptr(),
               ld_z=bits.ld, idx=L.ptr(self.idx), code=L.ptr(self.code_live), ld_code=self.E, K=self.K, E=self.E, g=self.g,
               dz=dbits.ptr(), ld_dz=dbits.ld, bad=L.ptr(self.stat, 2))
        return dbits

    # ---- host side ---------------------------------------------------------------------------------------------------------------------
    def stats(self):
        """The last step's figures, read from the device (a synchronisation: call where the host syncs anyway).  RuntimeError when a
        row was left out of the average because an element reached ZS_VQ_MAX_ABS, or an index was outside [0, K)."""
        stat = self.stat.cpu().numpy()
        if stat[1]:
            raise RuntimeError('--vq_train: %d encoder rows held a value of magnitude >= %g (or not finite) and were left out of the '
                               "codebook's average" % (int(stat[1]), MAX_ABS))
        if stat[0] or stat[2]:
            raise RuntimeError('--vq_train: zs_vq_assign gave %d indices outside [0, %d)' % (int(stat[0]) + int(stat[2]), self.K))
        head = self.acc[:self._sum_at].cpu().numpy()
        cnt = head[self._cnt_at:].view(np.int32)[:self.K]
        used = int(head[:1].view(np.int32)[0])
        out = {'loss_vq': float(self.loss.item()), 'used': used, 'K': self.K, 'perplexity': perplexity(cnt)}
        if self.restart is not None:
            out.update(restarts=int(stat[3]), skipped=int(stat[4]), dead=int((self.N < self.restart).sum().item()))
        return out

    def state_dict(self):
        return {'code': self.code, 'cnorm': self.cnorm, 'N': self.N, 'm': self.m}

    def load_state_dict(self, sd):
        for k in ('code', 'cnorm', 'N', 'm'):
            dst, src = getattr(self, k), torch.as_tensor(sd[k])
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError('VqBottleneck: state %r has shape %s, this bottleneck %s' % (k, tuple(src.shape), tuple(dst.shape)))
        for k in ('code', 'cnorm', 'N', 'm'):
            getattr(self, k).copy_(torch.as_tensor(sd[k]).to(torch.float32))

    def ckpt_meta(self, iteration, s):
        """The meta fields of <checkpoint>.vq.npz after `iteration` iterations; s: stats()."""
        meta = {'trained_iterations': int(iteration), 'beta': self.beta, 'decay': self.decay, 'used': s['used']}
        if self.restart is not None:
            meta.update(restart=self.restart, restarts=s['restarts'])
        return meta

    def to_codebook(self, meta=None):
        """The codebook as the last step left it: a vq.VectorCodebook whose meta is the starting file's plus `meta`."""
        out = dict(self.base.meta)
        out.update(meta or {})
        return vq.VectorCodebook(self.code.cpu().numpy(), out)


def check_vq_train(args, enc_mode=None, c_in=None):
    """--vq_train, --vq_beta and --vq_decay are refused, before anything is built, where they cannot do what they say.  Called
    before hps is read (enc_mode None: the flag combinations) and again once enc_mode and the Decoder's width are known: then the
    file is read, and the loaded VectorCodebook returned (None without --vq_train)."""
    import os
    path = getattr(args, 'vq_train', None)
    if path is None:
        if getattr(args, 'rvq_train', None) is not None:       # the three options serve it too (rvq_train.check_rvq_train)
            return None
        for flag in ('vq_beta', 'vq_decay', 'vq_restart'):
            if getattr(args, flag, None) is not None:
                raise ValueError('--%s needs --vq_train or --rvq_train' % flag)
        return None
    others = [f for f in ('train', 'train_p', 'train_tgat', 'train_c') if getattr(args, f, False)]
    if others or not getattr(args, 'train_ae', False):
        raise ValueError('--vq_train trains the autoencoder through its codebook: it needs --train_ae and no other --train* mode'
                         + (' (got --%s)' % others[0] if others else ''))
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise ValueError("--vq_train runs on one GPU: the codebook's counts and sums would need an all-reduce (WORLD_SIZE = %s)"
                         % os.environ['WORLD_SIZE'])
    if getattr(args, 'resume', False):
        raise ValueError('--vq_train cannot be combined with --resume: the train-state file does not carry the codebook')
    if getattr(args, 'valid_every', None) is not None:
        raise ValueError('--vq_train cannot be combined with --valid_every: the validation step does not quantise')
    if getattr(args, 'vq_beta', None) is not None:
        check_beta(args.vq_beta)
    if getattr(args, 'vq_decay', None) is not None:
        check_decay(args.vq_decay)
    if getattr(args, 'vq_restart', None) is not None:
        check_restart(args.vq_restart)
    if enc_mode is None:
        return None
    vq.VectorCodebook.check_mode(enc_mode, "--vq_train needs enc_mode 'continues'")
    try:
        cb = vq.load_codebook(path, enc_mode, E=c_in)
    except ValueError as e:
        raise ValueError('--vq_train: %s' % e)
    if cb.kind == 'residual':
        raise ValueError("--vq_train: %s is a residual codebook (kind 'residual'): training through a residual codebook is not "
                         'supported, --vq_train takes a vector codebook (FILE.vq.npz)' % path)
    return cb


def ckpt_path(checkpoint):
    """<checkpoint name>.vq.npz: the codebook beside a checkpoint."""
    return checkpoint + '.vq.npz'

