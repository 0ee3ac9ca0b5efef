"""Training a 'continues' model through its residual codebook: `--rvq_train FILE.rvq.npz` puts the S-stage quantiser of
zs_amd.rvq between the Encoder and the Decoder of the --train_ae step.  Stage 0 snaps every encoder row to its nearest codeword, stage
s what stage s - 1 left over (zs_vq_assign, unchanged); the Decoder reads the sum of the S codewords exactly as conversion builds it
(zs_rvq_gather, unchanged) and hands its input gradient straight through; every stage commits its input to its codeword,
loss_vq = beta * mean sum_s r_{s+1}^2, whose gradient is 2 beta / (n E) (r_1 + .. + r_S); and every stage's codebook follows its own
input rows by the exponential moving average of vq_train (zs_vq_accum, zs_vq_ema and, with --vq_restart, zs_vq_restart, all
unchanged).  The glue on the step's critical path is csrc/zs_rvq_train.hip: zs_rvq_commit (one launch per stage: the residual, the sum
of the residuals, the index zs_vq_accum reads and the loss's partial sums in one pass over the row), zs_rvq_loss and zs_rvq_st_bwd.
Step t reads, in every stage, the codebook step t - 1 left: the averages are written to the `next` copies, which become the live ones at
the head of the next forward.  Everything is enqueued on the current stream with launch arguments that do not change between
iterations, so the captured step replays it; nothing adds floats atomically, so a run is bitwise reproducible.
tests/rvq_train_ref.py is the numpy definition.  Not in the reference, which has no codebook.
Quantiser dropout (`--rvq_dropout P`): with probability P a sample of the batch is decoded from s_b stages, uniform over
1 .. S, drawn on the device from the step's own seed stream (zs_rvq_drop_draw); the stages at or above s_b neither commit that
sample's rows nor count them (zs_rvq_commit_drop in place of zs_rvq_commit) and the Decoder reads the sum of its first s_b codewords
(zs_rvq_gather_frag in place of zs_rvq_gather), so every coarser bitrate --rvq_stages s offers is a trained operating point.
include/zs_amd_rvq_drop.h; the draw is csrc/zs_rvq_drop.hip, the other two are the commit's and the gather's own kernels with the mask
compiled in; tests/rvq_drop_ref.py is the numpy definition.  Without it nothing new is launched.
What this class shares with vq_train.VqBottleneck is vq_train.Bottleneck."""
import numpy as np
import torch

from . import _lib as L
from . import rvq, vq
from .vq_train import (BETA, DECAY, GOLDEN, MAX_ABS, PARTS, Bottleneck, check_beta, check_decay, check_restart,  # noqa: F401
                       check_train_flags, load_for, perplexity, restart_stride)

DROP_ONE = 1 << 24                 # zs_rvq_drop_draw compares 24 bits of the draw with floor(P 2^24)


def check_dropout(p, what='--rvq_dropout'):
    """P of quantiser dropout as a float: finite and in (0, 1] (and at least 2^-24, the draw's resolution), else ValueError."""
    try:
        v = float(p)
    except (TypeError, ValueError):
        raise ValueError('%s must be a number in (0, 1] (got %r)' % (what, p))
    if not np.isfinite(v) or not 0.0 < v <= 1.0:
        raise ValueError('%s must be in (0, 1] (got %r)' % (what, p))
    if drop_threshold(v) < 1:
        raise ValueError('%s must be at least 2^-24, the resolution of the draw (got %r)' % (what, p))
    return v


def drop_threshold(p):
    """thr = floor(P 2^24), the integer zs_rvq_drop_draw compares with (P 2^24 is exact in a double: a shift of the exponent)."""
    return int(np.floor(float(p) * DROP_ONE))


class RvqBottleneck(Bottleneck):
    """The device state (per stage code, cnorm, N, m) and the plan's buffers of the S-stage quantiser for `rows` encoder rows per
    step: vq_train.VqBottleneck's interface.  codebook: the rvq.ResidualCodebook the run starts from (code = vectors, N = 1,
    m = code); ctx: a layers.Ctx (device, compute dtype and the buffer of q)."""
    kind, flag, ckpt_suffix = 'residual', '--rvq_train', '.rvq.npz'
    over_text = "%s: %d rows of a stage held a value of magnitude >= %g (or not finite) and were left out of that stage's average"

    dropout = None

    def __init__(self, codebook, beta=BETA, decay=DECAY, rows=0, ctx=None, restart=None, dropout=None):
        """restart: None, or the threshold in (0, 1) below which a codeword of any stage that took no row this step is put back onto
        one of the rows that stage quantised (zs_vq_restart).  dropout: None, or P in (0, 1]: the probability with which a
        sample is decoded from a number of stages drawn uniformly from 1 .. S instead of all S."""
        if not isinstance(codebook, rvq.ResidualCodebook):
            raise ValueError('RvqBottleneck: a residual codebook (rvq.ResidualCodebook) is needed')
        self.S = codebook.S
        super(RvqBottleneck, self).__init__(codebook, beta, decay, rows, ctx, restart, stages=self.S)
        S, E, n, dev = self.S, self.E, self.rows, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.loss = torch.zeros(1 + S, **f32)                    # loss_vq of the last step, then every stage's share of it
        # sticky: bad idx (commit) | rows above MAX_ABS | bad frames (gather) | codewords restarted so far | restarts skipped
        self.stat = torch.zeros(5, **i32)
        # two fp32 [n, E] buffers in ping-pong: stage s reads r_s in one and writes r_{s+1} to the other; the fp32 copy of bf16
        # rows is the first one's first content.  zs_vq_accum, the average and the restart of stage s read r_s behind the commit
        # of stage s and in front of the commit of stage s + 1, which overwrites it: stream order keeps that safe.
        self.res = [torch.zeros(n, E, **f32), torch.zeros(n, E, **f32)]
        self.a = torch.zeros(n, E, **f32)                        # r_1 + .. + r_S, what the backward reads
        self._frag = {}                                          # (B, T') -> the device table of zs_rvq_gather
        self.dropout = None if dropout is None else check_dropout(dropout, 'RvqBottleneck: dropout')
        if self.dropout is not None:
            self.thr = drop_threshold(self.dropout)              # a host constant of the plan
            self.active = torch.zeros(S, **i32)                  # rows that took part in stage s in the last step
            self._s_use = {}                                     # B -> the stage count of every sample, int32 [B]
            self.s_use = None                                    # the one the last forward wrote

    def _table(self, B, T):
        """start[b] = b T', len[b] = T': the batch as the B fragments of zs_rvq_gather (built once per shape, before any capture)."""
        tab = self._frag.get((B, T))
        if tab is None:
            tab = self._frag[(B, T)] = (torch.arange(B, dtype=torch.int64, device=self.device) * T,
                                        torch.full((B,), T, dtype=torch.int32, device=self.device))
        return tab

    def _counts(self, B):
        """s_use int32 [B]: what zs_rvq_drop_draw writes for a batch of B samples (built once per shape, before any capture)."""
        t = self._s_use.get(B)
        if t is None:
            t = self._s_use[B] = torch.zeros(B, dtype=torch.int32, device=self.device)
        return t

    # ---- the step ----------------------------------------------------------------------------------------------------------------------
    def forward(self, bits, seed=0, seed_ptr=None):
        """bits: the Act [B, T', E] EncoderEngine.forward returns.  Enqueues, per stage, assign, commit, accum and the codebook's
        average (and the restart), then the loss and the gather; returns q, an Act the DecoderEngine takes as it takes bits.
        (seed, seed_ptr): the pair the encoder's forward of this step was given; with restart on, the rows that dead codewords take
        follow it.  With dropout the step's stage counts are drawn from the same pair first, every commit is zs_rvq_commit_drop and
        the gather zs_rvq_gather_frag."""
        ctx, S, K, E, n = self.ctx, self.S, self.K, self.E, self.rows
        self._check_forward(bits)
        st = ctx.stream
        start, length = self._table(bits.B, bits.T)
        self.code_live.copy_(self.code)                          # the codebooks the step before left
        self.cnorm_live.copy_(self.cnorm)
        self.acc.zero_()
        wide = ctx.tdt != torch.float32                          # the rows need an fp32 copy for zs_vq_accum
        drop = None
        if self.dropout is not None:
            if bits.B * bits.T != n:
                raise ValueError('RvqBottleneck: dropout needs %d samples of %d rows to be the %d rows' % (bits.B, bits.T, n))
            s_use = self.s_use = self._counts(bits.B)
            L.call('zs_rvq_drop_draw', 'ZsRvqDropDraw', st, seed=int(seed or 0) % (1 << 64), seed_ptr=seed_ptr, thr=self.thr, S=S,
                   n_frag=bits.B, rows_per_frag=bits.T, s_use=L.ptr(s_use), active=L.ptr(self.active))
            drop = dict(s_use=L.ptr(s_use), rows_per_frag=bits.T)
        for s in range(S):
            code, cn = self.code_live[s], self.cnorm_live[s]
            if s == 0:
                x, ld_x, f32 = bits.ptr(), bits.ld, 0
                rows32, ld32 = (L.ptr(self.res[0]), E) if wide else (x, ld_x)
            else:
                x = rows32 = L.ptr(self.res[s & 1])
                ld_x = ld32 = E
                f32 = 1
            vq.launch_assign(st, (L.ZS_F32 if f32 else ctx.dt), x, n, ld_x, code, cn, idx=self.idx[s], work=self.work)
            commit = dict(dtype=ctx.dt, src_f32=f32, first=int(s == 0), x=x, n=n, ld_x=ld_x,
                          idx=L.ptr(self.idx[s]), code=L.ptr(code), ld_code=E, K=K, E=E, r=L.ptr(self.res[(s + 1) & 1]), ld_r=E,
                          x_f32=(L.ptr(self.res[0]) if s == 0 and wide else None), ld_xf=(E if s == 0 and wide else 0),
                          idx_acc=L.ptr(self.idx_acc[s]), a=L.ptr(self.a), ld_a=E, partial=L.ptr(self.partial[s]), bad=L.ptr(self.stat),
                          over=L.ptr(self.stat, 1))
            if drop is None:
                L.call('zs_rvq_commit', 'ZsRvqCommit', st, **commit)
            else:
                L.call('zs_rvq_commit_drop', 'ZsRvqCommitDrop', st, stage=s, **dict(commit, **drop))
            self._average(s, rows32, ld32, seed, seed_ptr)
        L.call('zs_rvq_loss', 'ZsRvqLoss', st, partial=L.ptr(self.partial), S=S, scale=self.scale, loss=L.ptr(self.loss))
        q = ctx.act('rvq_q_%d_%d' % (bits.B, bits.T), bits.B, bits.T, E)
        if drop is None:
            rvq.launch_gather(st, ctx.dt, self.idx, S, self.code_live, start, length, bits.B, bits.T, q.ptr(), q.ld, self.stat[2:])
        else:
            code = self.code_live
            L.call('zs_rvq_gather_frag', 'ZsRvqGatherFrag', st, dtype=ctx.dt, idx=L.ptr(self.idx), n_idx=n, ld_idx=n, S=S, s_use=drop['s_use'],
                   code=L.ptr(code), ld_code=code.stride(1), plane_code=code.stride(0), K=K, E=E, start=L.ptr(start), len=L.ptr(length),
                   n_frag=bits.B, T=bits.T, dst=q.ptr(), ld_dst=q.ld, bad=L.ptr(self.stat, 2))
        self._bits = bits
        self.steps += 1
        return q

    def backward(self, dbits):
        """dbits: the Act [B, T', E] the Decoder's backward returns (d loss / d q).  Returns d loss / d z, written in place."""
        self._check_backward(dbits)
        L.call('zs_rvq_st_bwd', 'ZsRvqStBwd', self.ctx.stream, dtype=self.ctx.dt, dq=dbits.ptr(), n=self.rows, ld_dq=dbits.ld,
               a=L.ptr(self.a), ld_a=self.E, E=self.E, g=self.g, dz=dbits.ptr(), ld_dz=dbits.ld)
        return dbits

    # ---- host side ---------------------------------------------------------------------------------------------------------------------
    def stats(self):
        """The last step's figures, read from the device (a synchronisation: call where the host syncs anyway): loss_vq, K, S and
        `stages`, per stage dict(loss_vq, used, perplexity); `used` is the list of the stages' counts.  With dropout every stage also
        has `active`, the rows that took part in it, and the result `active` (their list) and `s_use_mean`, the mean stage count of
        the last step's samples; the rows a stage left out and the restarts skipped for them raise nothing.  RuntimeError when a row was
        left out of an average because an element reached ZS_VQ_MAX_ABS, or an index was outside [0, K)."""
        stat = self._checked_stat()
        head = self.acc[:, :self._sum_at].cpu().numpy()
        loss = self.loss.cpu().numpy()
        stages = []
        for s in range(self.S):
            cnt = head[s, self._cnt_at:].view(np.int32)[:self.K]
            stages.append({'loss_vq': float(loss[1 + s]), 'used': int(head[s, :1].view(np.int32)[0]), 'perplexity': perplexity(cnt)})
        out = {'loss_vq': float(loss[0]), 'K': self.K, 'S': self.S, 'stages': stages, 'used': [st['used'] for st in stages],
               'perplexity': [st['perplexity'] for st in stages]}
        if self.restart is not None:
            out.update(restarts=int(stat[3]), skipped=int(stat[4]), dead=[int(v) for v in (self.N < self.restart).sum(1).cpu()])
        if self.dropout is not None:
            active = [int(v) for v in self.active.cpu()]
            for stg, v in zip(stages, active):
                stg['active'] = v
            out.update(active=active, s_use_mean=(float(self.s_use.cpu().numpy().mean()) if self.s_use is not None else float(self.S)))
        return out

    def ckpt_meta(self, iteration, s):
        """The meta fields of <checkpoint>.rvq.npz after `iteration` iterations; s: stats()."""
        meta = super(RvqBottleneck, self).ckpt_meta(iteration, dict(s, used=list(s['used'])))
        if self.dropout is not None:
            meta.update(dropout=self.dropout)
        return meta


def check_rvq_train(args, enc_mode=None, c_in=None):
    """--rvq_train is refused, before anything is built, where it cannot do what it says.  Called before hps is read (enc_mode None:
    the flag combinations) and again once enc_mode and the Decoder's width are known: then the file is read, and the loaded
    ResidualCodebook returned (None without --rvq_train).  --vq_beta, --vq_decay and --vq_restart serve --vq_train or --rvq_train;
    without either, vq_train.check_vq_train refuses them."""
    path = getattr(args, 'rvq_train', None)
    if path is None:
        if getattr(args, 'rvq_dropout', None) is not None:
            if getattr(args, 'vq_train', None) is not None:
                raise ValueError('--rvq_dropout cannot be combined with --vq_train: a vector codebook has one stage and nothing to drop; '
                                 'it serves --rvq_train FILE.rvq.npz')
            raise ValueError('--rvq_dropout needs --rvq_train FILE.rvq.npz: it drops stages of the residual codebook the run trains '
                             'through')
        return None
    if getattr(args, 'rvq_dropout', None) is not None and getattr(args, 'vq_train', None) is not None:
        raise ValueError('--rvq_dropout cannot be combined with --vq_train: a vector codebook has one stage and nothing to drop')
    if getattr(args, 'vq_train', None) is not None:
        raise ValueError('--rvq_train cannot be combined with --vq_train: a run trains through one codebook, a residual one '
                         '(--rvq_train FILE.rvq.npz) or a vector one (--vq_train FILE.vq.npz)')
    check_train_flags(args, '--rvq_train', 'residual codebook', "every stage's", 'codebooks')
    if getattr(args, 'rvq_dropout', None) is not None:
        check_dropout(args.rvq_dropout)
    if enc_mode is None:
        return None
    rvq.ResidualCodebook.check_mode(enc_mode, "--rvq_train needs enc_mode 'continues'")
    cb = load_for('--rvq_train', path, enc_mode, c_in)
    if cb.kind != 'residual':
        raise ValueError("--rvq_train: %s is no residual codebook (kind %r): --rvq_train takes FILE.rvq.npz, as --fit_codebook K "
                         '--rvq S writes it; a vector codebook goes to --vq_train' % (path, cb.kind))
    return cb


def ckpt_path(checkpoint):
    """<checkpoint name>.rvq.npz: the residual codebook beside a checkpoint."""
    return checkpoint + RvqBottleneck.ckpt_suffix
