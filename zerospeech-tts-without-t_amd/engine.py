"""Forward / backward schedules of the autoencoder on the HIP kernels (channels-last, explicit tape).

EncoderEngine  <->  Encoder.forward          (reference model/model.py:440-489) and its autograd backward
DecoderEngine  <->  Decoder.forward          (reference model/model.py:344-365) and its autograd backward
PatcherEngine  <->  Spectrogram_Patcher.forward (reference model/model.py:532-549) and its backward to the parameters
Every arithmetic step is a libzs_amd.so kernel; torch only owns the memory.
"""
import functools
import os
import torch

from . import _lib as L
from .layers import (Act, ConvLayer, GruLayer, cast_rows, colsum_ok, fork_side, grad_combine, instnorm_bwd, instnorm_fwd, join_side,
                     next_uid, pack_operands, rup, weight_operand)

LRELU = L.ZS_ACT_LRELU


def _half_up(t):
    return (t + 1) // 2


def _norm_stats(ctx, training, prefix, key, n):
    """The InstanceNorm statistics (mean, rstd) a training pass keeps for its backward, as buffers prefix + 'mean' / 'rstd' + key
    of ctx; (None, None) otherwise."""
    if not training:
        return None, None
    return ctx.f32(prefix + 'mean' + key, n), ctx.f32(prefix + 'rstd' + key, n)


def ragged_lengths(who, lengths, training, B, T, lo):
    """A ragged batch's host `lengths` checked (inference only, B values in [lo, T]) -> int32 tensor [B] on the host."""
    if training:
        raise L.ZsError('%s: ragged batches are an inference feature' % who)
    l0 = torch.as_tensor(lengths, dtype=torch.int32).reshape(-1)
    if l0.numel() != B or int(l0.max()) > T or int(l0.min()) < lo:
        raise L.ZsError('%s: lengths must be %d values in [%d, %d]' % (who, B, lo, T))
    return l0


# enc_mode -> discretiser of zs_gumbel_st_fwd / _bwd ('multilabel_binary' runs zs_mbv_fwd / _bwd)
GUMBEL_MODES = {'one_hot': L.ZS_ENC_ONE_HOT, 'binary': L.ZS_ENC_BINARY, 'continues': L.ZS_ENC_CONTINUES}


def linear_width(enc_mode, E):
    """Output columns of the encoder's `linear` (model/model.py:391-398): the width of `enc`."""
    return {'multilabel_binary': 2 * E, 'binary': E * E}.get(enc_mode, E)


def operands_of(layers):
    """(weights, vectors): the operands() of several layers joined."""
    w, v = [], []
    for l in layers:
        lw, lv = l.operands()
        w += lw
        v += lv
    return w, v


class EncoderEngine(object):
    def __init__(self, ctx, P, G, c_in, c_h1, c_h2, c_h3, enc_size, ns, dp, seg_len, enc_mode='multilabel_binary'):
        """P / G: dicts name -> fp32 parameter / gradient tensors (reference state_dict names)."""
        self.ctx = ctx
        self.uid = next_uid()
        self.c_in, self.c1, self.c2, self.H, self.E = c_in, c_h1, c_h2, c_h3, enc_size
        self.mode = enc_mode
        self.n_lin = linear_width(enc_mode, enc_size)
        self.ns, self.dp = float(ns), float(dp)
        self.pad_mode = L.ZS_PAD_REFLECT if seg_len >= 64 else L.ZS_PAD_ZERO     # model/model.py:38
        if c_h1 % 8 or c_h2 % 8:
            raise ValueError('c_h1 and c_h2 must be multiples of 8 (16-byte rows)')
        mk = functools.partial(ConvLayer.from_params, ctx, P, G, pad_mode=self.pad_mode)
        self.conv1s = [mk('conv1s.%d' % i) for i in range(7)]
        self.conv2 = mk('conv2')
        self.convs = [(mk('conv%d' % a), mk('conv%d' % b, stride=2)) for a, b in ((3, 4), (5, 6), (7, 8))]
        self.dense = [(mk('dense%d' % a), mk('dense%d' % b)) for a, b in ((1, 2), (3, 4))]
        self.gru = GruLayer(ctx, P, G, 'RNN.', name='enc%d' % self.uid)
        self.linear = mk('linear')
        self.layers = self.conv1s + [self.conv2] + [l for p in self.convs for l in p] + [l for p in self.dense for l in p] + \
            [self.linear]
        self.ncat = 7 * c_h1 + c_in
        self.tape = None
        self.tapes = {}
        self.bank_d = None            # the bank's data-gradient operand (backward_input), packed on first use after pack()
        self.adam_plan = None         # optim.AdamPackPlan of this engine's operands (ZsModule.adam_pack_plan)

    def operands(self):
        """(weights, vectors) of every layer (layers.weight_operand / vector_operand): the one description that pack() and the
        fused optimizer step's plan (optim.AdamPackPlan) are built from."""
        w, v = operands_of(self.layers + [self.gru])
        if self.bank_d is not None:
            w += self._bank_d_operands()
        return w, v

    def pack(self):
        with L.pack_batch(self.ctx.stream):
            pack_operands(self.ctx, *self.operands())

    # ------------------------------------------------------------------------------------------
    def forward(self, x, training, noise=None, noise_kind=2, seed=0, drop_masks=None, seed_ptr=None, lengths=None, tape=None):
        """x: fp32 [B, T, c_in] contiguous on device.  Returns (bits Act [B,T',E] (T dtype, feeds the decoder),
        bits_f32 [B,T',E], logits_f32 [B,T',ld] with n_lin valid columns).  noise (Gumbel if noise_kind 0, uniform if 1): fp32
        [B,T',E,2] (multilabel_binary), [B,T',E] (one_hot), [B,T',E,E] (binary); continues takes none.
        lengths: host int sequence [B], frames per sample (ragged batch, inference only): sample b is computed exactly as if it ran
        alone with T = lengths[b] (padding, InstanceNorm statistics and the reverse GRU at its own end); its first
        ceil(ceil(ceil(lengths[b]/2)/2)/2) output rows are valid, the rest is garbage.
        tape: None, or a key (str) of a tape of its own: the buffers of this pass (outputs and the backward's tape) are then
        distinct from those of the untagged pass and of other keys, so that e.g. the autolocker's re-encode leaves the first
        encode's bits alive.  backward* use the tape of the latest forward unless given a key."""
        c, ns = self.ctx, self.ns
        B, T, F = x.shape
        Ls = [None] * 4
        if lengths is not None:
            l0 = ragged_lengths('EncoderEngine', lengths, training, B, T, 9)                  # MIN_LEN (convert.py:36)
            l1 = (l0 + 1) // 2; l2 = (l1 + 1) // 2; l3 = (l2 + 1) // 2
            self.last_lengths = l3
            ld = torch.stack([l0, l1, l2, l3]).to(c.device, non_blocking=True)
            Ls = [ld[i] for i in range(4)]
        assert F == self.c_in and x.dtype == torch.float32 and x.is_contiguous()
        st = c.stream
        c1, c2, H, E = self.c1, self.c2, self.H, self.E
        dp = self.dp if training else 0.0
        masks = drop_masks if drop_masks is not None else [None] * 6
        Ts = [T, _half_up(T), _half_up(_half_up(T)), _half_up(_half_up(_half_up(T)))]
        T4 = Ts[3]
        ksfx = '' if tape is None else '_' + str(tape)
        tag = '_%d_%d_%d' % (self.uid, B, T) + ksfx
        tp = {'B': B, 'T': T, 'Ts': Ts, 'training': training, 'seed': seed, 'masks': masks, 'dp': dp, 'seed_ptr': seed_ptr,
              'tag': tag, 'ksfx': ksfx}
        # norm k (InstanceNorm + Dropout + residual, model/model.py:421-427, 434-437): dropout stream k + 1 or drop_masks[k]
        drop = dict(p=dp, seed=seed, seed_ptr=seed_ptr)
        skey = lambda k, Tk: '%d_%d_%d_%d' % (self.uid, k, B, Tk) + ksfx

        xin = c.act('e_xin' + tag, B, T, F)
        cat = c.act('e_cat' + tag, B, T, self.ncat)
        cast_rows(c, L.ptr(x), F, xin, dst2=cat, col_off2=7 * c1, act2=LRELU, slope2=ns)                         # :445-446
        if c.overlap_wgrad and B * T >= 4096:
            # the seven bank convs are independent and each fills half the chip at most (N = 128): run them side by side
            sts = fork_side(c.device)
            for i, l in enumerate(self.conv1s):                                                               # :441-444
                with torch.cuda.stream(sts[i % len(sts)]):
                    l.fwd(xin, out=cat.sub(i * c1, c1), act=LRELU, slope=ns, lengths=Ls[0])
            join_side(c.device)
        else:
            for i, l in enumerate(self.conv1s):
                l.fwd(xin, out=cat.sub(i * c1, c1), act=LRELU, slope=ns, lengths=Ls[0])
        y2 = c.act('e_y2' + tag, B, T, c2)
        self.conv2.fwd(cat, out=y2, act=LRELU, slope=ns)                                                      # :447
        a = c.act('e_a0' + tag, B, T, c2)
        mean, rstd = _norm_stats(c, training, 'e_', skey(0, T), B * y2.ld)
        instnorm_fwd(c, y2, a, mean, rstd, self.pad_mode, lengths=Ls[0], stream_id=1, mask=masks[0], **drop)
        tp.update(xin=xin, cat=cat, y2=y2, a0=a, st0=(mean, rstd, 0), blocks=[], dense=[])
        for i, (la, lb) in enumerate(self.convs):                                                            # :448-450
            ya = c.act('e_ya%d' % i + tag, B, Ts[i], c2)
            la.fwd(a, out=ya, act=LRELU, slope=ns, lengths=Ls[i])
            yb = c.act('e_yb%d' % i + tag, B, Ts[i + 1], c2)
            lb.fwd(ya, out=yb, act=LRELU, slope=ns, lengths=Ls[i])
            an = c.act('e_a%d' % (i + 1) + tag, B, Ts[i + 1], c2)
            k = 1 + i
            mean, rstd = _norm_stats(c, training, 'e_', skey(k, Ts[i + 1]), B * yb.ld)
            instnorm_fwd(c, yb, an, mean, rstd, self.pad_mode, res_mode=L.ZS_RES_AVGPOOL2, res=a, lengths=Ls[i + 1],
                         res_lengths=Ls[i], stream_id=k + 1, mask=masks[k], **drop)
            tp['blocks'].append((a, ya, yb, (mean, rstd, k)))
            a = an
        cat2 = c.act('e_cat2' + tag, B, T4, c2 + 2 * H)
        for j, (la, lb) in enumerate(self.dense):                                                            # :452-453
            d1 = c.act('e_d1%d' % j + tag, B, T4, c2)
            la.fwd(a, out=d1, act=LRELU, slope=ns)
            d2 = c.act('e_d2%d' % j + tag, B, T4, c2)
            lb.fwd(d1, out=d2, act=LRELU, slope=ns)
            out = c.act('e_do%d' % j + tag, B, T4, c2) if j == 0 else Act(cat2.t, B, T4, c2, cat2.ld, 0, rup(c2, 32))
            k = 4 + j
            mean, rstd = _norm_stats(c, training, 'e_', skey(k, T4), B * d2.ld)
            instnorm_fwd(c, d2, out, mean, rstd, self.pad_mode, res_mode=L.ZS_RES_IDENTITY, res=a, lengths=Ls[3], stream_id=k + 1,
                         mask=masks[k], **drop)
            tp['dense'].append((a, d1, d2, (mean, rstd, k)))
            a = out
        gi = c.act('e_gi' + tag, B, T4, 6 * H)
        gates = c.raw('e_gates' + tag, B * T4 * 8 * H, c.tdt) if training else None
        self.gru.fwd(a, cat2, c2, gi, gates, lengths=Ls[3])                                                 # :454-455
        logits = c.act('e_logits' + tag, B, T4, self.n_lin, dtype=torch.float32)
        self.linear.fwd(cat2, out=logits, out_f32=True)                                                      # :475
        bits = c.act('e_bits' + tag, B, T4, E)
        bits_f32 = c.f32('e_bitsf' + tag, B * T4 * E)
        s = None
        if self.mode == 'multilabel_binary':
            y0 = c.f32('e_y0' + tag, B * T4 * E)
            L.call('zs_mbv_fwd', 'ZsMbvFwd', st, dtype=c.dt, logits=logits.ptr(), ld=logits.ld, logits_f32=1,
                   noise=L.ptr(noise), noise_kind=noise_kind, seed=seed, seed_ptr=seed_ptr, rows=B * T4, E=E, tau=0.1, bits=bits.ptr(),
                   ld_bits=bits.ld, bits_fill_cols=bits.ld, bits_f32=L.ptr(bits_f32), y0=L.ptr(y0))           # :476-480
        else:                                                                                                # :457-472
            soft = self.mode != 'continues'
            y0 = c.f32('e_y0' + tag, B * T4 * self.n_lin) if (training and soft) else None
            s = c.f32('e_s' + tag, B * T4 * E) if (training and self.mode == 'binary') else None
            L.call('zs_gumbel_st_fwd', 'ZsGumbelStFwd', st, dtype=c.dt, mode=GUMBEL_MODES[self.mode], logits=logits.ptr(),
                   ld=logits.ld, logits_f32=1, noise=(L.ptr(noise) if soft else None), noise_kind=noise_kind, seed=seed,
                   seed_ptr=seed_ptr, rows=B * T4, E=E, tau=0.1, slope=self.ns, bits=bits.ptr(), ld_bits=bits.ld,
                   bits_fill_cols=bits.ld, bits_f32=L.ptr(bits_f32), y=L.ptr(y0), s=L.ptr(s))
        tp.update(cat2=cat2, gates=gates, y0=y0, s=s, T4=T4, gru_in=a, logits=logits, bits_f32=bits_f32)
        self.tape = tp
        self.tapes[tape] = tp
        return bits, bits_f32[:B * T4 * E].view(B, T4, E), logits

    # ------------------------------------------------------------------------------------------
    def backward(self, dbits, dlogits_extra=None):
        """dbits: Act [B,T',E] gradient w.r.t. enc_act (may be None); dlogits_extra: Act [B,T',n_lin] gradient w.r.t. the
        pre-activation `enc` (speaker-classifier term of trainer.py:444).  Fills every encoder parameter gradient."""
        self.backward_main(dbits, dlogits_extra)
        self.backward_bank()

    def backward_main(self, dbits, dlogits_extra=None, param_grads=True, tape=None):
        """Everything but the conv bank's seven weight gradients (the last gradients of the step: data parallel training starts
        the all-reduce of the rest of the encoder before them, trainer.AEStep).
        param_grads=False: the data gradients alone (no weight gradient, no gradient buffer written), and conv2's data gradient
        over all 7*c_h1 + c_in columns of the concatenation; returns that Act (see backward_input)."""
        c, ns = self.ctx, self.ns
        tp = self.tape if tape is None else self.tapes[tape]
        assert tp is not None and tp['training']
        pg = param_grads
        B, T, Ts, T4 = tp['B'], tp['T'], tp['Ts'], tp['T4']
        c1, c2, H, E = self.c1, self.c2, self.H, self.E
        st = c.stream
        tag = tp['tag']
        cat2 = tp['cat2']
        drop, masks = dict(p=tp['dp'], seed=tp['seed'], seed_ptr=tp['seed_ptr']), tp['masks']     # as in forward()
        dlog = c.act('e_dlog' + tag, B, T4, self.n_lin)
        if dbits is not None:
            if self.mode == 'multilabel_binary':
                L.call('zs_mbv_bwd', 'ZsMbvBwd', st, dtype=c.dt, dbits=dbits.ptr(), ld_dbits=dbits.ld, y0=L.ptr(tp['y0']),
                       rows=B * T4, E=E, tau=0.1, dlogits=dlog.ptr(), ld=dlog.ld, fill_cols=dlog.ld)
            else:
                cont = self.mode == 'continues'          # leaky_relu backward reads the pre-activation itself
                y, ld_y = (tp['logits'].ptr(), tp['logits'].ld) if cont else (L.ptr(tp['y0']), self.n_lin)
                L.call('zs_gumbel_st_bwd', 'ZsGumbelStBwd', st, dtype=c.dt, mode=GUMBEL_MODES[self.mode], dbits=dbits.ptr(),
                       ld_dbits=dbits.ld, y=y, ld_y=ld_y, s=L.ptr(tp['s']), rows=B * T4, E=E, tau=0.1, slope=ns,
                       dlogits=dlog.ptr(), ld=dlog.ld, fill_cols=dlog.ld)
            if dlogits_extra is not None:
                dlog.t[:B * T4 * dlog.ld].add_(dlogits_extra.t[:B * T4 * dlogits_extra.ld])
        else:
            dlog = dlogits_extra
        if pg:
            self.linear.wgrad(dlog, cat2)
        dcat2 = c.act('e_dcat2' + tag, B, T4, cat2.C)
        self.linear.dgrad(dlog, T4, dcat2)
        dgi = c.act('e_dgi' + tag, B, T4, 6 * H)
        dgh = c.act('e_dgh' + tag, B, T4, 6 * H)
        gin = tp['gru_in']
        da = c.act('e_da_d' + tag, B, T4, c2)
        self.gru.bwd(dcat2, c2, cat2, c2, tp['gates'], gin, dgi, dgh, da, add_src=dcat2, param_grads=pg)
        for j in (1, 0):
            la, lb = self.dense[j]
            xin, d1, d2, (mean, rstd, k) = tp['dense'][j]
            dz2 = c.act('e_dz2%d' % j + tag, B, T4, c2)          # unique per block: read later by the side-stream wgrad
            instnorm_bwd(c, da, d2, mean, rstd, dz2, ns, stream_id=k + 1, mask=masks[k], **drop)
            if pg:
                lb.wgrad(dz2, d1)
            dz1 = c.act('e_dz1%d' % j + tag, B, T4, c2)
            lb.dgrad(dz2, T4, dz1, dact_src=d1, slope=ns)
            if pg:
                la.wgrad(dz1, xin)
            dn = c.act('e_da_d%d' % j + tag, B, T4, c2)
            la.dgrad(dz1, T4, dn, add_src=da)
            da = dn
        for i in (2, 1, 0):
            la, lb = self.convs[i]
            a, ya, yb, (mean, rstd, k) = tp['blocks'][i]
            dzb = c.act('e_dzb%d' % i + tag, B, Ts[i + 1], c2)
            instnorm_bwd(c, da, yb, mean, rstd, dzb, ns, stream_id=k + 1, mask=masks[k], **drop)
            if pg:
                lb.wgrad(dzb, ya)
            gp = c.act('e_gp%d' % i + tag, B, Ts[i] + 4, c2)
            lb.dgrad(dzb, Ts[i], gp)
            dza = c.act('e_dza%d' % i + tag, B, Ts[i], c2)
            grad_combine(c, gp, Ts[i], 2, 2, self.pad_mode, gp.ld, dza, ns, dact=ya)
            if pg:
                la.wgrad(dza, a)
            la.dgrad(dza, Ts[i], gp)
            dn = c.act('e_da%d' % i + tag, B, Ts[i], c2)
            grad_combine(c, gp, Ts[i], 2, 2, self.pad_mode, gp.ld, dn, ns, res_mode=L.ZS_RES_AVGPOOL2, res=da)
            da = dn
        y2, cat, xin = tp['y2'], tp['cat'], tp['xin']
        dz = c.act('e_dzy2' + tag, B, T, c2)
        mean, rstd, k = tp['st0']
        instnorm_bwd(c, da, y2, mean, rstd, dz, ns, stream_id=k + 1, mask=masks[k], **drop)
        dcat = c.act('e_dcat' + tag, B, T, self.ncat)
        if not pg:
            # every column: the bank's 7*c_h1 (through its data gradient) and the pass-through ones (the gradient w.r.t. the input)
            self.conv2.dgrad(dz, T, dcat, dact_src=cat, slope=ns)
            return dcat
        self.conv2.wgrad(dz, cat)
        # only the conv bank's 7*c_h1 columns are consumed: the pass-through columns of the concatenation are the gradient w.r.t.
        # the input spectrogram, which the reference computes and drops (utils.py:43-45) -- a third of this GEMM
        self.conv2.dgrad(dz, T, dcat, dact_src=cat, slope=ns, n_cols=7 * c1)
        self._bank = (dcat, xin)

    # ---- gradient w.r.t. the input spectrogram (the autolocker step, zs_amd.stage2.AutolockerStep) ----------------------------
    # The seven bank convolutions (k = 1..7, pads (k//2, k//2 - 1 + k%2)) are ONE 7-tap convolution over the input padded 3/3 with
    # the taps outside a kernel's own pad set to zero: every pad fits inside 3/3, and the inner rows of a reflect pad do not depend on
    # its width.  Their data gradient is then one transposed GEMM (K = 7 taps x 7*c_h1, 28 of the 49 tap blocks nonzero) into the
    # 3/3-padded domain, and one fold (zs_enc_dx_fold) that adds the padding rows back and the pass-through columns.
    BANK_PAD = 3

    def _bank_d_operands(self):
        """The transposed operand of the bank's 7-tap data gradient: rows = c_in (padded to 128), K = 7 slots x cp (cp = 7*c_h1
        padded to the K chunk); slot s of kernel i (k = i + 1) holds its tap j = s - 3 + k//2 in columns [s*cp + i*c_h1, +c_h1).
        One single-tap column block per (kernel, tap): no whole-parameter view, so `raw` pack jobs beside the layers' own."""
        c, c1 = self.ctx, self.c1
        ld, cp = self.bank_d_ld, self.bank_d_cp
        ops = []
        for i, l in enumerate(self.conv1s):
            k = l.k
            raw = [dict(dtype=c.dt, W=L.ptr(l.w, j), so=self.c_in * k, si=k, sj=1, Cout=c1, Cin=self.c_in, taps=1, transpose=1,
                        co_split2=0, inner_pad=c1, dst=L.ptr(self.bank_d), ldw=ld, n_rows=self.bank_d_rows, n_cols=c1, row_offset=0,
                        col_offset=(j + self.BANK_PAD - k // 2) * cp + i * c1) for j in range(k)]
            ops.append(weight_operand(l.w, c1, self.c_in, k, (self.c_in * k, k, 1), [], raw=raw))
        return ops

    def _bank_operand(self):
        if self.bank_d is None:
            c = self.ctx
            self.bank_d_cp = rup(7 * self.c1, c.kc)
            self.bank_d_ld = 7 * self.bank_d_cp
            self.bank_d_rows = rup(self.c_in, 128)
            self.bank_d = torch.zeros(self.bank_d_rows * self.bank_d_ld + 512, dtype=c.tdt, device=c.device)
            self.adam_plan = None                    # the optimizer's plan must re-pack this operand too
            with L.pack_batch(c.stream):
                pack_operands(c, self._bank_d_operands(), [])        # from now on pack() re-packs it with the other operands
        return self.bank_d

    def backward_input(self, dbits=None, dlogits=None, tape=None):
        """Gradient of a loss w.r.t. the encoder's INPUT spectrogram, for the tape of the latest forward (or of key `tape`):
        dbits (Act [B,T',E], w.r.t. enc_act) or dlogits (Act [B,T',n_lin], w.r.t. the pre-activation `enc`).  No weight gradient
        is computed and no gradient buffer of the encoder is written.  Returns dx fp32 [B, T, c_in], contiguous (the encoder's
        own buffer: valid until the next backward_input at this shape)."""
        if dbits is None and dlogits is None:
            raise ValueError('backward_input: dbits or dlogits')
        tp = self.tape if tape is None else self.tapes[tape]
        dcat = self.backward_main(dbits, dlogits, param_grads=False, tape=tape)
        c = self.ctx
        B, T, P = tp['B'], tp['T'], self.BANK_PAD
        W = self._bank_operand()
        if dcat.ld < self.bank_d_cp:          # the GEMM reads cp columns of every dcat row (K of one tap)
            raise L.ZsError('backward_input: concatenation rows of %d columns < K chunk %d' % (dcat.ld, self.bank_d_cp))
        g = c.act('e_gbank' + tp['tag'], B, T + 2 * P, self.c_in, dtype=torch.float32)
        L.call('zs_gemm_conv', 'ZsGemmConv', c.stream, dtype=c.dt, A=dcat.ptr(), lda=dcat.ld, a_batch_stride=T * dcat.ld, B=B, T_in=T,
               T_out=T + 2 * P, taps=7, stride=1, pad_left=0, pad_mode=L.ZS_PAD_ZERO, gather=1, cin_pad=self.bank_d_cp, W=L.ptr(W),
               ldw=self.bank_d_ld, N=self.c_in, n_pad=self.bank_d_rows, act=L.ZS_ACT_NONE, out=g.ptr(), ldc=g.ld,
               out_cols=g.ld, store_mode=L.ZS_STORE_ROWS, groups=1, out_f32=1)
        n = B * T * self.c_in
        dx = c.f32('e_dx' + tp['tag'], n)[:n].view(B, T, self.c_in)
        L.call('zs_enc_dx_fold', 'ZsEncDxFold', c.stream, dtype=c.dt, g=g.ptr(), ldg=g.ld, pass_through=dcat.ptr(7 * self.c1), ld_pass=dcat.ld, B=B, T=T, C=self.c_in, pad=P,
               pad_mode=self.pad_mode, dx=L.ptr(dx), ldx=self.c_in)
        return dx

    def backward_bank(self):
        dcat, xin = self._bank
        for i, l in enumerate(self.conv1s):
            l.wgrad(dcat.sub(i * self.c1, self.c1), xin)


class DecoderEngine(object):
    def __init__(self, ctx, P, G, c_in, c_out, c_h, c_a, ns, seg_len, output_mask=False):
        self.ctx = ctx
        self.uid = next_uid()
        self.E, self.F, self.ch, self.n_spk = c_in, c_out, c_h, c_a
        self.ns = float(ns)
        self.pad_mode = L.ZS_PAD_REFLECT if seg_len >= 64 else L.ZS_PAD_ZERO
        self.out_act = L.ZS_ACT_TANH if output_mask else L.ZS_ACT_SIGMOID
        if c_h % 32:
            raise ValueError('Decoder c_h must be a multiple of 32 (got %d)' % c_h)
        mk = functools.partial(ConvLayer.from_params, ctx, P, G, pad_mode=self.pad_mode)
        self.input_emb = mk('input_emb')
        self.convs = [(mk('conv%d' % a, split2=True), mk('conv%d' % b)) for a, b in ((1, 2), (3, 4), (5, 6))]
        self.dense = [(mk('dense%d' % a), mk('dense%d' % b)) for a, b in ((1, 2), (3, 4))]
        self.gru = GruLayer(ctx, P, G, 'RNN.', name='dec%d' % self.uid)
        self.dense5 = mk('dense5')                        # the literal cat[out, rnn, emb5 x T] GEMM (K = 3 c_h), model/model.py:357-358
        self.linear = mk('linear')
        self.emb = [P['emb%d.weight' % i] for i in range(1, 6)]
        self.gemb = [G['emb%d.weight' % i] for i in range(1, 6)]
        self.e_dense, self.e_rnn = 3, 4                   # emb4 feeds the dense blocks, emb5 the GRU input and append_emb
        self.layers = [self.input_emb] + [l for p in self.convs for l in p] + [l for p in self.dense for l in p] + \
            [self.dense5, self.linear]
        self.tape = None

    def operands(self):
        """(weights, vectors) of every layer: the one description of pack() and of the fused optimizer step's plan."""
        return operands_of(self.layers + [self.gru])

    def pack(self):
        with L.pack_batch(self.ctx.stream):
            pack_operands(self.ctx, *self.operands())

    def forward(self, bits, cidx, training, lengths=None):
        """bits: Act [B,T',E] (T dtype, zero padded); cidx int64 [B].  Returns x_dec Act fp32 [B, 8T', F].
        lengths: host int sequence [B], encoded frames per sample (ragged batch, inference only): sample b is computed as if it
        ran alone with T' = lengths[b]; its first 8 * lengths[b] output rows are valid."""
        c, ns, ch = self.ctx, self.ns, self.ch
        B, T0 = bits.B, bits.T
        Ls = [None] * 4
        if lengths is not None:
            l0 = ragged_lengths('DecoderEngine', lengths, training, B, T0, 2)        # reflect pad 1 of conv k3 needs 2 rows
            ld = torch.stack([l0, 2 * l0, 4 * l0, 8 * l0]).to(c.device, non_blocking=True)
            Ls = [ld[i] for i in range(4)]
        tag = '_%d_%d_%d' % (self.uid, B, T0)
        st = c.stream
        emb = self.emb
        tp = {'B': B, 'T0': T0, 'training': training, 'cidx': cidx, 'bits': bits, 'blocks': [], 'dense': []}
        x = c.act('d_x0' + tag, B, T0, ch)
        xe = c.act('d_xe0' + tag, B, T0, ch)
        self.input_emb.fwd(bits, out=x, out2=xe, vec2=emb[0], idx=cidx)                                   # :346, :319
        T = T0
        for i, (la, lb) in enumerate(self.convs):                                                        # :317-331
            ya = c.act('d_ya%d' % i + tag, B, T, 2 * ch) if training else None
            s = c.act('d_s%d' % i + tag, B, 2 * T, ch)
            la.fwd(xe, out=ya, act=LRELU, slope=ns, out2=s, vec2=emb[i], idx=cidx, store_mode2=L.ZS_STORE_SPLIT2, lengths=Ls[i])
            yb = c.act('d_yb%d' % i + tag, B, 2 * T, ch)
            lb.fwd(s, out=yb, act=LRELU, slope=ns, lengths=Ls[i + 1])
            xn = c.act('d_x%d' % (i + 1) + tag, B, 2 * T, ch)
            xen = c.act('d_xe%d' % (i + 1) + tag, B, 2 * T, ch)
            nxt = emb[i + 1] if i < 2 else emb[3]                                                        # emb2, emb3, then emb4 (:350)
            stt = _norm_stats(c, training, 'd_', '%d_c%d_%d_%d' % (self.uid, i, B, 2 * T), B * yb.ld)
            instnorm_fwd(c, yb, xn, *stt, self.pad_mode, res_mode=L.ZS_RES_UPSAMPLE2, res=x, lengths=Ls[i + 1], out2=xen, vec2=nxt,
                         idx=cidx)
            tp['blocks'].append((x, xe, ya, s, yb, stt, T))
            x, xe, T = xn, xen, 2 * T
        return self._fwd_dense(tp, x, xe, cidx, T, tag, B, training, Ls[3])

    def _fwd_dense(self, tp, x, xe, cidx, T, tag, B, training, lengths):
        """The two dense blocks, the GRU and the tail from x (and xe = x + emb[e_dense]) on; shared with PatcherEngine."""
        c, ns, ch, emb = self.ctx, self.ns, self.ch, self.emb
        ed, er = self.e_dense, self.e_rnn
        cat3 = c.act('d_cat3' + tag, B, T, 3 * ch)
        for j, (la, lb) in enumerate(self.dense):                                                        # :333-342, :350-351
            y1 = c.act('d_y1%d' % j + tag, B, T, ch)
            y1e = c.act('d_y1e%d' % j + tag, B, T, ch)
            la.fwd(xe, out=y1, act=LRELU, slope=ns, out2=y1e, vec2=emb[ed], idx=cidx)
            y2 = c.act('d_y2%d' % j + tag, B, T, ch)
            lb.fwd(y1e, out=y2, act=LRELU, slope=ns)
            xn = c.act('d_dx%d' % j + tag, B, T, ch) if j == 0 else Act(cat3.t, B, T, ch, cat3.ld, 0, ch)
            xen = c.act('d_dxe%d' % j + tag, B, T, ch)
            stt = _norm_stats(c, training, 'd_', '%d_d%d_%d_%d' % (self.uid, j, B, T), B * y2.ld)
            instnorm_fwd(c, y2, xn, *stt, self.pad_mode, res_mode=L.ZS_RES_IDENTITY, res=x, lengths=lengths, out2=xen,
                         vec2=(emb[ed] if j == 0 else emb[er]), idx=cidx)
            tp['dense'].append((x, xe, y1, y1e, y2, stt))
            x, xe = xn, xen
        H = ch // 2
        gi = c.act('d_gi' + tag, B, T, 6 * H)
        gates = c.raw('d_gates' + tag, B * T * 8 * H, c.tdt) if training else None
        # :352-356, and append_emb (:357) rides on the recurrence's stores (third block of cat3 = emb5[c_b] at every t)
        self.gru.fwd(xe, cat3, ch, gi, gates, bcast=(emb[er], cidx, 2 * ch), lengths=lengths)
        h5 = c.act('d_h5' + tag, B, T, ch)
        self.dense5.fwd(cat3, out=h5, act=LRELU, slope=ns)                                                # :358-359
        return self._fwd_tail(c, tp, h5, cat3, gates, xe, T, tag, B)

    def _fwd_tail(self, c, tp, h5, cat3, gates, xe, T, tag, B):
        xdec = c.act('d_xdec' + tag, B, T, self.F, dtype=torch.float32)
        self.linear.fwd(h5, out=xdec, act=self.out_act, out_f32=True)                                    # :360-364
        tp.update(cat3=cat3, gates=gates, gru_in=xe, h5=h5, T=T)
        self.tape = tp
        return xdec

    def backward(self, dlogit, need_dbits=True, param_grads=True):
        """dlogit: Act [B,T,F] gradient w.r.t. the pre-sigmoid output.  Fills (overwrites) every decoder parameter
        gradient.  Returns dbits Act [B,T',E].
        param_grads=False (voice adaptation, zs_amd.voice): the data-gradient chain alone -- the same launches on the main stream,
        which leave the per-sample embedding sums in self._embsum (slots 0..4: emb1..emb5, fp32 [B, c_h] each) -- without any
        weight-gradient launch, side stream or zs_emb_scatter: no gradient buffer is written."""
        self.backward_head(dlogit, param_grads)
        return self.backward_convs(need_dbits, param_grads)

    def backward_head(self, dlogit, param_grads=True):
        """linear, dense5, the GRU and the two dense blocks: the gradients of dense1 .. linear (a contiguous range of the flat
        gradient buffer) are final when this returns and the side streams have been joined -- data parallel training starts their
        all-reduce here, under the conv blocks' backward (trainer.AEStep)."""
        c, ns, ch, tp = self.ctx, self.ns, self.ch, self.tape
        assert tp is not None and tp['training']
        B, T0, T = tp['B'], tp['T0'], tp['T']
        tag = '_%d_%d_%d' % (self.uid, B, T0)
        cat3, h5 = tp['cat3'], tp['h5']
        H = ch // 2
        ed, er = self.e_dense, self.e_rnn
        self._embsum = c.f32('d_embsum' + tag, 6 * B * ch)      # slots 0..4: per-sample sums for emb1..emb5; 5: column sums of dz5
        self._embsum.zero_()
        if param_grads:
            self.linear.wgrad(dlogit, h5)
        dz5 = c.act('d_dz5' + tag, B, T, ch)
        # the embedding parts of the k = 1 data gradients (per-sample column sums) come out of the GEMM epilogues when whole
        # samples fit a tile (ZsGemmConv.colsum); otherwise a zs_grad_combine pass over the gradient computes them
        fuse = colsum_ok(T) and os.environ.get('ZS_FUSE_COLSUM', '1') == '1'
        esum = lambda k: L.ptr(self._embsum, k * B * ch)       # per-sample sums for embedding k (finished by zs_emb_scatter)
        slot = lambda k, col0=0: (esum(k), ch, col0)
        # append_emb's block of dense5 (model/model.py:357) multiplies a vector that is constant over time, so its input gradient
        # is only needed summed over t: sum_t (dz5[b,t] W5e) = (sum_t dz5[b,t]) W5e -- the column sums of dz5 (epilogue of the
        # GEMM that produces it) times the block, a B-row GEMM, instead of a third of dense5's data gradient
        thin5 = fuse and ch % 128 == 0 and os.environ.get('ZS_THIN_EMB5', '1') == '1'
        self.linear.dgrad(dlogit, T, dz5, dact_src=h5, slope=ns, colsum=(slot(5) if thin5 else None), colsum_post=True)
        if param_grads:
            self.dense5.wgrad(dz5, cat3)
        dcat3 = c.act('d_dcat3' + tag, B, T, 3 * ch)
        if thin5:
            self.dense5.dgrad(dz5, T, dcat3, n_cols=2 * ch)
            s32 = Act(self._embsum, B, 1, ch, ch, 5 * B * ch)
            sT = c.act('d_s5' + tag, B, 1, ch)
            cast_rows(c, s32.ptr(), ch, sT)
            slot4 = Act(self._embsum, B, 1, ch, ch, er * B * ch)
            self.dense5.dgrad(sT, 1, slot4, add_src=slot4, out_f32=True, add_f32=True, n_cols=ch, n_off=2 * ch)
        elif fuse:                                                                           # d emb5 via append_emb: the third
            self.dense5.dgrad(dz5, T, dcat3, colsum=slot(er, 2 * ch), out_cols=2 * ch)        # column block is summed, not stored
        else:
            self.dense5.dgrad(dz5, T, dcat3)
            grad_combine(c, dcat3.sub(2 * ch, ch), T, 0, 0, self.pad_mode, ch, None, ns, emb_sum=esum(er))
        dgi = c.act('d_dgi' + tag, B, T, 6 * H)
        dgh = c.act('d_dgh' + tag, B, T, 6 * H)
        gp = c.act('d_gpA' + tag, B, T + 2, ch)
        gpv = Act(gp.t, B, T, ch, gp.ld)
        dx = c.act('d_dxA' + tag, B, T, ch)
        if fuse:                                                                                     # out+emb5 (:353)
            self.gru.bwd(dcat3, ch, cat3, ch, tp['gates'], tp['gru_in'], dgi, dgh, dx, add_src=dcat3.sub(0, ch), colsum=slot(er),
                         param_grads=param_grads)
        else:
            self.gru.bwd(dcat3, ch, cat3, ch, tp['gates'], tp['gru_in'], dgi, dgh, gpv, param_grads=param_grads)
            grad_combine(c, gpv, T, 0, 0, self.pad_mode, ch, dx, ns, emb_sum=esum(er), res_mode=L.ZS_RES_IDENTITY, res=dcat3.sub(0, ch))
        for j in (1, 0):
            la, lb = self.dense[j]
            xin, xe, y1, y1e, y2, stt = tp['dense'][j]
            dz2 = c.act('d_dz2%d' % j + tag, B, T, ch)           # unique per block: read later by the side-stream wgrad
            instnorm_bwd(c, dx, y2, *stt, dz2, ns)
            if param_grads:
                lb.wgrad(dz2, y1e)
            dz1 = c.act('d_dz1%d' % j + tag, B, T, ch)
            if fuse:
                lb.dgrad(dz2, T, dz1, dact_src=y1, slope=ns, colsum=slot(ed))
            else:
                lb.dgrad(dz2, T, gpv)
                grad_combine(c, gpv, T, 0, 0, self.pad_mode, ch, dz1, ns, emb_sum=esum(ed), dact=y1)
            if param_grads:
                la.wgrad(dz1, xe)
            dn = c.act('d_dxD%d' % j + tag, B, T, ch)
            if fuse:
                la.dgrad(dz1, T, dn, add_src=dx, colsum=slot(ed))
            else:
                la.dgrad(dz1, T, gpv)
                grad_combine(c, gpv, T, 0, 0, self.pad_mode, ch, dn, ns, emb_sum=esum(ed), res_mode=L.ZS_RES_IDENTITY, res=dx)
            dx = dn
        self._bw = (dx, gp, tag)

    def backward_convs(self, need_dbits=True, param_grads=True):
        """The three conv blocks, the embeddings and input_emb.  Returns dbits.  param_grads: see backward()."""
        c, ns, ch, tp = self.ctx, self.ns, self.ch, self.tape
        dx, gp, tag = self._bw
        B, T0 = tp['B'], tp['T0']
        for i in (2, 1, 0):
            la, lb = self.convs[i]
            xin, xe, ya, s, yb, stt, Ti = tp['blocks'][i]
            esum = L.ptr(self._embsum, i * B * ch)                   # per-sample sums for emb_i+1
            T2 = 2 * Ti
            dzb = c.act('d_dzb%d' % i + tag, B, T2, ch)
            instnorm_bwd(c, dx, yb, *stt, dzb, ns)
            if param_grads:
                lb.wgrad(dzb, s)
            gp2 = Act(gp.t, B, T2 + 2, ch, gp.ld)
            lb.dgrad(dzb, T2, gp2)
            dza = c.act('d_dza%d' % i + tag, B, Ti, 2 * ch)
            grad_combine(c, gp2, T2, 1, 1, self.pad_mode, ch, dza, ns, emb_sum=esum, dact=ya, unshuffle=1)   # pixel_shuffle^T, +emb (:323-324)
            if param_grads:
                la.wgrad(dza, xe)
            gp1 = Act(gp.t, B, Ti + 2, ch, gp.ld)
            la.dgrad(dza, Ti, gp1)
            dn = c.act('d_dxC%d' % i + tag, B, Ti, ch)
            grad_combine(c, gp1, Ti, 1, 1, self.pad_mode, ch, dn, ns, emb_sum=esum, res_mode=L.ZS_RES_UPSAMPLE2,
                         res=dx)                                                                # x+emb (:319) and upsample(x) (:329)
            dx = dn
        # nn.Embedding backward, fixed sample order.  Only the optimizer needs these: off the main chain, side by side
        sts = fork_side(c.device) if (c.overlap_wgrad and param_grads) else None
        for k in (range(5) if param_grads else ()):
            st_k = sts[k % len(sts)].cuda_stream if sts is not None else c.stream
            L.call('zs_emb_scatter', 'ZsEmbScatter', st_k, emb_sum=L.ptr(self._embsum, k * B * ch), emb_ld=ch,
                   idx=L.ptr(tp['cidx']), B=B, demb=L.ptr(self.gemb[k]), demb_ld=ch, n_rows=self.n_spk, C=ch, accumulate=0)
        bits = tp['bits']
        if param_grads:
            self.input_emb.wgrad(dx, bits)
        dbits = None
        if need_dbits:
            dbits = c.act('d_dbits' + tag, B, T0, self.E)
            self.input_emb.dgrad(dx, T0, dbits)
        return dbits


class PatcherEngine(DecoderEngine):
    """Spectrogram_Patcher.forward (reference model/model.py:532-549) and its backward to the parameter gradients (stage 2 steps
    only the patcher: no gradient w.r.t. its input).  The decoder's two dense blocks, GRU and tail at the input's own time
    resolution, behind one K = c_in linear (input_layer, no activation) instead of the conv blocks; emb1 feeds all four dense
    layers, emb2 the GRU input and append_emb."""

    def __init__(self, ctx, P, G, c_in, c_out, c_h, c_a, ns):
        self.ctx = ctx
        self.uid = next_uid()
        self.E, self.F, self.ch, self.n_spk = c_in, c_out, c_h, c_a
        self.ns = float(ns)
        self.pad_mode = L.ZS_PAD_ZERO                     # every layer is a Linear: no time padding anywhere
        self.out_act = L.ZS_ACT_SIGMOID
        if c_h % 32:
            raise ValueError('Spectrogram_Patcher c_h must be a multiple of 32 (got %d)' % c_h)
        mk = functools.partial(ConvLayer.from_params, ctx, P, G, pad_mode=self.pad_mode)
        self.input_layer = mk('input_layer')
        self.dense = [(mk('dense%d' % a), mk('dense%d' % b)) for a, b in ((1, 2), (3, 4))]
        self.gru = GruLayer(ctx, P, G, 'RNN.', name='sp%d' % self.uid)
        self.dense5 = mk('dense5')
        self.linear = mk('linear')
        self.emb = [P['emb1.weight'], P['emb2.weight']]
        self.gemb = [G['emb1.weight'], G['emb2.weight']]
        self.e_dense, self.e_rnn = 0, 1
        self.layers = [self.input_layer] + [l for p in self.dense for l in p] + [self.dense5, self.linear]
        self.tape = None

    def forward(self, xd, cidx, training, lengths=None):
        """xd: Act fp32 [B, T, c_in] (a decoder's output rows, any ld >= c_in); cidx int64 [B].  Returns Act fp32 [B, T, c_out]
        (after the sigmoid).  lengths: host int sequence [B], frames per sample (ragged batch, inference only): sample b is computed
        as if it ran alone with T = lengths[b] (InstanceNorm statistics and the reverse GRU over its own frames); its first
        lengths[b] output rows are valid."""
        c, ch = self.ctx, self.ch
        B, T = xd.B, xd.T
        ln = None
        if lengths is not None:
            ln = ragged_lengths('PatcherEngine', lengths, training, B, T, 1).to(c.device, non_blocking=True)
        tag = '_%d_%d_%d' % (self.uid, B, T)
        xin = c.act('p_xin' + tag, B, T, self.E)
        cast_rows(c, xd.ptr(), xd.ld, xin)
        tp = {'B': B, 'T0': T, 'training': training, 'cidx': cidx, 'xin': xin, 'dense': []}
        x = c.act('d_x0' + tag, B, T, ch)
        xe = c.act('d_xe0' + tag, B, T, ch)
        self.input_layer.fwd(xin, out=x, out2=xe, vec2=self.emb[0], idx=cidx)                          # :537, + emb1 (:523)
        return self._fwd_dense(tp, x, xe, cidx, T, tag, B, training, ln)                                # :539-549

    def backward(self, dlogit, need_dbits=False):
        """dlogit: Act [B, T, c_out] gradient w.r.t. the pre-sigmoid output.  Fills (overwrites) every parameter gradient; weight
        gradients may still run on the side streams (join_side)."""
        if need_dbits:
            raise L.ZsError('PatcherEngine: the gradient w.r.t. the input spectrogram is not computed')
        self.backward_head(dlogit)
        dx, _, _ = self._bw
        c, tp, B, ch = self.ctx, self.tape, self.tape['B'], self.ch
        for k in range(2):                                 # nn.Embedding backward, fixed sample order
            L.call('zs_emb_scatter', 'ZsEmbScatter', c.stream, emb_sum=L.ptr(self._embsum, k * B * ch), emb_ld=ch, idx=L.ptr(tp['cidx']),
                   B=B, demb=L.ptr(self.gemb[k]), demb_ld=ch, n_rows=self.n_spk, C=ch, accumulate=0)
        self.input_layer.wgrad(dx, tp['xin'])
        return None


class ClassifierEngine(object):
    """SpeakerClassifier.forward (reference model/model.py:262-280) and its backward: four conv blocks on the
    T' = T/8 code sequence (conv k5/k3 + lrelu, InstanceNorm, Dropout, identity residual on blocks 2 and 3) and a
    final un-padded Conv1d whose kernel spans the whole sequence (k = seg_len/8) -> logits [B, n_class]."""

    def __init__(self, ctx, P, G, c_in, c_h, n_class, dp, ns, seg_len):
        self.ctx, self.uid = ctx, next_uid()
        self.c_in, self.c_h, self.n_class = c_in, c_h, n_class
        self.ns, self.dp = float(ns), float(dp)
        self.pad_mode = L.ZS_PAD_REFLECT if seg_len >= 64 else L.ZS_PAD_ZERO
        mk = functools.partial(ConvLayer.from_params, ctx, P, G, pad_mode=self.pad_mode)
        self.blocks = [(mk('conv1'), mk('conv2'), False), (mk('conv3'), mk('conv4'), True), (mk('conv5'), mk('conv6'), True),
                       (mk('conv7'), mk('conv8'), False)]
        self.conv9 = mk('conv9', padded=False)
        self.layers = [l for b in self.blocks for l in b[:2]] + [self.conv9]
        self.tape = None

    def operands(self):
        """(weights, vectors) of every layer: the one description of pack() and of the fused optimizer step's plan."""
        return operands_of(self.layers)

    def pack(self):
        with L.pack_batch(self.ctx.stream):
            pack_operands(self.ctx, *self.operands())

    def forward(self, x, training, seed=0, drop_masks=None):
        """x: Act [B, T', c_in] in the compute dtype.  Returns logits Act fp32 [B, 1, n_class]."""
        c, ns = self.ctx, self.ns
        B, T = x.B, x.T
        if T != self.conv9.k:
            raise L.ZsError('SpeakerClassifier expects %d encoded frames (got %d)' % (self.conv9.k, T))
        tag = '_%d_%d_%d' % (self.uid, B, T)
        dp = self.dp if training else 0.0
        masks = drop_masks if drop_masks is not None else [None] * 4
        tp = {'B': B, 'T': T, 'training': training, 'seed': seed, 'masks': masks, 'dp': dp, 'x': x, 'blocks': []}
        a = x
        for i, (la, lb, res) in enumerate(self.blocks):
            ya = c.act('c_ya%d' % i + tag, B, T, la.Cout)
            la.fwd(a, out=ya, act=LRELU, slope=ns)
            yb = c.act('c_yb%d' % i + tag, B, T, lb.Cout)
            lb.fwd(ya, out=yb, act=LRELU, slope=ns)
            out = c.act('c_o%d' % i + tag, B, T, lb.Cout)
            mean, rstd = _norm_stats(c, training, 'c_', '%d' % i + tag, B * yb.ld)
            instnorm_fwd(c, yb, out, mean, rstd, self.pad_mode, res_mode=(L.ZS_RES_IDENTITY if res else L.ZS_RES_NONE),
                         res=(a if res else None), p=dp, seed=seed, stream_id=20 + i, mask=masks[i])
            tp['blocks'].append((a, ya, yb, (mean, rstd, i), res))
            a = out
        logits = c.act('c_logits' + tag, B, 1, self.n_class, dtype=torch.float32)
        self.conv9.fwd(a, out=logits, out_f32=True)
        tp['last'] = a
        self.tape = tp
        return logits

    def backward(self, dlogits_f32, ld, need_dx=True, param_grads=True):
        """dlogits_f32: fp32 tensor [B, ld] (from zs_softmax_ce).  Returns dx Act [B, T', c_in] (or None)."""
        c, ns, tp = self.ctx, self.ns, self.tape
        B, T = tp['B'], tp['T']
        tag = '_%d_%d_%d' % (self.uid, B, T)
        dl = c.act('c_dl' + tag, B, 1, self.n_class)
        cast_rows(c, L.ptr(dlogits_f32), ld, dl)
        if param_grads:
            self.conv9.wgrad(dl, tp['last'])
        da = c.act('c_da_last' + tag, B, T, self.conv9.Cin)
        self.conv9.dgrad(dl, T, da)
        for i in (3, 2, 1, 0):
            la, lb, _ = self.blocks[i]
            a, ya, yb, stt, res = tp['blocks'][i]
            mean, rstd, k = stt
            dzb = c.act('c_dzb%d' % i + tag, B, T, lb.Cout)
            instnorm_bwd(c, da, yb, mean, rstd, dzb, ns, p=tp['dp'], seed=tp['seed'], stream_id=20 + k, mask=tp['masks'][k])
            if param_grads:
                lb.wgrad(dzb, ya)
            gp = c.act('c_gp%d' % i + tag, B, T + lb.pad_l + lb.pad_r, lb.Cin)
            lb.dgrad(dzb, T, gp)
            dza = c.act('c_dza%d' % i + tag, B, T, la.Cout)
            grad_combine(c, gp, T, lb.pad_l, lb.pad_r, self.pad_mode, gp.ld, dza, ns, dact=ya)
            if param_grads:
                la.wgrad(dza, a)
            if i == 0 and not need_dx:
                return None
            gp2 = c.act('c_gq%d' % i + tag, B, T + la.pad_l + la.pad_r, la.Cin)
            la.dgrad(dza, T, gp2)
            dn = c.act('c_da%d' % i + tag, B, T, la.Cin)
            grad_combine(c, gp2, T, la.pad_l, la.pad_r, self.pad_mode, gp2.ld, dn, ns, res_mode=(L.ZS_RES_IDENTITY if res else L.ZS_RES_NONE),
                         res=(da if res else None))
            da = dn
        return da
