"""Drop-in Encoder / Decoder / SpeakerClassifier / Spectrogram_Patcher modules (reference: model/model.py:231-549).

Same constructor arguments, same parameter names and shapes (so reference checkpoints load with
load_state_dict), same forward signatures and return tuples in the reference's [B, C, T] layout.
The torch.nn layers created here are parameter CONTAINERS only (they give identical initialisation and
state_dict keys); their forward is never called -- all arithmetic runs in libzs_amd.so through
zs_amd.engine.  All parameters of a module live in one flat fp32 buffer (`flat`), their gradients in
`gflat` (one RCCL all-reduce / one fused Adam launch per net).
"""
import os

import torch
import torch.nn as nn

from . import _lib as L
from .engine import ClassifierEngine, DecoderEngine, EncoderEngine, PatcherEngine, linear_width
from .layers import Act, Ctx, cast_rows, rup


def default_dtype():
    return os.environ.get('ZS_DTYPE', 'fp32')


class ZsModule(nn.Module):
    """Flat-parameter storage + lazy engine construction."""

    def __init__(self, dtype=None):
        super(ZsModule, self).__init__()
        self._zs_dtype = dtype or default_dtype()
        self._zs = {'flat': None, 'gflat': None, 'engine': None, 'ctx': None, 'version': None, 'offsets': None}

    # -- flat storage --------------------------------------------------------------------------
    def _flatten(self):
        params = list(self.named_parameters())
        if not params:
            return
        dev = params[0][1].device
        offs, n = {}, 0
        for name, p in params:
            offs[name] = n
            n += rup(p.numel(), 4)
        flat = torch.zeros(n, dtype=torch.float32, device=dev)
        gflat = torch.zeros(n, dtype=torch.float32, device=dev)
        for name, p in params:
            o = offs[name]
            flat[o:o + p.numel()].copy_(p.data.reshape(-1).float())
            p.data = flat[o:o + p.numel()].view(p.shape)
            p.grad = gflat[o:o + p.numel()].view(p.shape)
        self._zs.update(flat=flat, gflat=gflat, offsets=offs, engine=None, ctx=None, version=None)

    def _apply(self, fn, *a, **kw):
        out = super(ZsModule, self)._apply(fn, *a, **kw)
        self._flatten()
        return out

    def flat_params(self):
        if self._zs['flat'] is None:
            self._flatten()
        return self._zs['flat'], self._zs['gflat']

    def grad_view(self, name):
        o = self._zs['offsets'][name]
        p = dict(self.named_parameters())[name]
        return self._zs['gflat'][o:o + p.numel()].view(p.shape)

    def flat_range(self, first, last):
        """(lo, hi) element range of the flat parameter / gradient buffers that holds the parameters `first` .. `last`
        (registration order), e.g. a gradient bucket of the data-parallel all-reduce."""
        if self._zs['flat'] is None:
            self._flatten()
        offs = self._zs['offsets']
        p = dict(self.named_parameters())[last]
        lo, hi = offs[first], offs[last] + rup(p.numel(), 4)
        if lo >= hi:
            raise ValueError('flat_range: %s does not precede %s' % (first, last))
        return lo, hi

    def mark_dirty(self):
        self._zs['version'] = None

    def repack(self):
        """Re-pack the GEMM operands from the fp32 master weights now (stream-ordered) and mark them current."""
        z = self._zs
        if z['engine'] is None:
            self._engine()
        else:
            z['engine'].pack()
            self.mark_packed()

    def mark_packed(self):
        """The GEMM operands hold the current master weights (re-packed on the device, stream-ordered)."""
        self._zs['version'] = sum(p._version for p in self.parameters())

    def adam_pack_plan(self):
        """The plan of the fused optimizer step (optim.AdamPackPlan) over this net's flat buffer and its engine's operands, or None
        for an engine that does not describe its operands.  Built once per engine (an engine is rebuilt after a move to another
        device or dtype) and again when the engine gains an operand; the operands have been packed in full by then."""
        eng = self._engine()
        if not hasattr(eng, 'operands'):
            return None
        if getattr(eng, 'adam_plan', None) is None:
            from .optim import AdamPackPlan
            eng.adam_plan = AdamPackPlan(self._zs['flat'], eng.ctx, *eng.operands())
        return eng.adam_plan

    def adam_pack_jobs(self, dtype=None):
        """The job list of that plan from parameter shapes alone (no GPU: the layers are laid out on the meta device):
        optim.plan_jobs' (jobs, rest_weights, rest_vectors), already checked to cover the flat buffer exactly once."""
        from .layers import PlanCtx
        from .optim import plan_jobs
        flat, gflat = self.flat_params()
        P = {k: p.data for k, p in self.named_parameters()}
        G = {k: self.grad_view(k) for k, _ in self.named_parameters()}
        eng = self._make_engine(PlanCtx(dtype or self._zs_dtype), P, G)
        return plan_jobs(flat, *eng.operands())

    def set_compute_dtype(self, dtype):
        if dtype != self._zs_dtype:
            self._zs_dtype = dtype
            self._zs.update(engine=None, ctx=None, version=None)

    # -- engine --------------------------------------------------------------------------------
    def _engine(self):
        z = self._zs
        if z['flat'] is None:
            self._flatten()
        if z['engine'] is None:
            dev = z['flat'].device
            if dev.type != 'cuda':
                raise L.ZsError('zs_amd modules compute on an MI355X only: move the module to a cuda device '
                                '(there is no CPU fallback path)')
            z['ctx'] = Ctx(dev, self._zs_dtype)
            P = {k: p.data for k, p in self.named_parameters()}
            G = {k: self.grad_view(k) for k, _ in self.named_parameters()}
            z['engine'] = self._make_engine(z['ctx'], P, G)
            z['version'] = None
        ver = sum(p._version for p in self.parameters())
        if z['version'] != ver:
            z['engine'].pack()
            z['version'] = ver
        return z['engine']

    def load_state_dict(self, *a, **kw):
        out = super(ZsModule, self).load_state_dict(*a, **kw)
        self.mark_dirty()
        return out


ENC_MODES = ('multilabel_binary', 'one_hot', 'binary', 'continues')


class Encoder(ZsModule):
    """model/model.py:368-489.  enc_mode 'multilabel_binary' (zs_mbv_fwd), 'one_hot', 'binary' (zs_gumbel_st_fwd, Gumbel-softmax
    straight-through) or 'continues' (leaky_relu); 'gumbel_t' is not built."""

    def __init__(self, c_in=513, c_h1=128, c_h2=512, c_h3=128, ns=0.2, dp=0.5, enc_size=512, seg_len=64,
                 enc_mode='continues', dtype=None):
        super(Encoder, self).__init__(dtype)
        self.ns, self.dp, self.enc_size, self.seg_len, self.enc_mode = ns, dp, enc_size, seg_len, enc_mode
        self.c_in, self.c_h1, self.c_h2, self.c_h3 = c_in, c_h1, c_h2, c_h3
        if enc_mode not in ENC_MODES:
            if enc_mode == 'gumbel_t':
                raise NotImplementedError("enc_mode 'gumbel_t' (softmax over time) is not built: use one of %s" % ', '.join(ENC_MODES))
            raise NotImplementedError('Invalid encoding mode!')
        if enc_mode in ('one_hot', 'continues'):
            assert enc_size % 2 == 0                                                              # model/model.py:396
        if enc_mode == 'binary' and enc_size > 64:
            raise ValueError("enc_mode 'binary' supports enc_size <= 64 (its linear layer has enc_size^2 = %d outputs)" % enc_size ** 2)
        if enc_mode == 'one_hot' and enc_size > 1024:
            raise ValueError("enc_mode 'one_hot' supports enc_size <= 1024 (got %d)" % enc_size)
        self.n_lin = linear_width(enc_mode, enc_size)
        self.conv1s = nn.ModuleList([nn.Conv1d(c_in, c_h1, kernel_size=k) for k in range(1, 8)])
        self.conv2 = nn.Conv1d(len(self.conv1s) * c_h1 + c_in, c_h2, kernel_size=1)
        self.conv3 = nn.Conv1d(c_h2, c_h2, kernel_size=5)
        self.conv4 = nn.Conv1d(c_h2, c_h2, kernel_size=5, stride=2)
        self.conv5 = nn.Conv1d(c_h2, c_h2, kernel_size=5)
        self.conv6 = nn.Conv1d(c_h2, c_h2, kernel_size=5, stride=2)
        self.conv7 = nn.Conv1d(c_h2, c_h2, kernel_size=5)
        self.conv8 = nn.Conv1d(c_h2, c_h2, kernel_size=5, stride=2)
        self.dense1 = nn.Linear(c_h2, c_h2)
        self.dense2 = nn.Linear(c_h2, c_h2)
        self.dense3 = nn.Linear(c_h2, c_h2)
        self.dense4 = nn.Linear(c_h2, c_h2)
        self.RNN = nn.GRU(input_size=c_h2, hidden_size=c_h3, num_layers=1, bidirectional=True)
        self.linear = nn.Linear(c_h2 + 2 * c_h3, self.n_lin)

    def _make_engine(self, ctx, P, G):
        return EncoderEngine(ctx, P, G, self.c_in, self.c_h1, self.c_h2, self.c_h3, self.enc_size, self.ns, self.dp, self.seg_len,
                             enc_mode=self.enc_mode)

    def noise_shape(self, B, T4):
        """Shape of the U / G this mode draws for B samples of T4 encoded frames (the reference's torch.rand shape), or None."""
        E = self.enc_size
        return {'multilabel_binary': (B, T4, E, 2), 'one_hot': (B, T4, E), 'binary': (B, T4, E, E)}.get(self.enc_mode)

    def check_noise(self, x, U=None, G=None):
        """ValueError (before any launch) if U / G does not fit this mode's noise for input x [B, c_in, T]."""
        noise = G if G is not None else U
        if noise is None or self.enc_mode == 'multilabel_binary':
            return
        B, T = x.shape[0], x.shape[2]
        want = self.noise_shape(B, (((T + 1) // 2 + 1) // 2 + 1) // 2)
        if want is None:
            raise ValueError("enc_mode %r draws no noise: U / G must be None" % self.enc_mode)
        if tuple(noise.shape) != want:
            raise ValueError('enc_mode %r: %s must have shape %s, got %s' % (self.enc_mode, 'G' if G is not None else 'U', want,
                                                                             tuple(noise.shape)))

    def forward(self, x, U=None, G=None, drop_masks=None, seed=None, lengths=None):
        """x [B, c_in, T] -> (enc_act [B, E, T/8], enc [B, n_lin, T/8]), n_lin = 2E (multilabel_binary), E (one_hot, continues)
        or E^2 (binary).  The Gumbel-softmax draws noise in eval mode too (reference behaviour, model/model.py:95-98): pass U
        (uniform) or G (Gumbel), shaped [B, T/8, E, 2] / [B, T/8, E] / [B, T/8, E, E] by mode, to make it reproducible;
        otherwise a counter-hash stream seeded from torch's RNG is used.  'continues' takes no noise.
        lengths (eval only): frames per sample of a ragged batch padded to T -- every sample is computed exactly as if it were
        forwarded alone with its own length (the reference forwards such fragments one at a time, convert.py:154-165); the
        first ceil(lengths[b] / 8) output frames of sample b are valid."""
        self.check_noise(x, U=U, G=G)
        eng = self._engine()
        xb = x.detach().permute(0, 2, 1).contiguous().float()
        noise, kind = None, 2
        if G is not None:
            noise, kind = G.to(xb.device, torch.float32).contiguous(), 0
        elif U is not None:
            noise, kind = U.to(xb.device, torch.float32).contiguous(), 1
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        masks = None
        if drop_masks is not None:
            masks = [m.to(xb.device, torch.uint8).contiguous() if m is not None else None for m in drop_masks]
        bits, bits_f32, logits = eng.forward(xb, self.training, noise=noise, noise_kind=kind, seed=seed, drop_masks=masks, lengths=lengths)
        self._last_bits = bits
        enc_act = bits_f32.permute(0, 2, 1).clone()
        enc = logits.valid().permute(0, 2, 1).clone()
        return enc_act, enc


class Decoder(ZsModule):
    """model/model.py:283-365."""

    def __init__(self, c_in=512, c_out=513, c_h=512, c_a=8, ns=0.2, seg_len=64, output_mask=False, dtype=None):
        super(Decoder, self).__init__(dtype)
        self.output_mask, self.ns, self.seg_len = output_mask, ns, seg_len
        self.c_in, self.c_out, self.c_h, self.c_a = c_in, c_out, c_h, c_a
        self.conv1 = nn.Conv1d(c_h, 2 * c_h, kernel_size=3)
        self.conv2 = nn.Conv1d(c_h, c_h, kernel_size=3)
        self.conv3 = nn.Conv1d(c_h, 2 * c_h, kernel_size=3)
        self.conv4 = nn.Conv1d(c_h, c_h, kernel_size=3)
        self.conv5 = nn.Conv1d(c_h, 2 * c_h, kernel_size=3)
        self.conv6 = nn.Conv1d(c_h, c_h, kernel_size=3)
        self.dense1 = nn.Linear(c_h, c_h)
        self.dense2 = nn.Linear(c_h, c_h)
        self.dense3 = nn.Linear(c_h, c_h)
        self.dense4 = nn.Linear(c_h, c_h)
        self.RNN = nn.GRU(input_size=c_h, hidden_size=c_h // 2, num_layers=1, bidirectional=True)
        self.dense5 = nn.Linear(2 * c_h + c_h, c_h)
        self.linear = nn.Linear(c_h, c_out)
        self.input_emb = nn.Linear(c_in, c_h)
        self.emb1 = nn.Embedding(c_a, c_h)
        self.emb2 = nn.Embedding(c_a, c_h)
        self.emb3 = nn.Embedding(c_a, c_h)
        self.emb4 = nn.Embedding(c_a, c_h)
        self.emb5 = nn.Embedding(c_a, c_h)

    def _make_engine(self, ctx, P, G):
        return DecoderEngine(ctx, P, G, self.c_in, self.c_out, self.c_h, self.c_a, self.ns, self.seg_len, self.output_mask)

    def emb_grad_views(self):
        return [self.grad_view('emb%d.weight' % i) for i in range(1, 6)]

    def forward(self, x, c, lengths=None):
        """x: enc_act [B, c_in, T'] (fp32);  c: int64 [B]  ->  [B, c_out, 8T'].
        lengths (eval only): encoded frames per sample of a ragged batch; the first 8 * lengths[b] output frames are valid."""
        _, xdec = self.forward_rows(x, c, lengths=lengths)
        return xdec.valid().permute(0, 2, 1).clone()

    def _forward_operand(self, B, T0, E, fill, c, dev, lengths):
        """The shared tail of forward_rows, forward_units and forward_indices: the engine's operand buffer [B, T0, E], filled by
        fill(ctx, bits) (what it returns is kept alive until the engine's launches are enqueued), the speaker index tensor and the
        engine.  Returns (bits, x_dec)."""
        eng = self._engine()
        ctx = eng.ctx
        bits = ctx.act('d_in_%d_%d_%d' % (eng.uid, B, T0), B, T0, E)
        keep = fill(ctx, bits)  # noqa: F841
        cidx = c.detach().to(dev, torch.int64).contiguous()
        return bits, eng.forward(bits, cidx, self.training, lengths=lengths)

    def forward_rows(self, x, c, lengths=None):
        """forward() without the copy out: (bits, x_dec), the input as the engine reads it (Act [B, T', c_in], compute dtype) and
        the output rows (Act fp32 [B, 8T', c_out]).  Both live in the engine's buffers, which the next forward of the same shape
        overwrites."""
        B, E, T0 = x.shape

        def fill(ctx, bits):
            xb = x.detach().permute(0, 2, 1).contiguous().float()
            cast_rows(ctx, L.ptr(xb), E, bits)
            return xb
        return self._forward_operand(B, T0, E, fill, c, x.device, lengths)

    def forward_units(self, packed, start, length, B, T0, c, lengths=None):
        """forward_rows() from bit-packed units (convert.pack_units): zs_units_unpack writes the chunk's operand [B, T0, c_in] from
        rows start[b] .. start[b] + length[b] of `packed` (uint8 [n_units, row_bytes] on the device; start int64 [B] and length
        int32 [B] device tables), zeros behind each fragment's rows.  The same buffer, and then the same launches, as forward_rows."""
        E = self.c_in
        if packed.dtype != torch.uint8 or packed.dim() != 2 or packed.shape[1] < (E + 7) // 8 or not packed.is_contiguous():
            raise ValueError('Decoder.forward_units: packed must be contiguous uint8 [n_units, >= %d]' % ((E + 7) // 8))

        def fill(ctx, bits):
            L.call('zs_units_unpack', 'ZsUnitsUnpack', ctx.stream, dtype=ctx.dt, packed=L.ptr(packed), n_units=packed.shape[0],
                   row_bytes=packed.shape[1], E=E, start=L.ptr(start), len=L.ptr(length), n_frag=B, T=T0, dst=bits.ptr(), ld_dst=bits.ld)
        return self._forward_operand(B, T0, E, fill, c, packed.device, lengths)

    def forward_indices(self, idx, code, start, length, B, T0, c, bad, lengths=None):
        """forward_rows() from codeword indices (zs_amd.vq): zs_vq_gather writes the chunk's operand [B, T0, c_in] from the codewords
        code[idx[start[b]] .. idx[start[b] + length[b] - 1]] (idx int32 [n_idx], code fp32 [K, c_in], start int64 [B], length int32
        [B], all on the device), zeros behind each fragment's rows; bad int32 [1] counts the indices outside [0, K).  The same
        buffer, and then the same launches, as forward_rows."""
        from .vq import launch_gather
        E = self.c_in
        if idx.dtype != torch.int32 or idx.dim() != 1 or not idx.is_contiguous():
            raise ValueError('Decoder.forward_indices: idx must be contiguous int32 [n_idx]')
        if code.dtype != torch.float32 or code.dim() != 2 or code.shape[1] != E or not code.is_contiguous():
            raise ValueError('Decoder.forward_indices: code must be contiguous fp32 [K, %d]' % E)

        def fill(ctx, bits):
            launch_gather(ctx.stream, ctx.dt, idx, code, start, length, B, T0, bits.ptr(), bits.ld, bad)
        return self._forward_operand(B, T0, E, fill, c, idx.device, lengths)

    def forward_index_planes(self, idx, s_use, code, start, length, B, T0, c, bad, lengths=None):
        """forward_indices() under a residual codebook (zs_amd.rvq): zs_rvq_gather writes the chunk's operand [B, T0, c_in] as the sum,
        in fp32 in increasing stage, of the first s_use stages' codewords (idx int32 [S, n_idx]: a plane per stage, rows a multiple of
        n_idx apart; code fp32 [S, K, c_in]); a frame with a used index outside [0, K) is a zero row, counted once in bad."""
        from .rvq import launch_gather
        E = self.c_in
        if idx.dtype != torch.int32 or idx.dim() != 2 or idx.stride(1) != 1 or (idx.shape[0] > 1 and idx.stride(0) < idx.shape[1]):
            raise ValueError('Decoder.forward_index_planes: idx must be int32 [S, n_idx] with unit column stride')
        if code.dtype != torch.float32 or code.dim() != 3 or code.shape[2] != E or code.shape[0] < int(s_use) or not code.is_contiguous():
            raise ValueError('Decoder.forward_index_planes: code must be contiguous fp32 [>= %d stages, K, %d]' % (int(s_use), E))

        def fill(ctx, bits):
            launch_gather(ctx.stream, ctx.dt, idx, s_use, code, start, length, B, T0, bits.ptr(), bits.ld, bad)
        return self._forward_operand(B, T0, E, fill, c, idx.device, lengths)


class Spectrogram_Patcher(ZsModule):
    """model/model.py:505-549: the stage-2 generator of g_mode 'spectrogram', a post-filter on the decoder's output spectrogram
    (trainer.py:283-284: x_gen = x_dec + G(x_dec, c - shift)).  ins_norm1 / ins_norm2 have no parameters (no affine); the
    engine runs them as the InstanceNorm kernel."""

    def __init__(self, c_in=512, c_out=513, c_h=512, c_a=8, ns=0.2, seg_len=64, dtype=None):
        super(Spectrogram_Patcher, self).__init__(dtype)
        self.ns, self.seg_len = ns, seg_len
        self.c_in, self.c_out, self.c_h, self.c_a = c_in, c_out, c_h, c_a
        self.input_layer = nn.Linear(c_in, c_h)
        self.dense1 = nn.Linear(c_h, c_h)
        self.dense2 = nn.Linear(c_h, c_h)
        self.dense3 = nn.Linear(c_h, c_h)
        self.dense4 = nn.Linear(c_h, c_h)
        self.RNN = nn.GRU(input_size=c_h, hidden_size=c_h // 2, num_layers=1, bidirectional=True)
        self.dense5 = nn.Linear(2 * c_h + c_h, c_h)
        self.linear = nn.Linear(c_h, c_out)
        self.emb1 = nn.Embedding(c_a, c_h)
        self.emb2 = nn.Embedding(c_a, c_h)

    def _make_engine(self, ctx, P, G):
        return PatcherEngine(ctx, P, G, self.c_in, self.c_out, self.c_h, self.c_a, self.ns)

    def forward(self, x, c, lengths=None):
        """x: spectrogram [B, c_in, T] (fp32);  c: int64 [B]  ->  [B, c_out, T] (after the sigmoid).
        lengths (eval only): frames per sample of a ragged batch padded to T; the first lengths[b] output frames are valid."""
        eng = self._engine()
        ctx = eng.ctx
        xb = x.detach().permute(0, 2, 1).contiguous().float()
        B, T, F = xb.shape
        if F != self.c_in:
            raise ValueError('Spectrogram_Patcher expects %d channels (got %d)' % (self.c_in, F))
        xa = Act(xb.reshape(-1), B, T, F, F)
        cidx = c.detach().to(xb.device, torch.int64).contiguous()
        out = eng.forward(xa, cidx, self.training, lengths=lengths)
        return out.valid().permute(0, 2, 1).clone()


class SpeakerClassifier(ZsModule):
    """model/model.py:231-280."""

    def __init__(self, c_in=512, c_h=512, n_class=8, dp=0.1, ns=0.01, seg_len=128, dtype=None):
        super(SpeakerClassifier, self).__init__(dtype)
        self.dp, self.ns, self.seg_len = dp, ns, seg_len
        self.c_in, self.c_h, self.n_class = c_in, c_h, n_class
        self.conv1 = nn.Conv1d(c_in, c_h, kernel_size=5)
        self.conv2 = nn.Conv1d(c_h, c_h, kernel_size=5)
        self.conv3 = nn.Conv1d(c_h, c_h, kernel_size=5)
        self.conv4 = nn.Conv1d(c_h, c_h, kernel_size=5)
        self.conv5 = nn.Conv1d(c_h, c_h, kernel_size=5)
        self.conv6 = nn.Conv1d(c_h, c_h, kernel_size=5)
        self.conv7 = nn.Conv1d(c_h, c_h // 2, kernel_size=3)
        self.conv8 = nn.Conv1d(c_h // 2, c_h // 4, kernel_size=3)
        if seg_len == 128:
            self.conv9 = nn.Conv1d(c_h // 4, n_class, kernel_size=16)
        elif seg_len == 64:
            self.conv9 = nn.Conv1d(c_h // 4, n_class, kernel_size=8)
        elif seg_len == 32:
            self.conv9 = nn.Conv1d(c_h // 4, n_class, kernel_size=4)
        else:
            raise NotImplementedError('Segement length {} is not supported!'.format(seg_len))

    def _make_engine(self, ctx, P, G):
        return ClassifierEngine(ctx, P, G, self.c_in, self.c_h, self.n_class, self.dp, self.ns, self.seg_len)

    def input_act(self, x_btc_f32):
        """fp32 [B, T', c_in] (contiguous, on the device) -> Act in the compute dtype."""
        eng = self._engine()
        ctx = eng.ctx
        B, T, C = x_btc_f32.shape
        a = ctx.act('c_in_%d_%d_%d' % (eng.uid, B, T), B, T, C)
        cast_rows(ctx, L.ptr(x_btc_f32), x_btc_f32.stride(1), a)
        return a

    def forward(self, x, drop_masks=None, seed=None):
        """x: enc [B, c_in, T'] -> logits [B, n_class]."""
        eng = self._engine()
        xb = x.detach().permute(0, 2, 1).contiguous().float()
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        masks = None
        if drop_masks is not None:
            masks = [m.to(xb.device, torch.uint8).contiguous() if m is not None else None for m in drop_masks]
        logits = eng.forward(self.input_act(xb), self.training, seed=seed, drop_masks=masks)
        return logits.valid()[:, 0, :].clone()
