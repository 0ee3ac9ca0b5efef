"""Stage 2 training steps (reference trainer.py:257-294, 467-560): the patchGAN discriminator / generator updates with the
WGAN-GP penalty and the optional target-guided reconstruction step (--train_p / --train_tgat).

One D step  (trainer.py:470-497):  loss = -beta_dis * mean(D(x_t) - D(x_gen)) + beta_clf * CE(D_clf(x_t), c_t - shift)
                                            + lambda * gp(D; x_t, x_gen);      clip(PatchDiscriminator), Adam(0.5, 0.9)
One G step  (trainer.py:514-533):  loss = beta_clf * CE(D_clf(x_gen), c_t - shift) - beta_gen * mean D(x_gen);
                                            clip(Generator), Adam
Target-guided (trainer.py:535-541): loss_rec = mean|gen_step(Encoder(x_t), c_t) - x_t|;  Adam WITHOUT clipping.
x_gen = gen_step(Encoder(x_s), c_t) = x_dec + x_dec * Generator(enc, c_t - shift)   ('targeted_residual', trainer.py:266-278),
                                     = x_dec + Generator(x_dec, c_t - shift)          ('spectrogram', trainer.py:283-284: the
                                       Spectrogram_Patcher post-filters the decoder's output; x_dec is a constant to it).

Only the network that the reference's optimizer steps receives gradients here: the reference lets autograd fill the
gradients of Encoder / Decoder (and of the discriminator in the G step) as well but never uses them (reset_grad is called on
the stepped net only and the other optimizers are not stepped in this mode), so they are not computed.
"""
import torch

from . import _lib as L
from . import layers, parallel
from .layers import join_side
from .optim import NetOpt, softmax_ce

G_MODES = ('naive', 'targeted', 'targeted_residual', 'spectrogram')


class PatchGANStep(object):
    def __init__(self, encoder, decoder, generator, discriminator, hps, g_mode, ema=None):
        self.Encoder, self.Decoder, self.Generator, self.D = encoder, decoder, generator, discriminator
        self.hps, self.g_mode = hps, g_mode
        if g_mode not in G_MODES:
            raise NotImplementedError('Invalid generator mode to call gen_step()!')
        self.shift = 0 if g_mode == 'naive' else int(hps.n_speakers - hps.n_target_speakers)
        self.device = encoder.flat_params()[0].device
        self.gen_opt = NetOpt(generator, hps.lr, ema=ema)                     # ema: a weight average of the generator and of the
        self.patch_opt = NetOpt(discriminator, hps.lr, ema=ema)              # critic, moved by their own Adam launches (NetOpt)
        dev = self.device
        self.loss_clf = torch.zeros(1, dtype=torch.float32, device=dev)
        self.correct = torch.zeros(1, dtype=torch.int32, device=dev)
        self.loss_rec = torch.zeros(1, dtype=torch.float32, device=dev)
        self._l1part = torch.zeros(1024, dtype=torch.float32, device=dev)
        self.step_no = 0

    def state_dict(self):
        """The training state beside the weights: the two optimizers (an AutolockerStep built from a PatchGANStep shares them:
        one step object, one state) and step_no, the counter the encoder's seeds derive from."""
        return {'gen': self.gen_opt.state_dict(), 'patch': self.patch_opt.state_dict(), 'step_no': int(self.step_no)}

    def load_state_dict(self, sd):
        self.gen_opt.load_state_dict(sd['gen'])
        self.patch_opt.load_state_dict(sd['patch'])
        self.step_no = int(sd['step_no'])

    def check_targets(self, c_host):
        """c_host: speaker indices of a target batch, still on the HOST.  Raises like the reference's Generator embedding would
        for a speaker outside the target range (an index outside the table would read past it on the GPU)."""
        lo, hi = self.shift, self.shift + int(self.Generator.c_a)
        if c_host.numel() and (int(c_host.min()) < lo or int(c_host.max()) >= hi):
            raise RuntimeError('This generator can only convert to target speakers!')

    # ---- gen_step (trainer.py:266-278) ---------------------------------------------------------------------------------------
    def gen_forward(self, x_btf, c, train_generator, noise=None, noise_kind=2, drop_masks=None, seed=None, x_dec=None):
        """x_btf fp32 [B, T, F] (source batch), c int64 [B] target speakers -> x_gen fp32 [B, T_out, F] contiguous.
        x_dec ('spectrogram' only): fp32 [B, T, F], a decoder output to post-filter in place of Decoder(Encoder(x_btf), c) (x_btf
        is then unused): the patcher sees nothing else."""
        enc, dec, gen = self.Encoder, self.Decoder, self.Generator
        enc.train(); dec.train(); gen.train()
        ge = gen._engine()
        ctx = ge.ctx
        # c - shift_c (trainer.py:277-279).  The range of c is checked where the batch is still on the host (check_targets(),
        # called once per host batch by the training loop / DevicePrefetcher): no device-to-host sync per step here
        cg = (c - self.shift) if self.shift else c
        if x_dec is not None:
            if self.g_mode != 'spectrogram':
                raise ValueError("gen_forward(x_dec=...) post-filters a given spectrogram: g_mode 'spectrogram' only")
            B, T, F = x_dec.shape
            xsrc = x_dec.contiguous()
            xd = ge.ctx.act('s2_xdin_%d_%d' % (B, T), B, T, F, dtype=torch.float32)
            layers.cast_rows(ge.ctx, L.ptr(xsrc), F, xd, dst_f32=True)
        else:
            ee, de = enc._engine(), dec._engine()
            ctx = de.ctx
            if seed is None:
                self.step_no += 1
                seed = (self.step_no * 0x9E3779B97F4A7C15 + 12345) % (1 << 62) + 7 * parallel.rank()
            bits, self._enc_f32, _ = ee.forward(x_btf, True, noise=noise, noise_kind=noise_kind, seed=seed, drop_masks=drop_masks)  # encode_step
            xd = de.forward(bits, c, False)                                   # Decoder(enc, c)
        if self.g_mode == 'spectrogram':
            m = ge.forward(xd, cg.contiguous(), train_generator)              # Generator(x_dec, c - shift_c) (trainer.py:283)
        else:
            m = ge.forward(bits, cg.contiguous(), train_generator)            # Generator(enc, c - shift_c)
        B, T, F = xd.B, xd.T, xd.C
        st = ctx.stream
        x_gen = ctx.f32('s2_xgen_%d_%d' % (B, T), B * T * F)[:B * T * F].view(B, T, F)
        L.check(L.lib().zs_gen_combine_fwd(xd.ptr(), m.ptr(), xd.ld, L.ptr(x_gen), B * T, F, int(self.g_mode == 'targeted_residual'), st),
                'zs_gen_combine_fwd')
        self._xd, self._m = xd, m
        return x_gen

    def _gen_backward(self, dx_gen):
        """dx_gen fp32 [B, T, F] contiguous -> Generator parameter gradients (x_dec is a constant here)."""
        ge = self.Generator._engine()
        xd, m = self._xd, self._m
        B, T, F = dx_gen.shape
        dpre = ge.ctx.act('s2_dpre_%d_%d' % (B, T), B, T, F)
        L.call('zs_gen_combine_bwd', 'ZsGenCombineBwd', ge.ctx.stream, dtype=ge.ctx.dt, dx_gen=L.ptr(dx_gen), ld_dx=F, xd=xd.ptr(), m=m.ptr(),
               ld_in=m.ld, dpre=dpre.ptr(), ldo=dpre.ld, fill_cols=dpre.ld, rows=B * T, F=F, mode=int(self.g_mode == 'targeted_residual'),
               tanh_out=int(getattr(self.Generator, 'output_mask', False)))
        ge.backward(dpre, need_dbits=False)
        join_side(self.device)

    def _ce(self, logits, c, grad_scale):
        """CE(logits, c - shift) (trainer.py:297-304, shift=True) -> dlogits fp32 [B, n_class] * grad_scale; loss / #correct on device."""
        tgt = ((c - self.shift) if self.shift else c).contiguous()
        return softmax_ce(self.D._engine().ctx, logits, tgt, self.loss_clf, self.correct, grad_scale)

    # ---- D step -----------------------------------------------------------------------------------------------------------------
    def d_step(self, x_s, x_t, c_t, alpha=None, masks=None, update=True, x_gen=None, **gen_kw):
        """x_s / x_t: fp32 [B, T, F] source / target batches, c_t int64 [B].  masks: optional [real, fake, interpolate] lists of six
        [B, C] Dropout2d keep masks; alpha: optional fp32 [B] interpolation weights (utils.py:59).  Returns device scalars."""
        hps, D = self.hps, self.D
        D.train()
        eng = D._engine()
        B = x_t.shape[0]
        if x_gen is None:
            x_gen = self.gen_forward(x_s, c_t, False, **gen_kw)
        mk = masks if masks is not None else [None, None, None]
        eng.zero_grads()
        val_r, logits_r = eng.forward(x_t.contiguous(), 'real', True, masks=mk[0], classify=True)
        dl = self._ce(logits_r, c_t, hps.beta_clf)                             # loss_clf on the REAL logits (trainer.py:491)
        eng.backward('real', dval=torch.full((B,), -float(hps.beta_dis) / B, device=self.device), dlogits=dl)
        val_f, _ = eng.forward(x_gen, 'fake', True, masks=mk[1], classify=False)
        eng.backward('fake', dval=torch.full((B,), float(hps.beta_dis) / B, device=self.device))
        w_dis = (val_r - val_f).mean()                                         # trainer.py:261 (B scalars: host-side glue)
        if alpha is None:
            alpha = torch.rand(B, device=self.device)
        n = x_t[0].numel()
        xi = eng.ctx.f32('s2_xi_%d' % B, B * n)[:B * n].view(x_t.shape)
        st = eng.ctx.stream
        L.check(L.lib().zs_lerp_rows(L.ptr(x_t.contiguous()), L.ptr(x_gen), L.ptr(alpha.float().contiguous()), L.ptr(xi), B, n, st), 'zs_lerp_rows')
        eng.forward(xi, 'inter', True, masks=mk[2], classify=False)
        gp = eng.gp_backward('inter', float(hps.lambda_))
        eng.flush_grads()
        if update:
            self.patch_opt.step(hps.max_grad_norm)
        return {'w_dis': w_dis, 'gp': gp[:1], 'real_loss_clf': self.loss_clf, 'correct': self.correct, 'real_logits': logits_r}

    # ---- G step -----------------------------------------------------------------------------------------------------------------
    def g_step(self, x_s, x_t, c_t, masks=None, update=True, x_gen=None, **gen_kw):
        hps, D = self.hps, self.D
        D.train()
        eng = D._engine()
        B = x_t.shape[0]
        have_tape = x_gen is None
        if x_gen is None:
            x_gen = self.gen_forward(x_s, c_t, True, **gen_kw)
        val_f, logits_f = eng.forward(x_gen, 'gfake', True, masks=masks, classify=True)
        dl = self._ce(logits_f, c_t, hps.beta_clf)
        loss_adv = -val_f.mean()
        dx = eng.backward('gfake', dval=torch.full((B,), -float(hps.beta_gen) / B, device=self.device), dlogits=dl, need_dx=True,
                          param_grads=False)
        if have_tape:
            self._gen_backward(dx)
            if update:
                self.gen_opt.step(hps.max_grad_norm)
        return {'loss_adv': loss_adv, 'fake_loss_clf': self.loss_clf, 'correct': self.correct, 'dx_gen': dx, 'fake_logits': logits_f}

    # ---- target-guided step (teacher forcing, trainer.py:535-541) -----------------------------------------------------------------
    def tg_step(self, x_t, c_t, update=True, **gen_kw):
        x_gen = self.gen_forward(x_t, c_t, True, **gen_kw)
        n = x_gen.numel()
        d = self.Generator._engine().ctx.f32('s2_dl1_%d' % n, n)[:n].view(x_gen.shape)
        st = torch.cuda.current_stream(self.device).cuda_stream
        L.check(L.lib().zs_l1_plain(L.ptr(x_gen), L.ptr(x_t.contiguous()), n, 1.0, L.ptr(self._l1part), L.ptr(self.loss_rec), L.ptr(d), st),
                'zs_l1_plain')
        self._gen_backward(d)
        if update:
            self.gen_opt.step(0.0)                                             # no grad_clip in the reference here
        return self.loss_rec


class AutolockerStep(PatchGANStep):
    """The autolocker mode of the reference (trainer.py:563-611): the generator is trained so that the encoder, run again on the
    converted spectrogram, gives back the source's discrete units.

    One step:  enc_act = Encoder(x_s);  x_gen = gen_step(enc_act, c_t);  re_enc = Encoder(x_gen)  (train mode, fresh noise);
               loss = BCELoss(re_enc, enc_act.detach());  clip(Generator, max_grad_norm);  Adam.  The target-guided half is tg_step.
    Only the generator is stepped, and only its gradients are computed: the encoder's backward is its input gradient alone
    (EncoderEngine.backward_input), the encoder's and decoder's parameter gradients are neither computed nor touched.
    multilabel_binary only: both enc_act and re_enc are then exactly 0 / 1, the loss is 100 * mismatches / N and its gradient
    +-1e12 / N at the mismatches (torch clamps the logs at -100 and the backward's denominator at 1e-12).  The other encoder modes
    give values that BCELoss rejects (one_hot / binary: 1 + ulp) or that are unbounded (continues)."""

    ENC_MODE = 'multilabel_binary'

    def __init__(self, encoder, decoder, generator, discriminator, hps, g_mode, ema=None):
        mode = getattr(encoder, 'enc_mode', None)
        if mode != self.ENC_MODE:
            raise ValueError("mode 'autolocker' needs enc_mode %r (BCE on the hard units), got %r" % (self.ENC_MODE, mode))
        super(AutolockerStep, self).__init__(encoder, decoder, generator, discriminator, hps, g_mode, ema=ema)
        self.loss_reenc = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._bce_part = torch.zeros(1024, dtype=torch.float64, device=self.device)

    def al_step(self, x_s, c_t, update=True, noise2=None, drop_masks2=None, seed2=None, **gen_kw):
        """x_s fp32 [B, T, F] source batch, c_t int64 [B] target speakers.  noise2 / drop_masks2 / seed2: the re-encode's Gumbel
        noise (same kind as gen_kw's noise_kind), Dropout keep masks and RNG seed (default: derived from the first encode's).
        Returns the re_enc loss (device scalar)."""
        ee = self.Encoder._engine()
        x_gen = self.gen_forward(x_s, c_t, True, **gen_kw)
        target = self._enc_f32
        if seed2 is None:
            seed = gen_kw.get('seed')
            seed = seed if seed is not None else (self.step_no * 0x9E3779B97F4A7C15 + 12345) % (1 << 62) + 7 * parallel.rank()
            seed2 = (seed * 0x2545F4914F6CDD1D + 0x632BE59BD9B4E019) % (1 << 62)
        _, re_enc, _ = ee.forward(x_gen, True, noise=noise2, noise_kind=gen_kw.get('noise_kind', 2), seed=seed2,
                                  drop_masks=drop_masks2, tape='al')
        tp = ee.tapes['al']
        c = ee.ctx
        B, T4, E = tp['B'], tp['T4'], ee.E
        if tuple(target.shape) != (B, T4, E):
            raise ValueError('al_step: the re-encode gives %s units, the first encode %s' % ((B, T4, E), tuple(target.shape)))
        dlog = c.act('e_dlog_al' + tp['tag'], B, T4, ee.n_lin)
        L.call('zs_bce_mbv_bwd', 'ZsBceMbvBwd', c.stream, dtype=c.dt, bits=L.ptr(tp['bits_f32']), y0=L.ptr(tp['y0']),
               target=L.ptr(target), rows=B * T4, E=E, tau=0.1, grad_scale=1.0, dlogits=dlog.ptr(), ld=dlog.ld, fill_cols=dlog.ld,
               partial=L.ptr(self._bce_part), loss_out=L.ptr(self.loss_reenc))
        dx = ee.backward_input(dlogits=dlog, tape='al')
        self._gen_backward(dx)
        self.last = {'x_gen': x_gen, 'enc_act': target, 're_enc': re_enc, 'dx_gen': dx}   # (inspection)
        if update:
            self.gen_opt.step(self.hps.max_grad_norm)
        return self.loss_reenc
