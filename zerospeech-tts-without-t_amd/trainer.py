"""Trainer surface of the reference (trainer.py:34-347) for the stage-1 autoencoder path.

`Trainer(hps, data_loader, g_mode, enc_mode, log_dir)` builds Encoder / Decoder / Generator with the
reference's constructor wiring (trainer.py:48-98), `train(model_path, flag, mode='pretrain_AE')` runs the
`--train_ae` loop (trainer.py:320-347), `save_model` / `load_model` use the reference's checkpoint dict,
`test_step` / `encoder_test_step` are the inference entry points convert.py calls.

One training step (`ae_step`) is: Encoder fwd -> Decoder fwd -> L1 -> Decoder bwd -> [async RCCL
all-reduce of decoder grads] -> Encoder bwd -> [all-reduce encoder grads] -> per-net grad norm -> fused
clip + Adam(lr, betas=(0.5, 0.9)) on the flat parameter buffers.  Everything is enqueued on one HIP
stream without host synchronisation; the loss is read back only when it is logged.
"""
import functools
import os

import numpy as np
import torch

from . import _lib as L
from . import parallel
from . import layers
from . import resume as train_state                # (Trainer.train has a parameter called resume)
from . import validation
from .layers import Act, join_side
from .model import Decoder, Encoder, SpeakerClassifier, Spectrogram_Patcher
from .patch import PatchDiscriminator, TargetClassifier
from .optim import NetOpt, check_ema, softmax_ce
from .stage2 import AutolockerStep, PatchGANStep
from .utils import Logger

TCLF_CLASSES = 3                       # TargetClassifier(n_class=3): V001, V002, 'None' (trainer.py:97, convert.py:402-407)


class AEStep(object):
    """The fused --train_ae iteration (trainer.py:322-332) for one Encoder/Decoder pair:
    fwd, L1, bwd, gradient all-reduce, per-net clip (utils.py:53-55) and Adam(betas=(0.5,0.9)) over both nets
    (trainer.py:65-66).  All state lives on the device; nothing here synchronises with the host.

    The step is one ordered list of actions (plan) that three executors share: eager (_execute), capture (_capture) and replay
    (_execute of the captured plan).  Graph mode (ZS_GRAPH=1, default): after two eager warm-up steps the ~600 kernel launches of a
    step are captured into hipGraphs and replayed, so the host cost per step is a handful of calls instead of ~15 ms of
    Python/ctypes launches.  Everything that changes from step to step lives in device memory (RNG seed, Adam step count:
    zs_step_counters).  One rank: one graph.  More than one rank: one graph per run of launches between two host actions (forward +
    decoder tail backward | decoder conv blocks | encoder backward | conv bank weight gradients | decoder optimizer | encoder
    optimizer), with the RCCL all-reduces of the gradient buckets launched eagerly between them, each as soon as its bucket is
    final."""

    def __init__(self, encoder, decoder, lr=1e-4, betas=(0.5, 0.9), max_grad_norm=5.0, use_graph=None, ema=None, vq=None):
        """vq (not in the reference): None, or a vq_train.VqBottleneck (or an rvq_train.RvqBottleneck, which has its interface:
        DESIGN 34): the step then quantises the encoder's rows in front of the Decoder and hands the Decoder's input gradient through
        it; its loss_vq stays beside loss_rec, in vq.loss."""
        self.Encoder, self.Decoder = encoder, decoder
        self.vq = vq
        self.adam_step = 0                   # the pair's Adam step count (on the device: _step_dev)
        self.opt = {name: NetOpt(net, lr, betas, max_grad_norm, reduce=False, ema=ema)      # ema: a weight average per net (NetOpt)
                    for name, net in (('enc', encoder), ('dec', decoder))}
        dev = encoder.flat_params()[0].device
        self.device = dev
        self._loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self._lpart = torch.zeros(1024, dtype=torch.float32, device=dev)
        self._seed_dev = torch.zeros(1, dtype=torch.int64, device=dev)      # uint64 bits, advanced by zs_step_counters
        self._step_dev = torch.zeros(1, dtype=torch.int32, device=dev)      # Adam step count on the device
        self.reducer = parallel.GradReducer()
        self.xdec = None
        self.use_graph = (os.environ.get('ZS_GRAPH', '1') == '1') if use_graph is None else bool(use_graph)
        self._graphs = {}            # (B, T, F) -> dict(graphs=[...], plan=[...], x=static x, c=static c)
        self._statics = {}           # (B, T, F) -> (x, c) handed out by static_inputs()
        self._eager_calls = 0
        self.graph_warmup = 2        # eager steps (same launches) before the capture

    # ---- training state beside the weights --------------------------------------------------------------------------
    def state_dict(self):
        """Adam moments and counts of both nets, adam_step, the device words of the captured step, and which path ran: the
        captured step draws its dropout / Gumbel seeds from _seed_dev, the eager one from adam_step."""
        return {'enc': self.opt['enc'].state_dict(), 'dec': self.opt['dec'].state_dict(), 'adam_step': int(self.adam_step),
                'seed_dev': self._seed_dev, 'step_dev': self._step_dev, 'use_graph': bool(self.use_graph)}

    def load_state_dict(self, sd):
        """Restore state_dict() in place, after the weights were loaded.  Raises ValueError, before anything is changed, for a
        state saved on the other execution path."""
        if bool(sd['use_graph']) != bool(self.use_graph):
            raise ValueError('train state: use_graph is %r in the file, %r in this run (the captured and the eager step draw '
                             'different random streams)' % (bool(sd['use_graph']), bool(self.use_graph)))
        self.opt['enc'].load_state_dict(sd['enc'])
        self.opt['dec'].load_state_dict(sd['dec'])
        self.adam_step = int(sd['adam_step'])
        self._seed_dev.copy_(sd['seed_dev'].view(-1))
        self._step_dev.fill_(self.adam_step)
        if self._eager_calls:                                # a captured step never looks at the version: re-pack now
            self.Encoder.repack()
            self.Decoder.repack()

    # ---- the step as a plan ----------------------------------------------------------------------------------------
    def l1_loss(self, de, x_btf, xdec):
        """loss_rec = mean |x_dec - x| (trainer.py:328) into self._loss (partial sums in self._lpart), on the current stream; xdec
        (the decoder engine de's output) is kept as self.xdec.  Returns dlogit, the gradient w.r.t. the pre-sigmoid output."""
        B, T, F = x_btf.shape
        ctx = de.ctx
        dlogit = ctx.act('t_dlogit_%d_%d' % (B, T), B, xdec.T, F)
        L.call('zs_l1_loss', 'ZsL1Loss', ctx.stream, dtype=ctx.dt, x_dec=xdec.ptr(), ld_dec=xdec.ld, x=L.ptr(x_btf), ldx=F,
               rows=B * xdec.T, F=F, dlogits=dlogit.ptr(), ldg=dlogit.ld, fill_cols=dlogit.ld, partial=L.ptr(self._lpart),
               loss_out=L.ptr(self._loss), grad_scale=1.0)
        self.xdec = xdec
        return dlogit

    def plan(self, x_btf, c, multi, counted, noise=None, noise_kind=2, drop_masks=None, seed=None):
        """The step as an ordered list of actions: ('run', fn) = launches on the current stream, ('reduce', net name, lo, hi) =
        start the all-reduce of that range (a bucket) of the net's flat gradient buffer, ('wait', net name) = the current stream
        waits for that net's all-reduces.  multi: the data-parallel step (parallel.multi_rank()).  counted: the seed and the Adam
        step count come from device memory (zs_step_counters) and the per-net clip + Adam + re-pack are the plan's last 'run'
        actions, as a captured step needs them; otherwise the caller's seed and no update (step() runs the host-counted
        optimizer_step after the plan).

        Several ranks: buckets in backward order.  Decoder dense1 .. linear (50 MB) start under the decoder's conv blocks, the conv
        blocks + embeddings (120 MB) under the encoder's backward, the encoder without its conv bank (47 MB) under the bank's seven
        weight gradients, the bank (7 MB) last; every 'run' ends with the side streams joined, so its gradients are final.  The
        decoder's clip + Adam + re-pack run while the encoder's all-reduces are still in flight.
        One rank (counted): the decoder's gradients are final once its backward (main stream) and its weight gradients (side
        streams) are done, so with layers.MULTI_STREAM its clip + Adam + re-pack run on a third stream under the encoder's backward."""
        enc, dec = self.Encoder, self.Decoder
        dev = self.device
        vq = self.vq
        if vq is not None and multi:
            raise ValueError("AEStep: the vector-codebook bottleneck runs on one rank (its counts and sums would need an all-reduce)")
        if counted:
            seed = parallel.rank()
        seed_ptr = L.ptr(self._seed_dev) if counted else None
        st = {}

        def forward():
            """Encoder + Decoder forward and the L1 loss; returns dlogit."""
            if counted:
                L.check(L.lib().zs_step_counters(L.ptr(self._seed_dev), L.ptr(self._step_dev),
                                                 torch.cuda.current_stream(dev).cuda_stream), 'zs_step_counters')
            ee, de = enc._engine(), dec._engine()
            bits, _, _ = ee.forward(x_btf, True, noise=noise, noise_kind=noise_kind, seed=seed, drop_masks=drop_masks,
                                    seed_ptr=seed_ptr)
            if vq is not None:
                bits = vq.forward(bits, seed, seed_ptr)                                   # the Decoder reads the codewords
            return self.l1_loss(de, x_btf, de.forward(bits, c, True))

        def update(name):
            return 'run', lambda: self.opt[name].device_step(L.ptr(self._step_dev))

        if multi:
            ee, de = enc._engine(), dec._engine()

            def fwd_and_dec_head():
                de.backward_head(forward())
                join_side(dev)

            def dec_convs():
                st['dbits'] = de.backward_convs()
                join_side(dev)

            def enc_main():
                ee.backward_main(st['dbits'])
                join_side(dev)

            def enc_bank():
                ee.backward_bank()
                join_side(dev)

            acts = [('run', fwd_and_dec_head), ('reduce', 'dec') + dec.flat_range('dense1.weight', 'linear.bias'), ('run', dec_convs),
                    ('reduce', 'dec') + dec.flat_range('conv1.weight', 'conv6.bias'),
                    ('reduce', 'dec') + dec.flat_range('input_emb.weight', 'emb5.weight'),
                    ('run', enc_main), ('reduce', 'enc') + enc.flat_range('conv2.weight', 'linear.bias'),
                    ('run', enc_bank), ('reduce', 'enc') + enc.flat_range('conv1s.0.weight', 'conv1s.6.bias'), ('wait', 'dec')]
            return acts + ([update('dec'), ('wait', 'enc'), update('enc')] if counted else [('wait', 'enc')])

        def fwd_and_dec_bwd():
            dlogit = forward()
            st['dbits'] = dec._engine().backward(dlogit)                               # loss.backward(), trainer.py:330

        def dec_update_aside():
            os_ = layers.opt_stream(dev)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(dev))
            os_.wait_event(ev)
            for side in layers.side_events(dev):
                os_.wait_event(side)
            with torch.cuda.stream(os_):
                self.opt['dec'].device_step(L.ptr(self._step_dev))

        def enc_bwd():
            enc._engine().backward(st['dbits'] if vq is None else vq.backward(st['dbits']))
            join_side(dev)

        def join_dec_update():
            ev = torch.cuda.Event()
            ev.record(layers.opt_stream(dev))
            torch.cuda.current_stream(dev).wait_event(ev)

        if not counted:
            return [('run', fwd_and_dec_bwd), ('run', enc_bwd)]
        if layers.MULTI_STREAM:
            return [('run', fwd_and_dec_bwd), ('run', dec_update_aside), ('run', enc_bwd), update('enc'), ('run', join_dec_update)]
        return [('run', fwd_and_dec_bwd), ('run', enc_bwd), update('enc'), update('dec')]

    def _execute(self, acts, counted=False):
        """Run a plan eagerly (or replay a captured one): 'run' actions launch, the reduce / wait actions are issued from the host.
        counted: the plan carries its own Adam update, the one place where a counted step advances adam_step."""
        for a in acts:
            if a[0] == 'run':
                a[1]()
            elif a[0] == 'reduce':
                self.reducer.start(self.opt[a[1]].net.flat_params()[1][a[2]:a[3]], tag=a[1])
            else:
                self.reducer.finish(a[1])
        if counted:
            self.adam_step += 1

    def step(self, x_btf, c, noise=None, noise_kind=2, drop_masks=None, seed=None, update=True):
        """x_btf: fp32 [B, T, F] on the device (the loader's native layout), c: int64 [B].
        Returns the device scalar holding loss_rec."""
        enc, dec = self.Encoder, self.Decoder
        enc.train(); dec.train()
        if noise is None and drop_masks is None and seed is None and update and self.use_graph:
            return self._graph_step(x_btf, c)
        if seed is None:
            seed = (self.adam_step + 1) * 0x9E3779B97F4A7C15 % (1 << 63) + parallel.rank()
        self._execute(self.plan(x_btf, c, parallel.multi_rank(), False, noise, noise_kind, drop_masks, seed))
        if update:
            self.optimizer_step()
        return self._loss

    # ---- graph mode ------------------------------------------------------------------------------------------------
    def _warm_up_or_capture(self, x_btf, c, capture, prologue=None):
        """Before a shape's graphs exist: the first graph_warmup calls run the counted step eagerly on (x_btf, c) -- the launches
        of the captured step; every buffer allocated, every workspace grown -- and return None; after them, return capture().
        prologue: launches in front of an eager step (the ones capture() puts in front of the captured one, see _capture)."""
        if self._eager_calls < self.graph_warmup:
            self._eager_calls += 1
            if prologue is not None:
                prologue()
            self._execute(self.plan(x_btf, c, parallel.multi_rank(), True), counted=True)
            return None
        return capture()

    def _graph_step(self, x_btf, c):
        key = tuple(x_btf.shape)
        ent = self._graphs.get(key)
        if ent is None:
            ent = self._warm_up_or_capture(x_btf, c, lambda: self._capture(*(self._statics.get(key) or (x_btf.clone(), c.clone()))))
            if ent is None:
                return self._loss
            self._graphs[key] = ent
        if x_btf.data_ptr() != ent['x'].data_ptr():        # (a loader that fills static_inputs() directly skips these copies)
            ent['x'].copy_(x_btf, non_blocking=True)
        if c.data_ptr() != ent['c'].data_ptr():
            ent['c'].copy_(c, non_blocking=True)
        self._execute(ent['plan'], counted=True)
        return self._loss

    def static_inputs(self, B, T, F):
        """(x fp32 [B, T, F], c int64 [B]): the device buffers the captured step of this shape reads its batch from.  A loader that
        writes the next batch straight into them and passes them to step() saves the device-to-device copy of the batch (67 MB
        at B = 256) that step() otherwise makes in front of every replay.  Call before the first step of that shape."""
        key = (B, T, F)
        if key not in self._statics:
            if key in self._graphs:
                ent = self._graphs[key]
                self._statics[key] = (ent['x'], ent['c'])
            else:
                self._statics[key] = (torch.zeros(B, T, F, dtype=torch.float32, device=self.device),
                                      torch.zeros(B, dtype=torch.int64, device=self.device))
        return self._statics[key]

    def _capture(self, xs, cs, prefetch=(), prologue=None):
        """Capture the counted step on the static inputs xs, cs: each run of consecutive 'run' actions becomes one hipGraph, a host
        action ends it.  Returns the entry whose plan is the step with every graph as a 'run' of its replay.  prefetch: (src
        pinned, dst) pairs, the H2D copy of the NEXT batch, forked at the start of the first graph and joined at its end (one
        rank: the end of the step) -- it runs on its own stream beside the kernels of this step.  prologue: launches captured in
        front of the first graph's step on the step's own stream (PoolFedStep: the gather of THIS batch into xs, cs)."""
        graphs, plan = self._capture_plan(self.plan(xs, cs, parallel.multi_rank(), True), prefetch, prologue)
        return {'graphs': graphs, 'plan': plan, 'x': xs, 'c': cs}

    def _capture_plan(self, acts, prefetch=(), prologue=None):
        """Capture any plan (the step's, or ValidStep's forward-only one) as _capture describes; returns (graphs, captured plan)."""
        torch.cuda.synchronize(self.device)
        graphs, plan, runs = [], [], []
        pool = None

        def close():
            nonlocal pool
            if not runs:
                return
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool, capture_error_mode='thread_local'):   # other threads (RCCL watchdog) may call HIP
                fetched = self._fork_fetch(prefetch) if prefetch and not graphs else None
                if prologue is not None and not graphs:
                    prologue()
                for fn in runs:
                    fn()
                if fetched is not None:                            # the branch joins inside the graph it forked in
                    torch.cuda.current_stream(self.device).wait_event(fetched)
            pool = g.pool()
            graphs.append(g)
            plan.append(('run', g.replay))
            del runs[:]

        for a in acts:
            if a[0] == 'run':
                runs.append(a[1])
            else:
                close()
                plan.append(a)
        close()
        return graphs, plan

    def _fork_fetch(self, pairs):
        """Inside a capture: copy each pinned src to its device dst by zs_host_fetch kernel nodes (they read the pinned buffers over
        PCIe, zs_amd.h) on the copy stream, forked from the current stream here.  Returns the event that ends the branch.
        Measured with kernel traces: wherever the branch forks, the executor of this ROCm stack does not run it
        truly beside the chain (the 1.2 ms transfer costs 1.1-1.4 ms of step time); forking at the very start of the graph and
        joining at the very end is the cheapest placement."""
        main = torch.cuda.current_stream(self.device)
        cs_ = layers.copy_stream(self.device) if layers.MULTI_STREAM else main      # (one stream: layers.MULTI_STREAM)
        ev0 = torch.cuda.Event()
        ev0.record(main)
        cs_.wait_event(ev0)
        with torch.cuda.stream(cs_):
            for src, dst in pairs:
                L.check(L.lib().zs_host_fetch(L.ptr(src), L.ptr(dst), dst.numel() * dst.element_size(), 32, cs_.cuda_stream),
                        'zs_host_fetch')
            ev = torch.cuda.Event()
            ev.record(cs_)
        return ev

    def host_feeder(self, loader):
        """Iterator that runs one training step per `next()` on the batches of a HOST loader (`next(loader)` -> (c int64 [B],
        x fp32 [B, T, F]) CPU tensors, the reference's DataLoader contract): see HostFedStep."""
        return HostFedStep(self, loader)

    def pool_feeder(self, loader):
        """Iterator that runs one training step per `next()` on the batches of a pool.PoolLoader, gathered on the device at the
        head of the (captured) step: see PoolFedStep."""
        return PoolFedStep(self, loader)

    def grad_norms(self):
        """Squared per-net gradient norms as device scalars (Encoder, Decoder are clipped separately).  With more than one
        rank the gradient buffers hold the SUM over ranks after the reduce (the 1/world is applied inside zs_adam_clip):
        these are the squared norms of that sum, i.e. world^2 times those of the averaged gradient."""
        return [self.opt['enc'].sqnorm(), self.opt['dec'].sqnorm()]

    def optimizer_step(self):
        """grad_clip([Encoder, Decoder], max_grad_norm) + ae_opt.step()  (trainer.py:331-332)."""
        self.grad_norms()
        self.adam_step += 1
        self.opt['enc'].adam(self.adam_step)
        self.opt['dec'].adam(self.adam_step)
        self._step_dev.fill_(self.adam_step)


class ValidStep(object):
    """Held-out validation of an AEStep's Encoder / Decoder pair (validation.py): a forward-only plan beside AEStep.plan, run by
    the AEStep's own executors (eager, capture, replay).

    Batch m of the M-batch pass: Encoder forward with training=False on its own tape key ('valid': buffers of its own), its Gumbel
    noise from the counter-hash stream seeded VALID_SEED + m (a host constant of the plan; 'continues' draws none); Decoder
    forward with training=False (the decoder's buffers are shared with the training step, which rewrites every one of them before
    it reads it); zs_eval_accum into one device table.  The plan reads inputs of its own (the whole set lies in HBM: the training
    step's static inputs may already hold the prefetched next batch) and writes scalars of its own: it launches no
    zs_step_counters, touches none of _seed_dev, _step_dev, adam_step, _loss, _lpart, xdec, and draws nothing from torch's
    generators, so the training run computes bit for bit what it computes without validation.  run() ends with the one D2H copy
    of the table (under 20 KB), the only host synchronisation of a validation.  (The engines' forward also makes its tape the
    'latest forward' one that backward* default to; every training step forwards before it backpropagates, so none ever reads it.)  With graphs on, the first run() is eager (every
    buffer allocated) and the second captures the M-batch pass into one hipGraph that later ones replay."""

    def __init__(self, ae, vset, batches, n_speakers):
        self.ae, dev = ae, ae.device
        self.M, self.n_speakers = int(batches), int(n_speakers)
        self.x = vset.x[:self.M].to(dev, torch.float32).contiguous()          # [M, B, T, F]
        self.c = vset.c[:self.M].to(dev, torch.int64).contiguous()            # [M, B]
        if int(self.c.min()) < 0 or int(self.c.max()) >= self.n_speakers:    # (zs_eval_accum would skip them; the decoder's embedding lookup would not)
            raise ValueError('validation set: speaker id outside [0, %d)' % self.n_speakers)
        _, self.B, self.T, self.F = self.x.shape
        enc = ae.Encoder
        self.units = enc.enc_mode != 'continues'
        self.E = enc.enc_size if self.units else 0
        self.layout, total = validation.table_layout(self.n_speakers, self.E)
        self.table = torch.zeros(total, dtype=torch.int64, device=dev)
        self.work = torch.zeros(self.B * L.ZS_EVAL_PARTS, dtype=torch.float64, device=dev)
        self._captured = None
        self._runs = 0

    def _word(self, name):
        return L.ptr(self.table, self.layout[name][0])

    def _batch(self, m):
        ae = self.ae
        ee, de = ae.Encoder._engine(), ae.Decoder._engine()
        x, c = self.x[m], self.c[m]
        bits, bits_f32, _ = ee.forward(x, False, noise_kind=2, seed=validation.VALID_SEED + m, tape='valid')
        xdec = de.forward(bits, c, False)
        if xdec.T != self.T:
            raise ValueError('validation: the decoder returns %d frames for segments of %d' % (xdec.T, self.T))
        u = self.units
        L.call('zs_eval_accum', 'ZsEvalAccum', de.ctx.stream, x_dec=xdec.ptr(), ld_dec=xdec.ld, x=L.ptr(x), ldx=self.F, c=L.ptr(c),
               B=self.B, T=self.T, F=self.F, n_speakers=self.n_speakers, work=L.ptr(self.work), spk_sum=self._word('spk_sum'),
               spk_cnt=self._word('spk_cnt'), bad=self._word('bad'), bits_f32=L.ptr(bits_f32) if u else None,
               T4=bits_f32.shape[1], E=bits_f32.shape[2], ones=self._word('ones') if u else None,
               flips=self._word('flips') if u else None, rows=self._word('rows') if u else None, pairs=self._word('pairs') if u else None)

    def plan(self):
        return [('run', self.table.zero_)] + [('run', functools.partial(self._batch, m)) for m in range(self.M)]

    def run(self):
        """One validation on the current weights.  Returns validation.split_table's dict of host arrays."""
        ae = self.ae
        ae.Encoder._engine(); ae.Decoder._engine()                            # (a re-pack after load_state_dict stays outside the capture)
        if ae.use_graph and self._runs >= 1:
            if self._captured is None:
                self._captured = ae._capture_plan(self.plan())
            ae._execute(self._captured[1])
        else:
            ae._execute(self.plan())
        self._runs += 1
        host = self.table.cpu().numpy()                                       # the only host sync of a validation
        return validation.split_table(host, self.n_speakers, self.E)


class HostFedStep(object):
    """The --train_ae step fed from host memory with the H2D copy INSIDE the captured step (the reference
    copies the 67 MB batch synchronously in front of every iteration, trainer.py:238-244).

    Two static device inputs X[0], X[1] and two pinned staging buffers P[0], P[1]; graph k computes the step on X[k] and, as a
    parallel branch on the copy stream, copies P[1-k] -> X[1-k] (the NEXT batch).  Step i replays graph i % 2, so the copy of batch
    i+1 runs on the DMA engine beside the kernels of step i and costs no time on the critical path.  The host stages batch i+2 into
    P[i % 2] after it has seen the end of step i-1 (the last reader of that buffer): it runs at most two steps ahead of the GPU.
    Until the graphs exist (the AEStep's eager warm-up steps) batches go through a plain synchronous copy."""

    def __init__(self, ae, loader):
        self.ae, self.loader, self.dev = ae, loader, ae.device
        self.i = 0
        self.P = self.PC = self.X = self.C = None
        self.ents = None
        self.done = [torch.cuda.Event(), torch.cuda.Event()]
        self._next = self._fetch()

    def _fetch(self):
        c, x = next(self.loader)[:2]
        c = c.long().contiguous()
        n_spk = self.ae.Decoder.c_a
        if c.numel() and (int(c.min()) < 0 or int(c.max()) >= n_spk):         # an index outside the embedding tables would fault the GPU
            raise ValueError('speaker index outside [0, %d) in the batch' % n_spk)
        return c, x.float().contiguous()

    def _alloc(self, c, x):
        def pair(shape, dtype):
            # storage rounded up to 16 bytes (zs_host_fetch granularity); zero-initialised: never a stale speaker index
            n = 1
            for d in shape:
                n *= d
            es = torch.empty(0, dtype=dtype).element_size()
            n_pad = (n * es + 15) // 16 * 16 // es
            host = [torch.zeros(n_pad, dtype=dtype).pin_memory() for _ in range(2)]
            devt = [torch.zeros(n_pad, dtype=dtype, device=self.dev) for _ in range(2)]
            return host, devt, [h[:n].view(shape) for h in host], [d[:n].view(shape) for d in devt]
        self._Pfull, self._Xfull, self.P, self.X = pair(tuple(x.shape), torch.float32)
        self._PCfull, self._Cfull, self.PC, self.C = pair(tuple(c.shape), torch.int64)

    def __iter__(self):
        return self

    def __next__(self):
        ae = self.ae
        c, x = self._next
        if self.P is None:
            self._alloc(c, x)
        if self.ents is None:
            self.X[0].copy_(x); self.C[0].copy_(c)                            # batch i -> X[0]
            if not ae.use_graph:
                ae.step(self.X[0], self.C[0])
            else:
                # capture graph k on X[k] with the fetch of the other slot as a branch (speaker ids first)
                self.ents = ae._warm_up_or_capture(self.X[0], self.C[0], lambda: [
                    ae._capture(self.X[k], self.C[k], prefetch=((self._PCfull[1 - k], self._Cfull[1 - k]),
                                                                (self._Pfull[1 - k], self._Xfull[1 - k]))) for k in range(2)])
            self._next = self._fetch()
            if self.ents is None:                                                 # graphs off, or a warm-up step: done
                return ae._loss
            self.i = 0
            self.P[1].copy_(self._next[1]); self.PC[1].copy_(self._next[0])      # batch i+1 -> P[1]
        k = self.i % 2
        ae._execute(self.ents[k]['plan'], counted=True)                          # step i on X[k]; P[1-k] -> X[1-k] beside it
        self.done[k].record(torch.cuda.current_stream(self.dev))
        # stage batch i+2 into P[k]: its last reader was graph 1-k at step i-1
        self._next = self._fetch()                                            # = batch i+2 (batch i+1 is already in P[1-k])
        if self.i >= 1:
            self.done[1 - k].synchronize()
        self.PC[k].copy_(self._next[0])
        self.P[k].copy_(self._next[1])
        self.i += 1
        return ae._loss


class PoolFedStep(object):
    """The --train_ae step fed from a pool.DevicePool, the sibling of HostFedStep: the captured step begins with the gather of its
    batch into AEStep.static_inputs and the cursor's advance (pool.PoolLoader.gather_into), on the step's own stream -- no forked
    branch, no pinned buffer, one set of graphs -- so a replay serves the next batch and the host never waits.  The AEStep's
    eager warm-up steps, and every step when graphs are off, run the same launches eagerly."""

    def __init__(self, ae, loader):
        self.ae, self.loader = ae, loader
        loader.require(n_speakers=ae.Decoder.c_a)                             # an index outside the embedding tables would fault the GPU
        self.x, self.c = ae.static_inputs(loader.batch_size, loader.seg_len, loader.F)
        self.ent = None

    def _gather(self):
        self.loader.gather_into(self.x, self.c)

    def __iter__(self):
        return self

    def __next__(self):
        ae = self.ae
        if not ae.use_graph:
            self._gather()
            return ae.step(self.x, self.c)
        if self.ent is None:
            self.ent = ae._warm_up_or_capture(self.x, self.c, lambda: ae._capture(self.x, self.c, prologue=self._gather),
                                              prologue=self._gather)
            if self.ent is None:                                              # a warm-up step: done
                return ae._loss
        ae._execute(self.ent['plan'], counted=True)
        return ae._loss


class ClfStep(object):
    """Speaker-classifier side of stage 1 (trainer.py:349-465): the D step trains SpeakerClassifier on the encoder's
    pre-activation `enc` (CE, per-net clip, Adam betas (0.5, 0.9)); the G step trains Encoder+Decoder with
    loss_rec - alpha * loss_clf (the classifier only passes the gradient through)."""

    def __init__(self, ae, classifier, lr=1e-4, betas=(0.5, 0.9), max_grad_norm=5.0, ema=None):
        self.ae, self.clf = ae, classifier
        self.device = ae.device
        self.opt = NetOpt(classifier, lr, betas, max_grad_norm, reduce=False, ema=ema)     # reduced in d_step, even without an update
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.correct = torch.zeros(1, dtype=torch.int32, device=self.device)

    adam_step = property(lambda self: self.opt.t)

    def state_dict(self):
        """The classifier's optimizer (its count t seeds d_step); the autoencoder's state is the AEStep's own."""
        return {'clf': self.opt.state_dict()}

    def load_state_dict(self, sd):
        self.opt.load_state_dict(sd['clf'])

    def _classify(self, logits_act, c, grad_scale, seed, drop_masks=None):
        """enc logits Act fp32 [B,T',n_lin] (the encoder's pre-activation: 2E, E or E^2 columns by enc_mode) -> (classifier engine,
        grad_scale * dCE/dlogits fp32 [B, n_class]); the CE loss and #correct in self.loss / self.correct."""
        clf = self.clf
        clf.train()
        ce = clf._engine()
        x = clf.input_act(logits_act.valid())
        out = ce.forward(x, True, seed=seed, drop_masks=drop_masks)
        return ce, softmax_ce(ce.ctx, out.valid()[:, 0], c, self.loss, self.correct, grad_scale)

    def d_step(self, x_btf, c, alpha_dis=1.0, seed=None, update=True, noise=None, noise_kind=2, drop_masks=None, clf_masks=None):
        """One classifier update (trainer.py:352-366 / 396-411).  Returns (loss_clf, n_correct) device scalars."""
        enc = self.ae.Encoder
        enc.train()
        ee = enc._engine()
        if seed is None:
            seed = (self.adam_step + 1) * 0x9E3779B97F4A7C15 % (1 << 62) + 17 * parallel.rank()
        _, _, logits = ee.forward(x_btf, True, noise=noise, noise_kind=noise_kind, seed=seed, drop_masks=drop_masks)
        ce, dl = self._classify(logits, c, alpha_dis, seed + 1, clf_masks)
        ce.backward(dl, dl.stride(0), need_dx=False)
        join_side(self.device)
        if parallel.world_size() > 1:
            self.ae.reducer.start(self.clf.flat_params()[1])
            self.ae.reducer.finish()
        if update:
            self.optimizer_step()
        return self.loss, self.correct

    def optimizer_step(self):
        self.opt.step()

    def g_step(self, x_btf, c, alpha, seed=None, update=True, noise=None, noise_kind=2, drop_masks=None, clf_masks=None):
        """One autoencoder update with the adversarial term (trainer.py:427-447): loss = loss_rec - alpha * loss_clf.
        Returns (loss_rec, loss_clf, n_correct) device scalars."""
        ae = self.ae
        enc, dec = ae.Encoder, ae.Decoder
        enc.train(); dec.train()
        ee, de = enc._engine(), dec._engine()
        if seed is None:
            seed = (ae.adam_step + 1) * 0x9E3779B97F4A7C15 % (1 << 62) + 31 * parallel.rank()
        bits, _, logits = ee.forward(x_btf, True, noise=noise, noise_kind=noise_kind, seed=seed, drop_masks=drop_masks)
        dlogit = ae.l1_loss(de, x_btf, de.forward(bits, c, True))
        ce, dl = self._classify(logits, c, -float(alpha), seed + 1, clf_masks)           # maximise the classification loss
        dbits = de.backward(dlogit)
        dx = ce.backward(dl, dl.stride(0), need_dx=True, param_grads=False)
        multi = parallel.multi_rank()
        if multi:
            join_side(self.device)
            ae.reducer.start(dec.flat_params()[1])
        ee.backward(dbits, dlogits_extra=dx)
        join_side(self.device)
        if multi:
            ae.reducer.start(enc.flat_params()[1])
            ae.reducer.finish()
        if update:
            ae.optimizer_step()
        return ae._loss, self.loss, self.correct


def tclf_labels(c, n_speakers, n_target_speakers, g_mode):
    """The t_classify targets (trainer.py:617-624) from HOST speaker ids: c[c < 100] = 102, then c - shift_c with
    shift_c = n_speakers - n_target_speakers (100 -> V001 = 0, 101 -> V002 = 1, every other speaker -> 'None' = 2 for the
    english / surprise sets).  Raises ValueError where the reference could not run: g_mode 'naive' (it defines no shift_c) and a
    target outside [0, 3) (nn.CrossEntropyLoss would fail; here it would index past the logits on the GPU)."""
    if g_mode == 'naive':
        raise ValueError("t_classify needs shift_c = n_speakers - n_target_speakers, which the reference defines only for a g_mode "
                         "other than 'naive'")
    c = torch.as_tensor(c).long().clone()
    c[c < 100] = 102
    y = c - int(n_speakers - n_target_speakers)
    if y.numel() and (int(y.min()) < 0 or int(y.max()) >= TCLF_CLASSES):
        raise ValueError('t_classify target %d outside [0, %d): relabelled speaker ids (c < 100 -> 102) minus shift_c = %d must be '
                         '100, 101 or 102' % (int(y.min()) if int(y.min()) < 0 else int(y.max()), TCLF_CLASSES,
                                                 int(n_speakers - n_target_speakers)))
    return y


class TclfStep(object):
    """One --train_c iteration (trainer.py:615-628): TargetClassifier forward in train mode (Dropout2d p = dp), CE on the relabelled
    targets, backward to the parameters only, clip_grad_norm(max_grad_norm) + Adam(lr, betas (0.5, 0.9)).  The relabel runs on
    the device (no host sync); the targets are range-checked on the host by tclf_labels before a batch is copied over."""

    def __init__(self, classifier, lr, max_grad_norm, shift, ema=None):
        self.clf, self.shift = classifier, int(shift)
        self.opt = NetOpt(classifier, lr, betas=(0.5, 0.9), max_norm=max_grad_norm, ema=ema)
        dev = classifier.flat_params()[0].device
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.correct = torch.zeros(1, dtype=torch.int32, device=dev)

    def state_dict(self):
        return {'clf': self.opt.state_dict()}

    def load_state_dict(self, sd):
        self.opt.load_state_dict(sd['clf'])

    def step(self, x_btf, c, masks=None, update=True):
        """x_btf fp32 [B, T, 513], c int64 [B] raw speaker ids on the device.  masks: optional six [B, C] Dropout2d keep masks.
        Returns (loss, n_correct) device scalars; parameter gradients are left in the classifier's flat gradient buffer."""
        clf = self.clf
        clf.train()
        eng = clf._engine()
        y = c.masked_fill(c < 100, 102) - self.shift                           # c[c < 100] = 102; c - shift_c
        eng.zero_grads()
        _, logits = eng.forward(x_btf.contiguous(), 'tclf', True, masks=masks, classify=True, need_val=False)
        dl = softmax_ce(eng.ctx, logits, y, self.loss, self.correct)
        eng.backward('tclf', dlogits=dl, need_dx=False, param_grads=True)
        eng.flush_grads()
        if update:
            self.opt.step()
        return self.loss, self.correct


PREFIX = 'module.'                       # on the keys of the two nets the reference wraps in nn.DataParallel (_ckpt_sources puts it there)


def strip_prefix(sd):
    """A state dict of a checkpoint without the prefix of the wrapped nets: what net.load_state_dict takes."""
    return {(k[len(PREFIX):] if k.startswith(PREFIX) else k): v for k, v in sd.items()}


class _Slot(int):
    """Placeholder of a device tensor in the skeleton of a state tree: the index of its snapshot buffer."""


def _fill_slots(skel, pin):
    """The state tree of a snapshot: every _Slot of `skel` replaced by a pageable copy of its pinned buffer."""
    if isinstance(skel, _Slot):
        return pin[skel].clone()
    if isinstance(skel, dict):
        return {k: _fill_slots(v, pin) for k, v in skel.items()}
    if isinstance(skel, list):
        return [_fill_slots(v, pin) for v in skel]
    return skel


class Trainer(object):
    ema = None                             # the decay of the weight averages (__init__ sets it; the default serves a Trainer made without it)

    valid = None                           # the ValidConfig of the held-out validation (__init__ sets it)
    vq = None                              # the vq_train.VqBottleneck of a run that trains through its codebook (build_model sets it)
    vq_train = None
    _best_due = False

    def __init__(self, hps, data_loader, g_mode, enc_mode, log_dir='./log/', dtype=None, device=None, ema=None, valid=None,
                 vq_train=None, rvq_dropout=None):
        """vq_train (not in the reference): None, or (vq.VectorCodebook, beta, decay): train(mode='pretrain_AE') then trains through
        that codebook (vq_train.VqBottleneck inside the AEStep), logs loss_vq, the codewords used and the perplexity, and
        writes <checkpoint>.vq.npz beside every checkpoint.  Every other mode runs without the quantiser.  A fourth element is the
        threshold below which dead codewords are restarted; the log and the file's meta then carry the restarts.
        The codebook's kind picks the bottleneck: an rvq.ResidualCodebook trains through its S stages (rvq_train.RvqBottleneck,
        DESIGN 34), the log carries every stage's share of codewords used and the file is <checkpoint>.rvq.npz.
        rvq_dropout (not in the reference): None, or P in (0, 1]: quantiser dropout of that residual bottleneck; the log
        then carries every stage's share of active rows.
        valid (not in the reference): None, or a validation.ValidConfig: train(mode='pretrain_AE') then validates on its set
        every `every` iterations and after the last one (ValidStep), logs and records the result and keeps the best checkpoint.
        ema (not in the reference): None, or the decay in [0, 1) of an exponential moving average of the weights that every
        optimizer this trainer builds keeps beside its net (optim.NetOpt); the checkpoints then carry `<net>_ema` entries."""
        self.hps = hps
        self.ema = check_ema(ema)
        self.valid = validation.check_config(valid, hps) if valid is not None else None
        self.vq_train = vq_train
        self.rvq_dropout = rvq_dropout
        if rvq_dropout is not None and (vq_train is None or getattr(vq_train[0], 'kind', None) != 'residual'):
            raise ValueError('rvq_dropout needs vq_train with a residual codebook (rvq.ResidualCodebook)')
        if vq_train is not None:
            from .vq import VectorCodebook
            VectorCodebook.check_mode(enc_mode, "vq_train needs enc_mode 'continues'")
        self._vstep = None                                                 # ValidStep, built on first use
        self.best_loss = self.best_iteration = None                        # the lowest valid_loss_rec so far and its iteration
        self._best_due = False                                             # the next periodic resumable checkpoint also writes -ae-best
        self.data_loader = data_loader
        self._prefetch = None
        self.model_kept = []
        self.max_keep = hps.max_to_keep
        self.logger = Logger(log_dir)
        self.g_mode = g_mode
        self.enc_mode = enc_mode
        self.dtype = dtype or os.environ.get('ZS_DTYPE', 'fp32')
        if device is None:
            if not torch.cuda.is_available():
                raise L.ZsError('zs_amd.Trainer needs an MI355X (torch.cuda.is_available() is False); no CPU fallback')
            device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0')))
        self.device = torch.device(device)
        self.log_every = int(os.environ.get('ZS_LOG_EVERY', '1'))
        self.ckpt_every = int(os.environ.get('ZS_CKPT_EVERY', '1000'))     # the reference saves every 1000 iterations (trainer.py:345)
        self._consumed = {'data': 0, 'source': 0, 'target': 0}             # batches the steps have taken from each loader (resume)
        self._writer = None                                                # train_state.Writer of the resumable checkpoints
        self._snap = None                                                  # their device snapshot + pinned host buffers
        self.build_model()

    # ---- model (trainer.py:48-98) -------------------------------------------------------------
    def build_model(self):
        hps, ns = self.hps, self.hps.ns
        dev, dt = self.device, self.dtype
        self.Encoder = Encoder(ns=ns, dp=hps.enc_dp, enc_size=hps.enc_size, seg_len=hps.seg_len, enc_mode=self.enc_mode,
                               dtype=dt).to(dev)
        self.Decoder = Decoder(ns=ns, c_in=hps.enc_size, c_h=hps.emb_size, c_a=hps.n_speakers, seg_len=hps.seg_len,
                               dtype=dt).to(dev)
        if self.g_mode == 'naive':
            self.Generator = Decoder(ns=ns, c_in=hps.enc_size, c_h=hps.emb_size, c_a=hps.n_speakers, seg_len=hps.seg_len,
                                     dtype=dt).to(dev)
        elif self.g_mode in ('targeted', 'targeted_residual'):
            self.Generator = Decoder(ns=ns, c_in=hps.enc_size, c_h=hps.emb_size, c_a=hps.n_target_speakers, seg_len=hps.seg_len,
                                     output_mask=(self.g_mode == 'targeted_residual'), dtype=dt).to(dev)
        elif self.g_mode == 'spectrogram':                                        # trainer.py:77-78
            self.Generator = Spectrogram_Patcher(ns=ns, c_in=513, c_h=hps.emb_size, c_a=hps.n_target_speakers, seg_len=hps.seg_len,
                                                 dtype=dt).to(dev)
        elif self.g_mode in ('enhanced', 'tacotron'):
            raise NotImplementedError('g_mode %r (stage-2 generator) is not built: use naive, targeted, targeted_residual or '
                                      'spectrogram' % self.g_mode)
        else:
            raise NotImplementedError('Invalid Generator mode!')
        enc_size = hps.enc_size
        self.SpeakerClassifier = SpeakerClassifier(ns=ns, c_in=(enc_size * enc_size if self.enc_mode == 'binary' else
                                                                (2 * enc_size if self.enc_mode == 'multilabel_binary' else enc_size)),
                                                   c_h=hps.emb_size, n_class=hps.n_speakers, dp=hps.dis_dp, seg_len=hps.seg_len,
                                                   dtype=dt).to(dev)
        # ---stage two--- (trainer.py:85-97; nn.DataParallel there is a single-GPU identity: one process per GPU here)
        self.PatchDiscriminator = PatchDiscriminator(ns=ns, n_class=(hps.n_speakers if self.g_mode == 'naive' else hps.n_target_speakers),
                                                     seg_len=hps.seg_len, dtype=dt).to(dev)
        self.TargetClassifier = TargetClassifier(ns=ns, n_class=3, seg_len=hps.seg_len, dtype=dt).to(dev)
        self.ae = AEStep(self.Encoder, self.Decoder, lr=hps.lr, betas=(0.5, 0.9), max_grad_norm=hps.max_grad_norm, ema=self.ema)
        if self.vq_train is not None:                   # the --train_ae loop alone: train() hands it to the AEStep for that mode
            from .vq_train import Bottleneck, encoded_rows
            cb, beta, decay = self.vq_train[:3]
            restart = self.vq_train[3] if len(self.vq_train) > 3 else None      # the threshold of zs_vq_restart
            cb.check_width(hps.enc_size, 'vq_train')
            more = {'dropout': self.rvq_dropout} if self.rvq_dropout is not None else {}
            bottleneck = Bottleneck.of_kind(cb.kind)    # the codebook's kind picks the bottleneck
            self.vq = bottleneck(cb, beta, decay, encoded_rows(hps.batch_size, hps.seg_len), layers.Ctx(dev, dt), restart=restart, **more)
        self.clf = ClfStep(self.ae, self.SpeakerClassifier, lr=hps.lr, betas=(0.5, 0.9), max_grad_norm=hps.max_grad_norm, ema=self.ema)
        self.s2 = None                      # PatchGANStep, built on first use (its optimizer state is 2 x 53 M floats)
        self.source_loader = self.target_loader = None
        self.testing_shift_c = None
        self.tclf = None                    # TclfStep, built on first use (--train_c)
        self.tclf_loaded = False            # load_model restored target_classifier
        self.sync_params()

    def nets(self):
        return [self.Encoder, self.Decoder, self.Generator, self.SpeakerClassifier, self.PatchDiscriminator, self.TargetClassifier]

    def named_nets(self):
        """[(checkpoint key, net)] in the order of nets()."""
        return list(zip(train_state.NET_NAMES, self.nets()))

    def add_duo_loader(self, source_loader, target_loader):
        """trainer.py:171-173."""
        self.source_loader, self.target_loader = source_loader, target_loader
        self._duo = None

    def stage2(self, autolocker=False):
        """The stage-2 step object.  autolocker=True: an AutolockerStep (raises ValueError before any launch unless enc_mode is
        multilabel_binary); a PatchGANStep built earlier hands it its optimizers (the reference has one gen_opt / patch_opt)."""
        if autolocker and not isinstance(self.s2, AutolockerStep):
            al = AutolockerStep(self.Encoder, self.Decoder, self.Generator, self.PatchDiscriminator, self.hps, self.g_mode, ema=self.ema)
            if self.s2 is not None:                 # (al's own optimizers, moments and averages included, are dropped here)
                al.gen_opt, al.patch_opt, al.step_no = self.s2.gen_opt, self.s2.patch_opt, self.s2.step_no
            self.s2 = al
        if self.s2 is None:
            self.s2 = PatchGANStep(self.Encoder, self.Decoder, self.Generator, self.PatchDiscriminator, self.hps, self.g_mode, ema=self.ema)
        return self.s2

    def sync_params(self):
        """Data parallel: every rank starts from rank 0's weights (each process seeds torch's RNG differently, so the freshly
        built replicas differ); the Adam moments start at zero everywhere.  Called after build_model and load_model.  Every
        weight average that exists restarts from the weights (only a train state restores one that differs from them)."""
        parallel.broadcast_params(self.nets())
        for opt in self.ema_opts().values():
            opt.reset_ema()

    def ema_opts(self):
        """{checkpoint key of a net: its NetOpt} for every net that has a weight average now (steps built lazily count once they
        exist), in the order of nets(); empty without ema."""
        if self.ema is None:
            return {}
        s2, tclf = self.s2, self.tclf
        opts = (('encoder', self.ae.opt['enc']), ('decoder', self.ae.opt['dec']), ('generator', s2.gen_opt if s2 is not None else None),
                ('classifier', self.clf.opt), ('patch_discriminator', s2.patch_opt if s2 is not None else None),
                ('target_classifier', tclf.opt if tclf is not None else None))
        return {k: o for k, o in opts if o is not None and o.ema is not None}

    def reset_keep(self):
        self.model_kept = []

    # ---- checkpoints (trainer.py:103-168) -----------------------------------------------------
    def _ckpt_blocking(self):
        """The checkpoint dict (the reference's, plus `<net>_ema` entries with weight averages) as CPU tensors, by blocking copies
        on the calling thread: the layout of _ckpt_sources, which the resumable checkpoints fill from their snapshot, filled
        here by one copy per source an entry uses (its flat buffer and each buffer outside it); one entry's host copies are
        alive at a time."""
        srcs, layout, _ = self._ckpt_sources({})
        ckpt = {}
        for key, pre, ents in layout:
            host = {s: srcs[s].detach().cpu() for s in {e[1] for e in ents}}
            ckpt[key] = {pre + k: host[s][o:o + n].view(shape).clone() for k, s, o, n, shape in ents}
        return ckpt

    def save_model(self, model_path, name, iteration, model_all=True):
        """model_all: the reference's parameter, kept for its signature; no caller passes False and every file holds all six nets."""
        new_model_path = '{}-{}-{}'.format(model_path, name, iteration)
        train_state.atomic_save(self._ckpt_blocking(), new_model_path)
        for old in train_state.roll_window(self.model_kept, new_model_path, self.max_keep):
            train_state.remove_checkpoint(old)                                 # its train-state file, if it has one, goes with it

    # ---- train state beside the checkpoint (no counterpart in the reference; see resume.py) --------
    def _steps(self, tag=None):
        """The step objects whose state a checkpoint of mode tag `tag` carries (None: every one that is built)."""
        have = {'ae': self.ae, 'clf': self.clf, 's2': self.s2, 'tclf': self.tclf}
        names = {'ae': ('ae',), 'c': ('clf',), 's1': ('ae', 'clf'), 's2': ('s2',), 'tclf': ('tclf',)}.get(tag, tuple(have))
        return {n: have[n] for n in names if have[n] is not None}

    def _state_tree(self, tag, iteration, target_guided, autolocker):
        """The state file's dict as it stands now, its tensors still where they live (the steps' own device buffers)."""
        st = train_state.describe(self, tag, target_guided, autolocker)
        st.update(iteration=int(iteration), steps={n: s.state_dict() for n, s in self._steps(tag).items()},
                  consumed=dict(self._consumed), model_kept=[os.path.basename(p) for p in self.model_kept],
                  rng={'cpu': torch.get_rng_state(), 'cuda': torch.cuda.get_rng_state(self.device)})
        if 'valid' in st:                                                 # (describe: a validating pretrain_AE run)
            st.update(best_loss=self.best_loss, best_iteration=self.best_iteration)
        return st

    def save_state(self, path, tag=None, iteration=0, target_guided=False, autolocker=None):
        """Write the train state (resume.py: everything but the weights) to `path`, synchronously.  tag: the mode tag it is
        recorded under ('ae' / 'c' / 's1' / 's2' / 'tclf'; None: '' and the state of every step object that is built)."""
        autolocker = isinstance(self.s2, AutolockerStep) if autolocker is None else autolocker
        tree = self._state_tree(tag, iteration, target_guided, autolocker)
        tree['tag'] = tag or ''
        train_state.atomic_save(train_state.map_tensors(tree, lambda t: t.detach().cpu().clone()), path)

    def load_state(self, path, tag=None, target_guided=None, autolocker=None, ckpt_dir=None, state=None):
        """Restore what save_state wrote, after the weights were loaded: optimizer moments and counts, step counters, loader
        positions, torch's RNG states and the rolling window.  tag / target_guided / autolocker: what the file must have been
        written for (None: whatever it says).  Every recorded field is compared with this run first: ValueError naming the
        field, before any launch.  ckpt_dir: where the window's checkpoints (recorded by file name) lie; default: the
        directory above the state file's.  state: the file's dict, already loaded and validated (train(resume=True) reads it once).
        Returns the file's dict."""
        if state is not None:
            return self._restore_state(state, ckpt_dir or os.path.dirname(os.path.dirname(os.path.abspath(path))))
        st = torch.load(path, map_location='cpu', weights_only=True)
        pick = lambda given, key: st.get(key) if given is None else given
        train_state.validate(st, train_state.describe(self, pick(tag, 'tag'), pick(target_guided, 'target_guided'),
                                                      pick(autolocker, 'autolocker')))
        return self._restore_state(st, ckpt_dir or os.path.dirname(os.path.dirname(os.path.abspath(path))))

    def _seek(self, counts):
        """Put every loader at the position after counts[name] batches and drop the prefetchers, which run ahead of the steps:
        they are rebuilt at the new position."""
        self._consumed = {k: int(counts[k]) for k in ('data', 'source', 'target')}
        for loader, k in ((self.data_loader, 'data'), (self.source_loader, 'source'), (self.target_loader, 'target')):
            if loader is None:
                continue
            if hasattr(loader, 'set_cursor'):                             # pool.PoolLoader: the batch number lives on the device
                loader.set_cursor(self._consumed[k])
            else:
                loader.index = 0
                loader.skip(self._consumed[k])
        self._prefetch = self._duo = self._tclf_prefetch = None

    def _restore_state(self, st, ckpt_dir):
        if 's2' in st['steps']:
            self.stage2(autolocker=bool(st['autolocker']))
        if 'tclf' in st['steps']:
            self.tclf_step()
        steps = self._steps()
        for name, sd in st['steps'].items():
            steps[name].load_state_dict(sd)
        self._seek(st['consumed'])
        if parallel.rank() == 0:                                          # the generator state is rank 0's; other ranks keep their own
            torch.set_rng_state(st['rng']['cpu'])
            torch.cuda.set_rng_state(st['rng']['cuda'], self.device)
        self.model_kept = [os.path.join(ckpt_dir, name) for name in st['model_kept']]
        if 'valid' in st:
            self.best_loss, self.best_iteration = st.get('best_loss'), st.get('best_iteration')
        return st

    def _load_all_nets(self, ckpt_path):
        """All six nets from a checkpoint of this build's own loop, strictly (load_model prints and goes on)."""
        all_model = torch.load(ckpt_path, map_location='cpu', weights_only=True)
        for key, net in self.named_nets():
            net.load_state_dict(strip_prefix(all_model[key]))
        self.sync_params()                                                # (the averages restart from these weights; load_state follows)

    def _reserve(self, srcs):
        """(device snapshot buffers, pinned host buffers) for the tensors `srcs`, allocated when their shapes first appear."""
        sig = [(tuple(s.shape), s.dtype) for s in srcs]
        if self._snap is None or self._snap['sig'] != sig:
            self._snap = {'sig': sig, 'dev': [torch.empty_like(s) for s in srcs],
                          'pin': [torch.empty(s.shape, dtype=s.dtype, pin_memory=True) for s in srcs]}
        return self._snap['dev'], self._snap['pin']

    def _snapshot(self, srcs):
        """Stream-ordered copies of the device tensors `srcs` into the reserved snapshot buffers (current stream: the next step's
        Adam is ordered behind them) and from there to pinned host memory on the copy stream.  Returns (pinned tensors, the event
        recorded after the last copy).  The buffers are allocated once; the caller keeps one snapshot in flight at most."""
        dev, pin = self._reserve(srcs)
        main, cs = torch.cuda.current_stream(self.device), layers.copy_stream(self.device)
        for d, s in zip(dev, srcs):
            d.copy_(s, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(main)
        cs.wait_event(ev)
        done = torch.cuda.Event()
        with torch.cuda.stream(cs):
            for p, d in zip(pin, dev):
                p.copy_(d, non_blocking=True)
            done.record(cs)
        return pin, done

    def _checkpoint_async(self, model_path, name, iteration, target_guided, autolocker, best=False):
        """A resumable checkpoint off the training thread's critical path: enqueue the snapshot (_snapshot) of the six flat
        parameter buffers and of every tensor of the state tree, then hand a worker thread the job of waiting for the event,
        building the checkpoint dict (save_model's) and the state dict from the pinned memory and writing both.
        best: the snapshot written to validation.best_path(model_path) alone: no state file, not in the rolling window (it takes
        the state tree's tensors along so that the one set of snapshot buffers serves both kinds).  A periodic checkpoint whose
        iteration's validation was a new best (_best_due) writes the best file too, from its one snapshot."""
        if self._writer is None:
            self._writer = train_state.Writer()
        self._writer.wait()                                               # one checkpoint in flight; its failure raises here
        new_path = validation.best_path(model_path) if best else '{}-{}-{}'.format(model_path, name, iteration)
        drop = [] if best else train_state.roll_window(self.model_kept, new_path, self.max_keep)
        also_best, self._best_due = (not best) and self._best_due, False
        srcs, layout, skel = self._ckpt_sources(self._state_tree(name, iteration, target_guided, autolocker))
        pin, done = self._snapshot(srcs)

        def job():
            done.synchronize()                                            # the worker's only GPU call
            ckpt = {key: {pre + k: pin[s][o:o + n].view(shape).clone() for k, s, o, n, shape in ents} for key, pre, ents in layout}
            train_state.atomic_save(ckpt, new_path)
            if also_best:
                train_state.atomic_save(ckpt, validation.best_path(model_path))
            if not best:
                train_state.atomic_save(_fill_slots(skel, pin), train_state.state_path(new_path))
            for old in drop:
                train_state.remove_checkpoint(old)
        self._writer.submit(job)

    def _ckpt_sources(self, tree):
        """What a resumable checkpoint copies: (srcs, layout, skel).  srcs: the device tensors (flat parameter buffers, moments, words);
        layout: per net (checkpoint key, key prefix, [(parameter name, index into srcs, offset, numel, shape)]), in
        state_dict order; skel: the state tree with every device tensor replaced by its index into srcs (_Slot).  With weight
        averages the layout goes on with the `<net>_ema` entries: the net's entries over the average's slot -- the one the state
        tree put it in, where the tree carries that optimizer: one copy serves the state file and the checkpoint."""
        srcs, layout, flat_slot = [], [], {}
        for key, net in zip(train_state.NET_NAMES, self.nets()):
            flat, offs = net.flat_params()[0], net._zs['offsets']
            slot, ents = len(srcs), []
            flat_slot[key] = slot
            srcs.append(flat)
            for k, v in net.state_dict().items():
                if k in offs:
                    ents.append((k, slot, offs[k], v.numel(), tuple(v.shape)))
                else:                                                     # a buffer outside the flat storage
                    ents.append((k, len(srcs), 0, v.numel(), tuple(v.shape)))
                    srcs.append(v.detach().reshape(-1))
            layout.append((key, 'module.' if key in ('patch_discriminator', 'target_classifier') else '', ents))

        slot_of = {}                                                      # data_ptr of a device tensor of the tree -> its slot

        def grab(t):
            if t.device.type == 'cpu':
                return t.clone()
            srcs.append(t.detach())
            slot_of[t.data_ptr()] = len(srcs) - 1
            return _Slot(len(srcs) - 1)
        skel = train_state.map_tensors(tree, grab)
        for key, opt in self.ema_opts().items():
            slot = slot_of.get(opt.ema.data_ptr())
            if slot is None:                                              # a net this mode's state does not carry
                slot = len(srcs)
                srcs.append(opt.ema)
            _, pre, ents = layout[train_state.NET_NAMES.index(key)]
            layout.append((key + '_ema', pre, [(k, slot if s == flat_slot[key] else s, o, n, shape) for k, s, o, n, shape in ents]))
        return srcs, layout, skel

    def load_model(self, model_path, load_model_list, verbose=True, clf_path=None, use_ema=False):
        """use_ema (not in the reference): each net is taken from the file's `<net>_ema` entry, the weight average a run with
        Trainer(ema=...) saved, where the file has one (else from `<net>`; the printed tag says which); ValueError when
        model_path has no such entry at all -- whatever clf_path holds: that file only lends its target_classifier, averaged
        where it has the average."""
        if verbose:
            print('[Trainer] - load model from {}'.format(model_path))
        load_model_list = load_model_list.split(', ')
        all_model = torch.load(model_path, map_location='cpu', weights_only=True)
        src = {k: k for k in train_state.NET_NAMES}
        if use_ema:
            src = train_state.ema_keys(all_model.keys(), train_state.NET_NAMES, model_path)
        if verbose:
            print('[Trainer] - ', end='')
        for key, net in self.named_nets():
            if key in load_model_list:
                tag = key
                try:
                    other = key == 'target_classifier' and clf_path is not None    # trainer.py:157-161: taken from ANOTHER checkpoint
                    file = torch.load(clf_path, map_location='cpu', weights_only=True) if other else all_model
                    entry = (key + '_ema' if use_ema and key + '_ema' in file else key) if other else src[key]
                    net.load_state_dict(strip_prefix(file[entry]))
                    tag = entry + ('_another' if other else '')
                    if key == 'target_classifier':
                        self.tclf_loaded = True
                    if verbose:
                        print('[%s], ' % tag, end='')
                except Exception as e:                                   # reference: bare except, prints [x - X]
                    print('[%s - X] (%s), ' % (tag, type(e).__name__), end='')
        if verbose:
            print('Loaded!')
        self.sync_params()

    # ---- inference (trainer.py:180-228) -------------------------------------------------------
    def set_eval(self):
        self.testing_shift_c = torch.tensor([int(self.hps.n_speakers - self.hps.n_target_speakers)], device=self.device)
        self.Encoder.eval()
        self.Decoder.eval()
        self.SpeakerClassifier.eval()
        self.Generator.eval()

    def test_step(self, x, c, enc_only=False, verbose=True, U=None, G=None):
        self.set_eval()
        x = x.to(self.device).permute(0, 2, 1)
        c = c.to(self.device)
        enc, _ = self.Encoder(x, U=U, G=G)
        x_dec = self.Decoder(enc, c)
        if not enc_only:
            if verbose:
                print('Testing with Autoencoder + Generator, encoding: ', enc.cpu().numpy())
            if self.g_mode != 'naive' and int((c - self.testing_shift_c)[0]) not in range(self.hps.n_target_speakers):
                raise RuntimeError('This generator can only convert to target speakers!')
            if self.g_mode == 'naive':
                x_dec = x_dec + self.Generator(enc, c)
            elif self.g_mode == 'targeted':
                x_dec = x_dec + self.Generator(enc, c - self.testing_shift_c)
            elif self.g_mode == 'targeted_residual':
                x_dec = (x_dec * 1.0) + (1.0 * x_dec * self.Generator(enc, c - self.testing_shift_c))
            elif self.g_mode == 'spectrogram':                                        # trainer.py:212-213
                x_dec = x_dec + self.Generator(x_dec, c - self.testing_shift_c)
            else:
                raise NotImplementedError('Invalid Generator mode!')
        elif verbose:
            print('Testing with Autoencoder only, encoding: ', enc.cpu().numpy())
        out = x_dec.cpu().numpy(), enc.cpu().numpy()
        layers.check_status(self.device)                  # the .cpu() above synchronised: a timed-out GRU pass raises here
        return out

    def encoder_test_step(self, x, U=None, G=None):
        self.set_eval()
        x = x.to(self.device).permute(0, 2, 1)
        enc, _ = self.Encoder(x, U=U, G=G)
        out = enc.cpu().numpy()
        layers.check_status(self.device)
        return out

    def classify(self, x):
        """trainer.py:231-235: x [B, T, 513] -> the TargetClassifier's eval-mode logits [B, 3] (numpy)."""
        self.set_eval()
        clf = self.TargetClassifier
        clf.eval()
        x = torch.as_tensor(x).to(self.device, torch.float32).contiguous()
        _, logits = clf._engine().forward(x, 'eval', False, classify=True, need_val=False)
        return logits.cpu().numpy()

    # ---- training pieces (trainer.py:238-254) --------------------------------------------------
    def permute_data(self, data, load_mel=False):
        C = data[0].to(self.device, non_blocking=True)
        X = data[1].to(self.device, non_blocking=True).permute(0, 2, 1)
        return C, X

    def encode_step(self, x):
        return self.Encoder(x)

    def decode_step(self, enc, c):
        return self.Decoder(enc, c)

    def clf_step(self, enc):
        return self.SpeakerClassifier(enc)

    def ae_step(self, x_btf, c, **kw):
        """One fused --train_ae iteration; see AEStep.step."""
        return self.ae.step(x_btf, c, **kw)

    # ---- the loop (trainer.py:316-347) -----------------------------------------------------------
    def _device_batches(self, loader, n_speakers=None, check=None):
        """The iterator of device batches `(c, x)` over `loader`: a pool.PoolLoader serves them itself, once its whole speaker column
        has passed the checks (host memory, before any launch); a host loader goes through a DevicePrefetcher that applies them to
        every batch."""
        from .pool import PoolLoader
        if isinstance(loader, PoolLoader):
            return loader.require(n_speakers=n_speakers, check=check)
        from .dataloader import DevicePrefetcher
        return DevicePrefetcher(loader, self.device, n_speakers=n_speakers, check=check)       # next batch copied under the current step

    def _took(self, *loaders):
        """Count one batch handed to a step from each named loader.  This, not the loaders' own index, is a run's position: the
        prefetchers run one batch ahead of the steps and HostFedStep two."""
        for name in loaders:
            self._consumed[name] += 1

    def _batch(self):
        if self._prefetch is None:
            self._prefetch = self._device_batches(self.data_loader, n_speakers=self.hps.n_speakers)
        batch = next(self._prefetch)
        self._took('data')
        return batch

    def _duo_batch(self):
        """next(source_loader), next(target_loader) through the prefetcher (trainer.py:472-475)."""
        if getattr(self, '_duo', None) is None:
            if self.source_loader is None or self.target_loader is None:
                raise RuntimeError('patchGAN needs add_duo_loader(source_loader, target_loader)')
            self._duo = (self._device_batches(self.source_loader, n_speakers=self.hps.n_speakers),
                         self._device_batches(self.target_loader, n_speakers=self.hps.n_speakers, check=self.stage2().check_targets))
        pair = next(self._duo[0]), next(self._duo[1])
        self._took('source', 'target')
        return pair

    def tclf_labels(self, c_host):
        """t_classify targets of a HOST batch (tclf_labels above with this trainer's hps / g_mode); raises ValueError."""
        return tclf_labels(c_host, self.hps.n_speakers, self.hps.n_target_speakers, self.g_mode)

    def tclf_step(self):
        if self.tclf is None:
            self.tclf = TclfStep(self.TargetClassifier, self.hps.lr, self.hps.max_grad_norm,
                                 self.hps.n_speakers - self.hps.n_target_speakers, ema=self.ema)
        return self.tclf

    def _tclf_batch(self):
        """next(data_loader) through a prefetcher whose check range-checks the relabelled targets of every batch on the host
        (tclf_labels, raising ValueError) before it is copied; the relabel the step uses runs on the device (TclfStep.step)."""
        if getattr(self, '_tclf_prefetch', None) is None:
            self._tclf_prefetch = self._device_batches(self.data_loader, check=self.tclf_labels)
        batch = next(self._tclf_prefetch)
        self._took('data')
        return batch

    def _log(self, iteration, iters, fmt, info, head=()):
        """One logged record: every rank reads the GRU status word (the .item() reads that made `info` synchronised the host
        already); rank 0 prints the line over the previous one and writes `info` to the logger every 100 iterations."""
        layers.check_status(self.device)
        if parallel.rank() == 0:
            print(fmt % (head + (iteration + 1, iters) + tuple(info.values())), end='\r')
            if iteration % 100 == 0:
                for tag, value in info.items():
                    self.logger.scalar_summary(tag, value, iteration + 1)

    def _loop(self, iters, model_path, ckpt_name, iteration_fn, start=0, keep_state=None, after_save=None):
        """The loop of every mode: iteration_fn(iteration, log) runs one iteration, log = self._log bound to it at a logged
        iteration (every log_every-th and the last) and None otherwise; rank 0 saves a checkpoint every ckpt_every iterations
        and then calls after_save(checkpoint path, iteration), when given.
        start: the first iteration (a resumed run).  keep_state: None, or (target_guided, autolocker) of a resumable run: its
        checkpoints carry a train-state file and are written by a worker thread (_checkpoint_async), which is waited for before
        this returns and when an exception leaves the loop."""
        is_main = parallel.rank() == 0
        if keep_state is not None and is_main and start < iters:
            self._reserve(self._ckpt_sources(self._state_tree(ckpt_name, start, *keep_state))[0])     # snapshot + pinned buffers, once
        try:
            for iteration in range(start, iters):
                log_now = (iteration % self.log_every == 0) or (iteration + 1 == iters)
                iteration_fn(iteration, functools.partial(self._log, iteration, iters) if log_now else None)
                if (iteration + 1) % self.ckpt_every == 0 and is_main:
                    if keep_state is not None:
                        self._checkpoint_async(model_path, ckpt_name, iteration + 1, *keep_state)
                    else:
                        self.save_model(model_path, ckpt_name, iteration + 1)
                    if after_save is not None:
                        after_save('{}-{}-{}'.format(model_path, ckpt_name, iteration + 1), iteration + 1)
                if keep_state is not None and self._writer is not None:
                    self._writer.poll()                                                   # a failed write raises at once
        except BaseException:
            try:
                self._finish_writer()
            except Exception:                                                             # the loop's own exception is the one to report
                pass
            raise
        self._finish_writer()                                                             # re-raises what the writer raised
        layers.check_status(self.device)                                                  # every rank, after the last step
        if is_main:
            print()

    def valid_step(self):
        if self._vstep is None:
            self._vstep = ValidStep(self.ae, self.valid.set, self.valid.batches, self.hps.n_speakers)
        return self._vstep

    def validate(self, iteration, model_path=None, flag='train', keep_state=None):
        """One held-out validation of the autoencoder's raw weights (with --ema too: validating the averages would need an operand
        re-pack round trip) after `iteration` iterations.  Every rank runs it, on the same set with the same noise, so all
        ranks agree without communication; rank 0 logs the record, prints one line, appends it to <ckpt_dir>/valid.jsonl and,
        when valid_loss_rec is lower than every earlier one, writes <model_path>-ae-best through the path the run's periodic
        checkpoints take (save_model's dict; the writer thread when resumable).  Returns the record."""
        hps = self.hps
        vs = self.valid_step()
        rec = validation.finish(vs.run(), vs.T, vs.F, units=vs.units,
                                target_ids=range(hps.n_speakers - hps.n_target_speakers, hps.n_speakers))
        layers.check_status(self.device)                                  # (run() synchronised: a timed-out GRU pass raises here)
        if parallel.rank() != 0:
            return rec
        for k in validation.SCALARS:
            if rec.get(k) is not None:
                self.logger.scalar_summary('%s/%s' % (flag, k), rec[k], iteration)
        print(validation.line(iteration, rec).ljust(60))                  # a line of its own: the loop's \r lines overwrite each other
        if model_path is not None:
            validation.append_record(validation.record_path(model_path), iteration, rec)
        if self.best_loss is None or rec['valid_loss_rec'] < self.best_loss:
            self.best_loss, self.best_iteration = rec['valid_loss_rec'], int(iteration)
            if model_path is not None:
                if keep_state is not None and iteration % self.ckpt_every == 0:
                    self._best_due = True                                 # this iteration's periodic checkpoint writes it, from its one snapshot
                elif keep_state is not None:
                    self._checkpoint_async(model_path, 'ae', iteration, *keep_state, best=True)
                else:
                    train_state.atomic_save(self._ckpt_blocking(), validation.best_path(model_path))
        return rec

    def _finish_writer(self):
        if self._writer is not None:
            self._writer.wait()

    def _resume_from(self, model_path, mode, target_guided, iters):
        """Trainer.train(resume=True) before its loop: load the newest checkpoint of this mode's tag under model_path's directory
        that has a train-state file (all six nets, then the state) and return its iteration; 0 when there is none; None when it
        already is the final iteration.  Every rank reads the same files."""
        tag, say = train_state.TAGS[mode], (print if parallel.rank() == 0 else (lambda *a: None))
        found = train_state.find_resumable(model_path, tag)
        records = validation.record_path(model_path) if (self.valid is not None and tag == 'ae' and parallel.rank() == 0) else None
        if found is None:
            if records is not None:
                validation.truncate_records(records, 0)
            say('[Trainer] - resume: no %s checkpoint with a train state beside %s, starting from iteration 0' % (tag, model_path))
            self._seek({'data': 0, 'source': 0, 'target': 0})             # a run's position is counted from the loaders' start
            return 0
        ckpt, state, _ = found
        # the file is validated against this run (ValueError) before a weight is touched or anything is launched
        st = torch.load(state, map_location='cpu', weights_only=True)
        train_state.validate(st, train_state.describe(self, tag, target_guided, mode == 'autolocker'))
        if records is not None:                                           # the records behind the restart point are written again
            validation.truncate_records(records, int(st['iteration']))
        self._load_all_nets(ckpt)
        self.load_state(state, state=st)
        it = int(st['iteration'])
        if it >= iters:
            say('[Trainer] - resume: %s is the final iteration (%d of %d), nothing left to train' % (ckpt, it, iters))
            return None
        say('[Trainer] - resume: %s, continuing at iteration %d of %d' % (ckpt, it, iters))
        return it

    def train(self, model_path, flag='train', mode='train', target_guided=False, resume=False):
        """resume=True (not in the reference): every checkpoint gets a train-state file (resume.py) and the run continues from the
        newest one under model_path's directory, bit for bit; without one it starts from iteration 0."""
        hps = self.hps
        resumable = bool(resume)
        keep_state = (bool(target_guided), mode == 'autolocker') if resumable else None

        def begin(iters):
            """The first iteration of the loop; None: the final checkpoint is already there."""
            return self._resume_from(model_path, mode, target_guided, iters) if resumable else 0

        if mode == 'pretrain_AE':                                                         # trainer.py:320-347
            start = begin(hps.enc_pretrain_iters)
            if start is None:
                return
            from .pool import PoolLoader
            if isinstance(self.data_loader, PoolLoader):
                feeder = self.ae.pool_feeder(self.data_loader.require(n_speakers=hps.n_speakers))   # the gather at the head of the step
            else:
                feeder = self.ae.host_feeder(self.data_loader) if self.ae.use_graph else None  # H2D of the next batch inside the graph

            vcfg, iters = self.valid, hps.enc_pretrain_iters
            if vcfg is not None and not resumable and parallel.rank() == 0:
                validation.truncate_records(validation.record_path(model_path), 0)              # a run from iteration 0: its own records

            def iteration_fn(iteration, log):
                if feeder is not None:
                    loss_t = next(feeder)
                    self._took('data')
                else:
                    c, x = self._batch()
                    loss_t = self.ae_step(x, c)
                if log and bn is not None:
                    info = {f'{flag}/pre_loss_rec': loss_t.item()}                             # (the host sync)
                    s = bn.stats()                                                             # raises for a row left out of the average
                    if 'stages' in s:                                                          # a residual codebook: every stage's share
                        info[f'{flag}/pre_loss_vq'] = s['loss_vq']
                        for i, stg in enumerate(s['stages']):
                            info.update({f'{flag}/vq_used_%d' % i: stg['used'] / float(s['K']),
                                         f'{flag}/vq_perplexity_%d' % i: stg['perplexity']})
                        line = 'pre_AE:[%06d/%06d], loss_rec=%.3f, loss_vq=%.4f' + ''.join(
                            ', used%d=%%.3f, perplexity%d=%%.1f' % (i, i) for i in range(len(s['stages'])))
                        if 'active' in s:                                                      # quantiser dropout: the rows of every stage
                            for i, v in enumerate(s['active']):
                                info[f'{flag}/vq_active_%d' % i] = v / float(bn.rows)
                            line += ''.join(', active%d=%%.3f' % i for i in range(len(s['active'])))
                    else:
                        info.update({f'{flag}/pre_loss_vq': s['loss_vq'], f'{flag}/vq_used': s['used'] / float(s['K']),
                                     f'{flag}/vq_perplexity': s['perplexity']})
                        line = 'pre_AE:[%06d/%06d], loss_rec=%.3f, loss_vq=%.4f, used=%.3f, perplexity=%.1f'
                    if bn.restart is not None:
                        info[f'{flag}/vq_restarts'] = s['restarts']
                        line += ', restarts=%d'
                    log(line, info)
                elif log:
                    log('pre_AE:[%06d/%06d], loss_rec=%.3f', {f'{flag}/pre_loss_rec': loss_t.item()})    # the only host sync
                if vcfg is not None and ((iteration + 1) % vcfg.every == 0 or iteration + 1 == iters):
                    self.validate(iteration + 1, model_path, flag, keep_state)                 # before this iteration's checkpoint

            def save_codebook(path, iteration):
                """<checkpoint>.vq.npz (.rvq.npz) beside the checkpoint: the file --codebook reads (the codebook's own save, format
                unchanged)."""
                s = bn.stats()
                bn.to_codebook(bn.ckpt_meta(iteration, s)).save(path + bn.ckpt_suffix)

            bn = self.vq
            if bn is not None:
                if resumable or vcfg is not None or parallel.multi_rank():
                    raise ValueError('vq_train cannot be combined with resume, validation or several ranks')
                self.ae.vq = bn
                self.ae._graphs.clear()                                                        # (a step captured without the quantiser)
            try:
                self._loop(hps.enc_pretrain_iters, model_path, 'ae', iteration_fn, start, keep_state,
                           after_save=(save_codebook if bn is not None else None))
            finally:
                if bn is not None:
                    self.ae.vq = None
                    self.ae._graphs.clear()
        elif mode == 'pretrain_C':                                                        # trainer.py:349-382
            start = begin(hps.dis_pretrain_iters)
            if start is None:
                return

            def iteration_fn(iteration, log):
                c, x = self._batch()
                loss_t, corr = self.clf.d_step(x, c)
                if log:
                    log('pre_C:[%06d/%06d], loss_clf=%.2f, acc=%.2f',
                        {f'{flag}/pre_loss_clf': loss_t.item(), f'{flag}/pre_acc': corr.item() / float(c.shape[0])})
            self._loop(hps.dis_pretrain_iters, model_path, 'c', iteration_fn, start, keep_state)
        elif mode == 'train':                                                             # trainer.py:384-465
            start = begin(hps.iters)
            if start is None:
                return

            def iteration_fn(iteration, log):
                if iteration < hps.lat_sched_iters:
                    current_alpha = hps.alpha_enc * (iteration / hps.lat_sched_iters)
                else:
                    current_alpha = hps.alpha_enc
                for step in range(hps.n_latent_steps):                                    # train D
                    c, x = self._batch()
                    loss_t, corr = self.clf.d_step(x, c, alpha_dis=hps.alpha_dis)
                    if log:
                        log('D-%d:[%06d/%06d], loss_clf=%.2f, acc=%.2f',
                            {f'{flag}/D_loss_clf': loss_t.item(), f'{flag}/D_acc': corr.item() / float(c.shape[0])}, (step,))
                c, x = self._batch()                                                      # train G
                l_rec, l_clf, corr = self.clf.g_step(x, c, current_alpha)
                if log:
                    log('G:[%06d/%06d], loss_rec=%.3f, loss_clf=%.2f, alpha=%.2e, acc=%.2f',
                        {f'{flag}/loss_rec': l_rec.item(), f'{flag}/G_loss_clf': l_clf.item(), f'{flag}/alpha': current_alpha,
                         f'{flag}/G_acc': corr.item() / float(c.shape[0])})
            self._loop(hps.iters, model_path, 's1', iteration_fn, start, keep_state)
        elif mode == 'patchGAN':                                                          # trainer.py:467-560
            s2 = self.stage2()
            B = float(hps.batch_size)
            start = begin(hps.patch_iters)
            if start is None:
                return

            def iteration_fn(iteration, log):
                for step in range(hps.n_patch_steps):                                     # train D
                    (_, x_s), (c_t, x_t) = self._duo_batch()
                    r = s2.d_step(x_s, x_t, c_t)
                    if log:
                        log('patch_D-%d:[%06d/%06d], w_dis=%.2f, gp=%.2f, loss_clf=%.2f, acc=%.2f',
                            {f'{flag}/w_dis': r['w_dis'].item(), f'{flag}/gp': r['gp'].item(),
                             f'{flag}/real_loss_clf': r['real_loss_clf'].item(), f'{flag}/real_acc': r['correct'].item() / B}, (step,))
                (_, x_s), (c_t, x_t) = self._duo_batch()                                  # train G
                r = s2.g_step(x_s, x_t, c_t)
                loss_rec = s2.tg_step(x_t, c_t) if target_guided else None                # teacher forcing (trainer.py:535-541)
                if log:
                    log('patch_G:[%06d/%06d], loss_adv=%.2f, loss_clf=%.2f, acc=%.2f, tg_rec=%.3f',
                        {f'{flag}/loss_adv': r['loss_adv'].item(), f'{flag}/fake_loss_clf': r['fake_loss_clf'].item(),
                         f'{flag}/fake_acc': r['correct'].item() / B, f'{flag}/tg_rec': loss_rec.item() if target_guided else 0.000})
            self._loop(hps.patch_iters, model_path, 's2', iteration_fn, start, keep_state)
        elif mode == 't_classify':                                                        # trainer.py:613-643
            if self.g_mode == 'naive':
                self.tclf_labels(torch.zeros(0, dtype=torch.int64))                        # raises: no shift_c
            start = begin(hps.tclf_iters)
            if start is None:
                return
            batch = [self._tclf_batch()]                                                  # the first batch is checked before any launch
            step = self.tclf_step()

            def iteration_fn(iteration, log):
                if batch[0] is None:
                    batch[0] = self._tclf_batch()
                (c, x), batch[0] = batch[0], None
                _, corr = step.step(x, c)
                if log:
                    log('Target Classifier:[%05d/%05d], acc=%.2f', {f'{flag}/acc': corr.item() / float(c.shape[0])})
            self._loop(hps.tclf_iters, model_path, 'tclf', iteration_fn, start, keep_state)
        elif mode == 'autolocker':                                                        # trainer.py:563-611
            s2 = self.stage2(autolocker=True)                                             # ValueError unless multilabel_binary
            start = begin(hps.patch_iters)
            if start is None:
                return

            def iteration_fn(iteration, log):
                (_, x_s), (c_t, x_t) = self._duo_batch()                                  # train G
                loss_reenc = s2.al_step(x_s, c_t)
                loss_rec = s2.tg_step(x_t, c_t) if target_guided else None                # teacher forcing, no clip
                if log:
                    log('patch_G:[%06d/%06d], re_enc=%.3f, tg_rec=%.3f',
                        {f'{flag}/re_enc': loss_reenc.item(), f'{flag}/tg_rec': loss_rec.item() if target_guided else 0.000})
            self._loop(hps.patch_iters, model_path, 's2', iteration_fn, start, keep_state)
        else:
            raise NotImplementedError("mode %r (Tacotron) is outside the path this build covers" % mode)
