"""The end of every training step: the softmax cross-entropy of a classifier head (softmax_ce) and clip_grad_norm_ + Adam over one
net's flat parameter buffer (NetOpt).  These are the only launch sites of zs_softmax_ce, zs_sqnorm, zs_adam_clip and zs_adam_pack."""
import ctypes

import torch

from . import _lib as L
from . import parallel
from .layers import pack_operands

MAX_TAPS = 7          # zs_adam_pack's weight tiles (PK_MAX_TAPS of the pack kernels)


def _in_flat(flat, t):
    return t.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() and t.device == flat.device


def plan_jobs(flat, weights, vectors):
    """The work list of zs_adam_pack over the flat buffer `flat` for the described operands (layers.weight_operand /
    vector_operand).  Returns (jobs, rest_weights, rest_vectors): jobs = dicts(kind 'weight' | 'vector' | 'range', off, len[, op])
    sorted by off and covering [0, flat.numel()) exactly once (check_cover); rest_* = what the fused launch cannot express as
    "every element of this parameter exactly once" and a zs_pack_weight_batch / zs_copy_vec_batch behind it re-packs: a
    parameter that is not dense in the flat buffer or has more than MAX_TAPS taps, a second layer over the same parameter, and
    `raw` views.  Such a parameter is updated by a range job.  Offsets and shapes only: no pointer is read."""
    jobs, rest_w, rest_v, taken = [], [], [], set()

    def dense(t, shape_strides):
        return _in_flat(flat, t) and t.storage_offset() not in taken and shape_strides

    for op in weights:
        w, (so, si, sj), k = op['w'], op['strides'], op['taps']
        ok = op['views'] and k <= MAX_TAPS and w.numel() == op['Cout'] * op['Cin'] * k and w.is_contiguous() and \
            (so, si) == (op['Cin'] * k, k) and (sj == 1 or k == 1)
        if dense(w, ok):
            taken.add(w.storage_offset())
            jobs.append(dict(kind='weight', off=w.storage_offset(), len=w.numel(), op=op))
            if op['raw']:
                rest_w.append(dict(op, views=[]))
        else:
            rest_w.append(op)
    for vc in vectors:
        b = vc['src']
        if dense(b, b.is_contiguous() and len(vc['copies']) <= 2):
            taken.add(b.storage_offset())
            jobs.append(dict(kind='vector', off=b.storage_offset(), len=b.numel(), op=vc))
        else:
            rest_v.append(vc)
    jobs.sort(key=lambda j: j['off'])
    out, end = [], 0
    for j in jobs:                                   # everything between them: other biases, embeddings, alignment gaps
        if j['off'] > end:
            out.append(dict(kind='range', off=end, len=j['off'] - end))
        out.append(j)
        end = j['off'] + j['len']
    if end < flat.numel():
        out.append(dict(kind='range', off=end, len=flat.numel() - end))
    check_cover(out, flat.numel())
    return out, rest_w, rest_v


def check_cover(jobs, n):
    """ZsError unless the jobs, in order, cover [0, n) exactly once: sorted, no overlap, no hole."""
    end = 0
    for i, j in enumerate(jobs):
        if j['len'] <= 0 or j['off'] != end:
            raise L.ZsError('adam_pack plan: job %d (%s) covers [%d, %d) but the jobs before it end at %d (%s)' %
                            (i, j['kind'], j['off'], j['off'] + j['len'], end, 'overlap' if j['off'] < end else 'hole'))
        end = j['off'] + j['len']
    if end != n:
        raise L.ZsError('adam_pack plan: the jobs cover [0, %d) of a buffer of %d elements' % (end, n))


class AdamPackPlan(object):
    """plan_jobs as the ZsAdamPackJob array of zs_adam_pack (host copy + the same bytes on the device) and the re-pack of the
    rest.  The pointers are static: a captured step replays the launch."""

    def __init__(self, flat, ctx, weights, vectors):
        self.ctx = ctx
        jobs, self.rest_w, self.rest_v = plan_jobs(flat, weights, vectors)
        J, V = L.STRUCTS['ZsAdamPackJob'], L.STRUCTS['ZsAdamPackView']
        self._keep = []                                        # device tensors the views point to (inverse permutations)
        arr = (J * len(jobs))()
        tiles = L.lib().zs_adam_pack_tiles
        total = 0
        for a, j in zip(arr, jobs):
            a.kind = {'weight': L.ZS_APJ_WEIGHT, 'vector': L.ZS_APJ_VECTOR, 'range': L.ZS_APJ_RANGE}[j['kind']]
            a.dtype, a.off, a.len = ctx.dt, j['off'], j['len']
            op = j.get('op')
            if j['kind'] == 'weight':
                a.Cout, a.Cin, a.taps, a.co_split2, a.n_views = op['Cout'], op['Cin'], op['taps'], op['co_split2'], len(op['views'])
                for i, v in enumerate(op['views']):
                    inv = None
                    if v['row_perm'] is not None:
                        inv = torch.empty_like(v['row_perm'])
                        inv[v['row_perm'].long()] = torch.arange(inv.numel(), dtype=inv.dtype, device=inv.device)
                        self._keep.append(inv)
                    a.view[i] = V(dst=L.ptr(v['dst'], v['dst_off']), ldw=v['ldw'], dst_elems=v['dst'].numel() - v['dst_off'],
                                  transpose=v['transpose'], inner_pad=v['inner_pad'], row_offset=v['row_offset'],
                                  col_offset=v['col_offset'], parity=int(v['parity']), row_inv=L.ptr(inv))
            elif j['kind'] == 'vector':
                a.n_views = len(op['copies'])
                for i, cp in enumerate(op['copies']):
                    a.view[i] = V(dst=L.ptr(cp['dst'], cp['dst_off']), ldw=1, dst_elems=cp['dst'].numel() - cp['dst_off'],
                                  vlen=cp['n'], src_offset=cp['src_offset'], src_stride=cp['src_stride'])
            a.tile_start = total
            n = tiles(ctypes.addressof(a))
            if n <= 0:
                L.check(n or -1, 'zs_adam_pack_tiles')
            total += n
        self.jobs, self.n, self.tiles = arr, len(jobs), total
        self.jobs_dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(flat.device)

    def launch(self, adam, part, n_part, stream):
        """zs_adam_pack with the ZsAdam struct `adam`, then the re-pack of what the fused launch does not cover."""
        L.check(L.lib().zs_adam_pack(ctypes.addressof(adam), ctypes.addressof(self.jobs), L.ptr(self.jobs_dev), self.n, part, n_part,
                                     stream), 'zs_adam_pack')
        if self.rest_w or self.rest_v:
            with L.pack_batch(stream):
                pack_operands(self.ctx, self.rest_w, self.rest_v)


def check_ema(decay):
    """None (no average), or the decay of a weight average as a float: ValueError unless 0 <= decay < 1."""
    if decay is None:
        return None
    decay = float(decay)
    if not 0.0 <= decay < 1.0:                       # NaN fails too
        raise ValueError('ema: the decay must lie in [0, 1) (got %r)' % decay)
    return decay


class NetOpt(object):
    """clip_grad_norm_(net, max_norm) + Adam(lr, betas) (utils.py:53-55, trainer.py:66) over ONE net's flat parameter buffer.
    step(): host step count t, bias correction computed here in double, weights re-packed lazily (mark_dirty).  device_step():
    the count read from device memory and the bias correction computed there (a captured step replays frozen arguments), weights
    re-packed at once.  reduce=True: step() first sums the gradients over ranks itself; reduce=False: the net's owner does.  The
    buffer then holds the SUM over ranks; zs_adam_clip applies the 1/world (grad_scale).
    ema: None, or the decay in [0, 1) of an exponential moving average of the weights, self.ema (fp32, the flat buffer's
    length, a copy of the weights at first): every update, on whichever path, moves it inside the Adam launch itself
    (ZsAdam.ema).  After the weights were loaded or broadcast: reset_ema()."""

    def __init__(self, net, lr, betas=(0.5, 0.9), max_norm=0.0, reduce=True, ema=None):
        self.net, self.lr, self.betas, self.max_norm, self.t = net, float(lr), betas, max_norm, 0
        flat, _ = net.flat_params()
        self.m, self.v = torch.zeros_like(flat), torch.zeros_like(flat)
        self.ema_decay = check_ema(ema)
        self.ema = flat.detach().clone() if self.ema_decay is not None else None
        self.sq = torch.zeros(1, dtype=torch.float32, device=flat.device)     # squared gradient norm (device scalar)
        self.part = torch.zeros(1024, dtype=torch.float64, device=flat.device)
        self.reducer = parallel.GradReducer() if reduce else None

    def reset_ema(self):
        """ema = the weights as they are now, in place (no-op without an average)."""
        if self.ema is not None:
            self.ema.copy_(self.net.flat_params()[0].detach())

    def state_dict(self):
        """{'m', 'v': the moment buffers themselves (device), 't': the host step count} and, with an average, 'ema': its buffer."""
        sd = {'m': self.m, 'v': self.v, 't': int(self.t)}
        if self.ema is not None:
            sd['ema'] = self.ema
        return sd

    def load_state_dict(self, sd):
        """Restore m, v, t and the average in place (the buffers keep their addresses: a captured step goes on reading them) and
        mark the net's packed weights stale: the caller has just loaded its master weights.  ValueError, before anything is
        changed, when the state has an average and this optimizer has none, or the other way round."""
        if ('ema' in sd) != (self.ema is not None):
            raise ValueError('optimizer state: ema is %s in the state, %s in this optimizer' %
                             ('on' if 'ema' in sd else 'off', 'on' if self.ema is not None else 'off'))
        for k in ('m', 'v') + (('ema',) if self.ema is not None else ()):
            if tuple(sd[k].shape) != tuple(self.m.shape):
                raise ValueError('optimizer state: %s has %d elements, the net has %d' % (k, sd[k].numel(), self.m.numel()))
        self.m.copy_(sd['m'])
        self.v.copy_(sd['v'])
        if self.ema is not None:
            self.ema.copy_(sd['ema'])
        self.t = int(sd['t'])
        self.net.mark_dirty()

    def sqnorm(self):
        """The squared norm of the net's gradient into self.sq, on the current stream.  Returns self.sq."""
        _, gflat = self.net.flat_params()
        st = torch.cuda.current_stream(gflat.device).cuda_stream
        L.check(L.lib().zs_sqnorm(L.ptr(gflat), gflat.numel(), L.ptr(self.part), L.ptr(self.sq), st), 'zs_sqnorm')
        return self.sq

    def _adam_args(self, bc1, bc2, max_norm, step_ptr=None):
        flat, gflat = self.net.flat_params()
        b1, b2 = self.betas
        return dict(p=L.ptr(flat), g=L.ptr(gflat), m=L.ptr(self.m), v=L.ptr(self.v), n=flat.numel(), lr=self.lr, beta1=b1, beta2=b2,
                    eps=1e-8, bc1=bc1, bc2=bc2, sumsq=L.ptr(self.sq), max_norm=float(max_norm) if max_norm else 0.0,
                    write_clipped_grad=0, step_ptr=step_ptr, grad_scale=1.0 / parallel.world_size(), ema=L.ptr(self.ema),
                    ema_decay=self.ema_decay)

    def _adam(self, bc1, bc2, max_norm, step_ptr=None):
        L.call('zs_adam_clip', 'ZsAdam', torch.cuda.current_stream(self.m.device).cuda_stream,
               **self._adam_args(bc1, bc2, max_norm, step_ptr))

    def adam(self, t, max_norm=None):
        """clip + Adam step number t (host-side bias correction) with the norm already in self.sq, then mark_dirty."""
        b1, b2 = self.betas
        self._adam(1.0 - b1 ** t, 1.0 - b2 ** t, self.max_norm if max_norm is None else max_norm)
        self.net.mark_dirty()

    def step(self, max_norm=None):
        """[all-reduce] + sqnorm + Adam with the host-counted step.  max_norm: this step's clip (default: the constructor's)."""
        if self.reducer is not None and parallel.world_size() > 1:
            self.reducer.start(self.net.flat_params()[1])
            self.reducer.finish()
        self.sqnorm()
        self.t += 1
        self.adam(self.t, max_norm)

    def device_step(self, step_ptr):
        """Clip + Adam with the step count at step_ptr (int32, device) and the re-pack of the net's GEMM operands, on the current
        stream.  With the "adam_pack" knob and a net whose engine describes its operands: the first stage of the norm and ONE
        zs_adam_pack launch (it finishes the norm, updates and writes the packed views).  Otherwise sqnorm + zs_adam_clip + a
        full re-pack."""
        plan = self.net.adam_pack_plan() if L.get_option('adam_pack') else None
        if plan is None:
            self.sqnorm()
            self._adam(1.0, 1.0, self.max_norm, step_ptr=step_ptr)
            self.net.repack()
            return
        _, gflat = self.net.flat_params()
        st = torch.cuda.current_stream(gflat.device).cuda_stream
        n_part = L.lib().zs_sqnorm_stage1(L.ptr(gflat), gflat.numel(), L.ptr(self.part), st)
        if n_part <= 0:
            L.check(n_part or -1, 'zs_sqnorm_stage1')
        kw = self._adam_args(1.0, 1.0, self.max_norm, step_ptr=step_ptr)
        adam = L.STRUCTS['ZsAdam'](**{k: v for k, v in kw.items() if v is not None})
        plan.launch(adam, L.ptr(self.part), n_part, st)
        self.net.mark_packed()


def softmax_ce(ctx, logits, target, loss, correct, grad_scale=1.0):
    """nn.CrossEntropyLoss (mean) and cal_acc of a classifier head (trainer.py:297-313).  logits fp32 [B, n_class] (rows may be
    strided, columns adjacent) and target int64 [B] on the device; the loss and #correct go to the device scalars `loss` (fp32)
    and `correct` (int32).  Returns grad_scale * dCE/dlogits, fp32 [B, n_class]: a buffer of the classifier's context `ctx`."""
    B, n = logits.shape
    dl = ctx.f32('ce_dlogits_%d_%d' % (B, n), B * n)[:B * n].view(B, n)
    L.call('zs_softmax_ce', 'ZsSoftmaxCE', ctx.stream, logits=L.ptr(logits), ld=logits.stride(0), target=L.ptr(target), B=B,
           n_class=n, loss_out=L.ptr(loss), dlogits=L.ptr(dl), ldg=n, grad_scale=float(grad_scale), correct_out=L.ptr(correct))
    return dl
