"""The end of every training step: the softmax cross-entropy of a classifier head (softmax_ce) and clip_grad_norm_ + Adam over one
net's flat parameter buffer (NetOpt).  These are the only launch sites of zs_softmax_ce, zs_sqnorm and zs_adam_clip."""
import torch

from . import _lib as L
from . import parallel


class NetOpt(object):
    """clip_grad_norm_(net, max_norm) + Adam(lr, betas) (utils.py:53-55, trainer.py:66) over ONE net's flat parameter buffer.
    step(): host step count t, bias correction computed here in double, weights re-packed lazily (mark_dirty).  device_step():
    the count read from device memory and the bias correction computed there (a captured step replays frozen arguments), weights
    re-packed at once.  reduce=True: step() first sums the gradients over ranks itself; reduce=False: the net's owner does.  The
    buffer then holds the SUM over ranks; zs_adam_clip applies the 1/world (grad_scale)."""

    def __init__(self, net, lr, betas=(0.5, 0.9), max_norm=0.0, reduce=True):
        self.net, self.lr, self.betas, self.max_norm, self.t = net, float(lr), betas, max_norm, 0
        flat, _ = net.flat_params()
        self.m, self.v = torch.zeros_like(flat), torch.zeros_like(flat)
        self.sq = torch.zeros(1, dtype=torch.float32, device=flat.device)     # squared gradient norm (device scalar)
        self.part = torch.zeros(1024, dtype=torch.float64, device=flat.device)
        self.reducer = parallel.GradReducer() if reduce else None

    def state_dict(self):
        """{'m', 'v': the moment buffers themselves (device), 't': the host step count}."""
        return {'m': self.m, 'v': self.v, 't': int(self.t)}

    def load_state_dict(self, sd):
        """Restore m, v and t in place (the buffers keep their addresses: a captured step goes on reading them) and mark the
        net's packed weights stale: the caller has just loaded its master weights."""
        for k in ('m', 'v'):
            if tuple(sd[k].shape) != tuple(self.m.shape):
                raise ValueError('optimizer state: %s has %d elements, the net has %d' % (k, sd[k].numel(), self.m.numel()))
        self.m.copy_(sd['m'])
        self.v.copy_(sd['v'])
        self.t = int(sd['t'])
        self.net.mark_dirty()

    def sqnorm(self):
        """The squared norm of the net's gradient into self.sq, on the current stream.  Returns self.sq."""
        _, gflat = self.net.flat_params()
        st = torch.cuda.current_stream(gflat.device).cuda_stream
        L.check(L.lib().zs_sqnorm(L.ptr(gflat), gflat.numel(), L.ptr(self.part), L.ptr(self.sq), st), 'zs_sqnorm')
        return self.sq

    def _adam(self, bc1, bc2, max_norm, step_ptr=None):
        flat, gflat = self.net.flat_params()
        b1, b2 = self.betas
        L.call('zs_adam_clip', 'ZsAdam', torch.cuda.current_stream(flat.device).cuda_stream, p=L.ptr(flat), g=L.ptr(gflat),
               m=L.ptr(self.m), v=L.ptr(self.v), n=flat.numel(), lr=self.lr, beta1=b1, beta2=b2, eps=1e-8, bc1=bc1, bc2=bc2,
               sumsq=L.ptr(self.sq), max_norm=float(max_norm) if max_norm else 0.0, write_clipped_grad=0, step_ptr=step_ptr,
               grad_scale=1.0 / parallel.world_size())

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
        """sqnorm + Adam with the step count at step_ptr (int32, device) + re-pack, on the current stream."""
        self.sqnorm()
        self._adam(1.0, 1.0, self.max_norm, step_ptr=step_ptr)
        self.net.repack()


def softmax_ce(ctx, logits, target, loss, correct, grad_scale=1.0):
    """nn.CrossEntropyLoss (mean) and cal_acc of a classifier head (trainer.py:297-313).  logits fp32 [B, n_class] (rows may be
    strided, columns adjacent) and target int64 [B] on the device; the loss and #correct go to the device scalars `loss` (fp32)
    and `correct` (int32).  Returns grad_scale * dCE/dlogits, fp32 [B, n_class]: a buffer of the classifier's context `ctx`."""
    B, n = logits.shape
    dl = ctx.f32('ce_dlogits_%d_%d' % (B, n), B * n)[:B * n].view(B, n)
    L.call('zs_softmax_ce', 'ZsSoftmaxCE', ctx.stream, logits=L.ptr(logits), ld=logits.stride(0), target=L.ptr(target), B=B,
           n_class=n, loss_out=L.ptr(loss), dlogits=L.ptr(dl), ldg=n, grad_scale=float(grad_scale), correct_out=L.ptr(correct))
    return dl
