"""fp64 definitions of the stage-2 gather / fold / loss glue (include/zs_amd.h: zs_conv2d_gather, zs_conv2d_fold, zs_conv2d_unpad,
zs_enc_dx_fold, zs_bce_mbv_bwd, zs_gen_combine_bwd, zs_l1_plain), written as the header states them.  The forward operators
copy values from a padded source; each transpose is the explicit scatter of the same index map: it walks the SOURCE side of the
forward (one `+=` per value the forward copied), never the per-output gather of partners that the kernels use.
Arrays are numpy, channels-last [B, H, W, C]; the loops run over positions and taps and are vectorised over batch and channels.
No GPU, no package import: test_patch_ref_host.py checks this module, test_gpu_patch_glue.py checks the kernels against it."""
import numpy as np

REFLECT, ZERO = 'reflect', 'zero'


def src_index(p, n, mode):
    """Index in [0, n) that position p of the padded domain (unpadded coordinates: p < 0 and p >= n are padding) copies, or
    None where zero padding supplies the value."""
    if 0 <= p < n:
        return p
    if mode == ZERO:
        return None
    q = -p if p < 0 else 2 * (n - 1) - p
    assert 0 <= q < n, 'reflect padding must be smaller than the dimension'
    return q


def out_len(n, k, s, pad):
    return (n + 2 * pad - k) // s + 1


def pad_axis(x, axis, pad, mode):
    """x padded by `pad` positions on both sides of `axis`."""
    n = x.shape[axis]
    shape = list(x.shape)
    shape[axis] = n + 2 * pad
    out = np.zeros(shape, dtype=np.float64)
    for u in range(n + 2 * pad):
        i = src_index(u - pad, n, mode)
        if i is not None:
            dst = [slice(None)] * x.ndim
            dst[axis] = u
            src = list(dst)
            src[axis] = i
            out[tuple(dst)] = x[tuple(src)]
    return out


def pad_axis_t(g, axis, pad, mode):
    """Transpose of pad_axis: every padded position adds into the position it copied."""
    n = g.shape[axis] - 2 * pad
    shape = list(g.shape)
    shape[axis] = n
    out = np.zeros(shape, dtype=np.float64)
    for u in range(n + 2 * pad):
        i = src_index(u - pad, n, mode)
        if i is not None:
            src = [slice(None)] * g.ndim
            src[axis] = u
            dst = list(src)
            dst[axis] = i
            out[tuple(dst)] += g[tuple(src)]
    return out


def gather_h(x, k, s, pad, mode, H_out=None):
    """[B, H, W, C] -> [B, H_out, W, k*C]:  out[b, ho, w, kh*C + c] = x[b, pad(s*ho + kh - pad), w, c]"""
    B, H, W, C = x.shape
    H_out = out_len(H, k, s, pad) if H_out is None else H_out
    out = np.zeros((B, H_out, W, k * C), dtype=np.float64)
    for ho in range(H_out):
        for kh in range(k):
            hi = src_index(s * ho + kh - pad, H, mode)
            if hi is not None:
                out[:, ho, :, kh * C:(kh + 1) * C] = x[:, hi]
    return out


def im2col(x, k, s, pad, mode, H_out=None):
    """[B, H, W, C] -> [B, H_out, W_out, k*k*C]:  out[b, ho, wo, (kh*k + kw)*C + c] = x[b, pad(s*ho + kh - pad), pad(s*wo + kw - pad), c]"""
    B, H, W, C = x.shape
    H_out = out_len(H, k, s, pad) if H_out is None else H_out
    W_out = out_len(W, k, s, pad)
    out = np.zeros((B, H_out, W_out, k * k * C), dtype=np.float64)
    for ho in range(H_out):
        for kh in range(k):
            hi = src_index(s * ho + kh - pad, H, mode)
            for wo in range(W_out):
                for kw in range(k):
                    wi = src_index(s * wo + kw - pad, W, mode)
                    if hi is not None and wi is not None:
                        t = kh * k + kw
                        out[:, ho, wo, t * C:(t + 1) * C] = x[:, hi, wi]
    return out


def fold_h(gp, k, s, pad, mode, H_in, Wd):
    """Transpose of  x -> gather_h(pad_axis(x, W))  (the data gradient of a Conv2d as zs_gemm_conv(gather=1) leaves it).
    gp [B, H_out, rows >= Wd + 2 pad, k*C]; rows past Wd + 2 pad (ZsConv2dFold.gp_rows) carry nothing.  -> [B, H_in, Wd, C]"""
    B, H_out, rows, kc = gp.shape
    C = kc // k
    assert kc == k * C and rows >= Wd + 2 * pad
    out = np.zeros((B, H_in, Wd, C), dtype=np.float64)
    for ho in range(H_out):
        for kh in range(k):
            hi = src_index(s * ho + kh - pad, H_in, mode)
            if hi is None:
                continue
            for wp in range(Wd + 2 * pad):
                wi = src_index(wp - pad, Wd, mode)
                if wi is not None:
                    out[:, hi, wi] += gp[:, ho, wp, kh * C:(kh + 1) * C]
    return out


def col2im(gp, k, s, pad, mode, H_in, Wd):
    """Transpose of im2col.  gp [B, H_out, W_out, k*k*C] -> [B, H_in, Wd, C]"""
    B, H_out, W_out, kkc = gp.shape
    C = kkc // (k * k)
    assert kkc == k * k * C and W_out == out_len(Wd, k, s, pad)
    out = np.zeros((B, H_in, Wd, C), dtype=np.float64)
    for ho in range(H_out):
        for kh in range(k):
            hi = src_index(s * ho + kh - pad, H_in, mode)
            if hi is None:
                continue
            for wo in range(W_out):
                for kw in range(k):
                    wi = src_index(s * wo + kw - pad, Wd, mode)
                    if wi is not None:
                        t = kh * k + kw
                        out[:, hi, wi] += gp[:, ho, wo, t * C:(t + 1) * C]
    return out


def class_shape(Hp, Wp, ph, pw):
    return (Hp - ph + 1) // 2, (Wp - pw + 1) // 2


def pad_split(x, pad, mode, Hp, Wp):
    """The forward whose transpose zs_conv2d_unpad is: [B, H, W, C] padded on both axes, cut to its first Hp x Wp positions and
    dealt to the four parity classes -> (g00, g01, g10, g11), class (ph, pw) [B, Hc(ph), Wc(pw), C] holding (2 h2 + ph, 2 w2 + pw)."""
    xp = pad_axis(pad_axis(x, 1, pad, mode), 2, pad, mode)[:, :Hp, :Wp]
    return tuple(np.ascontiguousarray(xp[:, ph::2, pw::2]) for ph in (0, 1) for pw in (0, 1))


def unpad(g00, g01, g10, g11, pad, mode, H, W, Hp, Wp, add=None):
    """out[b, h, w, c] = sum of the class gradients at the padded positions (hp < Hp, wp < Wp) that copied (h, w)  (+ add)"""
    g = {(0, 0): g00, (0, 1): g01, (1, 0): g10, (1, 1): g11}
    for (ph, pw), a in g.items():
        assert a.shape[1:3] == class_shape(Hp, Wp, ph, pw), (a.shape, Hp, Wp, ph, pw)
    B, C = g00.shape[0], g00.shape[3]
    out = np.zeros((B, H, W, C), dtype=np.float64)
    for hp in range(Hp):
        h = src_index(hp - pad, H, mode)
        if h is None:
            continue
        for wp in range(Wp):
            w = src_index(wp - pad, W, mode)
            if w is not None:
                out[:, h, w] += g[(hp & 1, wp & 1)][:, hp >> 1, wp >> 1]
    return out if add is None else out + add


def enc_dx_fold(g, pad, mode, pass_through=None):
    """g [B, T + 2 pad, C] -> dx [B, T, C]: the transpose of padding along T, plus the pass-through rows"""
    out = pad_axis_t(np.asarray(g, dtype=np.float64), 1, pad, mode)
    return out if pass_through is None else out + pass_through


def bce_mbv(x, y, y0, tau, grad_scale):
    """torch.nn.BCELoss (mean, logs clamped at -100) of x against y and the MBV straight-through backward.  x, y, y0: float32
    [rows, E].  1 - x is taken in fp32, as ATen and the kernel take it (the fp64 value of 1 - x for x = 1 - 2^-24 is the same, but
    for x = 1e-7 the fp32 difference is what log() and the denominator see); everything after that is fp64.
    -> (per-element loss [rows, E], dlogits [rows, 2E])"""
    x, y, y0 = (np.asarray(a, dtype=np.float32) for a in (x, y, y0))
    omx = (np.float32(1) - x).astype(np.float64)
    xd, yd, y0d = x.astype(np.float64), y.astype(np.float64), y0.astype(np.float64)
    with np.errstate(divide='ignore'):
        l = -(yd * np.maximum(np.log(xd), -100.0) + (1 - yd) * np.maximum(np.log(omx), -100.0))
    gs = float(np.float32(grad_scale)) if grad_scale != 0 else 1.0
    dx = (xd - yd) / np.maximum(xd * omx, 1e-12) * gs / x.size
    d0 = dx * y0d * (1 - y0d) / float(np.float32(tau))
    return l, np.stack([d0, -d0], axis=-1).reshape(x.shape[0], -1)


def gen_combine_bwd(dx_gen, xd, m, mode, tanh_out):
    dx_gen, xd, m = (np.asarray(a, dtype=np.float64) for a in (dx_gen, xd, m))
    return dx_gen * (xd if mode else 1.0) * ((1 - m * m) if tanh_out else m * (1 - m))


def l1_plain(a, b, scale):
    """-> (mean|a - b|, sign(a - b) * scale / n)"""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return np.abs(d).mean(), np.sign(d) * float(np.float32(scale)) / d.size
