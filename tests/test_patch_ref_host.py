"""The fp64 definitions of tests/patch_ref.py, which test_gpu_patch_glue.py holds the stage-2 glue kernels against: each forward
equals F.pad + F.unfold (torch's own padding and im2col), each transpose satisfies <A x, g> == <x, A^T g> in fp64 to 1e-12
relative, for reflect and zero padding, every (k, stride, pad) the GPU module uses and H_in down to pad + 1.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import patch_ref as R  # noqa: E402

KSP = [(5, 2, 2), (3, 1, 1), (5, 1, 2), (7, 2, 3), (4, 2, 1)]
MODES = [R.REFLECT, R.ZERO]
B, C = 2, 3


def sizes(pad):
    """(H_in, Wd): H_in down to pad + 1; a width that is neither a multiple of the stride nor of the tap count"""
    return [(pad + 1, pad + 1), (pad + 2, 9), (12, 7), (7, pad + 1)]


def torch_pad(x, pad, mode, axes):
    """x [B, H, W, C] float64 -> padded along the given axes of (H, W) by F.pad, still channels-last"""
    t = torch.from_numpy(x).permute(0, 3, 1, 2)                                  # [B, C, H, W]
    ph, pw = (pad if 'h' in axes else 0), (pad if 'w' in axes else 0)
    t = F.pad(t, (pw, pw, ph, ph), mode='reflect' if mode == R.REFLECT else 'constant')
    return t


def rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def rand(rng, *shape):
    return rng.standard_normal(shape)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ksp', KSP, ids=lambda t: 'k%d_s%d_p%d' % t)
def test_forwards_equal_unfold(ksp, mode):
    k, s, pad = ksp
    rng = np.random.default_rng(1)
    for H, W in sizes(pad):
        x = rand(rng, B, H, W, C)
        Ho, Wo = R.out_len(H, k, s, pad), R.out_len(W, k, s, pad)
        # im2col: unfold's channel order is (c, kh, kw), ours (kh, kw, c)
        u = F.unfold(torch_pad(x, pad, mode, 'hw'), (k, k), stride=s).reshape(B, C, k, k, Ho, Wo).permute(0, 4, 5, 2, 3, 1)
        assert np.array_equal(R.im2col(x, k, s, pad, mode), u.reshape(B, Ho, Wo, k * k * C).numpy()), (H, W)
        # gather_h: a k x 1 window of the H-padded image
        u = F.unfold(torch_pad(x, pad, mode, 'h'), (k, 1), stride=(s, 1)).reshape(B, C, k, Ho, W).permute(0, 3, 4, 2, 1)
        assert np.array_equal(R.gather_h(x, k, s, pad, mode), u.reshape(B, Ho, W, k * C).numpy()), (H, W)
        # fewer output rows are a prefix
        if Ho > 1:
            assert np.array_equal(R.gather_h(x, k, s, pad, mode, H_out=Ho - 1), R.gather_h(x, k, s, pad, mode)[:, :Ho - 1])
            assert np.array_equal(R.im2col(x, k, s, pad, mode, H_out=Ho - 1), R.im2col(x, k, s, pad, mode)[:, :Ho - 1])
        # pad_axis itself
        assert np.array_equal(R.pad_axis(R.pad_axis(x, 1, pad, mode), 2, pad, mode), torch_pad(x, pad, mode, 'hw').permute(0, 2, 3, 1).numpy())


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ksp', KSP, ids=lambda t: 'k%d_s%d_p%d' % t)
def test_fold_and_col2im_are_the_transposes(ksp, mode):
    k, s, pad = ksp
    rng = np.random.default_rng(2)
    for H, W in sizes(pad):
        full = R.out_len(H, k, s, pad)
        for Ho in sorted({full, max(1, full - 1)}):
            x = rand(rng, B, H, W, C)
            # fold_h: A = gather_h after padding W; the spare rows of gp (gp_rows) carry values that must not count
            Ax = R.gather_h(R.pad_axis(x, 2, pad, mode), k, s, pad, mode, H_out=Ho)
            for spare in (0, 1):
                g = rand(rng, B, Ho, W + 2 * pad + spare, k * C)
                lhs = float((Ax * g[:, :, :W + 2 * pad]).sum())
                rhs = float((x * R.fold_h(g, k, s, pad, mode, H, W)).sum())
                print('fold_h H %d W %d Ho %d spare %d: %.3g' % (H, W, Ho, spare, rel(lhs, rhs)))
                assert rel(lhs, rhs) <= 1e-12
            Ax = R.im2col(x, k, s, pad, mode, H_out=Ho)
            g = rand(rng, *Ax.shape)
            lhs, rhs = float((Ax * g).sum()), float((x * R.col2im(g, k, s, pad, mode, H, W)).sum())
            print('col2im H %d W %d Ho %d: %.3g' % (H, W, Ho, rel(lhs, rhs)))
            assert rel(lhs, rhs) <= 1e-12


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('pad', [1, 2])
def test_unpad_is_the_transpose_of_pad_and_split(pad, mode):
    rng = np.random.default_rng(3)
    for H, W in [(pad + 1, pad + 1), (pad + 2, 6), (6, 5), (5, pad + 1)]:
        for dh, dw in [(0, 0), (1, 0), (0, 1), (1, 1)]:                           # Hp / Wp at H + 2 pad and one below: odd and even
            Hp, Wp = H + 2 * pad - dh, W + 2 * pad - dw
            x = rand(rng, B, H, W, C)
            Ax = R.pad_split(x, pad, mode, Hp, Wp)
            assert sum(a.size for a in Ax) == B * Hp * Wp * C
            g = [rand(rng, *a.shape) for a in Ax]
            add = rand(rng, B, H, W, C)
            lhs = float(sum((a * b).sum() for a, b in zip(Ax, g)))
            rhs = float((x * R.unpad(*g, pad, mode, H, W, Hp, Wp)).sum())
            assert rel(lhs, rhs) <= 1e-12, (H, W, Hp, Wp)
            assert np.array_equal(R.unpad(*g, pad, mode, H, W, Hp, Wp, add=add), R.unpad(*g, pad, mode, H, W, Hp, Wp) + add)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('pad', [0, 1, 3])
def test_enc_dx_fold_is_the_transpose_of_padding(pad, mode):
    rng = np.random.default_rng(4)
    for T in sorted({pad + 1, pad + 2, 2 * pad + 1, 11}):
        x, g, pt = rand(rng, B, T, C), rand(rng, B, T + 2 * pad, C), rand(rng, B, T, C)
        Ax = R.pad_axis(x, 1, pad, mode)
        ref = F.pad(torch.from_numpy(x).permute(0, 2, 1), (pad, pad), mode='reflect' if mode == R.REFLECT else 'constant').permute(0, 2, 1).numpy()
        assert np.array_equal(Ax, ref)
        lhs, rhs = float((Ax * g).sum()), float((x * R.enc_dx_fold(g, pad, mode)).sum())
        assert rel(lhs, rhs) <= 1e-12, T
        assert np.array_equal(R.enc_dx_fold(g, pad, mode, pass_through=pt), R.enc_dx_fold(g, pad, mode) + pt)
        if mode == R.ZERO:
            assert np.array_equal(R.enc_dx_fold(g, pad, mode), g[:, pad:pad + T])


def test_bce_mbv_against_autograd():
    """loss and d loss / d x against torch's fp64 BCELoss; the MBV factor against its formula; the hard-unit statement of the header"""
    rng = np.random.default_rng(5)
    rows, E, tau, gs = 7, 5, 0.7, 0.5
    x = rng.uniform(0.02, 0.98, (rows, E)).astype(np.float32)
    y = (rng.uniform(size=(rows, E)) < 0.5).astype(np.float32)
    y0 = rng.uniform(0.02, 0.98, (rows, E)).astype(np.float32)
    l, dl = R.bce_mbv(x, y, y0, tau, gs)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    loss = F.binary_cross_entropy(xt, torch.from_numpy(y).double())
    loss.backward()
    assert rel(float(l.mean()), loss.item()) <= 1e-7               # (1 - x in fp32: 2^-24 relative in log(1 - x))
    d0 = xt.grad.numpy() * gs * y0.astype(np.float64) * (1 - y0.astype(np.float64)) / float(np.float32(tau))
    assert np.allclose(dl[:, 0::2], d0, rtol=2e-7, atol=0) and np.array_equal(dl[:, 1::2], -dl[:, 0::2])
    # hard units: 100 per mismatch, +-1e12 / N at the mismatches, 0 elsewhere
    xh = (rng.uniform(size=(rows, E)) < 0.5).astype(np.float32)
    l, dl = R.bce_mbv(xh, y, y0, tau, 0.0)
    mis = xh != y
    assert np.array_equal(l, 100.0 * mis)
    want = np.where(mis, (xh.astype(np.float64) - y) * 1e12 / (rows * E), 0.0) * y0.astype(np.float64) * (1 - y0.astype(np.float64)) / float(np.float32(tau))
    assert np.allclose(dl[:, 0::2], want, rtol=1e-15, atol=0)


def test_gen_combine_bwd_and_l1_plain_against_autograd():
    rng = np.random.default_rng(6)
    xd, pre, dxg = rand(rng, 4, 9), rand(rng, 4, 9), rand(rng, 4, 9)
    for mode in (0, 1):
        for tanh_out in (0, 1):
            p = torch.from_numpy(pre).requires_grad_(True)
            m = torch.tanh(p) if tanh_out else torch.sigmoid(p)
            xg = torch.from_numpy(xd) + (torch.from_numpy(xd) * m if mode else m)          # Trainer.gen_step
            xg.backward(torch.from_numpy(dxg))
            assert np.allclose(R.gen_combine_bwd(dxg, xd, m.detach().numpy(), mode, tanh_out), p.grad.numpy(), rtol=1e-12, atol=1e-15)
    a, b = rand(rng, 33), rand(rng, 33)
    b[::8] = a[::8]
    at = torch.from_numpy(a).requires_grad_(True)
    loss = (at - torch.from_numpy(b)).abs().mean()
    (loss * 0.3).backward()
    l, d = R.l1_plain(a, b, 0.3)
    assert rel(l, loss.item()) <= 1e-15 and np.allclose(d, at.grad.numpy(), rtol=1e-7, atol=0) and (d[::8] == 0).all()
