"""f64 restatement of the downsampling ModulatedConv2d (stylegan2/model.py:181-277, downsample branch) in the library's
re-associated form, shared by tests/test_modconv_down.py (which pins it to the reference's recorded output on the CPU) and
tests/test_modconv_down_gpu.py (which holds the HIP path to it):

    xb     = upfirdn2d(x, fir, pad=(pad0, pad1))                          pads: stylegan2/model.py:212-216
    y[b,o] = (scale * d[b,o]) * sum_{i,k} W[o,i,k] * (s[b,i] * xb[b,i, 2. + k])
    d[b,o] = rsqrt(sum_i s[b,i]^2 * wsq[o,i] + 1e-8),  wsq = scale^2 sum_k W^2,  s = EqualLinear(style) (bias_init 1)

Plain torch, differentiable to any order, dtype of the inputs (the tests pass float64).
"""
import math

import torch
import torch.nn.functional as F


def down_pads(fir_size: int, k: int):
    p = (fir_size - 2) + (k - 1)
    return (p + 1) // 2, p // 2


def blur(x, fir, pad):
    """upfirdn2d(x, fir, up=1, down=1, pad): zero padding, correlation with the flipped FIR, per channel."""
    c = x.shape[1]
    xp = F.pad(x, (pad[0], pad[1], pad[0], pad[1]))
    kern = torch.flip(fir.to(x.dtype), [0, 1])[None, None].repeat(c, 1, 1, 1)
    return F.conv2d(xp, kern, groups=c)


def styles(style, mw, mb):
    """EqualLinear(style_dim, Cin, bias_init=1) without activation: F.linear(style, W / sqrt(style_dim), bias)."""
    return F.linear(style, mw * (1.0 / math.sqrt(mw.shape[1])), mb)


def modconv_down_s(x, s, w, fir, demodulate=True, eps=1e-8):
    """The layer from the already-transformed style ``s`` [B, Cin]; ``w`` [Cout, Cin, k, k]."""
    cout, cin, k, _ = w.shape
    scale = 1.0 / math.sqrt(cin * k * k)
    xb = blur(x, fir, down_pads(fir.shape[0], k))
    y = F.conv2d(xb * s[:, :, None, None], w, stride=2) * scale
    if demodulate:
        wsq = (w * w).sum((2, 3)) * (scale * scale)
        y = y * torch.rsqrt((s * s) @ wsq.t() + eps)[:, :, None, None]
    return y


def modconv_down(x, style, w5, mw, mb, fir, demodulate=True, eps=1e-8):
    """``w5`` [1, Cout, Cin, k, k] (the reference's parameter), ``style`` [B, style_dim]."""
    return modconv_down_s(x, styles(style, mw, mb), w5[0], fir, demodulate, eps)
