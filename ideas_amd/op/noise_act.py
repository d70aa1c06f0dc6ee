"""``noise_bias_act`` on the HIP kernels ``ideas_noise_bias_act`` / ``ideas_noise_bias_act_bwd`` (csrc/noise_act.hip).

The tail of the reference's ``StyledConv`` (stylegan2/model.py:335-341): ``NoiseInjection`` (``out + weight * noise``, :280-291), then
the ``FusedLeakyReLU``'s bias add and activation -- three passes over the feature map there, one here:

    out = leaky_relu(x + noise_weight * noise + bias[c], negative_slope) * scale

``noise`` is ``[B, 1, H, W]`` or ``[1, 1, H, W]`` (the generator's registered buffers broadcast over the batch); ``noise_weight`` is the
one-element ``NoiseInjection.weight`` and is read on the device.  The backward is one pass as well (gx, the bias gradient, the
scalar weight gradient without floating-point atomics and, where the noise is being optimised, its gradient); it is
``once_differentiable``: inside ``op.modulated_conv.second_order()`` (the path-length regulariser differentiates the synthesis
network twice) the op is the composition ``fused_leaky_relu(x + noise_weight * noise, bias, ...)``, as it is for f16 / f64 tensors.
Accepts NCHW-contiguous and channels_last tensors; the output is channels_last.  No CPU branch.
"""
from __future__ import annotations

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib
from .fused_act import bias_sink, fused_leaky_relu

CL = torch.channels_last


def _nhwc(t: torch.Tensor, dtype) -> torch.Tensor:
    t = t if t.dtype == dtype else t.to(dtype)
    return t if t.is_contiguous(memory_format=CL) else t.contiguous(memory_format=CL)


def _f32c(t: torch.Tensor) -> torch.Tensor:
    t = t if t.dtype == torch.float32 else t.float()
    return t if t.is_contiguous() else t.contiguous()


class _NoiseBiasAct(Function):
    @staticmethod
    def forward(ctx, x, noise, noise_weight, bias, slope: float, scale: float):
        x = _nhwc(x, x.dtype)
        b, c, h, w = x.shape
        nz, nw, bs = _f32c(noise), _f32c(noise_weight), _f32c(bias)
        out = torch.empty_like(x)
        rc = _lib.load().ideas_noise_bias_act(_lib.ptr(out), _lib.ptr(x), _lib.ptr(nz), _lib.ptr(nw), _lib.ptr(bs), b, c, h, w, nz.shape[0],
                                              slope, scale, _lib.act_dtype(x), _lib.stream_ptr())
        _lib.check(rc, "ideas_noise_bias_act")
        ctx.slope, ctx.scale = slope, scale
        ctx.bias_ref = bias
        ctx.noise_meta, ctx.nw_meta, ctx.x_dtype = (noise.dtype, tuple(noise.shape)), (noise_weight.dtype, tuple(noise_weight.shape)), x.dtype
        ctx.save_for_backward(out, nz, nw)
        return out

    @staticmethod
    @once_differentiable          # raw kernels: a create_graph pass must run inside second_order() and raises otherwise
    def backward(ctx, gy):
        out, nz, nw = ctx.saved_tensors
        b, c, h, w = out.shape
        need_x, need_n, need_w, need_b = ctx.needs_input_grad[:4]
        gy = _nhwc(gy, out.dtype)
        gx = torch.empty_like(out)
        gb = tgt = None
        if need_b:
            tgt = bias_sink(ctx.bias_ref)      # gradient sink: the kernel adds the bias gradient straight into bias.grad
            gb = tgt if tgt is not None else torch.zeros(c, device=out.device, dtype=torch.float32)
        gnw = torch.empty(1, device=out.device, dtype=torch.float32)
        gn = torch.empty_like(nz) if need_n else None
        fold = need_n and nz.shape[0] == 1 and b > 1
        ws = torch.empty(_lib.NOISE_ACT_MAX_PARTIALS + ((b * h * w + 1) // 2 if fold else 0), device=out.device, dtype=torch.float64)
        rc = _lib.load().ideas_noise_bias_act_bwd(_lib.ptr(gx), _lib.ptr(gb), _lib.ptr(gnw), _lib.ptr(gn), _lib.ptr(ws), _lib.ptr(gy),
                                                  _lib.ptr(out), _lib.ptr(nz), _lib.ptr(nw), b, c, h, w, nz.shape[0], ctx.slope, ctx.scale,
                                                  _lib.act_dtype(out), _lib.stream_ptr())
        _lib.check(rc, "ideas_noise_bias_act_bwd")
        if gn is not None:
            gn = gn.to(ctx.noise_meta[0]).reshape(ctx.noise_meta[1])
        gw = gnw.to(ctx.nw_meta[0]).reshape(ctx.nw_meta[1]) if need_w else None
        if gb is not None:
            gb = None if tgt is not None else gb.to(ctx.bias_ref.dtype).reshape(ctx.bias_ref.shape)
        return (gx if need_x else None), gn, gw, gb, None, None


def noise_bias_act(x: torch.Tensor, noise: torch.Tensor, noise_weight: torch.Tensor, bias: torch.Tensor, negative_slope: float = 0.2,
                   scale: float = 2 ** 0.5) -> torch.Tensor:
    """``fused_leaky_relu(x + noise_weight * noise, bias, negative_slope, scale)`` in one pass over ``x`` ([B, C, H, W])."""
    if x.dim() != 4:
        raise RuntimeError("noise_bias_act expects a 4-D [B, C, H, W] tensor")
    b, c, h, w = x.shape
    if noise.dim() != 4 or noise.shape[1] != 1 or tuple(noise.shape[2:]) != (h, w) or noise.shape[0] not in (1, b):
        raise RuntimeError(f"noise_bias_act: noise must be [{b} or 1, 1, {h}, {w}], got {tuple(noise.shape)}")
    if noise_weight.numel() != 1:
        raise RuntimeError(f"noise_bias_act: noise_weight must have one element, got {tuple(noise_weight.shape)}")
    if bias.numel() != c:
        raise RuntimeError(f"noise_bias_act: bias has {bias.numel()} elements, expected {c}")
    _lib.require_cuda(x, noise, noise_weight, bias)
    from .modulated_conv import _SECOND_ORDER
    if (_SECOND_ORDER[0] and torch.is_grad_enabled()) or x.dtype in (torch.float16, torch.float64):
        _lib.op_dtype(x)
        inj = noise_weight.view(1, 1, 1, 1) * noise
        return fused_leaky_relu(x + (inj if inj.dtype == x.dtype else inj.to(x.dtype)), bias, negative_slope, scale)
    _lib.act_dtype(x)
    if x.numel() == 0:
        return torch.empty_like(x)
    return _NoiseBiasAct.apply(x, noise, noise_weight, bias, float(negative_slope), float(scale))
