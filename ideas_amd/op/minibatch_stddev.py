"""``minibatch_stddev`` on the HIP kernels ``ideas_mbstd_fwd`` / ``_bwd`` / ``_bwd2`` (csrc/minibatch_stddev.hip).

The block ``stylegan2.model.Discriminator.forward`` computes inline (stylegan2/model.py:697-705): with ``G = min(B, group)`` and
``M = B // G`` the batch is viewed as ``[G, M, feat, C // feat, H, W]`` (the group index is the outer one), the biased standard
deviation over the G samples is averaged over each channel chunk and all pixels, and the ``feat`` statistics are appended to
every sample as constant channels.  R1 differentiates through it, so the backward is a Function of its own whose backward is the
third kernel (the shape of ``UpFirDn2d`` / ``UpFirDn2dBackward``); that last step is ``once_differentiable``.  Accepts
NCHW-contiguous and channels_last f32 / bf16 tensors; the output is channels_last.  No CPU branch.
"""
from __future__ import annotations

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib

CL = torch.channels_last


def _nhwc(t: torch.Tensor, dtype) -> torch.Tensor:
    t = t if t.dtype == dtype else t.to(dtype)
    return t if t.is_contiguous(memory_format=CL) else t.contiguous(memory_format=CL)


def _workspace(x: torch.Tensor, m: int, feat: int) -> torch.Tensor:
    return torch.empty(m * feat * _lib.MBSTD_MAX_PARTIALS, device=x.device, dtype=torch.float64)


def _dims(x, group):
    b, c, h, w = x.shape
    return b, c, h, w, b // min(b, group)


class MinibatchStdDevBackward(Function):
    @staticmethod
    def forward(ctx, gout, x, group, feat, eps):
        b, c, h, w, m = _dims(x, group)
        gout = _nhwc(gout, x.dtype)
        gx = torch.empty_like(x)
        a = torch.empty(m * feat, device=x.device, dtype=torch.float32)
        rc = _lib.load().ideas_mbstd_bwd(_lib.ptr(gx), _lib.ptr(a), _lib.ptr(gout), _lib.ptr(x), b, c, h, w, group, feat, eps,
                                         _lib.act_dtype(x), _lib.stream_ptr())
        _lib.check(rc, "ideas_mbstd_bwd")
        ctx.save_for_backward(x, a)
        ctx.group, ctx.feat, ctx.eps = group, feat, eps
        return gx

    @staticmethod
    @once_differentiable
    def backward(ctx, ggx):
        x, a = ctx.saved_tensors
        b, c, h, w, m = _dims(x, ctx.group)
        ggx = _nhwc(ggx, x.dtype)
        dgout = torch.empty((b, c + ctx.feat, h, w), device=x.device, dtype=x.dtype, memory_format=CL)
        dx = torch.empty_like(x)
        rc = _lib.load().ideas_mbstd_bwd2(_lib.ptr(dgout), _lib.ptr(dx), _lib.ptr(_workspace(x, m, ctx.feat)), _lib.ptr(ggx), _lib.ptr(x),
                                          _lib.ptr(a), b, c, h, w, ctx.group, ctx.feat, ctx.eps, _lib.act_dtype(x), _lib.stream_ptr())
        _lib.check(rc, "ideas_mbstd_bwd2")
        return dgout, dx, None, None, None


class MinibatchStdDev(Function):
    @staticmethod
    def forward(ctx, x, group, feat, eps):
        b, c, h, w, m = _dims(x, group)                  # x: channels_last (minibatch_stddev converts in front of the node)
        out = torch.empty((b, c + feat, h, w), device=x.device, dtype=x.dtype, memory_format=CL)
        rc = _lib.load().ideas_mbstd_fwd(_lib.ptr(out), _lib.ptr(_workspace(x, m, feat)), _lib.ptr(x), b, c, h, w, group, feat, eps,
                                         _lib.act_dtype(x), _lib.stream_ptr())
        _lib.check(rc, "ideas_mbstd_fwd")
        ctx.save_for_backward(x)
        ctx.group, ctx.feat, ctx.eps = group, feat, eps
        return out

    @staticmethod
    def backward(ctx, gout):
        (x,) = ctx.saved_tensors
        return MinibatchStdDevBackward.apply(gout, x, ctx.group, ctx.feat, ctx.eps), None, None, None


def minibatch_stddev(x: torch.Tensor, group: int = 4, feat: int = 1, eps: float = 1e-8) -> torch.Tensor:
    """``cat([x, stddev statistics], 1)`` of the StyleGAN2 discriminator: ``[B, C, H, W] -> [B, C + feat, H, W]`` (channels_last)."""
    if x.dim() != 4:
        raise RuntimeError("minibatch_stddev expects a 4-D [B, C, H, W] tensor")
    group, feat = int(group), int(feat)
    b, c = x.shape[0], x.shape[1]
    if group < 1 or feat < 1 or b < 1:
        raise RuntimeError(f"minibatch_stddev: group = {group}, feat = {feat} and the batch size {b} must be positive")
    g = min(b, group)
    if b % g != 0:
        raise RuntimeError(f"minibatch_stddev: the batch size {b} is not divisible by the group size {g}")
    if c % feat != 0:
        raise RuntimeError(f"minibatch_stddev: {c} channels are not divisible by feat = {feat}")
    _lib.require_cuda(x)
    _lib.act_dtype(x)
    if g > 16:
        raise RuntimeError(f"minibatch_stddev: groups of more than 16 samples are not implemented (got {g})")
    # the layout conversion stays outside the node: the tensor the node saves is then its own input, so the backward's backward
    # hands d x on to whatever produced x
    x = x if x.is_contiguous(memory_format=CL) else x.contiguous(memory_format=CL)
    return MinibatchStdDev.apply(x, group, feat, float(eps))
