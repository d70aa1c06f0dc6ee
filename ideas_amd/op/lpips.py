"""``max_pool2x2`` and ``lpips_layer`` on the HIP kernels of csrc/lpips.hip: the two pieces of the LPIPS (VGG) perceptual distance
that the conv family does not cover.

``max_pool2x2(x)`` is ``F.max_pool2d(x, 2, 2)`` (the four pools of torchvision's VGG16 ``features``): ties go to the first element of
the window, a NaN is the maximum, an odd trailing row or column belongs to no window and gets a zero gradient.

``lpips_layer(f0, f1, w)`` is the head of one tap (stylegan2/lpips/networks_basic.py:70-78 with ``spatial=False``; ``normalize_tensor``
of lpips/__init__.py:42-44) in one pass instead of about ten elementwise / reduction launches:

    u_i = f_i / (sqrt(sum_c f_i^2) + 1e-10);   d[b] = mean_p sum_c w[c] (u_0 - u_1)^2          -> [B], float32

One deliberate difference from the reference: a pixel whose features are all zero has norm 0, where the reference's backward
evaluates 0/0 in sqrt's derivative and returns NaN for the pixel; here the pixel's gradient is zero.

Both are ``once_differentiable``: inside ``op.modulated_conv.second_order()``, and for f16 / f64 tensors, they are the plain torch
compositions (``max_pool2x2_composition`` / ``lpips_layer_composition``).  Accept NCHW-contiguous and channels_last tensors; the
pool's output is channels_last.  No CPU branch.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib

CL = torch.channels_last
EPS = 1e-10


def _nhwc(t: torch.Tensor, dtype) -> torch.Tensor:
    t = t if t.dtype == dtype else t.to(dtype)
    return t if t.is_contiguous(memory_format=CL) else t.contiguous(memory_format=CL)


def _use_composition(x: torch.Tensor) -> bool:
    from .modulated_conv import _SECOND_ORDER
    return (_SECOND_ORDER[0] and torch.is_grad_enabled()) or x.dtype in (torch.float16, torch.float64)


class _MaxPool2x2(Function):
    @staticmethod
    def forward(ctx, x):
        x = _nhwc(x, x.dtype)
        b, c, h, w = x.shape
        y = torch.empty((b, c, h // 2, w // 2), device=x.device, dtype=x.dtype, memory_format=CL)
        rc = _lib.load().ideas_maxpool2x2_fwd(_lib.ptr(y), _lib.ptr(x), b, c, h, w, _lib.act_dtype(x), _lib.stream_ptr())
        _lib.check(rc, "ideas_maxpool2x2_fwd")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    @once_differentiable          # raw kernels: a create_graph pass must run inside second_order() and raises otherwise
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        b, c, h, w = x.shape
        gy = _nhwc(gy, x.dtype)
        gx = torch.empty_like(x)
        rc = _lib.load().ideas_maxpool2x2_bwd(_lib.ptr(gx), _lib.ptr(gy), _lib.ptr(x), b, c, h, w, _lib.act_dtype(x), _lib.stream_ptr())
        _lib.check(rc, "ideas_maxpool2x2_bwd")
        return gx


def max_pool2x2_composition(x: torch.Tensor) -> torch.Tensor:
    return F.max_pool2d(x, kernel_size=2, stride=2)


def max_pool2x2(x: torch.Tensor) -> torch.Tensor:
    """``F.max_pool2d(x, kernel_size=2, stride=2)`` of ``x`` ([B, C, H, W], H, W >= 2)."""
    if x.dim() != 4:
        raise RuntimeError("max_pool2x2 expects a 4-D [B, C, H, W] tensor")
    if x.shape[2] < 2 or x.shape[3] < 2:
        raise RuntimeError(f"max_pool2x2: the input {tuple(x.shape)} is smaller than the 2x2 window")
    _lib.require_cuda(x)
    if _use_composition(x):
        _lib.op_dtype(x)
        return max_pool2x2_composition(x)
    _lib.act_dtype(x)
    if x.numel() == 0:
        return x.new_empty((x.shape[0], x.shape[1], x.shape[2] // 2, x.shape[3] // 2))
    return _MaxPool2x2.apply(x)


class _LpipsLayer(Function):
    @staticmethod
    def forward(ctx, f0, f1, w):
        f0 = _nhwc(f0, f0.dtype)
        f1 = _nhwc(f1, f0.dtype)
        b, c, h, wd = f0.shape
        wf = w.detach().reshape(-1)
        wf = (wf if wf.dtype == torch.float32 else wf.float()).contiguous()
        d = torch.empty(b, device=f0.device, dtype=torch.float32)
        ws = torch.empty(b * _lib.LPIPS_MAX_PARTIALS, device=f0.device, dtype=torch.float64)
        rc = _lib.load().ideas_lpips_layer_fwd(_lib.ptr(d), _lib.ptr(ws), _lib.ptr(f0), _lib.ptr(f1), _lib.ptr(wf), b, c, h, wd,
                                               _lib.act_dtype(f0), _lib.stream_ptr())
        _lib.check(rc, "ideas_lpips_layer_fwd")
        ctx.save_for_backward(f0, f1, wf)
        return d

    @staticmethod
    @once_differentiable
    def backward(ctx, gd):
        f0, f1, wf = ctx.saved_tensors
        b, c, h, wd = f0.shape
        need0, need1, need_w = ctx.needs_input_grad
        if need_w:
            raise RuntimeError("lpips_layer: the lin weights are frozen on the kernel path (training them is out of scope)")
        if not (need0 or need1):
            return None, None, None
        gd = (gd if gd.dtype == torch.float32 else gd.float()).contiguous()
        g0 = torch.empty_like(f0) if need0 else None
        g1 = torch.empty_like(f1) if need1 else None
        rc = _lib.load().ideas_lpips_layer_bwd(_lib.ptr(g0), _lib.ptr(g1), _lib.ptr(gd), _lib.ptr(f0), _lib.ptr(f1), _lib.ptr(wf), b, c, h,
                                               wd, _lib.act_dtype(f0), _lib.stream_ptr())
        _lib.check(rc, "ideas_lpips_layer_bwd")
        return g0, g1, None


def lpips_layer_composition(f0: torch.Tensor, f1: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """The same formulas as the reference writes them: normalise, difference, square, 1x1 weights, spatial mean."""
    u0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + EPS)
    u1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + EPS)
    d = ((u0 - u1) ** 2 * w.reshape(1, -1, 1, 1).to(f0.dtype)).sum(1).mean((1, 2))
    return d.float() if d.dtype in (torch.float16, torch.bfloat16) else d


def lpips_layer(f0: torch.Tensor, f1: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Per-sample LPIPS distance of one tap: ``f0``, ``f1`` [B, C, H, W], ``w`` the C non-negative lin weights -> [B]."""
    if f0.dim() != 4 or f0.shape != f1.shape:
        raise RuntimeError(f"lpips_layer expects two [B, C, H, W] tensors of one shape, got {tuple(f0.shape)} and {tuple(f1.shape)}")
    if f0.dtype != f1.dtype:
        raise RuntimeError(f"lpips_layer: f0 is {f0.dtype}, f1 is {f1.dtype}")
    if w.numel() != f0.shape[1]:
        raise RuntimeError(f"lpips_layer: w has {w.numel()} elements, expected {f0.shape[1]}")
    _lib.require_cuda(f0, f1, w)
    if _use_composition(f0):
        _lib.op_dtype(f0)
        return lpips_layer_composition(f0, f1, w)
    _lib.act_dtype(f0)
    if f0.shape[1] > 2048:
        raise RuntimeError(f"lpips_layer: at most 2048 channels, got {f0.shape[1]}")
    if f0.numel() == 0:
        raise RuntimeError("lpips_layer: empty input")
    return _LpipsLayer.apply(f0, f1, w)
