"""``pool3x3`` and ``global_avg_pool`` on the HIP kernels of csrc/pool.hip: the pools of the FID Inception-v3
(stylegan2/inception.py) that the conv family does not cover.

``pool3x3(x, mode)``: the three 3x3 windows of the network,

    MAX_S2           F.max_pool2d(x, 3, 2)                                 (the two stem pools, Mixed_6a, Mixed_7a)
    MAX_S1P1         F.max_pool2d(x, 3, 1, 1)                              (Mixed_7c: the reference's FIDInceptionE_2 patch)
    AVG_S1P1_VALID   F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)     (Mixed_5b .. 6e, 7b: TensorFlow's average)

``global_avg_pool(x)`` is ``F.adaptive_avg_pool2d(x, 1)`` with a float32 result [B, C, 1, 1].

Both are forward-only (the network is frozen): a tensor that requires grad while grad is enabled raises.  f16 / f64 tensors take the
plain torch compositions (``pool3x3_composition`` / ``global_avg_pool_composition``).  NCHW-contiguous and channels_last tensors are
accepted; the output is channels_last.  No CPU branch.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import _lib

CL = torch.channels_last
MAX_S2, MAX_S1P1, AVG_S1P1_VALID = _lib.POOL_MAX_S2, _lib.POOL_MAX_S1P1, _lib.POOL_AVG_S1P1_VALID
MODES = (MAX_S2, MAX_S1P1, AVG_S1P1_VALID)


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous(memory_format=CL) else t.contiguous(memory_format=CL)


def _forward_only(x: torch.Tensor, what: str) -> None:
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError(f"{what} is forward-only (the Inception network is frozen): call it under torch.no_grad() or on a "
                           "tensor that does not require grad")


def pool3x3_composition(x: torch.Tensor, mode: int) -> torch.Tensor:
    if mode == MAX_S2:
        return F.max_pool2d(x, kernel_size=3, stride=2)
    if mode == MAX_S1P1:
        return F.max_pool2d(x, kernel_size=3, stride=1, padding=1)
    return F.avg_pool2d(x, kernel_size=3, stride=1, padding=1, count_include_pad=False)


def pool3x3(x: torch.Tensor, mode: int) -> torch.Tensor:
    """The 3x3 pool ``mode`` (``MAX_S2``, ``MAX_S1P1`` or ``AVG_S1P1_VALID``) of ``x`` [B, C, H, W]."""
    if mode not in MODES:
        raise RuntimeError(f"pool3x3: mode must be MAX_S2, MAX_S1P1 or AVG_S1P1_VALID, got {mode!r}")
    if x.dim() != 4:
        raise RuntimeError("pool3x3 expects a 4-D [B, C, H, W] tensor")
    if mode == MAX_S2 and (x.shape[2] < 3 or x.shape[3] < 3):
        raise RuntimeError(f"pool3x3(MAX_S2): the input {tuple(x.shape)} is smaller than the 3x3 window")
    _lib.require_cuda(x)
    _forward_only(x, "pool3x3")
    if x.dtype in (torch.float16, torch.float64):
        return pool3x3_composition(x, mode)
    dt = _lib.act_dtype(x)
    b, c, h, w = x.shape
    oh, ow = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if mode == MAX_S2 else (h, w)
    y = torch.empty((b, c, oh, ow), device=x.device, dtype=x.dtype, memory_format=CL)
    if y.numel() == 0:
        return y
    x = _nhwc(x.detach())
    rc = _lib.load().ideas_pool3x3_fwd(_lib.ptr(y), _lib.ptr(x), b, c, h, w, int(mode), dt, _lib.stream_ptr())
    _lib.check(rc, "ideas_pool3x3_fwd")
    return y


def global_avg_pool_composition(x: torch.Tensor) -> torch.Tensor:
    return F.adaptive_avg_pool2d(x, 1)


def global_avg_pool(x: torch.Tensor) -> torch.Tensor:
    """``F.adaptive_avg_pool2d(x, 1)`` of ``x`` [B, C, H, W] -> [B, C, 1, 1], float32 for f32 and bf16 inputs."""
    if x.dim() != 4:
        raise RuntimeError("global_avg_pool expects a 4-D [B, C, H, W] tensor")
    _lib.require_cuda(x)
    _forward_only(x, "global_avg_pool")
    if x.dtype in (torch.float16, torch.float64):
        return global_avg_pool_composition(x)
    dt = _lib.act_dtype(x)
    b, c, h, w = x.shape
    if x.numel() == 0:
        raise RuntimeError("global_avg_pool: empty input")
    out = torch.empty((b, c), device=x.device, dtype=torch.float32)
    x = _nhwc(x.detach())
    rc = _lib.load().ideas_global_avg_pool(_lib.ptr(out), _lib.ptr(x), b, c, h, w, dt, _lib.stream_ptr())
    _lib.check(rc, "ideas_global_avg_pool")
    return out.view(b, c, 1, 1)
