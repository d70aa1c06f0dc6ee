"""Spatial channel attacks on the 8-bit container, on the HIP kernels of csrc/attack_spatial.hip: rescaling, Gaussian and median
filtering -- what a messenger or an image host does to a picture before it re-encodes it.

    resize_u8(u8, (H2, W2))        Pillow's ``Image.resize((W2, H2), Image.BILINEAR)`` on 8-bit images, byte for byte
    gaussian_blur_u8(u8, sigma)    a separable Gaussian of ceil(3 sigma) taps either side, renormalised at the border
    median_u8(u8, k)               the k x k median (k = 3 or 5) with replicated edges: Pillow's ``ImageFilter.MedianFilter(k)``

The first two are ONE kernel, ``ideas_resample_u8``: every output index is a short weighted window of input indices, given as the
tables of ``resample_tables`` -- integer coefficients in units of 2^-22, a horizontal pass rounded to bytes and a vertical pass on
those bytes.  The model is stated step by step in include/ideas_hip.h and restated in numpy by tests/spatial_ref.py; it is integer
arithmetic throughout, so results are defined to the byte.

All take the uint8 ``[B, H, W, C]`` bytes of ``quantize_image`` (C = 1 or 3) and return ``(u8, y)`` as ``op.attack`` does: ``y`` is
float32 ``[B, C, H, W]`` in channels_last memory, bitwise ``data.u8_to_f32`` of the returned bytes.  Device tensors only (no CPU
branch); forward-only.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from .attack import _bytes

KMAX = 32                     # include/ideas_hip.h::IDEAS_RESAMPLE_KMAX
PRECISION_BITS = 22           # Pillow's 32 - 8 - 2


@functools.lru_cache(maxsize=None)
def _tables(n_in: int, n_out: int, filter: str, sigma: Optional[float]) -> Tuple[np.ndarray, np.ndarray]:
    i = np.arange(n_out, dtype=np.float64)
    if filter == "bilinear":
        scale = n_in / n_out
        sup = max(scale, 1.0)
        c = (i + 0.5) * scale
        lo = np.maximum(0, np.trunc(c - sup + 0.5).astype(np.int64))
        hi = np.minimum(n_in, np.trunc(c + sup + 0.5).astype(np.int64))
    elif filter == "gauss":
        if n_out != n_in:
            raise ValueError(f"resample_tables: the gauss filter keeps the size, got {n_in} -> {n_out}")
        if sigma is None or not sigma > 0:
            raise ValueError(f"resample_tables: the gauss filter needs sigma > 0, got {sigma!r}")
        r = math.ceil(3.0 * sigma)
        c = i
        lo = np.maximum(0, np.arange(n_out) - r)
        hi = np.minimum(n_in, np.arange(n_out) + r + 1)
    else:
        raise ValueError(f"resample_tables: unknown filter {filter!r} (bilinear, gauss)")
    ksize = int((hi - lo).max())
    x = lo[:, None] + np.arange(ksize)[None, :]               # [n_out, ksize] input indices
    if filter == "bilinear":
        w = np.maximum(0.0, 1.0 - np.abs((x - c[:, None] + 0.5) / sup))
    else:
        w = np.exp(-((x - c[:, None]) ** 2) / (2.0 * sigma * sigma))
    w = np.where(x < hi[:, None], w, 0.0)
    total = w.sum(axis=1, keepdims=True)
    w = np.where(total != 0, w / np.where(total != 0, total, 1.0), w)
    kk = np.trunc(w * float(1 << PRECISION_BITS) + 0.5).astype(np.int32)
    lo, kk = lo.astype(np.int32), np.ascontiguousarray(kk)
    lo.setflags(write=False)
    kk.setflags(write=False)
    return lo, kk


def resample_tables(n_in: int, n_out: int, filter: str, sigma: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The windows of ``n_out`` outputs over ``n_in`` inputs as int32 arrays ``(lo [n_out], kk [n_out, ksize])``: ``lo[i]`` is the first
    input of output ``i`` and ``kk[i, j]`` the coefficient of input ``lo[i] + j`` in units of 2^-22, zero-padded to ``ksize``, the widest
    window.  Computed in f64 and cached (the arrays are read-only).

    ``"bilinear"`` is Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc``: ``scale = n_in / n_out``, ``sup = max(scale, 1)``,
    centre ``c = (i + 0.5) scale``, ``lo = max(0, int(c - sup + 0.5))``, ``hi = min(n_in, int(c + sup + 0.5))`` (``int`` truncates),
    ``w_x = max(0, 1 - |(x - c + 0.5) / sup|)`` for x in lo .. hi - 1 divided by their sum, ``kk = int(w 2^22 + 0.5)``.
    ``"gauss"`` (``n_out == n_in``): ``r = ceil(3 sigma)``, ``lo = max(0, i - r)``, ``hi = min(n, i + r + 1)``,
    ``w_x = exp(-(x - i)^2 / (2 sigma^2))`` divided by the sum of the taps kept -- the border renormalises -- and the same rounding."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"resample_tables: sizes must be positive, got {n_in} -> {n_out}")
    return _tables(n_in, n_out, str(filter), None if sigma is None else float(sigma))


_device_tables: Dict[tuple, Tuple[torch.Tensor, torch.Tensor, int]] = {}


def _on_device(n_in: int, n_out: int, filter: str, sigma: Optional[float], device: torch.device):
    """``resample_tables`` as device tensors, cached per argument tuple and device: -> (lo, kk, ksize)."""
    key = (n_in, n_out, filter, sigma, device.type, device.index if device.index is not None else torch.cuda.current_device())
    hit = _device_tables.get(key)
    if hit is None:
        lo, kk = resample_tables(n_in, n_out, filter, sigma)
        if kk.shape[1] > KMAX:
            raise RuntimeError(f"resample: a window of {kk.shape[1]} taps ({filter}, {n_in} -> {n_out}, sigma {sigma}) exceeds {KMAX}")
        hit = (torch.from_numpy(lo.copy()).to(device), torch.from_numpy(kk.copy()).to(device), int(kk.shape[1]))
        _device_tables[key] = hit
    return hit


def _resample(u8: torch.Tensor, h2: int, w2: int, horiz, vert, what: str) -> Tuple[torch.Tensor, torch.Tensor]:
    b, h, w, c = u8.shape
    out = torch.empty((b, h2, w2, c), device=u8.device, dtype=torch.uint8)
    y = torch.empty((b, c, h2, w2), device=u8.device, dtype=torch.float32, memory_format=torch.channels_last)
    if u8.numel():
        h_lo, h_kk, hk = horiz if horiz is not None else (None, None, 0)
        v_lo, v_kk, vk = vert if vert is not None else (None, None, 0)
        rc = _lib.load().ideas_resample_u8(_lib.ptr(out), _lib.ptr(y), _lib.ptr(u8), b, c, h, w, h2, w2, _lib.ptr(h_lo), _lib.ptr(h_kk),
                                           hk, _lib.ptr(v_lo), _lib.ptr(v_kk), vk, _lib.stream_ptr())
        _lib.check(rc, what)
    return out, y


def resize_u8(u8: torch.Tensor, size: Tuple[int, int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """``u8`` resized to ``size = (H2, W2)`` as Pillow's ``Image.resize((W2, H2), Image.BILINEAR)`` does on 8-bit images: the horizontal
    pass first, rounded to bytes, then the vertical pass; a direction that keeps its size is skipped.  -> ``(u8, y)``.  One launch."""
    u8 = _bytes(u8, "resize_u8")
    h2, w2 = int(size[0]), int(size[1])
    if h2 <= 0 or w2 <= 0:
        raise RuntimeError(f"resize_u8: the size must be positive, got {size!r}")
    b, h, w, c = u8.shape
    horiz = _on_device(w, w2, "bilinear", None, u8.device) if w2 != w else None
    vert = _on_device(h, h2, "bilinear", None, u8.device) if h2 != h else None
    return _resample(u8, h2, w2, horiz, vert, "ideas_resample_u8 (resize)")


def gaussian_blur_u8(u8: torch.Tensor, sigma: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """``u8`` through a separable Gaussian of standard deviation ``sigma`` pixels, ``ceil(3 sigma)`` taps either side (at most
    ``(KMAX - 1) / 2``), each window renormalised to the taps inside the image; bytes between the passes.  -> ``(u8, y)``.  One launch."""
    u8 = _bytes(u8, "gaussian_blur_u8")
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma > 0) or 2 * math.ceil(3.0 * sigma) + 1 > KMAX:
        raise RuntimeError(f"gaussian_blur_u8: sigma must be positive with at most {KMAX} taps (2 ceil(3 sigma) + 1), got {sigma!r}")
    b, h, w, c = u8.shape
    return _resample(u8, h, w, _on_device(w, w, "gauss", sigma, u8.device), _on_device(h, h, "gauss", sigma, u8.device),
                     "ideas_resample_u8 (gaussian blur)")


def median_u8(u8: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The per-channel median over the ``k`` x ``k`` window (``k`` = 3 or 5) of the edge-replicated image, as Pillow's
    ``ImageFilter.MedianFilter(k)``.  -> ``(u8, y)``.  One launch."""
    u8 = _bytes(u8, "median_u8")
    if k not in (3, 5):
        raise RuntimeError(f"median_u8: the window must be 3 or 5, got {k!r}")
    b, h, w, c = u8.shape
    out = torch.empty_like(u8)
    y = torch.empty((b, c, h, w), device=u8.device, dtype=torch.float32, memory_format=torch.channels_last)
    if u8.numel():
        rc = _lib.load().ideas_median_u8(_lib.ptr(out), _lib.ptr(y), _lib.ptr(u8), b, c, h, w, int(k), _lib.stream_ptr())
        _lib.check(rc, "ideas_median_u8")
    return out, y
