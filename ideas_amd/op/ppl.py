"""The two small-step kernels of perceptual path length (stylegan2/ppl.py) around the generator and the VGG.

``path_endpoints(latent, t, eps, mode)``: ``latent`` [2B, D] holds the two ends of path i in rows 2i, 2i + 1; row 2i of the result is
``f(a, b, t_i)`` and row 2i + 1 is ``f(a, b, t_i + eps)`` with ``f`` = ``lerp`` or ``slerp`` -- the four strided slices, the two
interpolations and the ``torch.stack(...).view(...)`` of ppl.py:73-76 in one launch (``ideas_path_endpoints``, csrc/ppl.hip).  ``lerp``
is bitwise the torch expression; ``slerp`` follows ppl.py:16-24 without a clamp, so identical ends give a row of NaN as they do there
(c = 0 / 0; or, should their dot product round below 1, a finite row without meaning -- there as well).

``pair_prepare(img, box, out_hw, shift, scale)``: ``img`` [2B, 3, H, W] -> [2B, 3, oh, ow], channels_last: the crop ``box`` = (y, x, h,
w), the bilinear resize (``align_corners=False``), LPIPS's ``(v - shift[c]) / scale[c]`` and the de-interleave -- sample 2i lands at
index i, sample 2i + 1 at B + i -- in one launch (``ideas_pair_prepare``, csrc/patchify.hip), so that ONE VGG pass serves both sides of
every pair.  f32 or bf16 (f32 arithmetic, one rounding at the store).

Both are forward only (they raise on an input that requires grad), have no CPU branch, and take their plain-torch ``*_composition``
for f64.  The compositions state what the kernels compute.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple, Union

import torch
import torch.nn.functional as F

from .. import _lib

CL = torch.channels_last
MODES = {"lerp": _lib.PATH_LERP, "slerp": _lib.PATH_SLERP, _lib.PATH_LERP: _lib.PATH_LERP, _lib.PATH_SLERP: _lib.PATH_SLERP}


def normalize(x: torch.Tensor) -> torch.Tensor:
    return x / torch.sqrt(x.pow(2).sum(-1, keepdim=True))


def slerp(a: torch.Tensor, b: torch.Tensor, t) -> torch.Tensor:
    """Spherical interpolation of the directions of ``a`` and ``b`` (ppl.py:16-24): no clamp, so ``a == b`` gives NaN."""
    a, b = normalize(a), normalize(b)
    d = (a * b).sum(-1, keepdim=True)
    p = t * torch.acos(d)
    c = normalize(b - d * a)
    return normalize(a * torch.cos(p) + c * torch.sin(p))


def lerp(a: torch.Tensor, b: torch.Tensor, t) -> torch.Tensor:
    return a + (b - a) * t


def _mode(mode: Union[str, int]) -> int:
    if mode not in MODES:
        raise RuntimeError(f"path_endpoints: mode is 'lerp' (0) or 'slerp' (1), got {mode!r}")
    return MODES[mode]


def _forward_only(what: str, *tensors: torch.Tensor) -> None:
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError(f"{what} is forward only: an input requires grad (call it under torch.no_grad())")


def path_endpoints_composition(latent: torch.Tensor, t: torch.Tensor, eps: float, mode: Union[str, int]) -> torch.Tensor:
    """ppl.py:73-76 as the reference writes it (``lerp``), and the same with its ``slerp``."""
    f = slerp if _mode(mode) == _lib.PATH_SLERP else lerp
    a, b = latent[::2], latent[1::2]
    e0 = f(a, b, t[:, None])
    e1 = f(a, b, t[:, None] + eps)
    return torch.stack([e0, e1], 1).view(*latent.shape)


def path_endpoints(latent: torch.Tensor, t: torch.Tensor, eps: float, mode: Union[str, int] = "lerp") -> torch.Tensor:
    """``latent`` [2B, D] (1 <= D <= 4096), ``t`` [B], float32 -> [2B, D]: rows 2i / 2i + 1 are the path's points at t_i / t_i + eps."""
    m = _mode(mode)
    if latent.dim() != 2 or latent.shape[0] % 2 or t.dim() != 1 or 2 * t.shape[0] != latent.shape[0]:
        raise RuntimeError(f"path_endpoints expects latent [2B, D] and t [B], got {tuple(latent.shape)} and {tuple(t.shape)}")
    _lib.require_cuda(latent, t)
    _forward_only("path_endpoints", latent, t)
    if latent.dtype != t.dtype:
        raise RuntimeError(f"path_endpoints: latent is {latent.dtype}, t is {t.dtype}")
    if latent.dtype == torch.float64:
        return path_endpoints_composition(latent, t, eps, m)
    if latent.dtype != torch.float32:
        raise RuntimeError(f"path_endpoints takes float32 (float64 on the composition), got {latent.dtype}")
    b, d = t.shape[0], latent.shape[1]
    if b == 0 or d == 0:
        raise RuntimeError("path_endpoints: empty input")
    if d > _lib.PATH_MAX_DIM:
        raise RuntimeError(f"path_endpoints: at most {_lib.PATH_MAX_DIM} latent dimensions, got {d}")
    lat, tt = latent.detach().contiguous(), t.detach().contiguous()
    out = torch.empty_like(lat)
    rc = _lib.load().ideas_path_endpoints(_lib.ptr(out), _lib.ptr(lat), _lib.ptr(tt), float(eps), b, d, m, _lib.stream_ptr())
    _lib.check(rc, "ideas_path_endpoints")
    return out


def _triple(v, what: str):
    v = [float(x) for x in (v.detach().flatten().tolist() if torch.is_tensor(v) else v)]
    if len(v) != 3:
        raise RuntimeError(f"pair_prepare: {what} has {len(v)} values, expected 3")
    return v


def pair_prepare_composition(img: torch.Tensor, box: Sequence[int], out_hw: Tuple[int, int], shift, scale) -> torch.Tensor:
    """Crop, ``F.interpolate`` (skipped when the box has the output's size), ``(v - shift) / scale``, even samples then odd ones.
    bf16: the arithmetic in f32, one rounding at the end, as the kernel."""
    y0, x0, h, w = (int(v) for v in box)
    x = img[:, :, y0:y0 + h, x0:x0 + w]
    x = x.float() if x.dtype == torch.bfloat16 else x
    if (h, w) != tuple(out_hw):
        x = F.interpolate(x, size=tuple(out_hw), mode="bilinear", align_corners=False)
    sh = torch.tensor(_triple(shift, "shift"), device=img.device, dtype=torch.float32).to(x.dtype).view(1, 3, 1, 1)
    sc = torch.tensor(_triple(scale, "scale"), device=img.device, dtype=torch.float32).to(x.dtype).view(1, 3, 1, 1)
    x = (x - sh) / sc
    return torch.cat([x[::2], x[1::2]], 0).to(img.dtype)


def pair_prepare(img: torch.Tensor, box: Sequence[int], out_hw: Tuple[int, int], shift, scale) -> torch.Tensor:
    """``img`` [2B, 3, H, W] (NCHW-contiguous or channels_last; float32 / bfloat16) -> [2B, 3, oh, ow] channels_last: ``box`` = (y, x,
    h, w) cropped, resized to ``out_hw``, ``(v - shift[c]) / scale[c]``; sample 2i at index i, sample 2i + 1 at B + i."""
    if img.dim() != 4 or img.shape[0] % 2:
        raise RuntimeError(f"pair_prepare expects [2B, 3, H, W], got {tuple(img.shape)}")
    _lib.require_cuda(img)
    _forward_only("pair_prepare", img)
    sh, sc = _triple(shift, "shift"), _triple(scale, "scale")
    box = tuple(int(v) for v in box)
    oh, ow = (int(v) for v in out_hw)
    if len(box) != 4:
        raise RuntimeError(f"pair_prepare: box is (y, x, h, w), got {box}")
    if img.dtype == torch.float64:
        return pair_prepare_composition(img, box, (oh, ow), sh, sc)
    dt = _lib.act_dtype(img)
    n, c, h, w = img.shape
    if n == 0:
        raise RuntimeError("pair_prepare: empty input")
    x = img.detach()
    x = x if x.is_contiguous(memory_format=CL) else x.contiguous(memory_format=CL)
    y = torch.empty((n, c, max(oh, 0), max(ow, 0)), device=img.device, dtype=img.dtype, memory_format=CL)
    rc = _lib.load().ideas_pair_prepare(_lib.ptr(y), _lib.ptr(x), (C.c_int * 4)(*box), (C.c_float * 3)(*sh), (C.c_float * 3)(*sc),
                                        n // 2, c, h, w, oh, ow, dt, _lib.stream_ptr())
    _lib.check(rc, "ideas_pair_prepare")
    return y
