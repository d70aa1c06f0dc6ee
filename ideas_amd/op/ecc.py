"""Payload coding on the HIP kernels of csrc/ecc.hip: the raw calls.  The code (K = 7 convolutional code 171 / 133, punctured to 1/2,
2/3 or 3/4, one zero-terminated codeword and one interleaver per image) is defined in include/ideas_hip.h ("Payload coding");
``ideas_amd.ecc`` plans it for an image size and is what callers use.

    ecc_encode(info, n, k, rate, P, Pinv, fill)   packed info rows [B, k / 8] -> packed message rows [B, ceil(n / 8)]
    ecc_soft(z, sigma, gain)                      the extractor's output [B, L] -> int8 soft values [B, L * sigma], positive favours 1
    ecc_viterbi(soft, n, k, rate, P, workspace)   int8 [B, n] -> (packed info rows [B, k / 8], int32 [B] final metrics)

Device tensors only (no CPU branch); forward-only.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _lib
from .stego import _check_sigma, _rows, packed_bytes

RATE_1_2, RATE_2_3, RATE_3_4 = 0, 1, 2     # include/ideas_hip.h::IDEAS_ECC_RATE_*
TAIL = 6
LDS_STEPS = 4096                            # csrc/ecc.hip::LDS_CAP / 8: the longest codeword whose survivors stay in LDS


def ecc_encode(info: torch.Tensor, n: int, k: int, rate: int, P: int, Pinv: int, fill: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``info`` uint8 [B, k / 8] -> the coded message rows uint8 [B, ceil(n / 8)]; ``fill`` (packed rows of that shape, or None for
    zeros) supplies the message bits no coded bit lands on."""
    _lib.require_cuda(info, fill)
    n, k = int(n), int(k)
    if k <= 0 or k % 8:
        raise RuntimeError(f"ecc_encode: k must be a positive multiple of 8, got {k}")
    info = _rows(info, k // 8, "ecc_encode(info)")
    b = info.shape[0]
    if fill is not None:
        fill = _rows(fill, packed_bytes(n), "ecc_encode(fill)")
        if fill.shape[0] != b:
            raise RuntimeError("ecc_encode: fill must have one row per image")
    coded = torch.empty((b, packed_bytes(n)), device=info.device, dtype=torch.uint8)
    if b:
        rc = _lib.load().ideas_ecc_encode(_lib.ptr(coded), _lib.ptr(info), _lib.ptr(fill), b, n, k, int(rate), int(P), int(Pinv),
                                          _lib.stream_ptr())
        _lib.check(rc, "ideas_ecc_encode")
    return coded


def ecc_soft(z: torch.Tensor, sigma: int, gain: float = 64.0) -> torch.Tensor:
    """``z`` [B, L] (float32 or bfloat16) -> int8 [B, L * sigma]: per message bit the scaled difference of the squared distances to the
    nearest bin centre with that bit 0 and with that bit 1."""
    sigma = _check_sigma(sigma)
    _lib.require_cuda(z)
    if z.dim() != 2 or z.shape[1] == 0:
        raise RuntimeError("ecc_soft expects a [B, L] tensor")
    dt = _lib.act_dtype(z)
    z = z.detach().contiguous()
    b, L = z.shape
    soft = torch.empty((b, L * sigma), device=z.device, dtype=torch.int8)
    if b:
        rc = _lib.load().ideas_ecc_soft(_lib.ptr(soft), _lib.ptr(z), b, L, sigma, float(gain), dt, _lib.stream_ptr())
        _lib.check(rc, "ideas_ecc_soft")
    return soft


def ecc_viterbi(soft: torch.Tensor, n: int, k: int, rate: int, P: int, workspace: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``soft`` int8 [B, n] -> ``(info, metric)``: the decoded packed rows uint8 [B, k / 8] and the final metric of state 0, int32 [B].
    ``workspace`` (int64 [B, k + 6], contents undefined afterwards) moves the survivors from LDS to global memory; it is needed above
    ``LDS_STEPS`` steps and selects that route whenever it is given."""
    _lib.require_cuda(soft, workspace)
    n, k = int(n), int(k)
    if soft.dtype != torch.int8 or soft.dim() != 2 or soft.shape[1] != n:
        raise RuntimeError(f"ecc_viterbi: expected soft values int8 [B, {n}], got {soft.dtype} {tuple(soft.shape)}")
    if k <= 0 or k % 8:
        raise RuntimeError(f"ecc_viterbi: k must be a positive multiple of 8, got {k}")
    soft = soft.contiguous()
    b = soft.shape[0]
    if workspace is not None and (workspace.dtype != torch.int64 or tuple(workspace.shape) != (b, k + TAIL) or not workspace.is_contiguous()):
        raise RuntimeError(f"ecc_viterbi: workspace must be a contiguous int64 [{b}, {k + TAIL}]")
    info = torch.empty((b, k // 8), device=soft.device, dtype=torch.uint8)
    metric = torch.empty((b,), device=soft.device, dtype=torch.int32)
    if b:
        rc = _lib.load().ideas_ecc_viterbi(_lib.ptr(info), _lib.ptr(metric), _lib.ptr(soft), _lib.ptr(workspace), b, n, k, int(rate),
                                           int(P), _lib.stream_ptr())
        _lib.check(rc, "ideas_ecc_viterbi")
    return info, metric
