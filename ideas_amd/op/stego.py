"""The steganography codec on the HIP kernels of csrc/stego.hip: messages as PACKED bits, and the container image's trip through an
8-bit file.

Packed bits: a uint8 tensor ``[B, ceil(L * sigma / 8)]``; message bit ``j`` of image ``b`` is ``(bits[b, j >> 3] >> (7 - (j & 7))) & 1``
and element ``l`` of the secret tensor takes message bits ``[l * sigma, (l + 1) * sigma)``, most significant first -- the order of
``message[:, i::sigma]`` in ``utils.message_to_tensor``.  ``pack_bits`` / ``unpack_bits`` bridge to the ``[B, n]`` 0/1 float messages
of ``utils.py``.

    bits_to_tensor(bits, L, sigma, delta, jitter)  ==  utils.message_to_tensor(unpack_bits(bits, L * sigma), sigma, delta, jitter)
    unpack_bits(tensor_to_bits(z, sigma), L * sigma)  ==  utils.tensor_to_message(z, sigma)
    quantize_image(x)  ->  (the bytes save_image(normalize=True, range=(-1, 1)) writes,  data.u8_to_f32 of those bytes)

bit for bit.  Device tensors only (no CPU branch); forward-only.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch

from .. import _lib

CL = torch.channels_last


def _check_sigma(sigma: int) -> int:
    if int(sigma) != sigma or not 1 <= int(sigma) <= 8:
        raise RuntimeError(f"sigma must be an integer in 1..8, got {sigma!r}")
    return int(sigma)


def packed_bytes(n_bits: int) -> int:
    return (int(n_bits) + 7) // 8


def pack_bits(message01: torch.Tensor) -> torch.Tensor:
    """``[B, n]`` 0/1 values (any dtype, any device) -> uint8 ``[B, ceil(n / 8)]``, most significant bit first, pad bits zero."""
    if message01.dim() != 2:
        raise RuntimeError("pack_bits expects a [B, n] message")
    b, n = message01.shape
    m = (message01 != 0).to(torch.uint8)
    pad = -n % 8
    if pad:
        m = torch.cat((m, m.new_zeros(b, pad)), 1)
    w = torch.tensor([128, 64, 32, 16, 8, 4, 2, 1], dtype=torch.int32, device=m.device)
    return (m.view(b, -1, 8).to(torch.int32) * w).sum(2).to(torch.uint8)


def unpack_bits(bits: torch.Tensor, n: int) -> torch.Tensor:
    """uint8 ``[B, nbytes]`` -> float32 ``[B, n]`` of 0/1: the first ``n`` message bits of every row."""
    if bits.dim() != 2 or bits.dtype != torch.uint8 or not 0 <= n <= bits.shape[1] * 8:
        raise RuntimeError("unpack_bits expects a uint8 [B, nbytes] tensor with nbytes * 8 >= n")
    sh = torch.tensor([7, 6, 5, 4, 3, 2, 1, 0], dtype=torch.int32, device=bits.device)
    m = (bits.to(torch.int32).unsqueeze(2) >> sh) & 1
    return m.reshape(bits.shape[0], -1)[:, :n].to(torch.float32)


def _rows(bits: torch.Tensor, nbytes: int, what: str) -> torch.Tensor:
    if bits.dtype != torch.uint8 or bits.dim() != 2 or bits.shape[1] != nbytes:
        raise RuntimeError(f"{what}: expected packed bits uint8 [B, {nbytes}], got {bits.dtype} {tuple(bits.shape)}")
    return bits.contiguous()


def bits_to_tensor(bits: torch.Tensor, L: int, sigma: int, delta: float, jitter: Optional[torch.Tensor] = None,
                   generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """Packed bits ``[B, ceil(L * sigma / 8)]`` -> the secret tensor float32 ``[B, L]``.  ``jitter`` (U[0,1), ``[B, L]``) makes the
    draw explicit; without it and with ``delta > 0`` it is drawn here on the device from ``generator``; with ``delta == 0`` and no
    jitter the bin centres come out."""
    sigma = _check_sigma(sigma)
    _lib.require_cuda(bits, jitter)
    L = int(L)
    if L <= 0:
        raise RuntimeError("bits_to_tensor: L must be positive")
    bits = _rows(bits, packed_bytes(L * sigma), "bits_to_tensor")
    b = bits.shape[0]
    if jitter is None and delta > 0:
        jitter = torch.rand(b, L, device=bits.device, dtype=torch.float32, generator=generator)
    if jitter is not None:
        if tuple(jitter.shape) != (b, L):
            raise RuntimeError(f"bits_to_tensor: jitter must be [{b}, {L}], got {tuple(jitter.shape)}")
        jitter = jitter.detach().to(torch.float32).contiguous()
    z = torch.empty((b, L), device=bits.device, dtype=torch.float32)
    if b == 0:
        return z
    rc = _lib.load().ideas_bits_to_tensor(_lib.ptr(z), _lib.ptr(bits), _lib.ptr(jitter), b, L, sigma, float(delta),
                                          _lib.stream_ptr())
    _lib.check(rc, "ideas_bits_to_tensor")
    return z


def tensor_to_bits(z: torch.Tensor, sigma: int, ref: Optional[torch.Tensor] = None
                   ) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """The secret tensor ``[B, L]`` (float32 or bfloat16) -> packed decisions uint8 ``[B, ceil(L * sigma / 8)]``.  With ``ref``
    (packed bits of the same shape) also ``n_err`` int32 ``[B]``: the number of message bits of each image that differ from it."""
    sigma = _check_sigma(sigma)
    _lib.require_cuda(z, ref)
    if z.dim() != 2 or z.shape[1] == 0:
        raise RuntimeError("tensor_to_bits expects a [B, L] tensor")
    dt = _lib.act_dtype(z)
    b, L = z.shape
    nbytes = packed_bytes(L * sigma)
    z = z.detach().contiguous()
    bits = torch.empty((b, nbytes), device=z.device, dtype=torch.uint8)
    n_err = None
    if ref is not None:
        ref = _rows(ref, nbytes, "tensor_to_bits(ref)")
        if ref.shape[0] != b:
            raise RuntimeError("tensor_to_bits: ref must have one row per image")
        n_err = torch.empty((b,), device=z.device, dtype=torch.int32)
    if b:
        rc = _lib.load().ideas_tensor_to_bits(_lib.ptr(bits), _lib.ptr(n_err), _lib.ptr(z), _lib.ptr(ref), b, L, sigma, dt,
                                              _lib.stream_ptr())
        _lib.check(rc, "ideas_tensor_to_bits")
    return bits if ref is None else (bits, n_err)


def quantize_image(x: torch.Tensor, dequantize: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """``x`` [B, C, H, W] in [-1, 1] (float32 or bfloat16, C = 1 or 3) -> ``(u8, y)``: ``u8`` uint8 [B, H, W, C], the bytes an 8-bit
    image file of the container holds, and ``y`` float32 [B, C, H, W] (channels_last memory, like ``data.u8_to_f32``'s result), the
    image a receiver decodes from them (None with ``dequantize=False``).  One launch."""
    _lib.require_cuda(x)
    if x.dim() != 4 or x.shape[1] not in (1, 3):
        raise RuntimeError(f"quantize_image expects [B, C, H, W] with C = 1 or 3, got {tuple(x.shape)}")
    dt = _lib.act_dtype(x)
    b, c, h, w = x.shape
    x = x.detach()
    if x.is_contiguous(memory_format=CL):
        layout = _lib.NHWC
    elif x.is_contiguous():
        layout = _lib.NCHW
    else:
        x, layout = x.contiguous(memory_format=CL), _lib.NHWC
    u8 = torch.empty((b, h, w, c), device=x.device, dtype=torch.uint8)
    y = torch.empty((b, c, h, w), device=x.device, dtype=torch.float32, memory_format=CL) if dequantize else None
    if u8.numel():
        rc = _lib.load().ideas_image_f32_to_u8(_lib.ptr(u8), _lib.ptr(y), _lib.ptr(x), b, c, h, w, layout, dt, _lib.stream_ptr())
        _lib.check(rc, "ideas_image_f32_to_u8")
    return u8, y
