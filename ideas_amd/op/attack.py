"""Channel attacks on the 8-bit container, on the HIP kernels of csrc/attack.hip, csrc/attack_jpeg.hip and csrc/jpeg_bytes.hip: what a container suffers
between sender and receiver.

    jpeg_roundtrip(u8, quality)   a baseline-JPEG (4:4:4) encode and decode in one launch -- the model is stated step by step in
                                  include/ideas_hip.h and restated in numpy by tests/attacks_ref.py
    jpeg_file_roundtrip(u8, quality, subsampling)
                                  the JPEG FILE libjpeg / Pillow writes (integer DCT, 4:2:0 by default, triangle upsampler), exact
                                  to the byte -- stated in include/ideas_hip.h, restated by tests/jpegfile_ref.py
    jpeg_file_encode(u8, quality, subsampling)
                                  that FILE itself, written on the device (csrc/jpeg_bytes.hip): Pillow's ``Image.save`` bytes --
                                  stated in include/ideas_hip.h, restated by tests/jpegbytes_ref.py; ``jpeg_files_to_host`` hands the
                                  files over as ``bytes``
    pixel_attack(u8, ...)         intensity (gain, offset), additive Gaussian noise (sigma) and salt and pepper (sp) in one launch

All take and return the uint8 ``[B, H, W, C]`` bytes of ``quantize_image`` (C = 1 or 3) together with ``y``, float32 ``[B, C, H, W]``
in channels_last memory: bitwise ``data.u8_to_f32`` of the returned bytes, the image a receiver decodes.  Device tensors only (no CPU
branch); forward-only.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from .. import _lib


def _bytes(u8: torch.Tensor, what: str) -> torch.Tensor:
    _lib.require_cuda(u8)
    if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] not in (1, 3):
        raise RuntimeError(f"{what} expects uint8 [B, H, W, C] with C = 1 or 3, got {u8.dtype} {tuple(u8.shape)}")
    return u8.contiguous()


def _outputs(u8: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    b, h, w, c = u8.shape
    return torch.empty_like(u8), torch.empty((b, c, h, w), device=u8.device, dtype=torch.float32, memory_format=torch.channels_last)


def jpeg_roundtrip(u8: torch.Tensor, quality: int, return_coef: bool = False):
    """``u8`` through a JPEG file of ``quality`` (1..100, the IJG scale; 4:4:4, no chroma subsampling) -> ``(u8, y)``, or
    ``(u8, y, coef)`` with ``return_coef``: the quantised DCT coefficients int16 ``[B, C, ceil(H/8), ceil(W/8), 64]`` at index
    ``8 u + v`` (u the vertical frequency; planes Y, Cb, Cr).  One launch."""
    u8 = _bytes(u8, "jpeg_roundtrip")
    if int(quality) != quality or not 1 <= int(quality) <= 100:
        raise RuntimeError(f"jpeg_roundtrip: quality must be an integer in 1..100, got {quality!r}")
    b, h, w, c = u8.shape
    out, y = _outputs(u8)
    coef = torch.empty((b, c, (h + 7) // 8, (w + 7) // 8, 64), device=u8.device, dtype=torch.int16) if return_coef else None
    if u8.numel():
        rc = _lib.load().ideas_jpeg_roundtrip(_lib.ptr(out), _lib.ptr(y), _lib.ptr(coef), _lib.ptr(u8), b, c, h, w, int(quality),
                                              _lib.stream_ptr())
        _lib.check(rc, "ideas_jpeg_roundtrip")
    return (out, y, coef) if return_coef else (out, y)


_SUBSAMPLING = {"4:4:4": 0, "4:2:0": 2, 0: 0, 2: 2}


def _file_args(u8: torch.Tensor, quality, subsampling, what: str) -> Tuple[torch.Tensor, int]:
    """The validation ``jpeg_file_roundtrip`` and ``jpeg_file_encode`` share -> (the contiguous bytes, the subsampling code)."""
    u8 = _bytes(u8, what)
    if int(quality) != quality or not 1 <= int(quality) <= 100:
        raise RuntimeError(f"{what}: quality must be an integer in 1..100, got {quality!r}")
    sub = _SUBSAMPLING.get(subsampling) if isinstance(subsampling, (str, int)) and not isinstance(subsampling, bool) else None
    if sub is None:
        raise RuntimeError(f"{what}: subsampling must be '4:4:4', '4:2:0', 0 or 2, got {subsampling!r}")
    return u8, sub


def jpeg_file_roundtrip(u8: torch.Tensor, quality: int, subsampling="4:2:0", return_coef: bool = False):
    """``u8`` through the JPEG FILE libjpeg / libjpeg-turbo writes at ``quality`` (1..100) with its defaults -- what Pillow's
    ``Image.save(f, "JPEG", quality=quality, subsampling=...)`` writes and ``Image.open`` reads back, byte for byte: the integer DCT,
    ``subsampling`` ``"4:2:0"`` (the default, also ``2``) or ``"4:4:4"`` (``0``), the triangle chroma upsampler -> ``(u8, y)``, or
    ``(u8, y, coef_y, coef_c)`` with ``return_coef``: the quantised coefficients int16 ``[B, ceil(H/8), ceil(W/8), 64]`` and
    ``[B, 2, cbh, cbw, 64]`` (Cb, Cr; the luma grid at 4:4:4, ``ceil(ceil(H/2)/8) x ceil(ceil(W/2)/8)`` at 4:2:0; ``None`` for
    C = 1) at index ``8 u + v``.  One launch, two at 4:2:0 with C = 3 (the workspace is allocated here)."""
    u8, sub = _file_args(u8, quality, subsampling, "jpeg_file_roundtrip")
    b, h, w, c = u8.shape
    out, y = _outputs(u8)
    coef_y = coef_c = None
    if return_coef:
        bh, bw = (h + 7) // 8, (w + 7) // 8
        coef_y = torch.empty((b, bh, bw, 64), device=u8.device, dtype=torch.int16)
        if c == 3:
            cbh, cbw = (bh, bw) if sub == 0 else (((h + 1) // 2 + 7) // 8, ((w + 1) // 2 + 7) // 8)
            coef_c = torch.empty((b, 2, cbh, cbw, 64), device=u8.device, dtype=torch.int16)
    if u8.numel():
        lib = _lib.load()
        nbytes = int(lib.ideas_jpeg_file_workspace_bytes(b, c, h, w, sub))
        work = torch.empty((nbytes,), device=u8.device, dtype=torch.uint8) if nbytes else None
        rc = lib.ideas_jpeg_file_roundtrip(_lib.ptr(out), _lib.ptr(y), _lib.ptr(coef_y), _lib.ptr(coef_c), _lib.ptr(work), _lib.ptr(u8),
                                           b, c, h, w, int(quality), sub, _lib.stream_ptr())
        _lib.check(rc, "ideas_jpeg_file_roundtrip")
    return (out, y, coef_y, coef_c) if return_coef else (out, y)


def jpeg_file_encode(u8: torch.Tensor, quality: int, subsampling="4:2:0", return_decoded: bool = False):
    """``u8`` as JPEG FILES, written on the device: the bytes of Pillow's ``Image.save(f, "JPEG", quality=quality, subsampling=...)``
    (a baseline file, the standard Huffman tables) -> ``(files, nbytes)``: uint8 ``[B, max_bytes]`` and int32 ``[B]``, file ``b`` being
    ``files[b, :nbytes[b]]`` (``jpeg_files_to_host`` cuts them out), or ``(files, nbytes, out, y)`` with ``return_decoded``: what
    ``jpeg_file_roundtrip`` returns, the image a receiver decodes from those files.  Arguments as ``jpeg_file_roundtrip``.  The round
    trip's launches, then four more and a memset (the workspace is allocated here)."""
    u8, sub = _file_args(u8, quality, subsampling, "jpeg_file_encode")
    b, h, w, c = u8.shape
    out, y, coef_y, coef_c = jpeg_file_roundtrip(u8, quality, sub, return_coef=True)
    lib = _lib.load()
    stride = int(lib.ideas_jpeg_file_max_bytes(c, h, w, sub))
    if stride == 0:
        raise RuntimeError(f"jpeg_file_encode: a JPEG file holds at most 65535 x 65535 pixels and 2^31 - 1 bytes, got {h} x {w}")
    files = torch.empty((b, stride), device=u8.device, dtype=torch.uint8)
    nbytes = torch.empty((b,), device=u8.device, dtype=torch.int32)
    if u8.numel():
        work = torch.empty((int(lib.ideas_jpeg_file_encode_workspace_bytes(b, c, h, w, sub)),), device=u8.device, dtype=torch.uint8)
        rc = lib.ideas_jpeg_file_encode(_lib.ptr(files), _lib.ptr(nbytes), stride, _lib.ptr(coef_y), _lib.ptr(coef_c), _lib.ptr(work),
                                        b, c, h, w, int(quality), sub, _lib.stream_ptr())
        _lib.check(rc, "ideas_jpeg_file_encode")
    return (files, nbytes, out, y) if return_decoded else (files, nbytes)


def _rows_to_host(files: torch.Tensor, nbytes: torch.Tensor, what: str):
    """``(files, nbytes)`` of a file writer on the host -> (uint8 array ``[B, 4 + max_bytes]``, the lengths riding in front of the
    rows; the lengths int32 ``[B]``), or None for B = 0.  ONE device-to-host copy and no synchronisation in front of it: the rows go
    over whole (the longest file is not known on the host)."""
    _lib.require_cuda(files, nbytes)
    if files.dtype != torch.uint8 or files.dim() != 2 or nbytes.dtype != torch.int32 or tuple(nbytes.shape) != (files.shape[0],):
        raise RuntimeError(f"{what} expects uint8 [B, max_bytes] and int32 [B], got {files.dtype} {tuple(files.shape)} and "
                           f"{nbytes.dtype} {tuple(nbytes.shape)}")
    if files.shape[0] == 0:
        return None
    host = torch.cat((nbytes.view(torch.uint8).view(-1, 4), files), dim=1).cpu().numpy()
    return host, host[:, :4].copy().view("<i4")[:, 0]


def jpeg_files_to_host(files: torch.Tensor, nbytes: torch.Tensor) -> List[bytes]:
    """``jpeg_file_encode``'s ``(files, nbytes)`` as a list of ``bytes``, one file each.  ONE device-to-host copy and no
    synchronisation in front of it: the lengths ride in front of the rows, whole (the longest file is not known on the host)."""
    rows = _rows_to_host(files, nbytes, "jpeg_files_to_host")
    if rows is None:
        return []
    host, lengths = rows
    if (lengths < 0).any():
        raise RuntimeError(f"jpeg_files_to_host: image(s) {[int(i) for i in (lengths < 0).nonzero()[0]]} hold a coefficient that has no "
                           "Huffman code")
    return [host[i, 4:4 + int(n)].tobytes() for i, n in enumerate(lengths)]


def _draw(fn, shape, generator: Optional[torch.Generator], device) -> torch.Tensor:
    """f32 draws on ``device``; a generator of another device (a CPU generator for a GPU run) draws there and the result is copied."""
    if generator is None or generator.device.type == device.type:
        return fn(shape, generator=generator, device=device, dtype=torch.float32)
    return fn(shape, generator=generator, device=generator.device, dtype=torch.float32).to(device)


def pixel_attack(u8: torch.Tensor, gain: float = 1.0, offset: float = 0.0, sigma: float = 0.0, sp: float = 0.0,
                 noise: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None,
                 generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``r = trunc(clamp((x - 127.5) * gain + 127.5 + offset + sigma * noise + 0.5, 0, 255))``, every step one f32 operation in that
    order, then salt and pepper: a pixel with ``u < sp / 2`` becomes 0 and one with ``u >= 1 - sp / 2`` becomes 255, in every channel.
    ``offset`` and ``sigma`` are in 8-bit levels.  ``noise`` (standard normal, ``[B, H, W, C]``) and ``u`` (U[0,1), ``[B, H, W]``)
    make the draws explicit; without them they are drawn here on the device from ``generator``, the noise first, and only those that
    are needed (``sigma != 0``, ``sp != 0``).  -> ``(u8, y)``.  One launch."""
    u8 = _bytes(u8, "pixel_attack")
    _lib.require_cuda(noise, u)
    b, h, w, c = u8.shape
    if noise is None and sigma != 0:
        noise = _draw(torch.randn, (b, h, w, c), generator, u8.device)
    if u is None and sp != 0:
        u = _draw(torch.rand, (b, h, w), generator, u8.device)
    if noise is not None:
        if tuple(noise.shape) != (b, h, w, c):
            raise RuntimeError(f"pixel_attack: noise must be [{b}, {h}, {w}, {c}], got {tuple(noise.shape)}")
        noise = noise.detach().to(torch.float32).contiguous()
    if u is not None:
        if tuple(u.shape) != (b, h, w):
            raise RuntimeError(f"pixel_attack: u must be [{b}, {h}, {w}], got {tuple(u.shape)}")
        u = u.detach().to(torch.float32).contiguous()
    out, y = _outputs(u8)
    if u8.numel():
        rc = _lib.load().ideas_pixel_attack(_lib.ptr(out), _lib.ptr(y), _lib.ptr(u8), _lib.ptr(noise), _lib.ptr(u), b, c, h, w,
                                            float(gain), float(offset), float(sigma), float(sp), _lib.stream_ptr())
        _lib.check(rc, "ideas_pixel_attack")
    return out, y
