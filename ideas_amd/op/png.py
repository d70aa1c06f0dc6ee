"""The PNG file of the 8-bit container, written on the HIP kernels of csrc/png_bytes.hip: the lossless channel a sender picks first.

    png_file_encode(u8)             the uint8 ``[B, H, W, C]`` bytes of ``quantize_image`` (C = 1 or 3) as PNG FILES -- row filters,
                                    Huffman-coded literals (no matches), Adler-32 and CRC-32, all on the device.  Stated to the byte in
                                    include/ideas_hip.h ("The PNG file, written"), restated by tests/png_ref.py.  Any PNG reader opens
                                    them to exactly ``u8``; they are NOT the bytes Pillow writes.
    png_files_to_host(files, nbytes)   the files as ``bytes``, behind one copy

Device tensors only (no CPU branch); forward-only.
"""
from __future__ import annotations

from typing import List, Tuple

import torch

from .. import _lib
from .attack import _bytes, _rows_to_host


def png_file_encode(u8: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``u8`` as PNG FILES, written on the device -> ``(files, nbytes)``: uint8 ``[B, max_bytes]`` and int32 ``[B]``, file ``b`` being
    ``files[b, :nbytes[b]]`` (``png_files_to_host`` cuts them out).  Four launches and a memset (the workspace is allocated here)."""
    u8 = _bytes(u8, "png_file_encode")
    b, h, w, c = u8.shape
    lib = _lib.load()
    stride = int(lib.ideas_png_file_max_bytes(c, h, w)) if h > 0 and w > 0 else 0
    if stride == 0:
        raise RuntimeError(f"png_file_encode: a file holds at least one pixel and at most 2^31 - 1 bytes, got {h} x {w} x {c}")
    files = torch.empty((b, stride), device=u8.device, dtype=torch.uint8)
    nbytes = torch.empty((b,), device=u8.device, dtype=torch.int32)
    if b:
        nwork = int(lib.ideas_png_file_encode_workspace_bytes(b, c, h, w))
        if nwork == 0:
            raise RuntimeError(f"png_file_encode: a call takes at most 2^31 - 1 rows, got {b} x {h}")
        work = torch.empty((nwork,), device=u8.device, dtype=torch.uint8)
        rc = lib.ideas_png_file_encode(_lib.ptr(files), _lib.ptr(nbytes), stride, _lib.ptr(u8), _lib.ptr(work), b, c, h, w, _lib.stream_ptr())
        _lib.check(rc, "ideas_png_file_encode")
    return files, nbytes


def png_files_to_host(files: torch.Tensor, nbytes: torch.Tensor) -> List[bytes]:
    """``png_file_encode``'s ``(files, nbytes)`` as a list of ``bytes``, one file each.  ONE device-to-host copy and no
    synchronisation in front of it: the lengths ride in front of the rows, whole (the longest file is not known on the host)."""
    rows = _rows_to_host(files, nbytes, "png_files_to_host")
    if rows is None:
        return []
    host, lengths = rows
    return [host[i, 4:4 + int(n)].tobytes() for i, n in enumerate(lengths)]
