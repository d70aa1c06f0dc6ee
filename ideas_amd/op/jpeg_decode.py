"""The JPEG FILE, read on the device (csrc/jpeg_decode.hip): what the receiver's ``Image.open`` does, without the host in the loop.

    parse_jpeg(data)                 the header of one baseline file, on the host -> ``JpegInfo`` (or ``UnsupportedJpeg``)
    jpeg_file_decode(files)          files that share shape, subsampling and Huffman tables -> ``(u8 [B, H, W, C], y, status)``:
                                     ONE host-to-device copy, then the kernels; no synchronisation
    jpeg_file_decode_grouped(files)  any mix of tables: one call a group, the bytes in input order; raises on a corrupt file

The contract is stated in include/ideas_hip.h ("The JPEG file, read") and restated by tests/jpegdecode_ref.py.  ``u8`` and ``y`` are
those of ``jpeg_file_roundtrip``: Pillow's pixels, and what ``data.u8_to_f32`` makes of them.  Device only; forward-only.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib

# natural index 8 u + v of zigzag position k
_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                    62, 63])


class UnsupportedJpeg(Exception):
    """A well-formed JPEG file that is not the kind the device decoder reads; ``reason`` says why."""

    def __init__(self, reason: str):
        super().__init__(reason)
        self.reason = reason


class CorruptJpeg(RuntimeError):
    """Files whose scan the device decoder flagged; ``indices`` are their positions in the call's input."""

    def __init__(self, message: str, indices: List[int]):
        super().__init__(message)
        self.indices = indices


@dataclass
class JpegInfo:
    c: int
    h: int
    w: int
    subsampling: int               # 0 = 4:4:4 (and every one-component file), 2 = 4:2:0
    qt: np.ndarray                 # uint16 [C, 64], natural order
    huff: bytes                    # [C, 2, 16 + 256]: per component its DC and AC table, counts then symbols, zero-padded
    scan_offset: int               # the first byte behind the SOS header


def parse_jpeg(data: bytes) -> JpegInfo:
    """The header of a baseline JPEG file.  ``UnsupportedJpeg`` for anything other than SOF0, 8-bit samples, 8-bit DQT, 1 or 3
    components, sampling 11-11-11 or 22-11-11, no restart interval, one scan over all components with Ss = 0, Se = 63, Ah = Al = 0, and
    no Adobe APP14 with a transform other than 1 on three components.  ``ValueError`` for a header that is truncated or inconsistent."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise ValueError("not a JPEG file: no SOI marker")
    qts: Dict[int, np.ndarray] = {}
    hts: Dict[Tuple[int, int], bytes] = {}
    frame = None                   # (h, w, [(id, sampling, tq)])
    adobe: Optional[int] = None
    pos = 2
    while True:
        if pos + 2 > n:
            raise ValueError("truncated JPEG header: no SOS marker")
        if data[pos] != 0xFF:
            raise ValueError(f"corrupt JPEG header: byte {pos} is no marker")
        m = data[pos + 1]
        if m == 0xFF:                                        # a fill byte
            pos += 1
            continue
        pos += 2
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            continue
        if m == 0xD9:
            raise ValueError("JPEG file without a scan")
        if pos + 2 > n:
            raise ValueError("truncated JPEG header")
        seglen = data[pos] << 8 | data[pos + 1]
        if seglen < 2 or pos + seglen > n:
            raise ValueError("truncated JPEG header")
        seg = data[pos + 2:pos + seglen]
        pos += seglen
        if m == 0xDB:
            i = 0
            while i < len(seg):
                if seg[i] >> 4:
                    raise UnsupportedJpeg("16-bit DQT")
                if i + 65 > len(seg):
                    raise ValueError("truncated DQT segment")
                t = np.zeros(64, np.uint16)
                t[_ZIGZAG] = np.frombuffer(seg, np.uint8, 64, i + 1)
                if (t == 0).any():
                    raise ValueError("a quantisation table holds a zero")
                qts[seg[i] & 15] = t
                i += 65
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                if i + 17 > len(seg):
                    raise ValueError("truncated DHT segment")
                count = sum(seg[i + 1:i + 17])
                if count > 256 or i + 17 + count > len(seg):
                    raise ValueError("truncated DHT segment")
                hts[(seg[i] >> 4, seg[i] & 15)] = bytes(seg[i + 1:i + 17 + count]).ljust(272, b"\0")
                i += 17 + count
        elif m == 0xC0:
            if len(seg) < 6 or len(seg) < 6 + 3 * seg[5]:
                raise ValueError("truncated SOF segment")
            if seg[0] != 8:
                raise UnsupportedJpeg(f"{seg[0]}-bit samples")
            if seg[5] not in (1, 3):
                raise UnsupportedJpeg(f"{seg[5]} components")
            frame = (seg[1] << 8 | seg[2], seg[3] << 8 | seg[4], [(seg[6 + 3 * k], seg[7 + 3 * k], seg[8 + 3 * k]) for k in range(seg[5])])
        elif 0xC1 <= m <= 0xCF and m not in (0xC8, 0xCC):
            raise UnsupportedJpeg("a progressive file (SOF2)" if m == 0xC2 else f"frame type SOF{m - 0xC0}")
        elif m == 0xDD:
            if len(seg) < 2:
                raise ValueError("truncated DRI segment")
            if seg[0] << 8 | seg[1]:
                raise UnsupportedJpeg("restart markers (DRI)")
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]
        elif m == 0xDA:
            break
    if frame is None:
        raise ValueError("SOS in front of SOF")
    h, w, comps = frame
    c = len(comps)
    if h == 0 or w == 0:
        raise UnsupportedJpeg("a frame without its size (DNL)")
    if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
        raise ValueError("corrupt SOS segment")
    if seg[0] != c:
        raise UnsupportedJpeg("more than one scan")
    if (seg[1 + 2 * c], seg[2 + 2 * c], seg[3 + 2 * c]) != (0, 63, 0):
        raise UnsupportedJpeg("a scan other than Ss = 0, Se = 63, Ah = Al = 0")
    sampling = tuple(s for _, s, _ in comps)
    if c == 3 and sampling not in ((0x11, 0x11, 0x11), (0x22, 0x11, 0x11)):
        raise UnsupportedJpeg("sampling " + "-".join(f"{s:02x}" for s in sampling) + " (only 4:4:4 and 4:2:0)")
    if c == 3 and adobe is not None and adobe != 1:
        raise UnsupportedJpeg(f"Adobe colour transform {adobe}")
    huff = b""
    for k, (cid, _, tq) in enumerate(comps):
        if seg[1 + 2 * k] != cid:
            raise UnsupportedJpeg("a scan whose components are not the frame's, in order")
        sel = seg[2 + 2 * k]
        if tq not in qts or (0, sel >> 4) not in hts or (1, sel & 15) not in hts:
            raise ValueError("a table the scan needs is not defined")
        huff += hts[(0, sel >> 4)] + hts[(1, sel & 15)]
    # behind the scan comes EOI: a second scan (or DHT, DQT, ... in front of one) is another kind of file
    i = data.find(b"\xff", pos)
    while i >= 0 and i + 1 < n and data[i + 1] == 0:
        i = data.find(b"\xff", i + 2)
    if i >= 0 and i + 1 < n and data[i + 1] != 0xD9:
        raise UnsupportedJpeg("restart markers in the scan" if 0xD0 <= data[i + 1] <= 0xD7 else "more than one scan")
    return JpegInfo(c, h, w, 2 if c == 3 and sampling[0] == 0x22 else 0, np.stack([qts[tq] for _, _, tq in comps]), huff, pos)


def _key(info: JpegInfo):
    return info.c, info.h, info.w, info.subsampling, info.huff


def _decode(files: Sequence[bytes], infos: Sequence[JpegInfo], device, return_coef: bool):
    if not torch.cuda.is_available():
        raise RuntimeError("ideas_amd ops run only on a HIP device (no CPU fallback)")
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError(f"ideas_amd ops run only on a HIP device (no CPU fallback); got device {device}")
    first = infos[0]
    for k, info in enumerate(infos):
        if _key(info) != _key(first):
            raise RuntimeError(f"jpeg_file_decode: file {k} differs from file 0 in shape, subsampling or Huffman tables "
                               "(jpeg_file_decode_grouped takes any mix)")
    b, c, h, w, sub = len(files), first.c, first.h, first.w, first.subsampling
    lengths = [len(f) - info.scan_offset for f, info in zip(files, infos)]
    stride = (max(max(lengths), 1) + 15) // 16 * 16
    # one pinned buffer, one copy: scans | lengths | tables | Huffman tables, each on a multiple of 16 bytes
    at_n = b * stride
    at_qt = at_n + (4 * b + 15) // 16 * 16
    at_huff = at_qt + (128 * b * c + 15) // 16 * 16
    host = torch.zeros(at_huff + 272 * 2 * c, dtype=torch.uint8).pin_memory()
    hv = host.numpy()
    for k, (f, info) in enumerate(zip(files, infos)):
        hv[k * stride:k * stride + lengths[k]] = np.frombuffer(f, np.uint8, lengths[k], info.scan_offset)
    hv[at_n:at_n + 4 * b] = np.asarray(lengths, "<i4").view(np.uint8)
    hv[at_qt:at_qt + 128 * b * c] = np.stack([info.qt for info in infos]).astype("<u2").reshape(-1).view(np.uint8)
    hv[at_huff:] = np.frombuffer(first.huff, np.uint8)
    with torch.cuda.device(device):
        dev = host.to(device, non_blocking=True)
        lib = _lib.load()
        nwork = int(lib.ideas_jpeg_file_decode_workspace_bytes(b, c, h, w, sub, stride))
        if nwork == 0:
            raise RuntimeError(f"jpeg_file_decode: {b} files of {h} x {w} x {c} are beyond what one call takes")
        work = torch.empty((nwork,), device=device, dtype=torch.uint8)
        out = torch.empty((b, h, w, c), device=device, dtype=torch.uint8)
        y = torch.empty((b, c, h, w), device=device, dtype=torch.float32, memory_format=torch.channels_last)
        status = torch.empty((b,), device=device, dtype=torch.int32)
        coef_y = coef_c = None
        if return_coef:
            bh, bw = (h + 7) // 8, (w + 7) // 8
            coef_y = torch.empty((b, bh, bw, 64), device=device, dtype=torch.int16)
            if c == 3:
                cbh, cbw = (bh, bw) if sub == 0 else ((h + 15) // 16, (w + 15) // 16)
                coef_c = torch.empty((b, 2, cbh, cbw, 64), device=device, dtype=torch.int16)
        rc = lib.ideas_jpeg_file_decode(_lib.ptr(out), _lib.ptr(y), _lib.ptr(coef_y), _lib.ptr(coef_c), _lib.ptr(status), dev.data_ptr(),
                                        dev.data_ptr() + at_n, stride, dev.data_ptr() + at_qt, dev.data_ptr() + at_huff, _lib.ptr(work),
                                        b, c, h, w, sub, _lib.stream_ptr())
        _lib.check(rc, "ideas_jpeg_file_decode")
    return (out, y, status, coef_y, coef_c) if return_coef else (out, y, status)


def jpeg_file_decode(files: Sequence[bytes], device=None, return_coef: bool = False):
    """JPEG files as ``bytes``, all of one ``(c, h, w, subsampling)`` and one set of Huffman tables (the quantisation tables may
    differ), decoded on the device -> ``(u8 [B, H, W, C], y [B, C, H, W] channels_last, status int32 [B])``: Pillow's pixels where
    ``status`` is 0; -1 marks a corrupt file, whose pixels are unspecified.  With ``return_coef`` also ``coef_y`` and ``coef_c`` in
    ``jpeg_file_roundtrip``'s layouts.  The scans, their lengths and the tables travel in ONE host-to-device copy from a pinned
    buffer; nothing is synchronised.  ``UnsupportedJpeg`` / ``ValueError`` from ``parse_jpeg``; ``RuntimeError`` naming the first file
    that does not match file 0."""
    files = [bytes(f) for f in files]
    if not files:
        raise RuntimeError("jpeg_file_decode: no files")
    return _decode(files, [parse_jpeg(f) for f in files], device, return_coef)


def jpeg_file_decode_grouped(files: Sequence[bytes], device=None) -> torch.Tensor:
    """Any JPEG files ``parse_jpeg`` takes, all of one ``(c, h, w)`` -> ``u8 [B, H, W, C]`` in input order: one ``jpeg_file_decode``
    per group of equal subsampling and Huffman tables.  Raises ``CorruptJpeg`` (a ``RuntimeError``) naming a corrupt file (this
    synchronises)."""
    files = [bytes(f) for f in files]
    if not files:
        raise RuntimeError("jpeg_file_decode_grouped: no files")
    infos = [parse_jpeg(f) for f in files]
    for k, info in enumerate(infos):
        if (info.c, info.h, info.w) != (infos[0].c, infos[0].h, infos[0].w):
            raise RuntimeError(f"jpeg_file_decode_grouped: file {k} is {info.h} x {info.w} x {info.c}, file 0 is "
                               f"{infos[0].h} x {infos[0].w} x {infos[0].c}")
    groups: Dict[tuple, List[int]] = {}
    for k, info in enumerate(infos):
        groups.setdefault(_key(info), []).append(k)
    outs, stats, order = [], [], []
    for members in groups.values():
        out, _, status = _decode([files[k] for k in members], [infos[k] for k in members], device, False)
        outs.append(out)
        stats.append(status)
        order += members
    out = outs[0] if len(outs) == 1 else torch.cat(outs)
    bad = (torch.cat(stats) != 0).nonzero().view(-1).tolist()
    if bad:
        bad = sorted(order[i] for i in bad)
        raise CorruptJpeg(f"jpeg_file_decode_grouped: file(s) {bad} are corrupt", bad)
    if order != sorted(order):
        out = out[torch.argsort(torch.tensor(order, device=out.device))]
    return out
