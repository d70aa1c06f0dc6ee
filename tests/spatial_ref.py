"""numpy restatement of the spatial channel attacks (include/ideas_hip.h "Spatial channel attacks"), written without looking at
ideas_amd/op/resample.py: the window tables one output at a time as Pillow's C code walks them, the two integer passes, and the median
by padding and sorting.  Everything is integer arithmetic once the tables exist, so every comparison against it is byte for byte."""
import math

import numpy as np

PRECISION_BITS = 22           # Pillow: 32 - 8 - 2
KMAX = 32


def _round_coeffs(rows):
    """rows: per output a list of f64 weights -> int32 [n_out, ksize], zero-padded; (int)(0.5 + w 2^22) as normalize_coeffs_8bpc."""
    ksize = max(len(r) for r in rows)
    kk = np.zeros((len(rows), ksize), np.int32)
    for i, r in enumerate(rows):
        for j, w in enumerate(r):
            kk[i, j] = int(0.5 + w * (1 << PRECISION_BITS)) if w >= 0 else int(-0.5 + w * (1 << PRECISION_BITS))
    return kk


def bilinear_tables(n_in, n_out):
    """ImagingResample's precompute_coeffs for the triangle filter (support 1)."""
    scale = n_in / n_out
    support = max(scale, 1.0)
    lo, rows = [], []
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5))
        w = []
        for x in range(xmin, xmax):
            t = abs((x - center + 0.5) / support)
            w.append(1.0 - t if t < 1.0 else 0.0)
        total = sum(w)
        if total != 0:
            w = [v / total for v in w]
        lo.append(xmin)
        rows.append(w)
    return np.array(lo, np.int32), _round_coeffs(rows)


def gauss_tables(n, sigma):
    r = math.ceil(3.0 * sigma)
    lo, rows = [], []
    for i in range(n):
        xmin, xmax = max(0, i - r), min(n, i + r + 1)
        w = [math.exp(-((x - i) ** 2) / (2.0 * sigma * sigma)) for x in range(xmin, xmax)]
        total = sum(w)
        lo.append(xmin)
        rows.append([v / total for v in w])
    return np.array(lo, np.int32), _round_coeffs(rows)


def one_pass(img, lo, kk, axis):
    """One direction of the model on uint8 [..., H, W, C]: s = 2^21 + sum kk p in wrapping 32-bit arithmetic, the signed sum >> 22,
    clamped.  Input indices are clamped into the image before the load."""
    img = np.moveaxis(np.asarray(img), axis, 0)
    n_in = img.shape[0]
    out = np.empty((len(lo),) + img.shape[1:], np.uint8)
    for i in range(len(lo)):
        s = np.full(img.shape[1:], 1 << 21, np.uint64)
        for j in range(kk.shape[1]):
            idx = min(max(int(lo[i]) + j, 0), n_in - 1)
            s = (s + np.uint64(int(kk[i, j]) & 0xFFFFFFFF) * img[idx].astype(np.uint64)) & np.uint64(0xFFFFFFFF)
        signed = s.astype(np.int64)
        signed = np.where(signed >= 1 << 31, signed - (1 << 32), signed)
        out[i] = np.clip(signed >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resample_ref(img, horiz=None, vert=None):
    """uint8 [..., H, W, C] through the horizontal pass (tables (lo, kk) or None: skipped), rounded to bytes, then the vertical one."""
    out = np.asarray(img)
    if horiz is not None:
        out = one_pass(out, horiz[0], horiz[1], out.ndim - 2)
    if vert is not None:
        out = one_pass(out, vert[0], vert[1], out.ndim - 3)
    return np.ascontiguousarray(out)


def resize_ref(img, size):
    """Pillow's Image.resize((W2, H2), BILINEAR) on uint8 [..., H, W, C]; size = (H2, W2)."""
    h, w = img.shape[-3], img.shape[-2]
    h2, w2 = size
    return resample_ref(img, bilinear_tables(w, w2) if w2 != w else None, bilinear_tables(h, h2) if h2 != h else None)


def scaled_size(h, w, factor):
    return max(1, math.floor(h * factor + 0.5)), max(1, math.floor(w * factor + 0.5))


def scale_ref(img, factor):
    """The ``scale:F`` stage: to F times the size, an 8-bit image, and back."""
    h, w = img.shape[-3], img.shape[-2]
    return resize_ref(resize_ref(img, scaled_size(h, w, factor)), (h, w))


def gblur_ref(img, sigma):
    h, w = img.shape[-3], img.shape[-2]
    return resample_ref(img, gauss_tables(w, sigma), gauss_tables(h, sigma))


def median_ref(img, k):
    """The per-channel k x k median of uint8 [..., H, W, C] with replicated edges."""
    img = np.asarray(img)
    r = k // 2
    h, w = img.shape[-3], img.shape[-2]
    pad = [(0, 0)] * (img.ndim - 3) + [(r, r), (r, r), (0, 0)]
    p = np.pad(img, pad, mode="edge")
    win = np.stack([p[..., dy:dy + h, dx:dx + w, :] for dy in range(k) for dx in range(k)], axis=-1)
    return np.ascontiguousarray(np.sort(win, axis=-1)[..., (k * k) // 2])
