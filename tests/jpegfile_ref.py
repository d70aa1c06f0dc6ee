"""CPU restatement of ``ideas_jpeg_file_roundtrip`` (include/ideas_hip.h "The JPEG file channel"), in numpy int64: what libjpeg 6b /
libjpeg-turbo with its defaults (the integer "islow" DCT, 4:2:0 or 4:4:4, fancy upsampling) decodes from what it encoded, without the
entropy coder, which is lossless.  Everything is an integer, so there is no tie window: tests/test_jpeg_file.py holds this file to
Pillow's own bytes, and tests/test_jpeg_file_gpu.py holds the kernel to this file, both with ``array_equal``.

``jpeg_file_ref(img, quality, subsampling)`` runs one image uint8 [H, W, C] and returns every intermediate the GPU test needs.  Every
product of the two transforms is asserted to fit 32 bits with factors below 2^23 (what the kernel's 24-bit multiplies need), and the
inverse's output is asserted to stay inside the -512 .. 511 over which the library's range table is a clamp.
"""
import numpy as np

from attacks_ref import quant_tables, rgb_to_ycc, ycc_to_rgb

# round(c * 2^13) for the twelve constants of the Loeffler-Ligtenberg-Moschytz 8-point DCT as libjpeg factors it
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172
CONST_BITS, PASS1_BITS = 13, 2


def _mul(a, k):
    """a * k, asserted to be a product the kernel's __mul24 forms exactly: |a| < 2^23 and |a k| < 2^31."""
    a = np.asarray(a, np.int64)
    assert np.abs(a).max(initial=0) < (1 << 23), "a transform operand leaves 24 bits"
    p = a * k
    assert np.abs(p).max(initial=0) < (1 << 31), "a transform product leaves 32 bits"
    return p


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _odd_part(t4, t5, t6, t7):
    """The shared odd half of both transforms: (t4, t5, t6, t7) -> the four rotated sums, before any descale."""
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = _mul(z3 + z4, F_1_175)
    t4, t5, t6, t7 = _mul(t4, F_0_298), _mul(t5, F_2_053), _mul(t6, F_3_072), _mul(t7, F_1_501)
    z1, z2 = _mul(z1, -F_0_899), _mul(z2, -F_2_562)
    z3, z4 = _mul(z3, -F_1_961) + z5, _mul(z4, -F_0_390) + z5
    return t4 + z1 + z3, t5 + z2 + z4, t6 + z2 + z3, t7 + z1 + z4


def fdct_pass(d, first):
    """One 8-point forward pass along the last axis.  first: the row pass (results scaled up by 4), else the column pass."""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << PASS1_BITS, (t10 - t11) << PASS1_BITS
    else:
        o[0], o[4] = descale(t10 + t11, PASS1_BITS), descale(t10 - t11, PASS1_BITS)
    z1 = _mul(t12 + t13, F_0_541)
    o[2] = descale(z1 + _mul(t13, F_0_765), n)
    o[6] = descale(z1 + _mul(t12, -F_1_847), n)
    a4, a5, a6, a7 = _odd_part(t4, t5, t6, t7)
    o[7], o[5], o[3], o[1] = descale(a4, n), descale(a5, n), descale(a6, n), descale(a7, n)
    return np.stack(o, -1)


def idct_pass(c, first):
    """One 8-point inverse pass along the last axis.  first: the column pass (DESCALE by 11), else the row pass (by 18)."""
    c = [c[..., i] for i in range(8)]
    z1 = _mul(c[2] + c[6], F_0_541)
    t2, t3 = z1 + _mul(c[6], -F_1_847), z1 + _mul(c[2], F_0_765)
    assert np.abs(c[0] + c[4]).max(initial=0) < (1 << 18)
    t0, t1 = (c[0] + c[4]) << CONST_BITS, (c[0] - c[4]) << CONST_BITS
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = _odd_part(c[7], c[5], c[3], c[1])
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS + 3
    o = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    assert max(np.abs(v).max(initial=0) for v in o) < (1 << 31) - (1 << 17)
    return np.stack([descale(v, n) for v in o], -1)


def blocks_of(plane):
    """[8 bh, 8 bw] -> [bh, bw, 8, 8]."""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def plane_of(blk):
    bh, bw = blk.shape[:2]
    return blk.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def encode_plane(padded, T):
    """Samples int64 [8 bh, 8 bw] in 0..255, table T [8, 8] -> quantised coefficients int64 [bh, bw, 8, 8] ([u, v], u vertical)."""
    f = blocks_of(padded) - 128
    rows = fdct_pass(f, True)                                               # along v
    c = fdct_pass(rows.swapaxes(-1, -2), False).swapaxes(-1, -2)            # along u: 8 F
    return np.sign(c) * ((np.abs(c) + 4 * T) // (8 * T))


def decode_plane(q, T):
    """Quantised coefficients [bh, bw, 8, 8] -> samples int64 [8 bh, 8 bw] in 0..255."""
    dq = q * T
    cols = idct_pass(dq.swapaxes(-1, -2), True).swapaxes(-1, -2)            # along u
    s = idct_pass(cols, False)                                              # along v
    assert s.min(initial=0) >= -512 and s.max(initial=0) <= 511, "outside the range over which the library's table is a clamp"
    return np.clip(plane_of(s) + 128, 0, 255)


def pad8(plane):
    h, w = plane.shape
    return np.pad(plane, ((0, -h % 8), (0, -w % 8)), mode="edge")


def downsample_420(plane):
    """Full-resolution chroma [H, W] -> [8 ceil(ch / 8), 8 ceil(cw / 8)]: the columns are padded BEFORE the 2x2 average, the rows
    (beyond an even count) AFTER it."""
    h, w = plane.shape
    ch, cw = (h + 1) // 2, (w + 1) // 2
    p = np.pad(plane, ((0, h % 2), (0, 16 * ((cw + 7) // 8) - w)), mode="edge")
    bias = np.tile(np.array([1, 2], np.int64), p.shape[1] // 4)
    c = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    return np.pad(c, ((0, -ch % 8), (0, 0)), mode="edge")


def upsample_420(c, h, w):
    """Decoded chroma [ch, cw] (the real samples only) -> [h, w]: the triangle filter, or plain replication when cw <= 2."""
    ch, cw = c.shape
    if cw <= 2:
        return np.repeat(np.repeat(c, 2, 0), 2, 1)[:h, :w]
    i = np.arange(ch)
    up, down = c[np.maximum(i - 1, 0)], c[np.minimum(i + 1, ch - 1)]
    s = np.empty((2 * ch, cw), np.int64)
    s[0::2], s[1::2] = 3 * c + up, 3 * c + down
    j = np.arange(cw)
    left, right = s[:, np.maximum(j - 1, 0)], s[:, np.minimum(j + 1, cw - 1)]
    out = np.empty((2 * ch, 2 * cw), np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4
    return out[:h, :w]


def subsampling_code(subsampling):
    code = {"4:4:4": 0, "4:2:0": 2, 0: 0, 2: 2}.get(subsampling)
    assert code is not None, subsampling
    return code


def jpeg_file_ref(img, quality, subsampling=2):
    """One image uint8 [H, W, C] -> dict(out uint8 [H, W, C], coef_y int16 [bh, bw, 64], coef_c int16 [2, cbh, cbw, 64] or None
    (C = 1), chroma uint8 [2, ch, cw]: the decoded half-resolution Cb, Cr, or None (C = 1, 4:4:4))."""
    img = np.asarray(img)
    h, w, c = img.shape
    assert c in (1, 3)
    sub = subsampling_code(subsampling)
    T = quant_tables(quality)
    planes = rgb_to_ycc(img) if c == 3 else img[..., 0].astype(np.int64)[None]
    qy = encode_plane(pad8(planes[0]), T[0])
    y = decode_plane(qy, T[0])[:h, :w]
    res = {"coef_y": qy.reshape(*qy.shape[:2], 64).astype(np.int16), "coef_c": None, "chroma": None}
    if c == 1:
        res["out"] = y[..., None].astype(np.uint8)
        return res
    if sub == 0:
        qc = np.stack([encode_plane(pad8(planes[k]), T[1]) for k in (1, 2)])
        full = [decode_plane(qc[k], T[1])[:h, :w] for k in (0, 1)]
    else:
        ch, cw = (h + 1) // 2, (w + 1) // 2
        qc = np.stack([encode_plane(downsample_420(planes[k]), T[1]) for k in (1, 2)])
        half = np.stack([decode_plane(qc[k], T[1])[:ch, :cw] for k in (0, 1)])
        res["chroma"] = half.astype(np.uint8)
        full = [upsample_420(half[k], h, w) for k in (0, 1)]
    res["coef_c"] = qc.reshape(*qc.shape[:3], 64).astype(np.int16)
    res["out"] = ycc_to_rgb(np.stack([y, full[0], full[1]]))
    return res
