"""CPU restatement of the channel attacks of csrc/attack.hip (include/ideas_hip.h "Channel attacks"), in numpy.

``jpeg_ref`` is the model of ``ideas_jpeg_roundtrip`` for one image: integer colour, replicated edges, the orthonormal 8x8 DCT in f64,
the IJG-scaled Annex K quantiser, the four rational coefficients (0,0), (0,4), (4,0), (4,4) in integers, and back.  It returns every
intermediate the GPU test needs: the unquantised ratios F / T, the quantised coefficients, the samples before the final rounding and
the bytes.  ``jpeg_from_coef`` is the decode half alone, from GIVEN coefficients.  ``pixel_attack_ref`` restates ``ideas_pixel_attack``
in f32, one rounding per step.

TOL, the tie window.  The kernel forms every 8-point pass as a sum of at most 8 products of f32 numbers, and a 2-D coefficient or
sample as two such passes.  With u = 2^-24 and the usual bound |fl(sum) - sum| <= n u sum|terms| (n = 8 additions and products, + 1 for
the rounded cosine), a pass over inputs of magnitude <= m errs by at most 9 u A m, where A = sum_j |b_k(j)| is 8 for the rows k = 0, 4
(weights +-1) and <= 5.23 for the others.  Level-shifted samples are <= 128 in magnitude.  Two passes: the second one's own error plus
the first one's carried through, 2 * 9 u * (A_u A_v * 128).  A non-rational coefficient has at most one index in {0, 4}:

    one index in {0, 4}:  scale 1 / (4 sqrt 2),  A_u A_v <= 8 * 5.23   ->  18 u * 5356 * 0.1768 = 1.02e-3
    no index in {0, 4}:   scale 1 / 4,           A_u A_v <= 5.23^2     ->  18 u * 3501 * 0.25   = 0.94e-3

The scaling, the division by T >= 1 and the + 0.5 add three more roundings of a number below 948: 3 u * 948 = 0.17e-3.  In all at most
1.2e-3 in units of F / T.  The decode side is the same two passes over dequantised coefficients of the same size (a quantised
coefficient times T differs from F by at most T / 2, and what that adds to a sample is bounded the same way), the + 128 and the + 0.5.
TOL = 1.5e-3 covers both with a quarter to spare.  Outside the window the kernel must agree with this file exactly.
"""
import numpy as np

TOL = 1.5e-3

LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64).reshape(8, 8)
CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                   47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64).reshape(8, 8)
S4 = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.int64)        # the k = 4 cosine row without its 1 / sqrt 2
S0 = np.ones(8, np.int64)
RATIONAL = np.zeros((8, 8), bool)
RATIONAL[np.ix_([0, 4], [0, 4])] = True


def quant_tables(quality):
    """int64 [2, 8, 8] (luminance, chrominance), index [u, v] with u the vertical frequency: Annex K scaled by the IJG rule."""
    q = int(quality)
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((np.stack((LUMA, CHROMA)) * s + 50) // 100, 1, 255)


def dct_matrix():
    """D[k, j] = (c(k) / 2) cos((2 j + 1) k pi / 16), f64: F = D f D^T is the orthonormal 8x8 DCT-II."""
    k, j = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    d = 0.5 * np.cos((2 * j + 1) * k * np.pi / 16)
    d[0] *= 1 / np.sqrt(2.0)
    return d


def rgb_to_ycc(img):
    """uint8 / int [H, W, 3] -> int64 planes [3, H, W] (Y, Cb, Cr), 16-bit fixed point as the IJG library's."""
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return np.stack((y, cb, cr))


def ycc_to_rgb(planes):
    """int64 planes [3, H, W] in 0..255 -> uint8 [H, W, 3]."""
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack((r, g, b), -1), 0, 255).astype(np.uint8)


def to_planes(img):
    img = np.asarray(img)
    assert img.ndim == 3 and img.shape[2] in (1, 3)
    return rgb_to_ycc(img) if img.shape[2] == 3 else img[..., 0].astype(np.int64)[None]


def to_blocks(planes):
    """[C, H, W] -> [C, bh, bw, 8, 8] of the planes padded to multiples of 8 by replicating the last row and column."""
    c, h, w = planes.shape
    p = np.pad(planes, ((0, 0), (0, -h % 8), (0, -w % 8)), mode="edge")
    return p.reshape(c, p.shape[1] // 8, 8, p.shape[2] // 8, 8).transpose(0, 1, 3, 2, 4)


def from_blocks(blk):
    c, bh, bw = blk.shape[:3]
    return blk.transpose(0, 1, 3, 2, 4).reshape(c, bh * 8, bw * 8)


def plane_tables(quality, c):
    t = quant_tables(quality)
    return t[[0, 1, 1][:c]][:, None, None]                    # [C, 1, 1, 8, 8]


def encode(img, quality):
    """-> (ratio f64 [C, bh, bw, 8, 8] = F / T before rounding, coef int16 [C, bh, bw, 64] at index 8 u + v)."""
    f = to_blocks(to_planes(img)) - 128
    c = f.shape[0]
    T = plane_tables(quality, c)
    D = dct_matrix()
    ratio = (D @ f.astype(np.float64) @ D.T) / T
    q = np.sign(ratio) * np.floor(np.abs(ratio) + 0.5)
    # the four rational coefficients: F = S / 8 with S an integer, rounded half away from zero in integers
    sgn = np.stack((S0, S4))
    S = np.einsum("ai,cyxij,bj->cyxab", sgn, f, sgn)          # [C, bh, bw, 2, 2], a, b index (0, 4)
    Tr = np.broadcast_to(T, f.shape)[..., ::4, ::4]
    qr = np.sign(S) * ((np.abs(S) + 4 * Tr) // (8 * Tr))
    ratio[..., ::4, ::4] = S / (8.0 * Tr)
    q[..., ::4, ::4] = qr
    return ratio, q.astype(np.int16).reshape(*q.shape[:3], 64)


def decode(coef, h, w, quality):
    """coef int [C, bh, bw, 64] -> (pre f64 [C, 8 bh, 8 bw]: the samples before floor(v + 0.5) and the clamp, bytes uint8 [h, w, C])."""
    coef = np.asarray(coef).astype(np.int64)
    c = coef.shape[0]
    dq = coef.reshape(*coef.shape[:3], 8, 8) * plane_tables(quality, c)
    D = dct_matrix()
    rest = np.where(RATIONAL, 0, dq).astype(np.float64)
    sgn = np.stack((S0, S4))
    eighths = np.einsum("ai,cyxab,bj->cyxij", sgn, dq[..., ::4, ::4], sgn)       # exact: an integer, to be divided by 8
    pre = from_blocks(D.T @ rest @ D + eighths / 8.0 + 128.0)
    planes = np.clip(np.floor(pre + 0.5), 0, 255).astype(np.int64)[:, :h, :w]
    out = ycc_to_rgb(planes) if c == 3 else planes[0][..., None].astype(np.uint8)
    return pre, out


def jpeg_ref(img, quality):
    """One image uint8 [H, W, C] through the model.  -> dict(ratio, coef, pre, out)."""
    img = np.asarray(img)
    ratio, coef = encode(img, quality)
    pre, out = decode(coef, img.shape[0], img.shape[1], quality)
    return {"ratio": ratio, "coef": coef, "pre": pre, "out": out}


def jpeg_from_coef(coef, h, w, quality):
    return decode(coef, h, w, quality)


def near_tie(v, tol=TOL):
    """|v| (coefficient ratios) or v (samples) within ``tol`` of k + 0.5."""
    a = np.abs(v)
    return np.abs(a - np.floor(a) - 0.5) <= tol


def pixel_attack_ref(x, gain=1.0, offset=0.0, sigma=0.0, sp=0.0, noise=None, u=None):
    """ideas_pixel_attack in numpy f32, one rounding per step.  x uint8 [..., H, W, C]; noise like x; u [..., H, W]."""
    f = np.float32
    with np.errstate(invalid="ignore"):
        v = (x.astype(np.float32) - f(127.5)) * f(gain)
        v = v + f(127.5)
        v = v + f(offset)
        if noise is not None:
            v = v + f(sigma) * noise.astype(np.float32)
        t = v + f(0.5)
        t = np.where(np.isnan(t), f(0), np.minimum(np.maximum(t, f(0)), f(255)))
    r = t.astype(np.int32).astype(np.uint8)
    if u is not None:
        half = f(sp) / f(2)
        uu = u.astype(np.float32)[..., None]
        r = np.where(uu < half, np.uint8(0), r)
        r = np.where(uu >= f(1) - half, np.uint8(255), r).astype(np.uint8)
    return r


def u8_to_f32_ref(u8):
    """(u8 / 255 - 0.5) / 0.5 in f32: what ideas_image_u8_to_f32(mean .5, std .5) makes of the bytes."""
    f = np.float32
    return (u8.astype(np.float32) / f(255) - f(0.5)) / f(0.5)
