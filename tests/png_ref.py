"""The PNG file written on the device (csrc/png_bytes.hip), restated in numpy: the contract of include/ideas_hip.h, "The PNG file,
written", step by step -- row filters and their choice, stripes, length-limited Huffman codes, the block header, bit packing and the
checksums.  Whole files as ``bytes``.  ``zlib`` is used for ``crc32`` and ``adler32`` only; tests/test_png_file.py holds these files
to zlib's inflate and to Pillow's reader."""
import struct
import zlib

import numpy as np

STRIPE_ROWS = 32              # include/ideas_hip.h::IDEAS_PNG_STRIPE_ROWS
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)       # RFC 1951 3.2.7
HEADER_MAX_BITS = 17 + 19 * 3 + 258 * 7
SIGNATURE = b"\x89PNG\r\n\x1a\n"


# ------------------------------------------------------------------------------------------------- filters
def filter_rows(img):
    """img uint8 [H, W, C] -> (filtered uint8 [H, 1 + W C]: the type byte and the residuals of every row; types [H])."""
    h, w, c = img.shape
    n = w * c
    raw = img.reshape(h, n).astype(np.int32)
    up = np.vstack([np.zeros((1, n), np.int32), raw[:-1]])                       # the RAW row above, zero above the first
    a = np.hstack([np.zeros((h, c), np.int32), raw[:, :n - c]]) if n > c else np.zeros((h, n), np.int32)
    cc = np.hstack([np.zeros((h, c), np.int32), up[:, :n - c]]) if n > c else np.zeros((h, n), np.int32)
    p = a + up - cc
    pa, pb, pc = np.abs(p - a), np.abs(p - up), np.abs(p - cc)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, cc))
    preds = (np.zeros_like(raw), a, up, (a + up) >> 1, paeth)
    res = np.stack([(raw - q) & 255 for q in preds])                             # [5, H, n]
    cost = np.where(res < 128, res, 256 - res).sum(axis=2)                       # |residual| as int8
    types = cost.argmin(axis=0)                                                  # the first minimum: a tie goes to the lowest type
    out = np.empty((h, n + 1), np.uint8)
    out[:, 0] = types
    out[:, 1:] = res[types, np.arange(h)]
    return out, types


# ------------------------------------------------------------------------------------------------- code lengths
def huffman_depths(freq):
    """The plain Huffman tree of the used symbols of ``freq``: leaves in ascending (frequency, symbol); the two lightest nodes are
    merged, a leaf before an internal node of the same weight, internal nodes in the order they were made.  -> (symbols in that leaf
    order, their depths)."""
    order = sorted((int(f), s) for s, f in enumerate(freq) if f > 0)
    n = len(order)
    w = [f for f, _ in order] + [0] * max(n - 1, 0)
    parent = [0] * (2 * n - 1)
    li, ii, nxt = 0, n, n
    for _ in range(n - 1):
        pick = []
        for _ in range(2):
            if li < n and (ii >= nxt or w[li] <= w[ii]):
                pick.append(li)
                li += 1
            else:
                pick.append(ii)
                ii += 1
        w[nxt] = w[pick[0]] + w[pick[1]]
        parent[pick[0]] = parent[pick[1]] = nxt
        nxt += 1
    depths = []
    for r in range(n):
        d, k = 0, r
        while k != 2 * n - 2:
            k = parent[k]
            d += 1
        depths.append(d)
    return [s for _, s in order], depths


def limited_lengths(freq, maxbits):
    """Code lengths of at most ``maxbits``: the depths of ``huffman_depths`` counted per length, depths beyond the limit counted at the
    limit, which can leave the Kraft sum above 1.  While it is, by ``over`` units of 2^-maxbits: the longest length below the limit that
    has a code gives one up, the length below it gains two, the limit loses one -- one unit less (the step of zlib's gen_bitlen).  The
    counts are handed out in leaf order, the longest lengths to the lightest leaves.  -> uint8 [len(freq)], 0 for unused symbols."""
    syms, depths = huffman_depths(freq)
    count = [0] * (maxbits + 1)
    for d in depths:
        count[min(max(d, 1), maxbits)] += 1
    over = sum(count[length] << (maxbits - length) for length in range(1, maxbits + 1)) - (1 << maxbits)
    for _ in range(max(over, 0)):
        bits = maxbits - 1
        while count[bits] == 0:
            bits -= 1
        count[bits] -= 1
        count[bits + 1] += 2
        count[maxbits] -= 1
    lens = np.zeros(len(freq), np.uint8)
    r = 0
    for length in range(maxbits, 0, -1):
        for _ in range(count[length]):
            lens[syms[r]] = length
            r += 1
    return lens


def canonical_codes(lens, maxbits):
    """RFC 1951 3.2.2 -> the codes, bit-reversed: as they go into the stream from its least significant bit."""
    count = np.bincount(lens, minlength=maxbits + 1)
    nxt, code = [0] * (maxbits + 1), 0
    for length in range(1, maxbits + 1):
        code = (code + (int(count[length - 1]) if length > 1 else 0)) << 1
        nxt[length] = code
    out = np.zeros(len(lens), np.uint32)
    for s, length in enumerate(lens):
        if length:
            out[s] = int(format(nxt[length], "0%db" % length)[::-1], 2)
            nxt[length] += 1
    return out


def plain_huffman_depth(freq):
    """The depth of the unrestricted tree (for the length-limit fixture)."""
    return max(huffman_depths(freq)[1])


# ------------------------------------------------------------------------------------------------- deflate
class Bits:
    """A bit string in stream order (bit k of the stream is bit k % 8 of byte k // 8)."""

    def __init__(self):
        self.parts = []

    def put(self, value, nbits):
        self.parts.append(((int(value) >> np.arange(nbits)) & 1).astype(np.uint8))

    def put_array(self, bits):
        self.parts.append(bits)

    def tobytes(self):
        return np.packbits(np.concatenate(self.parts), bitorder="little").tobytes()


def stripe_block(out, data, final):
    """One deflate block for the filtered bytes ``data`` of a stripe."""
    freq = np.bincount(data, minlength=257)
    freq[256] = 1
    lens = limited_lengths(freq, 15)
    codes = canonical_codes(lens, 15)
    seq = np.concatenate([lens, [1]]).astype(np.uint8)                           # 257 literal lengths, one distance code of length 1
    cl_freq = np.bincount(seq, minlength=19)                                     # no run-length symbols: 16, 17 and 18 stay unused
    cl_lens = limited_lengths(cl_freq, 7)
    cl_codes = canonical_codes(cl_lens, 7)
    ncl = max(k for k in range(19) if cl_lens[CL_ORDER[k]]) + 1
    ncl = max(ncl, 4)
    out.put(1 if final else 0, 1)
    out.put(2, 2)
    out.put(0, 5)                                                                # HLIT: 257 literal / length codes
    out.put(0, 5)                                                                # HDIST: 1 distance code
    out.put(ncl - 4, 4)
    for k in range(ncl):
        out.put(cl_lens[CL_ORDER[k]], 3)
    for v in seq:
        out.put(cl_codes[v], cl_lens[v])
    syms = np.concatenate([data.astype(np.int64), [256]])
    sl = lens[syms].astype(np.int64)
    at = np.cumsum(sl) - sl
    bits = np.zeros(int(sl.sum()), np.uint8)
    for k in range(15):
        m = sl > k
        bits[at[m] + k] = (codes[syms[m]] >> k) & 1
    out.put_array(bits)


def deflate(filtered):
    """filtered uint8 [H, 1 + W C] -> the deflate stream: one dynamic block per stripe of STRIPE_ROWS rows, literals only."""
    h = filtered.shape[0]
    out = Bits()
    for r0 in range(0, h, STRIPE_ROWS):
        stripe_block(out, filtered[r0:r0 + STRIPE_ROWS].reshape(-1), r0 + STRIPE_ROWS >= h)
    return out.tobytes()


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def png_file(img):
    """img uint8 [H, W, C], C = 1 or 3 -> (the file, the filtered bytes)."""
    h, w, c = img.shape
    assert c in (1, 3) and img.dtype == np.uint8
    filtered, _ = filter_rows(img)
    z = b"\x78\x01" + deflate(filtered) + struct.pack(">I", zlib.adler32(filtered.tobytes()))
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 0 if c == 1 else 2, 0, 0, 0)
    return SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"IDAT", z) + chunk(b"IEND", b""), filtered.tobytes()


def max_bytes(c, h, w):
    """ideas_png_file_max_bytes: every symbol at most 15 bits, every block header at most HEADER_MAX_BITS; 0 beyond 2^31 - 1."""
    if c not in (1, 3) or h <= 0 or w <= 0:
        return 0
    stripes = (h + STRIPE_ROWS - 1) // STRIPE_ROWS
    bits = stripes * (HEADER_MAX_BITS + 15) + 15 * h * (1 + w * c)
    total = 8 + 25 + 12 + 2 + (bits + 7) // 8 + 4 + 12
    return total if total <= 2 ** 31 - 1 else 0


def split_chunks(data):
    """The chunks of a PNG file -> [(type, payload, crc)]."""
    assert data[:8] == SIGNATURE
    at, out = 8, []
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        out.append((data[at + 4:at + 8], data[at + 8:at + 8 + n], struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0]))
        at += 12 + n
    assert at == len(data)
    return out


# ------------------------------------------------------------------------------------------------- fixtures
def pink_noise(h, w, c, seed):
    """Seeded 1/f noise as uint8 [h, w, c]: what a photograph's spectrum looks like."""
    rng = np.random.default_rng(seed)
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
    f = np.sqrt(fy * fy + fx * fx)
    f[0, 0] = 1.0
    planes = []
    for _ in range(c):
        spec = np.fft.fft2(rng.standard_normal((h, w))) / f
        x = np.real(np.fft.ifft2(spec))
        x = (x - x.mean()) / (x.std() + 1e-12)
        planes.append(np.clip(128 + 48 * x, 0, 255))
    return np.stack(planes, axis=2).round().astype(np.uint8)


def fibonacci_image():
    """One stripe (32 x 200 x 3) whose filtered bytes have Fibonacci-like frequencies, so that the plain Huffman tree is deeper than
    15.  The bytes are 0, 1, -1, 2, -2, ... in shuffled order, the commonest nearest to zero: independent draws around zero cost
    filter None less than any difference of two of them, so the rows stay as they are and the frequencies survive the filters."""
    fib = [1, 1]                                         # f(k) = f(k-1) + f(k-2) + 1: no ties for the tree to balance itself on
    while sum(fib) + fib[-1] + fib[-2] + 1 <= 32 * 600:
        fib.append(fib[-1] + fib[-2] + 1)
    fib[-1] += 32 * 600 - sum(fib)
    vals = []
    for k, f in enumerate(reversed(fib)):
        vals += [((k + 1) // 2 * (1 if k % 2 else -1)) % 256] * f
    vals = np.array(vals, np.uint8)
    np.random.default_rng(5).shuffle(vals)
    return vals.reshape(32, 200, 3)


def make_image(kind, h, w, c, seed=0):
    rng = np.random.default_rng([seed, h, w, c])
    if kind == "noise":
        return rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == "flat":
        return np.full((h, w, c), 77, np.uint8)
    if kind == "pink":
        return pink_noise(h, w, c, seed)
    if kind == "smooth":
        y, x = np.mgrid[0:h, 0:w]
        base = (3 * x + 2 * y)[..., None] + 40 * np.arange(c)
        return ((base + rng.integers(0, 4, (h, w, c))) % 256).astype(np.uint8)
    if kind == "fibonacci":
        assert (h, w, c) == (32, 200, 3)
        return fibonacci_image()
    raise ValueError(kind)


# name -> (kind, h, w, c): the fixtures tests/golden/png_pinned.npz records the files of
FIXTURES = {
    "one_grey": ("noise", 1, 1, 1),
    "one_rgb": ("noise", 1, 1, 3),
    "odd_rgb": ("noise", 13, 21, 3),
    "smooth_grey": ("smooth", 40, 24, 1),
    "stripe_32": ("smooth", 32, 33, 3),
    "stripe_33": ("smooth", 33, 33, 3),
    "stripe_70": ("noise", 70, 33, 3),
    "wide": ("smooth", 2, 1400, 3),
    "flat": ("flat", 40, 33, 3),
    "fibonacci": ("fibonacci", 32, 200, 3),
    "noise_64": ("noise", 64, 64, 3),
    "pink_64_grey": ("pink", 64, 64, 1),
    "pink_256": ("pink", 256, 256, 3),
}
CONTENT_LIKE = ("pink_256", "pink_64_grey")


def fixture(name):
    return make_image(*FIXTURES[name])
