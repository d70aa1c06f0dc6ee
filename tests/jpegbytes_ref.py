"""CPU restatement of ``ideas_jpeg_file_encode`` (include/ideas_hip.h "The JPEG file, written"): the baseline JPEG FILE that libjpeg /
libjpeg-turbo writes with its defaults -- Pillow's ``Image.save(f, "JPEG", quality=Q, subsampling=0|2)`` -- from the quantised
coefficients of tests/jpegfile_ref.py: header, Huffman coding with the Annex K tables, bit packing, byte stuffing.  Everything is
lossless and defined to the byte: tests/test_jpeg_bytes.py holds this file to Pillow's own files with ``==`` on ``bytes``, and
tests/test_jpeg_bytes_gpu.py holds the kernels to this file.

``encode_coefs`` takes the coefficient arrays (so that a test can plant any int16) and returns ``(file, stats)``; ``file`` is ``None``
where a coefficient has no code.  ``stats`` counts the branches the coder took, so that a test can assert that its inputs reach them.
"""
import numpy as np

from attacks_ref import quant_tables
from jpegfile_ref import jpeg_file_ref, subsampling_code

# natural index 8 u + v of zigzag position k
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])

# ISO/IEC 10918-1 Annex K.3 - K.6: the number of codes of each length 1..16, and the symbols in order of their codes
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
_RUNS = [[0x10 * r + n for n in range(11)] for r in range(16)]     # _RUNS[r][n] = (r << 4) | n


def _tail(first_rows):
    """The long 16-bit end of both AC tables: runs r = first .. 15 with the sizes lo(r) .. 10, row by row."""
    return [v for r, lo in first_rows for v in _RUNS[r][lo:]]


AC_VALS = (
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
     0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82]
    + _tail([(0, 9), (1, 6), (2, 5), (3, 4), (4, 3), (5, 3), (6, 3), (7, 3), (8, 3), (9, 2), (10, 2), (11, 2), (12, 2), (13, 2), (14, 1),
             (15, 1)]),
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
     0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1]
    + _tail([(1, 7), (2, 6), (3, 5), (4, 3), (5, 3), (6, 3), (7, 3), (8, 2), (9, 2), (10, 2), (11, 2), (12, 2), (13, 2), (14, 2),
             (15, 2)]))
assert [len(v) for v in AC_VALS] == [162, 162] and [sum(b) for b in AC_BITS] == [162, 162]
assert all(sorted(v) == sorted([0x00, 0xF0] + [0x10 * r + n for r in range(16) for n in range(1, 11)]) for v in AC_VALS)


def huffman_codes(bits, vals):
    """{symbol: (code, length)}: the canonical codes of Annex C, lengths ascending, codes counting up."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


DC_CODES = tuple(huffman_codes(b, v) for b, v in zip(DC_BITS, DC_VALS))
AC_CODES = tuple(huffman_codes(b, v) for b, v in zip(AC_BITS, AC_VALS))


def header(c, h, w, quality, sub):
    """The bytes in front of the scan: SOI, JFIF APP0, DQT per table, SOF0, DHT per table, SOS.  328 bytes for C = 1, 623 for C = 3."""
    T = quant_tables(quality).reshape(2, 64)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i in range(2 if c == 3 else 1):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(int(T[i][z]) for z in ZIGZAG)
    out += b"\xff\xc0" + bytes([0, 8 + 3 * c, 8, h >> 8, h & 255, w >> 8, w & 255, c])
    out += bytes([1, 0x22 if c == 3 and sub == 2 else 0x11, 0])
    if c == 3:
        out += bytes([2, 0x11, 1, 3, 0x11, 1])
    for i in range(2 if c == 3 else 1):
        out += b"\xff\xc4\x00\x1f" + bytes([0x00 + i]) + bytes(DC_BITS[i]) + bytes(DC_VALS[i])
        out += b"\xff\xc4\x00\xb5" + bytes([0x10 + i]) + bytes(AC_BITS[i]) + bytes(AC_VALS[i])
    out += b"\xff\xda" + bytes([0, 6 + 2 * c, c, 1, 0x00])
    if c == 3:
        out += bytes([2, 0x11, 3, 0x11])
    out += b"\x00\x3f\x00"
    assert len(out) == (623 if c == 3 else 328)
    return bytes(out)


def scan_geometry(c, h, w, sub):
    """(hs, MCU rows, MCU columns, blocks of the scan): an MCU is 8 hs x 8 hs pixels, hs = 2 only for C = 3 at 4:2:0."""
    hs = 2 if c == 3 and sub == 2 else 1
    mh, mw = -(-h // (8 * hs)), -(-w // (8 * hs))
    return hs, mh, mw, mh * mw * (hs * hs + (2 if c == 3 else 0))


def max_bytes(c, h, w, sub):
    """The bound of ideas_jpeg_file_max_bytes: header + 416 a block + 3."""
    return (623 if c == 3 else 328) + 416 * scan_geometry(c, h, w, sub)[3] + 3


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n, self.total = bytearray(), 0, 0, 0

    def put(self, value, nbits):
        self.acc = (self.acc << nbits) | value
        self.n += nbits
        self.total += nbits
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1


def _extra(v, nb):
    """The low nb bits of v for v >= 0, of v - 1 otherwise."""
    return (v if v >= 0 else v - 1) & ((1 << nb) - 1)


def _code_block(bits, blk, pred, dc, ac, stats):
    """One block in natural order (int list of 64) behind the predictor; returns False where a coefficient has no code."""
    d = blk[0] - pred
    nb = abs(d).bit_length()
    if nb > 11:
        return False
    stats["dc_cat11"] += nb == 11
    code, length = dc[nb]
    bits.put(code, length)
    bits.put(_extra(d, nb), nb)
    r, nonzero = 0, 0
    for k in range(1, 64):
        v = blk[ZIGZAG[k]]
        if v == 0:
            r += 1
            continue
        nonzero += 1
        while r > 15:
            bits.put(*ac[0xF0])
            stats["zrl"] += 1
            r -= 16
        nb = abs(v).bit_length()
        if nb > 10:
            return False
        stats["ac_cat10"] += nb == 10
        code, length = ac[(r << 4) | nb]
        bits.put(code, length)
        bits.put(_extra(v, nb), nb)
        r = 0
    if r:
        bits.put(*ac[0x00])
    stats["no_eob"] += r == 0
    stats["eob_only"] += nonzero == 0
    return True


def encode_coefs(coef_y, coef_c, h, w, c, quality, sub):
    """coef_y int [bh, bw, 64], coef_c int [2, cbh, cbw, 64] or None (index 8 u + v) -> (the file as bytes, or None where a coefficient
    has no code; stats)."""
    sub = subsampling_code(sub)
    hs, mh, mw, nblocks = scan_geometry(c, h, w, sub)
    coef_y = np.asarray(coef_y).astype(np.int64)
    bh, bw = coef_y.shape[:2]
    assert (bh, bw) == (-(-h // 8), -(-w // 8))
    cy = coef_y.tolist()
    if c == 3:
        coef_c = np.asarray(coef_c).astype(np.int64)
        assert coef_c.shape == (2, mh, mw, 64)                                   # the chroma block grid is the MCU grid
        cc = coef_c.tolist()
    stats = dict(zrl=0, ac_cat10=0, dc_cat11=0, no_eob=0, eob_only=0, stuffed=0, right_dummy=0, bottom_dummy=0, pad_bits=0, blocks=0)
    bits, pred = _Bits(), [0, 0, 0]
    for my in range(mh):
        for mx in range(mw):
            last = None
            for sy in range(hs):
                for sx in range(hs):
                    by, bx = my * hs + sy, mx * hs + sx
                    if by < bh and bx < bw:
                        blk = cy[by][bx]
                    else:                                                         # a dummy block: the DC of the luma block before it
                        blk = [last[0]] + [0] * 63
                        stats["bottom_dummy" if by >= bh else "right_dummy"] += 1
                    if not _code_block(bits, blk, pred[0], DC_CODES[0], AC_CODES[0], stats):
                        return None, stats
                    pred[0], last = blk[0], blk
                    stats["blocks"] += 1
            for p in range(2 if c == 3 else 0):
                blk = cc[p][my][mx]
                if not _code_block(bits, blk, pred[1 + p], DC_CODES[1], AC_CODES[1], stats):
                    return None, stats
                pred[1 + p] = blk[0]
                stats["blocks"] += 1
    assert stats["blocks"] == nblocks
    stats["pad_bits"] = -bits.total % 8
    if stats["pad_bits"]:
        bits.put((1 << stats["pad_bits"]) - 1, stats["pad_bits"])
    scan = bytes(bits.out)
    stats["stuffed"] = scan.count(b"\xff")
    data = header(c, h, w, quality, sub) + scan.replace(b"\xff", b"\xff\x00") + b"\xff\xd9"
    assert len(data) <= max_bytes(c, h, w, sub)
    return data, stats


def jpeg_bytes_ref(img, quality, subsampling=2):
    """One image uint8 [H, W, C] -> (the JPEG file as bytes, stats)."""
    img = np.asarray(img)
    h, w, c = img.shape
    res = jpeg_file_ref(img, quality, subsampling)
    return encode_coefs(res["coef_y"], res["coef_c"], h, w, c, quality, subsampling)


# ------------------------------------------------------------------------------------------------- the inputs of the tests
KINDS = ("noise", "smooth", "binary", "flat")


def make_image(kind, h, w, c):
    """uint8 [h, w, c], made by integer arithmetic alone (no generator whose stream could change): "noise" a multiplicative hash of
    the position, "smooth" a ramp, "binary" 0 / 255 in 4-pixel stripes that swap every 8 x 8 block -- whole blocks of one level next
    to striped ones, so that DC steps and single AC coefficients get as large as they can --, "flat" one level."""
    yy, xx, cc = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), np.arange(c, dtype=np.uint64), indexing="ij")
    if kind == "noise":
        v = ((yy * 1315423911 + xx * 2654435761 + cc * 97 + 12345) * 2246822519 >> 17) & 255
    elif kind == "smooth":
        v = (5 * yy + 3 * xx + 70 * cc) % 256
    elif kind == "binary":
        block = (yy // 8 + 2 * (xx // 8) + cc) % 4                              # 0: black, 1: white, 2, 3: stripes either way
        stripe = np.where(block == 2, (xx // 4) % 2, (yy // 4 + 1) % 2)
        v = np.where(block < 2, block, stripe) * 255
    else:
        assert kind == "flat", kind
        v = np.full_like(yy, 77)
    return v.astype(np.uint8)
