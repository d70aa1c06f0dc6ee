"""CPU restatement of ``ideas_jpeg_file_decode`` (include/ideas_hip.h "The JPEG file, read"): the header of a baseline JPEG file, a
SERIAL Huffman decode of its scan to the quantised coefficients and a status, and the pixels through tests/jpegfile_ref.py's inverse
transform, upsampler and colour conversion with the file's own tables.  Everything is an integer: tests/test_jpeg_decode.py holds
this file to Pillow's ``Image.open`` with ``array_equal``, and tests/test_jpeg_decode_gpu.py holds the kernels to this file.

``sync_rounds`` runs the fixed-point schedule of the device's synchronise kernel (subsequences of L bits, speculative start states,
hand the outputs on until nothing changes) and returns how many rounds it took, so that a test can prove that its input walks the loop.
"""
import numpy as np

from attacks_ref import ycc_to_rgb
from jpegbytes_ref import ZIGZAG, scan_geometry
from jpegfile_ref import decode_plane, upsample_420

SUBSEQ_BITS = 1024                 # include/ideas_hip.h::IDEAS_JPEG_SUBSEQ_BITS


class Unsupported(Exception):
    pass


def _be16(d, i):
    if i + 2 > len(d):
        raise ValueError("truncated JPEG header")
    return d[i] << 8 | d[i + 1]


def parse(data):
    """-> dict(c, h, w, subsampling, qt uint16 [C, 64] natural order, huff uint8 [C, 2, 272], scan_offset).  ``Unsupported`` for a
    file that is not baseline / 8-bit / 1 or 3 components / 4:4:4 or 4:2:0 / one scan / without restarts; ``ValueError`` for a
    truncated header."""
    d = bytes(data)
    if d[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    qt, ht, sof, adobe, i = {}, {}, None, None, 2
    while True:
        while _be16(d, i) == 0xFFFF:
            i += 1
        m = _be16(d, i)
        i += 2
        if m >> 8 != 0xFF:
            raise ValueError("no marker where one belongs")
        m &= 255
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            continue
        if m == 0xD9:
            raise ValueError("no scan")
        n = _be16(d, i)
        if n < 2 or i + n > len(d):
            raise ValueError("truncated JPEG header")
        body, i = d[i + 2:i + n], i + n
        if m == 0xDA:
            break
        if m == 0xDB:
            while body:
                if body[0] >> 4:
                    raise Unsupported("16-bit DQT")
                if len(body) < 65:
                    raise ValueError("truncated DQT")
                t = np.zeros(64, np.uint16)
                t[ZIGZAG] = list(body[1:65])
                if t.min() == 0:
                    raise ValueError("zero in a quantisation table")
                qt[body[0] & 15], body = t, body[65:]
        elif m == 0xC4:
            while body:
                k = sum(body[1:17])
                if len(body) < 17 + k or k > 256:
                    raise ValueError("truncated DHT")
                ht[body[0]] = np.frombuffer(body[1:17 + k].ljust(272, b"\0"), np.uint8)
                body = body[17 + k:]
        elif m == 0xC0:
            if len(body) < 6 or len(body) < 6 + 3 * body[5]:
                raise ValueError("truncated SOF")
            sof = body
        elif m == 0xC2:
            raise Unsupported("progressive")
        elif 0xC1 <= m <= 0xCF and m not in (0xC8, 0xCC):
            raise Unsupported("SOF%d" % (m - 0xC0))
        elif m == 0xDD:
            if _be16(body, 0):
                raise Unsupported("restart")
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
    if sof is None:
        raise ValueError("no SOF")
    if sof[0] != 8:
        raise Unsupported("precision")
    c, h, w = sof[5], _be16(sof, 1), _be16(sof, 3)
    if c not in (1, 3):
        raise Unsupported("components")
    if h == 0 or w == 0:
        raise Unsupported("DNL")
    comps = [tuple(sof[6 + 3 * k:9 + 3 * k]) for k in range(c)]
    if len(body) < 1 or len(body) != 4 + 2 * body[0]:
        raise ValueError("SOS")
    if body[0] != c:
        raise Unsupported("scans")
    if tuple(body[1 + 2 * c:]) != (0, 63, 0):
        raise Unsupported("spectral selection")
    samp = tuple(s for _, s, _ in comps)
    if c == 3 and samp not in ((0x11, 0x11, 0x11), (0x22, 0x11, 0x11)):
        raise Unsupported("sampling")
    if c == 3 and adobe not in (None, 1):
        raise Unsupported("Adobe transform")
    huff = np.zeros((c, 2, 272), np.uint8)
    for k, (cid, _, tq) in enumerate(comps):
        if body[1 + 2 * k] != cid:
            raise Unsupported("component order")
        sel = body[2 + 2 * k]
        if tq not in qt or (sel >> 4) not in ht or (0x10 | (sel & 15)) not in ht:
            raise ValueError("missing table")
        huff[k, 0], huff[k, 1] = ht[sel >> 4], ht[0x10 | (sel & 15)]
    end = _marker(d, i, len(d))
    if end is not None and d[end + 1] != 0xD9:
        raise Unsupported("restart" if 0xD0 <= d[end + 1] <= 0xD7 else "scans")
    return dict(c=c, h=h, w=w, subsampling=2 if c == 3 and samp[0] == 0x22 else 0, qt=np.stack([qt[tq] for _, _, tq in comps]), huff=huff,
                scan_offset=i)


def _marker(d, i, n):
    """the position of the first FF xx with xx != 00 in d[i:n], or None"""
    while True:
        i = d.find(b"\xff", i, n)
        if i < 0 or i + 1 >= n:
            return None
        if d[i + 1] != 0:
            return i
        i += 2


def unstuff(scan):
    """The entropy-coded segment -> its clean bytes: up to the first FF xx (xx != 00), without the 00 behind every FF."""
    scan = bytes(scan)
    end = _marker(scan, 0, len(scan))
    return scan[:len(scan) if end is None else end].replace(b"\xff\x00", b"\xff")


def _lut16(table):
    """One DHT table (16 counts + symbols) -> list of 65536: length << 8 | symbol for the code the 16 bits start with, 0 for none."""
    lut = np.zeros(1 << 16, np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(int(table[length - 1])):
            lo, hi = code << (16 - length), (code + 1) << (16 - length)
            if hi <= 1 << 16:
                lut[lo:hi] = length << 8 | int(table[16 + (k & 255)])
            code, k = code + 1, k + 1
        code <<= 1
    return lut.tolist()


class Stream:
    """The clean stream of one file with its tables: ``span`` is the decoder between two bit positions."""

    def __init__(self, info, scan):
        self.clean = unstuff(scan)
        self.nbits = 8 * len(self.clean)
        self.buf = self.clean + b"\xff" * 8                  # bits read past the end count as 1
        c = info["c"]
        self.hs, self.mh, self.mw, self.nblk = scan_geometry(c, info["h"], info["w"], info["subsampling"])
        self.nluma = self.hs * self.hs
        self.per_mcu = self.nluma + (2 if c == 3 else 0)
        self.luts = [[_lut16(info["huff"][k, t]) for t in (0, 1)] for k in range(c)]

    def span(self, p, slot, z, end, sink=None):
        """Symbols from state (p, slot, z) until p reaches ``end`` -> (p, slot, z, blocks finished).  sink(kind, a, b): ("dc", diff,
        None), ("ac", zigzag index, value), ("error", None, None), ("done", None, None)."""
        buf, done = self.buf, 0
        while p < end:
            comp = 0 if slot < self.nluma else slot - self.nluma + 1
            i = p >> 3
            bits = (int.from_bytes(buf[i:i + 5], "big") >> (8 - (p & 7))) & 0xFFFFFFFF
            e = self.luts[comp][1 if z else 0][bits >> 16]
            length, sym = e >> 8, e & 255
            bad = length == 0
            if bad:
                length = 16
            nb, run = (sym, 0) if z == 0 else (sym & 15, sym >> 4)
            bad = bad or nb > (11 if z == 0 else 10)
            finished = False
            if bad:
                p += length
                if sink:
                    sink("error", None, None)
                finished = True
            else:
                v = 0
                if nb:
                    v = (bits >> (32 - length - nb)) & ((1 << nb) - 1)
                    if v < 1 << (nb - 1):
                        v -= (1 << nb) - 1
                p += length + nb
                if z == 0:
                    if sink:
                        sink("dc", v, None)
                    z = 1
                elif nb == 0:
                    if run == 15:
                        z += 16
                        if z > 63:
                            if sink:
                                sink("error", None, None)
                            finished = True
                    else:
                        finished = True
                else:
                    z += run
                    if z > 63:
                        if sink:
                            sink("error", None, None)
                        finished = True
                    else:
                        if sink:
                            sink("ac", z, v)
                        z += 1
                        finished = z == 64
            if finished:
                if sink:
                    sink("done", None, None)
                done += 1
                z, slot = 0, (slot + 1) % self.per_mcu
        return p, slot, z, done


def decode_coefs(info, scan):
    """The serial decode -> (coef_y int16 [bh, bw, 64], coef_c int16 [2, mh, mw, 64] or None, status 0 / -1).  Blocks behind the
    scan's count (the padding bits decode as garbage) are ignored; a corrupt file's coefficients mean nothing."""
    s = Stream(info, scan)
    c, h, w = info["c"], info["h"], info["w"]
    bh, bw = -(-h // 8), -(-w // 8)
    cy = np.zeros((bh, bw, 64), np.int64)
    cc = np.zeros((2, s.mh, s.mw, 64), np.int64) if c == 3 else None
    state = dict(blk=0, bad=False, pred=[0, 0, 0])

    def target():
        """(array, index tuple, component) of block state["blk"]; array None for a dummy"""
        mcu, slot = divmod(state["blk"], s.per_mcu)
        my, mx = divmod(mcu, s.mw)
        if slot < s.nluma:
            by, bx = my * s.hs + (slot >> 1 if s.hs == 2 else 0), mx * s.hs + (slot & 1 if s.hs == 2 else 0)
            return (cy if by < bh and bx < bw else None), (by, bx), 0
        return cc, (slot - s.nluma, my, mx), slot - s.nluma + 1

    def sink(kind, a, b):
        if state["blk"] >= s.nblk:
            return
        if kind == "error":
            state["bad"] = True
        elif kind == "done":
            state["blk"] += 1
        else:
            arr, idx, comp = target()
            if kind == "dc":
                state["pred"][comp] += a
                state["bad"] |= not -2047 <= state["pred"][comp] <= 2047
                a, b = 0, state["pred"][comp]
            if arr is not None:
                arr[idx + (int(ZIGZAG[a]),)] = b

    done = s.span(0, 0, 0, s.nbits, sink)[3]
    status = -1 if state["bad"] or done < s.nblk else 0
    return cy.astype(np.int16), None if cc is None else cc.astype(np.int16), status


def pixels(info, coef_y, coef_c):
    """Steps 7-9 of the file channel with the file's tables -> uint8 [H, W, C]."""
    c, h, w = info["c"], info["h"], info["w"]
    T = info["qt"].astype(np.int64).reshape(c, 8, 8)

    def plane(q, t):
        return decode_plane(q.astype(np.int64).reshape(*q.shape[:2], 8, 8), t)

    y = plane(coef_y, T[0])[:h, :w]
    if c == 1:
        return y[..., None].astype(np.uint8)
    if info["subsampling"] == 0:
        full = [plane(coef_c[k], T[1 + k])[:h, :w] for k in (0, 1)]
    else:
        ch, cw = (h + 1) // 2, (w + 1) // 2
        full = [upsample_420(plane(coef_c[k], T[1 + k])[:ch, :cw], h, w) for k in (0, 1)]
    return ycc_to_rgb(np.stack([y, full[0], full[1]]))


def decode_ref(data):
    """One file -> dict(info, coef_y, coef_c, status, out uint8 [H, W, C] or None where the file is corrupt)."""
    info = parse(data)
    cy, cc, status = decode_coefs(info, bytes(data)[info["scan_offset"]:])
    return dict(info=info, coef_y=cy, coef_c=cc, status=status, out=pixels(info, cy, cc) if status == 0 else None)


def sync_rounds(data, L=SUBSEQ_BITS):
    """The fixed-point schedule of the synchronise kernel on one file -> (rounds, nsub): the number of rounds in which a subsequence was
    decoded.  Asserts the loop's bound (nsub + 1 rounds) and that the converged states are the serial decoder's."""
    info = parse(data)
    s = Stream(info, bytes(data)[info["scan_offset"]:])
    nsub = -(-s.nbits // L)
    ends = [min((i + 1) * L, s.nbits) for i in range(nsub)]
    state = [(i * L, 0, 0) for i in range(nsub)]
    dirty, out, rounds = [True] * nsub, [None] * nsub, 0
    for _ in range(nsub + 1):
        if not any(dirty):
            break
        rounds += 1
        for i in range(nsub):
            if dirty[i]:
                out[i] = s.span(*state[i], ends[i])
                dirty[i] = False
        for i in range(1, nsub):
            if out[i - 1][:3] != state[i]:
                state[i], dirty[i] = out[i - 1][:3], True
    assert not any(dirty), "no fixed point inside the bound"
    serial = (0, 0, 0)
    for i in range(nsub):
        assert state[i] == serial, (i, state[i], serial)
        serial = s.span(*serial, ends[i])[:3]
    return rounds, nsub
