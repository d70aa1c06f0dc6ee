"""Host-side checks of the JPEG file read on the device: the Python restatement (tests/jpegdecode_ref.py) against the pixels Pillow
reads, as recorded in tests/golden/jpegdecode.npz (written by tests/golden/make_golden_jpegdecode.py) and LIVE where Pillow is installed;
the header parser of the op against the restatement's; the restatement's coefficients against the encoder side's; the fixed-point
schedule of the synchronise kernel; the C ABI of csrc/jpeg_decode.hip with its size query and argument errors; extract.py's flag.
No GPU, no tolerances: everything is compared as bytes or with ``array_equal``."""
import ctypes
import hashlib
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import jpegbytes_ref as R
import jpegdecode_ref as D
from conftest import ROOT, Golden

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
SHAPES = [(1, 1), (8, 8), (9, 129), (17, 33), (24, 40), (23, 7), (64, 64)]
OPTIONS = (dict(quality=75, subsampling=2), dict(quality=30, subsampling=0), dict(quality=95, optimize=True),
           dict(quality=100, optimize=True, subsampling=0), dict(qtables=[list(range(1, 65)), [3] * 64]), dict(quality=1),
           dict(quality=75, subsampling=2, optimize=True))


@pytest.fixture(scope="module")
def gold():
    return Golden("jpegdecode.npz").z


@pytest.fixture(scope="module")
def old():
    return Golden("jpegfile_bytes.npz").z


# ------------------------------------------------------------------------------------------------- the restatement against Pillow
def test_fixture_is_small_and_names_its_libraries(gold):
    assert re.fullmatch(r"\d+\.\d+(\.\d+)?", str(gold["pillow_version"]))
    assert re.fullmatch(r"libjpeg(-turbo)? [\d.]+", str(gold["libjpeg_version"]))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpegdecode.npz")) < 100 * 1024
    tags = [k[5:] for k in gold.files if k.startswith("file/")]
    assert len(tags) == 9 and all("pixels/" + t in gold.files for t in tags)
    assert {t.split("/")[0] for t in tags} == {"opt95", "opt100", "qtables", "l420", "q1"}
    assert {t.split("/")[1] for t in tags} <= {"9x129x1", "9x129x3", "17x33x1", "17x33x3", "24x40x1", "24x40x3", "23x7x1", "23x7x3"}
    assert len([k for k in gold.files if k.startswith("sha256/")]) == 60


def test_restatement_is_the_recorded_pillow_pixels(gold, old):
    differing = []
    for key in gold.files:
        if key.startswith("file/"):
            r = D.decode_ref(gold[key].tobytes())
            if r["status"] != 0 or not np.array_equal(r["out"], gold["pixels/" + key[5:]]):
                differing.append(key)
    for key in old.files:
        if key.startswith("file/"):
            r = D.decode_ref(old[key].tobytes())
            if r["status"] != 0 or hashlib.sha256(r["out"].tobytes()).digest() != gold["sha256/" + key].tobytes():
                differing.append(key)
    assert not differing, differing


def test_recorded_files_leave_the_standard_stream(gold, old):
    """What the new fixture adds to the 60 standard files: Huffman tables of their own, tables no quality gives, and a one-channel file
    whose sampling byte says 22."""
    std = D.parse(old["file/17x33x3/noise/q75/s2"].tobytes())
    one = D.parse(old["file/17x33x1/noise/q75/s0"].tobytes())
    for key in gold.files:
        if key.startswith("file/opt"):
            info = D.parse(gold[key].tobytes())
            assert not np.array_equal(info["huff"], (std if info["c"] == 3 else one)["huff"]), key
    info = D.parse(gold["file/qtables/17x33x3/smooth"].tobytes())
    assert np.array_equal(np.sort(info["qt"][0]), np.arange(1, 65)) and (info["qt"][1:] == 3).all()
    data = gold["file/l420/9x129x1/noise"].tobytes()
    assert data[data.index(b"\xff\xc0") + 11] == 0x22 and D.parse(data)["subsampling"] == 0


@pytest.mark.parametrize("hw", SHAPES)
def test_restatement_is_live_pillow_in_every_pixel(hw):
    pytest.importorskip("PIL")
    from PIL import Image
    h, w = hw
    differing, n = [], 0
    for c in (1, 3):
        for kind in R.KINDS:
            img = R.make_image(kind, h, w, c)
            for kw in OPTIONS:
                buf = io.BytesIO()
                Image.fromarray(img[..., 0] if c == 1 else img).save(buf, "JPEG", **kw)
                with Image.open(io.BytesIO(buf.getvalue())) as im:
                    want = np.asarray(im, dtype=np.uint8).reshape(h, w, c)
                r = D.decode_ref(buf.getvalue())
                n += 1
                if r["status"] != 0 or not np.array_equal(r["out"], want):
                    differing.append((c, kind, kw))
    print(f"{h}x{w}: {len(differing)} of {n} files differ from Pillow's pixels")
    assert n == 2 * len(R.KINDS) * len(OPTIONS) and not differing, differing


@pytest.mark.parametrize("hw", [(9, 129), (17, 33), (24, 40), (23, 7)])
def test_decoded_coefficients_are_the_encoders(hw):
    """The files of the encoder's restatement, decoded: the coefficients they were coded from and the round trip's bytes."""
    h, w = hw
    for c in (1, 3):
        for kind in ("noise", "binary"):
            img = R.make_image(kind, h, w, c)
            for q, sub in ((75, 2), (100, 0), (1, 2)):
                want = R.jpeg_file_ref(img, q, sub)
                got = D.decode_ref(R.jpeg_bytes_ref(img, q, sub)[0])
                assert got["status"] == 0 and np.array_equal(got["coef_y"], want["coef_y"]), (hw, c, kind, q, sub)
                assert (c == 1 and got["coef_c"] is None) or np.array_equal(got["coef_c"], want["coef_c"]), (hw, c, kind, q, sub)
                assert np.array_equal(got["out"], want["out"])


# ------------------------------------------------------------------------------------------------- the parser
def test_parse_jpeg_is_the_restatements_parse(gold, old):
    from ideas_amd.op import parse_jpeg
    files = [z[k].tobytes() for z in (gold, old) for k in z.files if k.startswith("file/")]
    assert len(files) == 69
    for data in files:
        a, b = parse_jpeg(data), D.parse(data)
        assert (a.c, a.h, a.w, a.subsampling, a.scan_offset) == (b["c"], b["h"], b["w"], b["subsampling"], b["scan_offset"])
        assert a.qt.dtype == np.uint16 and np.array_equal(a.qt, b["qt"]) and a.huff == b["huff"].tobytes() and len(a.huff) == a.c * 2 * 272


def test_parse_jpeg_refuses_what_the_decoder_does_not_read(gold):
    from ideas_amd.op import UnsupportedJpeg, parse_jpeg
    reasons = {"progressive": "progressive", "422": "sampling 21-11-11", "restart": "restart"}
    seen = 0
    for name, word in reasons.items():
        if "refused/" + name in gold.files:
            data = gold["refused/" + name].tobytes()
            with pytest.raises(UnsupportedJpeg, match=word) as e:
                parse_jpeg(data)
            assert word in e.value.reason
            with pytest.raises(D.Unsupported):
                D.parse(data)
            seen += 1
    assert seen == 3                                                             # the Pillow that wrote the fixture writes all three
    good = gold["file/opt95/17x33x3/noise"].tobytes()
    sof = good.index(b"\xff\xc0")
    with pytest.raises(UnsupportedJpeg, match="12-bit samples"):
        parse_jpeg(good[:sof + 4] + b"\x0c" + good[sof + 5:])
    with pytest.raises(UnsupportedJpeg, match="16-bit DQT"):
        dqt = good.index(b"\xff\xdb")
        parse_jpeg(good[:dqt + 4] + b"\x10" + good[dqt + 5:])
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00"
    assert parse_jpeg(good[:2] + adobe + b"\x01" + good[2:]).scan_offset == parse_jpeg(good).scan_offset + 16
    with pytest.raises(UnsupportedJpeg, match="Adobe colour transform 0"):
        parse_jpeg(good[:2] + adobe + b"\x00" + good[2:])
    assert parse_jpeg(good[:2] + b"\xff\xdd\x00\x04\x00\x00" + good[2:]).h == 17     # a DRI with interval 0
    assert parse_jpeg(good[:2] + b"\xff\xfe\x00\x05abc" + b"\xff\xe5\x00\x03x" + good[2:]).w == 33      # COM and APPn are skipped
    for cut in (1, 3, 10, 30, sof + 6, parse_jpeg(good).scan_offset - 1):
        with pytest.raises(ValueError):
            parse_jpeg(good[:cut])
        with pytest.raises(ValueError):
            D.parse(good[:cut])
    with pytest.raises(ValueError):
        parse_jpeg(b"\x89PNG\r\n\x1a\n")


# ------------------------------------------------------------------------------------------------- the fixed point
def test_the_schedule_converges_to_the_serial_states():
    """sync_rounds asserts the bound and that the fixed point is the serial decoder's states, for every subsequence length tried."""
    noise = R.jpeg_bytes_ref(R.make_image("noise", 64, 64, 3), 100, 2)[0]
    flat = R.jpeg_bytes_ref(R.make_image("flat", 64, 64, 3), 75, 2)[0]
    for data in (noise, flat):
        for L in (64, 256, 1024):
            rounds, nsub = D.sync_rounds(data, L)
            assert 1 <= rounds <= nsub + 1, (rounds, nsub)
    assert D.sync_rounds(noise, 256)[0] >= 3
    assert D.SUBSEQ_BITS == 1024


def test_corruption_is_a_status_not_an_exception():
    data = R.jpeg_bytes_ref(R.make_image("noise", 24, 40, 3), 75, 2)[0]
    info = D.parse(data)
    scan = data[info["scan_offset"]:]
    assert D.decode_coefs(info, scan)[2] == 0
    assert D.decode_coefs(info, scan[:-2])[2] == 0                               # without EOI: the scan ends where the data ends
    assert D.decode_coefs(info, scan[:len(scan) // 2])[2] == -1                  # the data ends before the last block
    assert D.decode_coefs(info, b"")[2] == -1
    assert D.decode_coefs(info, scan[:-2] + b"\x00" * 40 + b"\xff\xd9")[2] == 0  # bits after the last block are ignored
    assert D.unstuff(b"\x12\xff\x00\x00\xff\x00\xff\xd9\x55") == b"\x12\xff\x00\xff" and D.unstuff(b"\x01\xff") == b"\x01\xff"


# ------------------------------------------------------------------------------------------------- C ABI and errors
def test_c_abi_declares_and_exports_the_entry_points():
    from ideas_amd import _lib, op
    hdr = open(os.path.join(ROOT, "include", "ideas_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bsize_t\s+ideas_jpeg_file_decode_workspace_bytes\s*\(", hdr)
    assert re.search(r"\bint\s+ideas_jpeg_file_decode\s*\(", hdr)
    for name in ("ideas_jpeg_file_decode_workspace_bytes", "ideas_jpeg_file_decode"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(_lib.load(), name).argtypes is not None
    m = re.search(r"#define\s+IDEAS_JPEG_SUBSEQ_BITS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == _lib.JPEG_SUBSEQ_BITS == D.SUBSEQ_BITS
    assert re.search(r"#define\s+IDEAS_ABI_VERSION\s+4\b", hdr)
    assert _lib.ABI_VERSION == 4 and _lib.load().ideas_abi_version() == 4        # additive within ABI 4
    mk = open(os.path.join(ROOT, "ideas_amd", "csrc", "Makefile")).read()
    assert "jpeg_decode.hip" in mk and re.search(r"^jpeg_decode\.\$\(O\):.*\n\t.*kernel-resource-usage", mk, re.M)
    for name in ("parse_jpeg", "jpeg_file_decode", "jpeg_file_decode_grouped", "UnsupportedJpeg", "JpegInfo"):
        assert name in op.__all__ and callable(getattr(op, name))


def test_size_query():
    from ideas_amd import _lib
    work = _lib.load().ideas_jpeg_file_decode_workspace_bytes
    for bad in ((2, 8, 8, 0), (0, 8, 8, 0), (3, 0, 8, 0), (3, 8, -1, 0), (3, 65536, 8, 0), (3, 8, 65536, 2), (3, 8, 8, 1), (3, 8, 8, 3)):
        assert work(1, *bad, 4096) == 0, bad
    assert work(0, 3, 8, 8, 2, 4096) == 0 and work(-1, 3, 8, 8, 2, 4096) == 0
    assert work(1, 3, 8, 8, 2, 0) == 0 and work(1, 3, 8, 8, 2, -5) == 0
    assert work(1, 3, 65535, 65535, 2, 1 << 40) == 0                             # more bits of scan than 31 bits count
    assert work(1 << 30, 3, 64, 64, 2, 4096) == 0                                # more blocks than 31 bits count
    # grows with the batch and with the rows, but a row longer than its blocks can fill adds nothing
    a, b, c = work(1, 3, 64, 64, 2, 1000), work(4, 3, 64, 64, 2, 1000), work(4, 3, 64, 64, 2, 2000)
    assert 0 < a < b < c
    assert work(4, 3, 64, 64, 2, 1 << 20) == work(4, 3, 64, 64, 2, 1 << 30) > c
    assert work(2, 1, 8, 8, 0, 1 << 40) < 4096


def test_c_abi_argument_checks_run_before_any_launch():
    """Answered in front of the launch (no device needed: the pointers are host buffers a launch would never survive)."""
    from ideas_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.addressof(buf)

    def dec(out=a, y=a, cy=a, cc=a, status=a, scans=a, nbytes=a, stride=4096, qt=a, huff=a, work=a, B=1, C=3, H=8, W=8, sub=2):
        return lib.ideas_jpeg_file_decode(out, y, cy, cc, status, scans, nbytes, stride, qt, huff, work, B, C, H, W, sub, None)
    for name in ("out", "status", "scans", "nbytes", "qt", "huff", "work"):
        assert dec(**{name: None}) == E_NULL, name
    for dim in ("B", "H", "W"):
        assert dec(**{dim: 0}) == E_SHAPE and dec(**{dim: -1}) == E_SHAPE, dim
    assert dec(H=65536) == E_SHAPE and dec(W=65536) == E_SHAPE
    assert dec(C=0) == E_SHAPE and dec(C=2) == E_SHAPE and dec(C=4) == E_SHAPE
    assert dec(stride=0) == E_SHAPE and dec(stride=-1) == E_SHAPE
    assert dec(C=1, H=65535, W=65535, stride=1 << 40) == E_SHAPE                 # a scan beyond 2^31 - 1 bits
    assert dec(B=1 << 20, H=4096, W=4096) == E_SHAPE                             # a batch beyond 2^31 - 1 blocks
    for sub in (1, 3, -1, 420):
        assert dec(sub=sub) == E_UNSUPPORTED and dec(sub=sub, C=1) == E_UNSUPPORTED, sub
    assert dec(sub=1, B=0) == E_SHAPE and dec(sub=1, out=None) == E_NULL and dec(B=0, work=None) == E_NULL    # NULL, SHAPE, UNSUPPORTED
    assert buf.raw == bytes(4096)


def test_op_validates_before_it_touches_the_device(gold):
    import torch
    from ideas_amd import op
    data = gold["file/opt95/17x33x3/noise"].tobytes()
    with pytest.raises(RuntimeError, match="no files"):
        op.jpeg_file_decode([])
    with pytest.raises(op.UnsupportedJpeg):
        op.jpeg_file_decode([data, gold["refused/422"].tobytes()])
    with pytest.raises(ValueError):
        op.jpeg_file_decode_grouped([data[:100]])
    with pytest.raises(RuntimeError, match="file 1 is 24 x 40 x 3"):
        op.jpeg_file_decode_grouped([data, gold["file/opt100/24x40x3/noise"].tobytes()])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            op.jpeg_file_decode([data])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.jpeg_file_decode([data], device="cpu")


# ------------------------------------------------------------------------------------------------- command line
def test_extract_help_shows_the_decoder_flag():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "extract.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for word in ("--jpeg_decoder", "{pillow,device}", "default: pillow"):
        assert word in r.stdout, word


def test_extract_refuses_an_unknown_decoder(capsys):
    import extract
    with pytest.raises(SystemExit) as e:
        extract.main(["--ckpt", "x.pt", "--out", "p", "--jpeg_decoder", "turbo", "a.jpg"])
    assert e.value.code == 2 and "--jpeg_decoder" in capsys.readouterr().err
