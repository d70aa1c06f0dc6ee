"""Host-side checks of the JPEG file written on the device: the Python restatement of the stream (tests/jpegbytes_ref.py) against
Pillow's own files, as recorded in tests/golden/jpegfile_bytes.npz (written by tests/golden/make_golden_jpegfile_bytes.py) and LIVE where
Pillow is installed; that the recorded set takes every branch of the coder; the size bound; the C ABI of csrc/jpeg_bytes.hip with its
size queries and argument errors; the op's validation and hide.py's flag.  No GPU, no tolerances: files are compared as ``bytes``."""
import ctypes
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpegbytes_ref as R
from conftest import ROOT, Golden

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
SHAPES = [(1, 1), (8, 8), (9, 129), (17, 33), (16, 16), (24, 40), (40, 24), (23, 7), (64, 64), (3, 50)]
QUALITIES = (1, 50, 75, 90, 100)


@pytest.fixture(scope="module")
def gold():
    return Golden("jpegfile_bytes.npz").z


def cases(z):
    """(key, kind, h, w, c, quality, subsampling) of every recorded file"""
    for key in z.files:
        if key.startswith("file/"):
            _, shape, kind, q, s = key.split("/")
            h, w, c = (int(v) for v in shape.split("x"))
            yield key, kind, h, w, c, int(q[1:]), int(s[1:])


@pytest.fixture(scope="module")
def restated(gold):
    """{key: (file, stats)} of the restatement for every recorded file, computed once"""
    return {key: R.jpeg_bytes_ref(R.make_image(kind, h, w, c), q, s) for key, kind, h, w, c, q, s in cases(gold)}


# ------------------------------------------------------------------------------------------------- the restatement against Pillow
def test_fixture_is_small_and_names_its_libraries(gold):
    assert re.fullmatch(r"\d+\.\d+(\.\d+)?", str(gold["pillow_version"]))
    assert re.fullmatch(r"libjpeg(-turbo)? [\d.]+", str(gold["libjpeg_version"]))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpegfile_bytes.npz")) < 100 * 1024
    assert len(list(cases(gold))) == 5 * 4 * (1 + 2)                             # shapes x (kind, quality) x (C = 1; C = 3 twice)


def test_restatement_is_the_recorded_pillow_files(gold, restated):
    differing = [key for key in restated if restated[key][0] != gold[key].tobytes()]
    assert not differing, differing


@pytest.mark.parametrize("hw", SHAPES)
def test_restatement_is_live_pillow_in_every_byte(hw):
    """The check the stream was written against: 0 differing files.  A one-channel image has one subsampling (mode "L")."""
    pytest.importorskip("PIL")
    from PIL import Image
    h, w = hw
    differing, n = [], 0
    for c in (1, 3):
        for kind in R.KINDS:
            img = R.make_image(kind, h, w, c)
            im = Image.fromarray(img[..., 0] if c == 1 else img)
            for q in QUALITIES:
                for sub in (0, 2):
                    buf = io.BytesIO()
                    im.save(buf, "JPEG", quality=q, subsampling=sub if c == 3 else 0)
                    n += 1
                    if R.jpeg_bytes_ref(img, q, sub)[0] != buf.getvalue():
                        differing.append((c, kind, q, sub))
    print(f"{h}x{w}: {len(differing)} of {n} files differ from Pillow's")
    assert n == 2 * len(R.KINDS) * len(QUALITIES) * 2 and not differing, differing


def test_one_channel_files_differ_from_pillow_at_420_in_the_sampling_byte_alone():
    """Pillow copies ``subsampling=2`` into the sampling factors of a one-channel file; the stream here says 11 for C = 1."""
    pytest.importorskip("PIL")
    from PIL import Image
    img = R.make_image("noise", 17, 33, 1)
    buf = io.BytesIO()
    Image.fromarray(img[..., 0]).save(buf, "JPEG", quality=75, subsampling=2)
    ours, theirs = R.jpeg_bytes_ref(img, 75, 2)[0], buf.getvalue()
    assert len(ours) == len(theirs) and [i for i in range(len(ours)) if ours[i] != theirs[i]] == [100]
    assert (ours[100], theirs[100]) == (0x11, 0x22)


def test_the_recorded_set_takes_every_branch(restated):
    total, pads = {}, set()
    for _, stats in restated.values():
        pads.add(stats["pad_bits"])
        for k, v in stats.items():
            total[k] = total.get(k, 0) + int(v)
    print(total, sorted(pads))
    for branch in ("zrl", "ac_cat10", "dc_cat11", "no_eob", "eob_only", "stuffed", "right_dummy", "bottom_dummy"):
        assert total[branch] > 0, branch
    assert 0 in pads and len(pads) > 1                                           # a file that ends on a byte, and files that do not


def test_dummy_blocks_copy_the_block_before_them():
    """17 x 33 at 4:2:0: the luma grid is 3 x 5 under 2 x 3 MCUs, so the last MCU column and row are half dummies.  Coding the real
    blocks in their place (as if the grid were complete, with the dummies' DCs) gives the same scan."""
    img = R.make_image("noise", 17, 33, 3)
    res = R.jpeg_file_ref(img, 100, 2)
    data, stats = R.encode_coefs(res["coef_y"], res["coef_c"], 17, 33, 3, 100, 2)
    assert stats["right_dummy"] == 3 and stats["bottom_dummy"] == 2 * 3 and stats["blocks"] == 6 * 6
    cy = np.zeros((4, 6, 64), np.int16)
    cy[:3, :5] = res["coef_y"]
    cy[:3, 5, 0] = cy[:3, 4, 0]                                                  # right edge: the block on the left
    cy[3, 0::2, 0] = cy[2, 1::2, 0]                                              # (1,0) copies (0,1) ...
    cy[3, 1::2, 0] = cy[3, 0::2, 0]                                              # ... and (1,1) copies (1,0)
    whole, stats = R.encode_coefs(cy, res["coef_c"], 32, 48, 3, 100, 2)
    assert stats["right_dummy"] == 0 and stats["bottom_dummy"] == 0
    assert whole[623:] == data[623:] and whole[:623] != data[:623]


def test_files_stay_inside_the_bound_and_headers_have_their_sizes(gold, restated):
    from ideas_amd import _lib
    bound = _lib.load().ideas_jpeg_file_max_bytes
    for key, kind, h, w, c, q, s in cases(gold):
        data = restated[key][0]
        assert bound(c, h, w, s) == R.max_bytes(c, h, w, s) and len(data) <= bound(c, h, w, s), key
        hdr = R.header(c, h, w, q, s)
        assert len(hdr) == (623 if c == 3 else 328) and data.startswith(hdr) and data.endswith(b"\xff\xd9"), key
        assert hdr.endswith(b"\x00\x3f\x00") and hdr[:4] == b"\xff\xd8\xff\xe0"


def test_a_coefficient_without_a_code_is_refused():
    cy = np.zeros((1, 1, 64), np.int16)
    for k, v, ok in ((5, 1023, True), (5, 1024, False), (5, -1024, False), (0, 2047, True), (0, 2048, False), (0, -2047, True),
                     (0, -2048, False)):
        cy[:] = 0
        cy[0, 0, k] = v
        assert (R.encode_coefs(cy, None, 8, 8, 1, 75, 0)[0] is not None) == ok, (k, v)


# ------------------------------------------------------------------------------------------------- C ABI and errors
def test_c_abi_declares_and_exports_the_entry_points():
    from ideas_amd import _lib, op
    hdr = open(os.path.join(ROOT, "include", "ideas_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bsize_t\s+ideas_jpeg_file_max_bytes\s*\(", hdr)
    assert re.search(r"\bsize_t\s+ideas_jpeg_file_encode_workspace_bytes\s*\(", hdr)
    assert re.search(r"\bint\s+ideas_jpeg_file_encode\s*\(", hdr)
    for name in ("ideas_jpeg_file_max_bytes", "ideas_jpeg_file_encode_workspace_bytes", "ideas_jpeg_file_encode"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(_lib.load(), name).argtypes is not None
    assert re.search(r"#define\s+IDEAS_ABI_VERSION\s+4\b", hdr)
    assert _lib.ABI_VERSION == 4 and _lib.load().ideas_abi_version() == 4        # additive within ABI 4
    mk = open(os.path.join(ROOT, "ideas_amd", "csrc", "Makefile")).read()
    assert "jpeg_bytes.hip" in mk and re.search(r"^jpeg_bytes\.\$\(O\):.*\n\t.*kernel-resource-usage", mk, re.M)
    for name in ("jpeg_file_encode", "jpeg_files_to_host"):
        assert name in op.__all__ and callable(getattr(op, name))


def test_size_queries():
    from ideas_amd import _lib
    lib = _lib.load()
    bound, work = lib.ideas_jpeg_file_max_bytes, lib.ideas_jpeg_file_encode_workspace_bytes
    assert bound(1, 8, 8, 0) == 328 + 416 + 3 and bound(1, 8, 8, 2) == 328 + 416 + 3
    assert bound(3, 8, 8, 0) == 623 + 416 * 3 + 3 and bound(3, 8, 8, 2) == 623 + 416 * 6 + 3       # one MCU: 4 luma blocks, 3 dummies
    assert bound(3, 200, 264, 2) == 623 + 416 * 1326 + 3 and bound(3, 17, 33, 2) == 623 + 416 * 36 + 3
    assert bound(3, 17, 33, 0) == 623 + 416 * 45 + 3 and bound(1, 65535, 65535, 0) == 0             # more than 2^31 - 1 bytes
    for bad in ((2, 8, 8, 0), (0, 8, 8, 0), (3, 0, 8, 0), (3, 8, -1, 0), (3, 65536, 8, 0), (3, 8, 65536, 2), (3, 8, 8, 1), (3, 8, 8, 3)):
        assert bound(*bad) == 0 and work(1, *bad) == 0, bad
    assert work(0, 3, 8, 8, 2) == 0 and work(-1, 3, 8, 8, 2) == 0 and work(1 << 30, 3, 64, 64, 2) == 0
    # the offsets (8 bytes a block), 208 bytes a block of unstuffed scan, and something for the lengths, the flags and the alignment
    for b, c, h, w, s in ((1, 1, 8, 8, 0), (3, 3, 17, 33, 2), (32, 3, 256, 256, 2)):
        blocks = (bound(c, h, w, s) - (623 if c == 3 else 328) - 3) // 416
        assert b * blocks * 216 <= work(b, c, h, w, s) <= b * (blocks * 216 + 64) + 64


def test_c_abi_argument_checks_run_before_any_launch():
    """Answered in front of the launch (no device needed: the pointers are host buffers a launch would never survive)."""
    from ideas_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.addressof(buf)

    def enc(files=a, nbytes=a, stride=None, cy=a, cc=a, work=a, B=1, C=3, H=8, W=8, q=75, sub=2):
        if stride is None:
            stride = int(lib.ideas_jpeg_file_max_bytes(C, H, W, sub)) or 1 << 20
        return lib.ideas_jpeg_file_encode(files, nbytes, stride, cy, cc, work, B, C, H, W, q, sub, None)
    for name in ("files", "nbytes", "cy", "cc", "work"):
        assert enc(**{name: None}) == E_NULL, name
    assert enc(cc=None, C=1, q=0) == E_UNSUPPORTED                               # coef_c is not looked at with C = 1
    for dim in ("B", "H", "W"):
        assert enc(**{dim: 0}) == E_SHAPE and enc(**{dim: -1}) == E_SHAPE, dim
    assert enc(H=65536) == E_SHAPE and enc(W=65536) == E_SHAPE
    assert enc(C=0) == E_SHAPE and enc(C=2) == E_SHAPE and enc(C=4) == E_SHAPE
    assert enc(stride=623 + 416 * 6 + 2) == E_SHAPE and enc(stride=0) == E_SHAPE and enc(stride=-1) == E_SHAPE
    assert enc(C=1, H=65535, W=65535, stride=1 << 40) == E_SHAPE                 # a file beyond 2^31 - 1 bytes
    assert enc(B=1 << 20, H=4096, W=4096, stride=1 << 40) == E_SHAPE             # a launch beyond 2^31 - 1 blocks
    assert enc(q=0) == E_UNSUPPORTED and enc(q=101) == E_UNSUPPORTED and enc(q=-5) == E_UNSUPPORTED
    for sub in (1, 3, -1, 420):
        assert enc(sub=sub, stride=1 << 20) == E_UNSUPPORTED and enc(sub=sub, C=1, stride=1 << 20) == E_UNSUPPORTED, sub
    assert enc(q=0, B=0) == E_SHAPE and enc(q=0, files=None) == E_NULL and enc(B=0, work=None) == E_NULL    # NULL, SHAPE, UNSUPPORTED
    assert buf.raw == bytes(4096)


def test_op_validates_before_it_touches_the_device():
    from ideas_amd import op
    img = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.jpeg_file_encode(img, 75)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.jpeg_files_to_host(torch.zeros(1, 8, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------- command line
def test_hide_help_shows_the_encoder_flag():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "hide.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for word in ("--jpeg_encoder", "pillow", "device"):
        assert word in r.stdout, word


def test_hide_refuses_an_unknown_encoder(capsys):
    import hide
    with pytest.raises(SystemExit) as e:
        hide.main(["--ckpt", "x.pt", "--payload", "p", "--out", "d", "--format", "jpeg", "--jpeg_encoder", "turbo"])
    assert e.value.code == 2 and "--jpeg_encoder" in capsys.readouterr().err
