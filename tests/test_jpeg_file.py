"""Host-side checks of the JPEG file channel: the numpy restatement (tests/jpegfile_ref.py) against Pillow's own encode-and-decode, as
recorded in tests/golden/jpegfile.npz (written by tests/golden/make_golden_jpegfile.py) and LIVE where Pillow is installed, the C ABI of
csrc/attack_jpeg.hip with its argument errors, the spec parser and hide.py's flags.  No GPU, no tolerances: every comparison is
``array_equal``."""
import ctypes
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import jpegfile_ref as J
from conftest import ROOT, Golden

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
IMAGES = ("smooth", "odd", "gray", "noise")
GOLDEN_QUALITIES = (10, 75, 95)
SHAPES = [(1, 1), (4, 4), (5, 3), (16, 2), (8, 8), (15, 9), (16, 16), (17, 23), (31, 16), (33, 40), (2, 50), (9, 129)]
QUALITIES = (1, 10, 50, 75, 95, 100)


@pytest.fixture(scope="module")
def gold():
    return Golden("attacks.npz")


@pytest.fixture(scope="module")
def pil():
    z = Golden("jpegfile.npz").z
    return lambda key: np.cumsum(z[key], axis=0, dtype=np.uint8)      # stored as differences from the row above


def make_images(h, w, c):
    """Seeded noise, a smooth image and a 0/255 image, uint8 [h, w, c]."""
    rng = np.random.default_rng(1000 * h + 10 * w + c)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([(5 * yy + 3 * xx + 70 * k) % 256 for k in range(c)], -1).astype(np.uint8)
    return {"noise": rng.integers(0, 256, (h, w, c), dtype=np.uint8), "smooth": smooth,
            "binary": (rng.integers(0, 2, (h, w, c)) * 255).astype(np.uint8)}


# ------------------------------------------------------------------------------------------------- the restatement against Pillow
def test_fixture_is_small_and_names_its_libraries():
    z = Golden("jpegfile.npz").z
    assert re.fullmatch(r"\d+\.\d+(\.\d+)?", str(z["pillow_version"]))
    assert re.fullmatch(r"libjpeg(-turbo)? [\d.]+", str(z["libjpeg_version"]))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpegfile.npz")) < 100 * 1024
    assert not any(k.startswith("img/") for k in z.files)                        # the images live in attacks.npz only
    assert len([k for k in z.files if k.startswith("rt/")]) == len(GOLDEN_QUALITIES) * 2 * len(IMAGES)


@pytest.mark.parametrize("sub", [0, 2])
@pytest.mark.parametrize("quality", GOLDEN_QUALITIES)
@pytest.mark.parametrize("name", IMAGES)
def test_restatement_is_the_recorded_pillow_round_trip(gold, pil, name, quality, sub):
    img = gold.z[f"img/{name}"]
    res = J.jpeg_file_ref(img, quality, sub)
    assert np.array_equal(res["out"], pil(f"rt/q{quality}/s{sub}/{name}"))
    h, w, c = img.shape
    assert res["coef_y"].shape == ((h + 7) // 8, (w + 7) // 8, 64) and res["coef_y"].dtype == np.int16
    if c == 1:
        assert res["coef_c"] is None and res["chroma"] is None
    elif sub == 0:
        assert res["coef_c"].shape == (2, (h + 7) // 8, (w + 7) // 8, 64) and res["chroma"] is None
    else:
        ch, cw = (h + 1) // 2, (w + 1) // 2
        assert res["coef_c"].shape == (2, (ch + 7) // 8, (cw + 7) // 8, 64) and res["chroma"].shape == (2, ch, cw)


@pytest.mark.parametrize("hw", SHAPES)
def test_restatement_is_live_pillow_in_every_byte(hw):
    """The check the model was written against: 0 differing images."""
    pytest.importorskip("PIL")
    from PIL import Image
    h, w = hw
    differing, n = [], 0
    for c in (1, 3):
        for kind, img in make_images(h, w, c).items():
            im = Image.fromarray(img[..., 0] if c == 1 else img)
            for q in QUALITIES:
                for sub in (0, 2):
                    buf = io.BytesIO()
                    im.save(buf, "JPEG", quality=q, subsampling=sub)
                    got = np.asarray(Image.open(io.BytesIO(buf.getvalue())), dtype=np.uint8).reshape(h, w, c)
                    n += 1
                    if not np.array_equal(J.jpeg_file_ref(img, q, sub)["out"], got):
                        differing.append((c, kind, q, sub))
    print(f"{h}x{w}: {len(differing)} of {n} round trips differ from Pillow")
    assert n == 2 * 3 * len(QUALITIES) * 2 and not differing, differing


def test_the_two_orders_of_padding_matter():
    """Columns are padded before the 2x2 average and rows after it: on a 10 x 10 image (chroma 5 x 5) the other order of either gives
    other planes, so the live check above does tell them apart."""
    img = make_images(10, 10, 3)["noise"]
    cb = J.rgb_to_ycc(img)[1]
    right = J.downsample_420(cb)
    assert right.shape == (8, 8)
    rows_first = J.downsample_420(np.pad(cb, ((0, 6), (0, 0)), mode="edge"))[:8]
    assert np.array_equal(rows_first[:5], right[:5]) and not np.array_equal(rows_first, right)
    cols_after = np.pad(J.downsample_420(cb)[:, :5], ((0, 0), (0, 3)), mode="edge")
    assert np.array_equal(cols_after[:, :5], right[:, :5]) and not np.array_equal(cols_after, right)


def test_narrow_images_replicate_their_chroma():
    """cw <= 2 (W <= 4): no triangle filter."""
    c = np.array([[10, 200], [90, 30], [0, 255]], np.int64)
    assert np.array_equal(J.upsample_420(c, 5, 3), np.repeat(np.repeat(c, 2, 0), 2, 1)[:5, :3])
    wide = J.upsample_420(np.pad(c, ((0, 0), (0, 1)), mode="edge"), 5, 5)
    assert wide[0, 1] == (3 * (4 * 10) + 4 * 200 + 7) >> 4                       # the filter, as soon as cw = 3


# ------------------------------------------------------------------------------------------------- C ABI and errors
def test_c_abi_declares_and_exports_the_entry_points():
    from ideas_amd import _lib, op
    hdr = open(os.path.join(ROOT, "include", "ideas_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bsize_t\s+ideas_jpeg_file_workspace_bytes\s*\(", hdr)
    assert re.search(r"\bint\s+ideas_jpeg_file_roundtrip\s*\(", hdr)
    for name in ("ideas_jpeg_file_workspace_bytes", "ideas_jpeg_file_roundtrip"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(_lib.load(), name).argtypes is not None
    assert re.search(r"#define\s+IDEAS_ABI_VERSION\s+4\b", hdr)
    assert _lib.ABI_VERSION == 4 and _lib.load().ideas_abi_version() == 4        # additive within ABI 4
    mk = open(os.path.join(ROOT, "ideas_amd", "csrc", "Makefile")).read()
    assert "attack_jpeg.hip" in mk and re.search(r"^attack_jpeg\.\$\(O\):.*\n\t.*kernel-resource-usage", mk, re.M)
    assert "jpeg_file_roundtrip" in op.__all__ and callable(op.jpeg_file_roundtrip)


def test_workspace_size_query():
    from ideas_amd import _lib
    size = _lib.load().ideas_jpeg_file_workspace_bytes
    assert size(3, 3, 17, 23, 2) == 2 * 3 * 9 * 12
    assert size(1, 3, 1, 1, 2) == 2 and size(2, 3, 16, 16, 2) == 2 * 2 * 8 * 8
    assert size(3, 3, 17, 23, 0) == 0 and size(3, 1, 17, 23, 2) == 0 and size(3, 1, 17, 23, 0) == 0
    assert size(0, 3, 17, 23, 2) == 0 and size(3, 3, -1, 23, 2) == 0 and size(3, 2, 17, 23, 2) == 0 and size(3, 3, 17, 23, 1) == 0


def test_c_abi_argument_checks_run_before_any_launch():
    """Answered in front of the launch (no device needed: the pointers are host buffers a launch would never survive)."""
    from ideas_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.addressof(buf)

    def rt(out=a, y=a, cy=a, cc=a, work=a, x=a, B=1, C=3, H=8, W=8, q=75, sub=2):
        return lib.ideas_jpeg_file_roundtrip(out, y, cy, cc, work, x, B, C, H, W, q, sub, None)
    assert rt(out=None) == E_NULL and rt(x=None) == E_NULL
    for dim in ("B", "H", "W"):
        assert rt(**{dim: 0}) == E_SHAPE and rt(**{dim: -1}) == E_SHAPE, dim
    assert rt(C=0) == E_SHAPE and rt(C=2) == E_SHAPE and rt(C=4) == E_SHAPE
    assert rt(q=0) == E_UNSUPPORTED and rt(q=101) == E_UNSUPPORTED and rt(q=-5) == E_UNSUPPORTED
    for sub in (1, 3, -1, 420):
        assert rt(sub=sub) == E_UNSUPPORTED and rt(sub=sub, C=1) == E_UNSUPPORTED, sub
    assert rt(work=None) == E_NULL                                               # 4:2:0 with C = 3 needs its workspace
    assert rt(q=0, B=0) == E_SHAPE and rt(q=0, x=None) == E_NULL and rt(work=None, q=0) == E_UNSUPPORTED       # NULL, SHAPE, UNSUPPORTED
    assert buf.raw == bytes(4096)


def test_op_validates_before_it_touches_the_device():
    from ideas_amd import op
    img = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.jpeg_file_roundtrip(img, 75)


# ------------------------------------------------------------------------------------------------- parsing
@pytest.mark.parametrize("spec,name", [("jpegfile:75", "jpegfile:75"), ("jpegfile:75:444", "jpegfile:75:444"), ("jpegfile:75:420", "jpegfile:75"),
                                       ("jpegfile:1", "jpegfile:1"), ("jpegfile:100:444", "jpegfile:100:444"),
                                       ("noise:3+jpegfile:75", "noise:3+jpegfile:75"), ("scale:0.5+jpegfile:75:444+jpeg:50", "scale:0.5+jpegfile:75:444+jpeg:50"),
                                       (" jpegfile:90:420 + median:3 ", "jpegfile:90+median:3")])
def test_parse_canonicalises_the_new_stages(spec, name):
    from ideas_amd import attacks
    a = attacks.parse(spec)
    assert a.name == name and callable(a)
    assert attacks.parse(a.name).name == a.name


@pytest.mark.parametrize("spec,stage", [("jpegfile", "jpegfile"), ("jpegfile:", "jpegfile:"), ("jpegfile:0", "jpegfile:0"),
                                        ("jpegfile:101", "jpegfile:101"), ("jpegfile:7.5", "jpegfile:7.5"), ("jpegfile:x", "jpegfile:x"),
                                        ("jpegfile:75:422", "jpegfile:75:422"), ("jpegfile:75:", "jpegfile:75:"),
                                        ("jpegfile:75:444:1", "jpegfile:75:444:1"), ("jpeg:75+jpegfile:75:4:2:0", "jpegfile:75:4:2:0")])
def test_parse_names_the_offending_stage(spec, stage):
    from ideas_amd import attacks
    with pytest.raises(ValueError) as e:
        attacks.parse(spec)
    assert repr(stage) in str(e.value)


def test_jpeg_stage_is_untouched_and_the_lists_name_the_new_one():
    from ideas_amd import attacks
    assert attacks.parse("jpeg:75").name == "jpeg:75"
    with pytest.raises(ValueError) as e:
        attacks.parse("jpeg:75:444")                                             # the suffix belongs to jpegfile only
    assert repr("jpeg:75:444") in str(e.value)
    with pytest.raises(ValueError) as e:
        attacks.parse("jpg:75")
    assert "jpegfile:Q" in str(e.value) and "jpeg:Q" in str(e.value)
    assert "jpegfile:Q" in attacks.__doc__ and "jpegfile:Q:444" in attacks.__doc__


# ------------------------------------------------------------------------------------------------- command lines
def test_hide_help_shows_the_new_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "hide.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--format", "png", "jpeg", "--jpeg_quality", "--jpeg_subsampling", "420", "444"):
        assert flag in r.stdout, flag


def test_hide_refuses_bad_jpeg_arguments(capsys):
    import hide
    for argv in (["--format", "gif"], ["--jpeg_quality", "0"], ["--jpeg_quality", "101"], ["--jpeg_subsampling", "422"]):
        with pytest.raises(SystemExit) as e:
            hide.main(["--ckpt", "x.pt", "--payload", "p", "--out", "d"] + argv)
        assert e.value.code == 2, argv
        capsys.readouterr()


def test_evaluate_command_line_knows_the_new_stage(capsys):
    import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--attack", "jpegfile:75:422", "x.pt"])
    assert e.value.code == 2 and "jpegfile:75:422" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--help"])
    assert e.value.code == 0 and "jpegfile:Q" in capsys.readouterr().out
