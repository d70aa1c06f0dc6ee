"""Host-side checks of the channel attacks: the C ABI of csrc/attack.hip and its argument errors, the numpy restatement of the JPEG
model (tests/attacks_ref.py) against PIL / libjpeg-turbo's tables and round trip as recorded in tests/golden/attacks.npz (written by
tests/golden/make_golden_attacks.py), the cap on near-ties the GPU test relies on, and the spec parser.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import attacks_ref as R
from conftest import ROOT, Golden

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
NAMES = ("ideas_jpeg_roundtrip", "ideas_pixel_attack")
QUALITIES = (1, 10, 50, 75, 90, 100)
IMAGES = ("smooth", "odd", "gray", "noise")
# mean |oracle - PIL's decode| in grey levels, measured over IMAGES x QUALITIES: the largest is 0.7760 (noise, quality 75; next
# odd at 100: 0.2650).  libjpeg's integer `islow` DCT against the ideal one flips single coefficients; 1.5 x the largest:
PIL_MEAN_ABS_BOUND = 1.5 * 0.7760
CAP = 0.01                    # of the non-rational coefficients / of the samples within TOL of a rounding tie


@pytest.fixture(scope="module")
def gold():
    return Golden("attacks.npz")


# ------------------------------------------------------------------------------------------------- C ABI and errors
def test_c_abi_declares_and_exports_both_entry_points():
    from ideas_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ideas_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
        assert getattr(_lib.load(), name).argtypes is not None
    assert re.search(r"#define\s+IDEAS_ABI_VERSION\s+4\b", hdr)
    assert _lib.ABI_VERSION == 4 and _lib.load().ideas_abi_version() == 4        # additive within ABI 4
    assert "attack.hip" in open(os.path.join(ROOT, "ideas_amd", "csrc", "Makefile")).read()


def test_c_abi_argument_checks_run_before_any_launch():
    """Answered in front of the launch (no device needed: the pointers are host buffers a launch would never survive)."""
    from ideas_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.addressof(buf)

    def jpeg(out=a, y=a, coef=a, x=a, B=1, C=3, H=8, W=8, quality=75):
        return lib.ideas_jpeg_roundtrip(out, y, coef, x, B, C, H, W, quality, None)
    assert jpeg(out=None) == E_NULL and jpeg(x=None) == E_NULL
    assert jpeg(B=0) == E_SHAPE and jpeg(H=0) == E_SHAPE and jpeg(W=-1) == E_SHAPE
    assert jpeg(C=2) == E_SHAPE and jpeg(C=4) == E_SHAPE and jpeg(C=0) == E_SHAPE
    assert jpeg(quality=0) == E_UNSUPPORTED and jpeg(quality=101) == E_UNSUPPORTED and jpeg(quality=-5) == E_UNSUPPORTED

    def pix(out=a, y=a, x=a, noise=a, u=a, B=1, C=3, H=2, W=2, gain=1.0, offset=0.0, sigma=1.0, sp=0.1):
        return lib.ideas_pixel_attack(out, y, x, noise, u, B, C, H, W, gain, offset, sigma, sp, None)
    assert pix(out=None) == E_NULL and pix(x=None) == E_NULL
    assert pix(noise=None) == E_NULL and pix(u=None) == E_NULL                    # needed: sigma != 0, sp != 0
    assert pix(B=0) == E_SHAPE and pix(H=-1) == E_SHAPE and pix(W=0) == E_SHAPE
    assert pix(C=2) == E_SHAPE and pix(C=0) == E_SHAPE
    assert pix(noise=None, sigma=0.0, B=0) == E_SHAPE and pix(u=None, sp=0.0, B=0) == E_SHAPE     # NULL is fine there


def test_ops_refuse_host_tensors():
    from ideas_amd import op
    img = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.jpeg_roundtrip(img, 75)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.pixel_attack(img, gain=0.5)


# ------------------------------------------------------------------------------------------------- the oracle against PIL
def test_fixture_holds_the_stated_images(gold):
    shapes = {"smooth": (40, 24, 3), "odd": (13, 21, 3), "gray": (16, 8, 1), "noise": (8, 8, 3)}
    for name, shape in shapes.items():
        img = gold.z[f"img/{name}"]
        assert img.dtype == np.uint8 and img.shape == shape
        for q in QUALITIES:
            assert gold.z[f"pil/q{q}/{name}"].shape == shape
    for name in ("dc_q50", "sample_q62", "sample_q1", "basis"):
        assert gold.z[f"tie/{name}"].dtype == np.uint8 and gold.z[f"tie/{name}"].shape[0] == 8
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "attacks.npz")) < 100 * 1024


@pytest.mark.parametrize("quality", QUALITIES)
def test_quantisation_tables_are_pils(gold, quality):
    assert np.array_equal(R.quant_tables(quality).reshape(2, 64), gold.z[f"pil/q{quality}/tables"])


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("name", IMAGES)
def test_oracle_against_pils_round_trip(gold, name, quality):
    img = gold.z[f"img/{name}"]
    pil = gold.z[f"pil/q{quality}/{name}"].astype(np.float64)
    out = R.jpeg_ref(img, quality)["out"].astype(np.float64)
    mse_model, mse_input = ((out - pil) ** 2).mean(), ((img - pil) ** 2).mean()
    mean_abs = np.abs(out - pil).mean()
    print(f"{name} q={quality}: mean |oracle - PIL| {mean_abs:.4f}, mse {mse_model:.4f} (input: {mse_input:.4f})")
    assert mse_model < mse_input
    assert mean_abs <= PIL_MEAN_ABS_BOUND


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("name", IMAGES)
def test_near_ties_are_rare_on_the_fixtures(gold, name, quality):
    """What the GPU test relies on: outside the window TOL it demands equality, so the window must leave nearly everything outside."""
    r = R.jpeg_ref(gold.z[f"img/{name}"], quality)
    ratio = r["ratio"][~np.broadcast_to(R.RATIONAL, r["ratio"].shape)]
    assert ratio.size == 60 * r["coef"].size // 64
    c, s = R.near_tie(ratio).mean(), R.near_tie(r["pre"]).mean()
    print(f"{name} q={quality}: {100 * c:.3f} % of coefficients, {100 * s:.3f} % of samples within {R.TOL} of a tie")
    assert c <= CAP and s <= CAP


def test_tie_images_sit_on_their_ties(gold):
    """The fixtures built to lie on exact ties do, in the oracle's exact arithmetic."""
    r = R.jpeg_ref(gold.z["tie/dc_q50"], int(gold.z["tie/dc_q50/quality"]))
    dc = r["ratio"][0, 0, :, 0, 0]
    assert np.array_equal(np.abs(dc) % 1, np.full(dc.shape, 0.5)) and (dc > 0).any() and (dc < 0).any()
    assert np.array_equal(r["coef"][0, 0, :, 0], np.sign(dc) * (np.abs(dc) + 0.5))           # half away from zero
    for name in ("sample_q62", "sample_q1"):
        r = R.jpeg_ref(gold.z[f"tie/{name}"], int(gold.z[f"tie/{name}/quality"]))
        assert np.array_equal(r["pre"] % 1, np.full(r["pre"].shape, 0.5)), name
    r = R.jpeg_ref(gold.z["tie/basis"], 100)
    assert not r["coef"].reshape(-1, 8, 8)[:, ~R.RATIONAL].any() and r["coef"][..., 4].any() and r["coef"][..., 36].any()
    assert np.array_equal(r["out"], gold.z["tie/basis"])                                     # T = 1: S / 8 is an integer here


def test_decode_from_given_coefficients_is_the_decode_half():
    img = np.random.default_rng(5).integers(0, 256, (13, 9, 3), dtype=np.uint8)
    r = R.jpeg_ref(img, 50)
    pre, out = R.jpeg_from_coef(r["coef"], 13, 9, 50)
    assert np.array_equal(pre, r["pre"]) and np.array_equal(out, r["out"]) and out.shape == img.shape
    flipped = r["coef"].copy()
    flipped[1, 0, 0, 3] += 1
    assert not np.array_equal(R.jpeg_from_coef(flipped, 13, 9, 50)[1], out)


def test_pixel_restatement_by_hand():
    x = np.array([[[[0], [100], [200], [255]]]], np.uint8)                        # [1, 1, 4, 1]
    assert R.pixel_attack_ref(x).reshape(-1).tolist() == [0, 100, 200, 255]
    assert R.pixel_attack_ref(x, gain=0.5).reshape(-1).tolist() == [64, 114, 164, 191]
    assert R.pixel_attack_ref(x, offset=20).reshape(-1).tolist() == [20, 120, 220, 255]
    nz = np.array([1, -1, np.nan, 0], np.float32).reshape(1, 1, 4, 1)
    assert R.pixel_attack_ref(x, sigma=5, noise=nz).reshape(-1).tolist() == [5, 95, 0, 255]
    u = np.array([0.0, 0.049, 0.96, 0.5], np.float32).reshape(1, 1, 4)
    assert R.pixel_attack_ref(x, sp=0.1, u=u).reshape(-1).tolist() == [0, 0, 255, 255]


# ------------------------------------------------------------------------------------------------- parsing
@pytest.mark.parametrize("spec", ["none", "jpeg:75", "noise:5", "sp:0.02", "gain:0.8", "offset:20", "offset:-7.5", "noise:3+jpeg:75",
                                  "gain:1.2+offset:-10+sp:0.1+jpeg:1", "none+jpeg:100"])
def test_parse_round_trips_names(spec):
    from ideas_amd import attacks
    a = attacks.parse(spec)
    assert a.name == spec and callable(a)
    assert attacks.parse(a.name).name == a.name
    assert attacks.parse(" " + spec.replace("+", " + ")).name == spec


@pytest.mark.parametrize("spec,stage", [("blur:3", "blur:3"), ("jpeg", "jpeg"), ("noise:", "noise:"), ("jpeg:abc", "jpeg:abc"),
                                        ("sp:nan", "sp:nan"), ("jpeg:0", "jpeg:0"), ("jpeg:101", "jpeg:101"), ("jpeg:7.5", "jpeg:7.5"),
                                        ("sp:1.5", "sp:1.5"), ("sp:-0.1", "sp:-0.1"), ("noise:-1", "noise:-1"),
                                        ("noise:3+jpeg:200", "jpeg:200"), ("jpeg:75+", ""), ("none:1", "none:1")])
def test_parse_names_the_offending_stage(spec, stage):
    from ideas_amd import attacks
    with pytest.raises(ValueError) as e:
        attacks.parse(spec)
    assert repr(stage) in str(e.value)


def test_parse_rejects_an_empty_spec():
    from ideas_amd import attacks
    with pytest.raises(ValueError):
        attacks.parse("")


def test_evaluate_command_line_accepts_attack(capsys):
    import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--help"])
    assert e.value.code == 0 and "--attack" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:                      # a bad spec is a usage error, before anything is loaded
        evaluate.main(["--attack", "none", "blur:3", "nowhere.pt"])
    assert e.value.code == 2 and "blur:3" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--attack", "jpeg:75", "--container", "float", "nowhere.pt"])
    assert e.value.code == 2


def test_evaluate_refuses_an_attack_on_the_float_container():
    from ideas_amd import attacks, stego
    with pytest.raises(ValueError, match="u8"):
        stego.evaluate({}, None, 1, 0.0, 4, 2, container="float", attack=attacks.parse("jpeg:75"))
