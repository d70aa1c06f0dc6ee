"""Host-side checks of the spatial channel attacks: the numpy restatement (tests/spatial_ref.py) against Pillow's own resize and median
as recorded in tests/golden/spatial.npz (written by tests/golden/make_golden_spatial.py), the window tables of op/resample.py, the
invariants of the model, the C ABI of csrc/attack_spatial.hip with its argument errors, and the spec parser.  No GPU, no tolerances."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import spatial_ref as R
from conftest import ROOT, Golden

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
NAMES = ("ideas_resample_u8", "ideas_median_u8")
IMAGES = ("smooth", "odd", "gray", "noise")
FACTORS = (0.25, 0.3, 0.5, 0.75, 1.5, 2.0, 3.7)
SIGMAS = (0.3, 1.0, 2.5, 4.0)


@pytest.fixture(scope="module")
def gold():
    return Golden("attacks.npz")


@pytest.fixture(scope="module")
def pil():
    z = Golden("spatial.npz").z
    return lambda key: np.cumsum(z[key], axis=0, dtype=np.uint8)      # stored as differences from the row above


# ------------------------------------------------------------------------------------------------- the oracle against Pillow
def test_fixture_is_small_and_names_its_pillow():
    z = Golden("spatial.npz").z
    assert re.fullmatch(r"\d+\.\d+(\.\d+)?", str(z["pillow_version"]))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "spatial.npz")) < 100 * 1024
    assert not any(k.startswith("img/") for k in z.files)                        # the images live in attacks.npz only
    assert len([k for k in z.files if k.startswith(("resize/f", "back/f"))]) == 2 * len(FACTORS) * len(IMAGES)


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("name", IMAGES)
def test_oracle_is_pillows_bilinear_resize(gold, pil, name, factor):
    img = gold.z[f"img/{name}"]
    h, w = img.shape[:2]
    small = R.resize_ref(img, R.scaled_size(h, w, factor))
    assert small.shape == pil(f"resize/f{factor:g}/{name}").shape
    assert np.array_equal(small, pil(f"resize/f{factor:g}/{name}"))
    assert np.array_equal(R.resize_ref(small, (h, w)), pil(f"back/f{factor:g}/{name}"))
    assert np.array_equal(R.scale_ref(img, factor), pil(f"back/f{factor:g}/{name}"))


def test_oracle_is_pillows_resize_when_one_axis_grows_and_one_shrinks(gold, pil):
    assert np.array_equal(R.resize_ref(gold.z["img/odd"], (20, 8)), pil("resize/aniso/odd"))
    assert pil("resize/aniso/odd").shape == (20, 8, 3)


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("name", IMAGES)
def test_oracle_is_pillows_median(gold, pil, name, k):
    assert np.array_equal(R.median_ref(gold.z[f"img/{name}"], k), pil(f"median/k{k}/{name}"))


def test_median_by_hand():
    img = np.arange(25, dtype=np.uint8).reshape(5, 5, 1)
    m3 = R.median_ref(img, 3)[..., 0]
    assert m3[2, 2] == 12 and m3[0, 0] == 1 and m3[4, 4] == 23 and m3[0, 2] == 3       # corner window: 0 0 0 1 1 5 5 6 6 -> ... 1
    assert R.median_ref(img, 5)[2, 2, 0] == 12


# ------------------------------------------------------------------------------------------------- the op's tables
def table_cases():
    """(n_in, n_out, filter, sigma) over the ranges ``attacks.parse`` allows, sizes 1 .. 512 (every size at the range's ends, a
    spread of sizes in between)."""
    for n in range(1, 513):
        factors = (0.25, 4.0) if n % 8 else (0.25, 0.3, 0.5, 0.75, 1.5, 2.0, 3.7, 4.0)
        for f in factors:
            m = max(1, math.floor(n * f + 0.5))
            yield n, m, "bilinear", None
            yield m, n, "bilinear", None
        for s in ((0.01, 4.0) if n % 8 else (0.01,) + SIGMAS + (1.7,)):
            yield n, n, "gauss", s


def test_tables_rows_sum_to_one_stay_inside_and_fit_kmax():
    from ideas_amd.op import resample_tables
    widest = 0
    for n_in, n_out, filt, sigma in table_cases():
        lo, kk = resample_tables(n_in, n_out, filt, sigma)
        assert lo.dtype == np.int32 and kk.dtype == np.int32 and lo.shape == (n_out,) and kk.shape[0] == n_out
        ksize = kk.shape[1]
        assert 1 <= ksize <= R.KMAX, (n_in, n_out, filt, sigma)
        assert (np.abs(kk.astype(np.int64).sum(1) - (1 << 22)) <= ksize / 2).all(), (n_in, n_out, filt, sigma)
        count = ksize - (np.cumsum(kk[:, ::-1] != 0, axis=1) == 0).sum(1)        # up to the last non-zero tap
        assert (lo >= 0).all() and (lo + count <= n_in).all(), (n_in, n_out, filt, sigma)
        assert (kk >= 0).all()
        widest = max(widest, ksize)
    assert widest == 25                                                         # sigma 4: ceil(12) taps either side


def test_tables_are_the_oracles():
    from ideas_amd.op import resample_tables
    for n_in, n_out, filt, sigma in table_cases():
        if n_in > 64 and n_in % 37:
            continue
        want = R.bilinear_tables(n_in, n_out) if filt == "bilinear" else R.gauss_tables(n_in, sigma)
        lo, kk = resample_tables(n_in, n_out, filt, sigma)
        assert np.array_equal(lo, want[0]) and np.array_equal(kk, want[1]), (n_in, n_out, filt, sigma)
    assert resample_tables(40, 20, "bilinear")[0] is resample_tables(40, 20, "bilinear")[0]          # cached
    with pytest.raises(ValueError):
        resample_tables(40, 20, "gauss", 1.0)
    with pytest.raises(ValueError):
        resample_tables(40, 40, "gauss")
    with pytest.raises(ValueError):
        resample_tables(40, 20, "lanczos")
    with pytest.raises(ValueError):
        resample_tables(0, 20, "bilinear")


def test_bilinear_table_by_hand():
    """4 -> 2: scale 2, centres 1 and 3, windows [0, 3) and [1, 4), weights 1 - |x - c + 0.5| / 2 = 3/4, 3/4, 1/4 and mirrored,
    divided by their sum 7/4."""
    from ideas_amd.op import resample_tables
    lo, kk = resample_tables(4, 2, "bilinear")
    assert lo.tolist() == [0, 1]
    one = 1 << 22
    assert kk.tolist() == [[int(3 / 7 * one + 0.5), int(3 / 7 * one + 0.5), int(1 / 7 * one + 0.5)],
                           [int(1 / 7 * one + 0.5), int(3 / 7 * one + 0.5), int(3 / 7 * one + 0.5)]]
    lo, kk = resample_tables(3, 3, "gauss", 0.3)                                  # one tap either side, the border renormalised
    assert lo.tolist() == [0, 0, 1] and kk.shape == (3, 3) and kk[0, 2] == 0 and kk[2, 2] == 0
    assert kk[1, 0] == kk[1, 2] and kk[0, 0] == kk[2, 1]


# ------------------------------------------------------------------------------------------------- invariants of the model
@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (13, 21)])
def test_constant_images_come_back_unchanged(hw):
    h, w = hw
    img = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256, h, w, 1))        # a batch of every value
    for f in FACTORS + (4.0,):
        assert np.array_equal(R.scale_ref(img, f), img), f
    for s in SIGMAS:
        assert np.array_equal(R.gblur_ref(img, s), img), s
    for k in (3, 5):
        assert np.array_equal(R.median_ref(img, k), img), k


@pytest.mark.parametrize("sigma", SIGMAS)
def test_gblur_commutes_with_transposition_up_to_pass_order(gold, sigma):
    """``gblur`` of the transposed image is the transpose of ``gblur`` with its passes in the other order, byte for byte, and one pass
    alone is its own transpose on the transposed image.  (Not the transpose of ``gblur`` itself: the model rounds to bytes between
    the passes, and horizontal-then-vertical differs from vertical-then-horizontal in 76 .. 138 of the 819 bytes of this image for
    sigma >= 1 -- none at sigma 0.3.  The byte-exact form of the symmetry is the one asserted.)"""
    img = gold.z["img/odd"]
    t = np.ascontiguousarray(img.transpose(1, 0, 2))
    tab_h, tab_w = R.gauss_tables(img.shape[0], sigma), R.gauss_tables(img.shape[1], sigma)
    assert np.array_equal(R.resample_ref(t, horiz=tab_h).transpose(1, 0, 2), R.resample_ref(img, vert=tab_h))
    vert_first = R.resample_ref(R.resample_ref(img, vert=tab_h), horiz=tab_w)
    assert np.array_equal(R.gblur_ref(t, sigma).transpose(1, 0, 2), vert_first)


# ------------------------------------------------------------------------------------------------- C ABI and errors
def test_c_abi_declares_and_exports_the_entry_points():
    from ideas_amd import _lib, op
    hdr = open(os.path.join(ROOT, "include", "ideas_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
        assert getattr(_lib.load(), name).argtypes is not None
    assert re.search(r"#define\s+IDEAS_RESAMPLE_KMAX\s+32\b", hdr)
    assert re.search(r"#define\s+IDEAS_ABI_VERSION\s+4\b", hdr)
    assert _lib.ABI_VERSION == 4 and _lib.load().ideas_abi_version() == 4        # additive within ABI 4
    mk = open(os.path.join(ROOT, "ideas_amd", "csrc", "Makefile")).read()
    assert "attack_spatial.hip" in mk and re.search(r"^attack_spatial\.\$\(O\):.*\n\t.*kernel-resource-usage", mk, re.M)
    for name in ("resize_u8", "gaussian_blur_u8", "median_u8", "resample_tables"):
        assert name in op.__all__ and callable(getattr(op, name))


def test_c_abi_argument_checks_run_before_any_launch():
    """Answered in front of the launch (no device needed: the pointers are host buffers a launch would never survive)."""
    from ideas_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.addressof(buf)

    def rs(out=a, y=a, x=a, B=1, C=3, H=8, W=8, H2=4, W2=4, h_lo=a, h_kk=a, hk=3, v_lo=a, v_kk=a, vk=3):
        return lib.ideas_resample_u8(out, y, x, B, C, H, W, H2, W2, h_lo, h_kk, hk, v_lo, v_kk, vk, None)
    assert rs(out=None) == E_NULL and rs(x=None) == E_NULL
    assert rs(h_lo=None) == E_NULL and rs(h_kk=None) == E_NULL and rs(v_lo=None) == E_NULL and rs(v_kk=None) == E_NULL
    for dim in ("B", "H", "W", "H2", "W2"):
        assert rs(**{dim: 0}) == E_SHAPE and rs(**{dim: -1}) == E_SHAPE, dim
    assert rs(C=0) == E_SHAPE and rs(C=2) == E_SHAPE and rs(C=4) == E_SHAPE
    assert rs(h_lo=None, h_kk=None) == E_SHAPE and rs(v_lo=None, v_kk=None) == E_SHAPE      # skipped, but W2 != W / H2 != H
    assert rs(h_lo=None, h_kk=None, W2=8, B=0) == E_SHAPE and rs(v_lo=None, v_kk=None, H2=8, B=0) == E_SHAPE    # (skipping is fine there)
    assert rs(hk=0) == E_UNSUPPORTED and rs(hk=33) == E_UNSUPPORTED and rs(hk=-1) == E_UNSUPPORTED
    assert rs(vk=0) == E_UNSUPPORTED and rs(vk=33) == E_UNSUPPORTED
    assert rs(hk=33, B=0) == E_SHAPE and rs(hk=33, x=None) == E_NULL                         # in the order NULL, SHAPE, UNSUPPORTED
    assert rs(h_lo=None, h_kk=None, W2=8, hk=99, vk=33) == E_UNSUPPORTED                    # a skipped direction's ksize is not looked at

    def med(out=a, y=a, x=a, B=1, C=3, H=8, W=8, K=3):
        return lib.ideas_median_u8(out, y, x, B, C, H, W, K, None)
    assert med(out=None) == E_NULL and med(x=None) == E_NULL
    assert med(B=0) == E_SHAPE and med(H=0) == E_SHAPE and med(W=-1) == E_SHAPE and med(C=2) == E_SHAPE and med(C=0) == E_SHAPE
    for k in (0, 1, 2, 4, 7, -3):
        assert med(K=k) == E_UNSUPPORTED, k
    assert med(K=4, B=0) == E_SHAPE


def test_ops_refuse_host_tensors():
    from ideas_amd import op
    img = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.resize_u8(img, (4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.gaussian_blur_u8(img, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.median_u8(img, 3)


# ------------------------------------------------------------------------------------------------- parsing
@pytest.mark.parametrize("spec", ["scale:0.5", "gblur:1.5", "median:5", "gblur:1+scale:0.5+jpeg:75", "scale:0.25", "scale:4", "gblur:4",
                                  "median:3", "scale:3.7+median:3+noise:2"])
def test_parse_round_trips_names(spec):
    from ideas_amd import attacks
    a = attacks.parse(spec)
    assert a.name == spec and callable(a)
    assert attacks.parse(a.name).name == a.name
    assert attacks.parse(" " + spec.replace("+", " + ")).name == spec


@pytest.mark.parametrize("spec,stage", [("scale:0.1", "scale:0.1"), ("scale:5", "scale:5"), ("gblur:0", "gblur:0"),
                                        ("gblur:4.5", "gblur:4.5"), ("median:4", "median:4"), ("median:7", "median:7"),
                                        ("scale:", "scale:"), ("median:3.5", "median:3.5"), ("gblur:-1", "gblur:-1"),
                                        ("gblur", "gblur"), ("jpeg:75+scale:9", "scale:9")])
def test_parse_names_the_offending_stage(spec, stage):
    from ideas_amd import attacks
    with pytest.raises(ValueError) as e:
        attacks.parse(spec)
    assert repr(stage) in str(e.value)


def test_unknown_attack_message_lists_the_new_stages():
    from ideas_amd import attacks
    with pytest.raises(ValueError) as e:
        attacks.parse("blur:3")
    for name in ("scale:F", "gblur:S", "median:K"):
        assert name in str(e.value)


def test_evaluate_command_line_refuses_a_bad_scale(capsys):
    import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--attack", "scale:9", "x.pt"])
    assert e.value.code == 2 and "scale:9" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--help"])
    out = capsys.readouterr().out
    assert e.value.code == 0 and "scale:F" in out and "gblur:S" in out and "median:K" in out
