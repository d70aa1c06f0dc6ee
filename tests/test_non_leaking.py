"""Host side of ideas_amd.non_leaking (adaptive discriminator augmentation) against tests/golden/non_leaking.npz, which
tests/golden/make_golden_non_leaking.py recorded from the reference's stylegan2/non_leaking.py and stylegan2/train.py:194-213.  No GPU."""
import ctypes
import math
import os
import re
import signal

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, Golden, rel_err

GRID_QUANTUM = 2.0 ** -20          # tests/golden/make_golden_non_leaking.py
AFFINE_TAGS = ("aff16", "aff24x20", "aff32", "aff32_c5")


@pytest.fixture(scope="module")
def gold():
    return Golden("non_leaking.npz")


@pytest.fixture(scope="module")
def NL():
    import ideas_amd.non_leaking as NL
    return NL


# ------------------------------------------------------------------------------------------------- matrices
@pytest.mark.parametrize("p", (0.3, 1.0))
@pytest.mark.parametrize("seed", range(4))
def test_seeded_matrices_are_the_references(gold, NL, seed, p):
    """Same f32 torch calls in the same order: the slack (1e-6 absolute on O(1) entries) covers a re-association only."""
    tag = f"mats/seed{seed}/p{p}"
    torch.manual_seed(seed)
    G = NL.sample_affine(p, 4, 32, 32)
    C = NL.sample_color(p, 4)
    assert G.dtype == C.dtype == torch.float32 and G.shape == (4, 3, 3) and C.shape == (4, 4, 4)
    eg, ec = float((G - gold.t(tag + "/G")).abs().max()), float((C - gold.t(tag + "/C")).abs().max())
    print(f"{tag}: |G - ref| {eg:.2e}  |C - ref| {ec:.2e}")
    assert eg <= 1e-6 and ec <= 1e-6
    pads = NL.get_padding(torch.inverse(G), 32, 32)
    assert all(isinstance(v, int) for v in pads) and list(pads) == gold.t(tag + "/pad").tolist()


def test_sym6_and_names(NL):
    assert len(NL.SYM6) == 12 and abs(sum(NL.SYM6) - math.sqrt(2)) < 1e-12        # an orthonormal wavelet low-pass
    for name in ("translate_mat", "rotate_mat", "scale_mat", "translate3d_mat", "rotate3d_mat", "scale3d_mat", "luma_flip_mat",
                 "saturation_mat", "lognormal_sample", "category_sample", "uniform_sample", "normal_sample", "bernoulli_sample",
                 "random_mat_apply", "sample_affine", "sample_color", "get_padding", "try_sample_affine_and_pad", "random_apply_affine",
                 "apply_color", "random_apply_color", "augment", "warp_theta", "AdaptiveAugment"):
        assert callable(getattr(NL, name)), name


def test_drawn_G_is_redrawn_until_a_reflect_pad_exists(NL):
    """G=None: the stream of sample_affine draws is consumed until one admits a reflect pad, as in the reference's loop."""
    img = torch.zeros(2, 3, 16, 16)
    for seed in range(6):
        torch.manual_seed(seed)
        n = 0
        while True:
            G = NL.sample_affine(1.0, 2, 16, 16)
            n += 1
            pads = NL.get_padding(torch.inverse(G), 16, 16)
            if max(pads) + 6 < 16:
                break
        torch.manual_seed(seed)
        img_pad, G2, pads2 = NL.try_sample_affine_and_pad(img, 1.0, 6, None)
        assert torch.equal(G, G2) and tuple(pads2) == tuple(pads)
        assert img_pad.shape == (2, 3, 16 + pads[2] + pads[3] + 12, 16 + pads[0] + pads[1] + 12)
    assert n >= 1


# ------------------------------------------------------------------------------------------------- warp_theta
def _ref_grid(gold, tag):
    return torch.from_numpy(np.cumsum(np.array(gold.z[f"{tag}/grid_dq"]), axis=2).astype(np.float64) * GRID_QUANTUM)


@pytest.mark.parametrize("tag", AFFINE_TAGS)
def test_warp_theta_reproduces_the_reference_grid(gold, NL, tag):
    """theta @ (ox, oy, 1) against the reference's final grid in pixels of img_2x, at every (ox, oy).  1e-4 pixel: f32 theta entries
    of magnitude up to ~2 times an index up to ~130 give about 2 * 130 * 6e-8 = 2e-5; the stored grid carries the reference's f32
    linspace (1e-5) and a 4.8e-7 quantisation."""
    x, G, pads = gold.t(tag + "/x"), gold.t(tag + "/G"), gold.t(tag + "/pads").tolist()
    theta = NL.warp_theta(G, tuple(x.shape[2:]), pads, len(NL.SYM6))
    assert theta.dtype == torch.float32 and theta.shape == (x.shape[0], 6)
    ref = _ref_grid(gold, tag)
    h2, w2 = gold.t(tag + "/img_2x_hw").tolist()
    assert ref.shape == (x.shape[0], h2, w2, 2) and (h2, w2) == NL.warp_hw(tuple(x.shape[2:]), pads, len(NL.SYM6))
    t = theta.double().view(-1, 2, 3)
    idx = torch.stack((torch.arange(w2, dtype=torch.float64).view(1, w2).expand(h2, w2),
                       torch.arange(h2, dtype=torch.float64).view(h2, 1).expand(h2, w2), torch.ones(h2, w2, dtype=torch.float64)), -1)
    got = torch.einsum("bij,hwj->bhwi", t, idx)
    err = float((got - ref).abs().max())
    print(f"{tag}: max |theta @ (ox, oy, 1) - reference grid| = {err:.2e} pixel over {ref.numel() // 2} positions")
    assert err <= 1e-4


def _upfirdn_torch(x, k, up=1, down=1):
    """upfirdn2d with pad (0, 0) from torch calls: zero-stuff, true convolution with k, decimate."""
    b, c, h, w = x.shape
    if up > 1:
        z = x.new_zeros(b, c, h * up, w * up)
        z[:, :, ::up, ::up] = x
        x = z
    y = F.conv2d(x.reshape(b * c, 1, *x.shape[2:]), torch.flip(k, (0, 1))[None, None])
    return y.reshape(b, c, *y.shape[2:])[:, :, ::down, ::down]


@pytest.mark.parametrize("tag", AFFINE_TAGS)
def test_affine_pipeline_from_warp_theta_and_grid_sample(gold, NL, tag):
    """The ops keep "no CPU branch", so this is NOT random_apply_affine's own f16 / f64 path: it is the same pipeline written
    here from torch calls -- reflect pad, zero-stuffing + F.conv2d for the two FIR passes, warp_theta (unrounded, float64) through
    op.augment.affine_warp_composition (the device-agnostic grid + stock F.grid_sample the ops fall back to), crop -- in float64
    against the reference's float64 output and input gradient.  Bounds: DESIGN.md's 1e-5 / 1e-4 of the largest element; the
    reference's grid, built from an f32 linspace, sits up to ~1.5e-5 pixel off the affine map it stands for."""
    from ideas_amd.op.augment import affine_warp_composition
    x = gold.t(tag + "/x").requires_grad_(True)
    G, pads = gold.t(tag + "/G"), gold.t(tag + "/pads").tolist()
    len_k = len(NL.SYM6)
    k1 = torch.tensor(NL.SYM6, dtype=torch.float64)
    k = torch.ger(k1, k1)
    img_pad, G2, pads2 = NL.try_sample_affine_and_pad(x, 1.0, (len_k + 1) // 2, G)
    assert G2 is G and list(pads2) == pads
    img_2x = _upfirdn_torch(img_pad, torch.flip(k, (0, 1)), up=2)
    assert tuple(img_2x.shape[2:]) == NL.warp_hw(tuple(x.shape[2:]), pads, len_k)
    theta = NL.warp_theta(G, tuple(x.shape[2:]), pads, len_k, dtype=torch.float64)
    down = _upfirdn_torch(affine_warp_composition(img_2x, theta, tuple(img_2x.shape[2:])), k, down=2)
    y = down[:, :, pads[2]:down.shape[2] - pads[3] - 1, pads[0]:down.shape[3] - pads[1] - 1]
    ref = gold.t(tag + "/y")
    assert y.shape == ref.shape == x.shape
    (gx,) = torch.autograd.grad((y * gold.t(tag + "/cot").double()).sum(), x)
    ey, eg = rel_err(y, ref), rel_err(gx, gold.t(tag + "/gx"))
    print(f"{tag}: y {ey:.2e}  gx {eg:.2e}")
    assert ey <= 1e-5 and eg <= 1e-4


def test_color_composition_matches_the_reference(gold):
    from ideas_amd.op.augment import color_affine_composition
    x = gold.t("col/x").requires_grad_(True)
    y = color_affine_composition(x, gold.t("col/C")[:, :3, :])
    (gx,) = torch.autograd.grad((y * gold.t("col/cot").double()).sum(), x)
    assert rel_err(y, gold.t("col/y")) <= 1e-6 and rel_err(gx, gold.t("col/gx")) <= 1e-6      # f64 against f32-stored f64 results


# ------------------------------------------------------------------------------------------------- AdaptiveAugment
def test_adaptive_augment_replays_the_reference(gold, NL):
    """The same arithmetic on the same f64 scalars: the sequence of p is equal as Python floats."""
    target, length = gold.t("ada/settings").tolist()
    preds = gold.t("ada/real_pred")
    ada = NL.AdaptiveAugment(target, length)
    got = [ada.tune(rp) for rp in preds]
    want = gold.t("ada/p").tolist()
    assert got == want
    assert max(want) > 0 and want[-1] == 0.0 and want[15] > want[14]          # it rose and came back to the bound


def test_adaptive_augment_reduce_sum_hook(gold, NL):
    target, length = gold.t("ada/settings").tolist()
    preds = gold.t("ada/real_pred")
    calls = []

    def reduce_sum(t):                       # eight ranks holding the same tensor
        calls.append(t.clone())
        return t * 8

    ada = NL.AdaptiveAugment(target, length, initial_p=0.0, reduce_sum=reduce_sum)
    got = [ada.tune(rp) for rp in preds]
    want = gold.t("ada/p_reduce8").tolist()
    assert got == want
    assert len(calls) == len(preds) and calls[0].shape == (2,) and calls[0][1] == 16
    assert 1.0 in want and want[-1] == 0.0 and any(0 < v < 1 for v in want[20:])    # rose, clamped at 1, fell, clamped at 0


def test_adaptive_augment_initial_p(NL):
    ada = NL.AdaptiveAugment(0.6, 4000, initial_p=0.25)
    assert ada.tune(torch.ones(16, 1)) == 0.25                                    # 16 predictions: no update yet


# ------------------------------------------------------------------------------------------------- the deliberate difference
def test_given_G_without_a_reflect_pad_raises(NL):
    """A 45-degree rotation of an 8x8 image needs more reflect padding than the image has: the reference's loop never ends, ours
    raises.  The alarm turns a spin into a failure instead of a hung suite."""
    def on_alarm(signum, frame):
        raise AssertionError("random_apply_affine did not return within 10 s")
    old = signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(10)
    try:
        G = NL.rotate_mat(torch.tensor([math.pi / 4]))
        with pytest.raises(RuntimeError, match="reflect padding"):
            NL.random_apply_affine(torch.zeros(1, 3, 8, 8), 1.0, G)
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


# ------------------------------------------------------------------------------------------------- ops and C ABI
def test_ops_raise_before_any_launch(NL):
    import ideas_amd.op as op
    with pytest.raises(RuntimeError, match="4-D"):
        op.affine_warp(torch.zeros(3, 4, 4), torch.zeros(1, 6), (4, 4))
    with pytest.raises(RuntimeError, match=r"theta must be \[2, 6\]"):
        op.affine_warp(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 3), (4, 4))
    with pytest.raises(RuntimeError, match="empty output"):
        op.affine_warp(torch.zeros(2, 3, 4, 4), torch.zeros(2, 6), (0, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.affine_warp(torch.zeros(2, 3, 4, 4), torch.zeros(2, 6), (4, 4))
    with pytest.raises(RuntimeError, match=r"\[B, 3, H, W\]"):
        op.color_affine(torch.zeros(2, 4, 4, 4), torch.zeros(2, 3, 4))
    with pytest.raises(RuntimeError, match="m must be"):
        op.color_affine(torch.zeros(2, 3, 4, 4), torch.zeros(2, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.color_affine(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4))


def test_c_abi_has_the_augment_entry_points():
    from ideas_amd import _lib
    names = ("ideas_affine_warp", "ideas_affine_warp_bwd", "ideas_color_affine")
    hdr = open(os.path.join(ROOT, "include", "ideas_hip.h")).read()
    declared = set(re.findall(r"\b(ideas_[a-z0-9_]+)\s*\(", hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert name in declared and name in _lib.EXPORTS and hasattr(raw, name), name
    lib = _lib.load()
    assert lib.ideas_abi_version() == 4
    # B = 0: IDEAS_E_SHAPE from the argument check, before any pointer is looked at or anything is launched
    assert lib.ideas_affine_warp(None, None, None, 0, 3, 8, 8, 8, 8, _lib.NCHW, _lib.F32, None) == -2
    assert lib.ideas_affine_warp_bwd(None, None, None, 2, 3, 8, 0, 8, 8, 1, _lib.NHWC, _lib.F32, None) == -2
    assert lib.ideas_color_affine(None, None, None, 2, 0, 8, _lib.NCHW, _lib.BF16, None) == -2
    assert lib.ideas_affine_warp(None, None, None, 1, 3, 8, 8, 8, 8, _lib.NCHW, _lib.F16, None) == -3      # IDEAS_E_UNSUPPORTED
    assert lib.ideas_affine_warp(None, None, None, 1, 3, 8, 8, 8, 8, _lib.NCHW, _lib.F32, None) == -1      # IDEAS_E_NULL
