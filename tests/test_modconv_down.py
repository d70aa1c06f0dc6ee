"""Host-side checks of the downsampling ModulatedConv2d (stylegan2/model.py:181-277, downsample branch): construction, state dict,
argument errors, the argument checks of its C entry point, and -- the anchor of tests/test_modconv_down_gpu.py -- that the f64
restatement the GPU tests compare against reproduces what the reference's own class computed (tests/golden/modconv_down.npz,
written by tests/golden/make_golden_modconv_down.py).  No GPU."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT, Golden, rel_err
import modconv_down_ref as R

TOL, GTOL = 1e-5, 1e-4


@pytest.fixture(scope="module")
def gold():
    return Golden("modconv_down.npz")


def _seeded_layer(init):
    from ideas_amd.model import ModulatedConv2d
    torch.manual_seed(init["seed"])
    return ModulatedConv2d(init["cin"], init["cout"], init["k"], 24, downsample=True)


def test_constructor_builds_the_downsample_branch(gold):
    from ideas_amd.model import Blur
    meta = gold.json("meta")
    m = _seeded_layer(meta["init"])
    assert m.downsample and not m.upsample
    assert isinstance(m.blur, Blur) and tuple(m.blur.pad) == (2, 2)          # p = (4 - 2) + (3 - 1) = 4 -> pads (2, 2)
    for c in meta["cases"]:
        from ideas_amd.model import ModulatedConv2d
        layer = ModulatedConv2d(c["cin"], c["cout"], c["k"], meta["style_dim"], demodulate=c["demodulate"], downsample=True)
        assert list(layer.blur.pad) == c["pad"] == list(R.down_pads(4, c["k"])), c


def test_state_dict_and_seeded_init_are_the_references(gold):
    init = gold.json("meta")["init"]
    m = _seeded_layer(init)
    sd = m.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == init["keys"]
    assert set(sd) == {"blur.kernel", "modulation.bias", "modulation.weight", "weight"}
    for k, v in sd.items():
        assert torch.equal(v, gold.t(f"init.sd/{k}")), k                      # same draws in the same order
    assert not any(k.startswith("blur") for k, _ in m.named_parameters())


def test_reference_state_dict_loads_strict(gold):
    from ideas_amd.model import ModulatedConv2d
    meta = gold.json("meta")
    c = meta["cases"][1]
    m = ModulatedConv2d(c["cin"], c["cout"], c["k"], meta["style_dim"], downsample=True)
    ref = {"weight": gold.t("down1.w"), "blur.kernel": gold.t("down1.fir"), "modulation.weight": gold.t("down1.mw"),
           "modulation.bias": gold.t("down1.mb")}
    res = m.load_state_dict(ref, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m.weight.detach(), ref["weight"]) and torch.equal(m.modulation.weight.detach(), ref["modulation.weight"])
    # the same-resolution memory layout: the conv weight [O, I, k, k] is channels_last (OHWI), read by the kernels without a copy
    assert m.weight[0].is_contiguous(memory_format=torch.channels_last)


def test_repr_matches_the_references(gold):
    init = gold.json("meta")["init"]
    assert repr(_seeded_layer(init)) == init["repr"]


def test_upsample_and_downsample_together_is_an_error():
    from ideas_amd.model import ModulatedConv2d
    import ideas_amd.op as op
    with pytest.raises(ValueError):
        ModulatedConv2d(8, 8, 3, 16, upsample=True, downsample=True)
    with pytest.raises(ValueError):
        op.modulated_conv2d(torch.zeros(1, 4, 8, 8), torch.zeros(1, 4, 4, 3, 3), torch.zeros(1, 4), upsample=True, downsample=True,
                            fir=torch.ones(4, 4))


def test_cpu_tensors_still_fail_loudly():
    from ideas_amd.model import ModulatedConv2d
    import ideas_amd.op as op
    m = ModulatedConv2d(8, 8, 3, 16, downsample=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 8, 8, 8), torch.zeros(1, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.modulated_conv2d(torch.zeros(1, 8, 8, 8), torch.zeros(1, 8, 8, 3, 3), torch.zeros(1, 8), downsample=True, fir=m.blur.kernel)


def test_styled_conv_keeps_the_references_signature():
    import inspect
    from ideas_amd.model import StyledConv_without_noise
    assert "downsample" not in inspect.signature(StyledConv_without_noise.__init__).parameters


# ------------------------------------------------------------------------------------------------- C ABI
def _params(_lib, **kw):
    f = dict(B=2, IH=33, IW=33, Cin=32, YH=16, YW=16, Cout=64, OH=16, OW=16, TY=3, TX=3, sy=2, sx=2, dy=1, dx=1, offy=0, offx=0,
             osy=1, osx=1, ooy=0, oox=0, reflect=0, act=0, alpha=0.2, act_gain=1.0, resid_gain=1.0, accumulate=0, gain=1.0)
    f.update(kw)
    return _lib.ConvParams(**f)


def test_c_abi_declares_and_exports_the_modulated_entry_point():
    from ideas_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ideas_hip.h")).read()
    assert re.search(r"\bint\s+ideas_b3_blur_conv_s2_mod\s*\(", hdr)
    assert "ideas_b3_blur_conv_s2_mod" in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "ideas_b3_blur_conv_s2_mod")
    assert _lib.load().ideas_abi_version() == 4                                # additive within ABI 4


def test_c_abi_argument_checks_run_before_any_launch():
    """NULL pointers and geometries the kernel does not cover are refused by the checks in front of the launch (no device needed):
    the pointers below are host buffers that a launch would never survive."""
    from ideas_amd import _lib
    lib = _lib.load()
    E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
    fir = (ctypes.c_float * 4)(0.125, 0.375, 0.375, 0.125)
    buf = ctypes.create_string_buffer(256)
    a = ctypes.addressof(buf)
    a += (-a) % 16
    ok = _params(_lib)
    assert lib.ideas_b3_blur_conv_s2_supported(ctypes.byref(ok), 32, 32, 2) == 1

    def call(y=a, x=a, wp=a, fh=fir, fv=fir, p=ok, xh=32, xw=32, pad0=2, s=a, d=a):
        return lib.ideas_b3_blur_conv_s2_mod(y, None, x, wp, fh, fv, s, d, None, None, None if p is None else ctypes.byref(p), xh, xw,
                                             pad0, None)
    assert call(y=None) == E_NULL
    assert call(x=None) == E_NULL and call(wp=None) == E_NULL and call(fh=None) == E_NULL and call(p=None) == E_NULL
    assert call(y=None, s=None, d=None) == E_NULL                              # the unmodulated route checks the same
    for bad in (_params(_lib, TY=5, TX=5), _params(_lib, sy=1, sx=1), _params(_lib, Cin=24), _params(_lib, Cout=6),
                _params(_lib, OH=15), _params(_lib, reflect=1)):
        assert call(p=bad) in (E_SHAPE, E_UNSUPPORTED)
    assert call(pad0=4) in (E_SHAPE, E_UNSUPPORTED) and call(xh=64) in (E_SHAPE, E_UNSUPPORTED)


# ------------------------------------------------------------------------------------------------- the restatement vs the reference
def test_f64_restatement_reproduces_the_reference(gold):
    """The formula the GPU tests hold the kernels to, evaluated in f64 on the CPU, against the output and the five gradients the
    reference's own ModulatedConv2d(downsample=True) produced in f32: pins the restatement to the reference, not to the product."""
    meta = gold.json("meta")
    assert len(meta["cases"]) >= 5
    assert {c["k"] for c in meta["cases"]} == {1, 3} and any(not c["demodulate"] for c in meta["cases"])
    for c in meta["cases"]:
        t = f"down{c['i']}"
        x, st, w, mw, mb = (gold.t(f"{t}.{n}").double().requires_grad_(True) for n in ("x", "style", "w", "mw", "mb"))
        y = R.modconv_down(x, st, w, mw, mb, gold.t(f"{t}.fir").double(), demodulate=c["demodulate"])
        assert list(y.shape[2:]) == c["out_hw"], c
        e = rel_err(y, gold.t(f"{t}.y"))
        print(t, "y", e)
        assert e < TOL, (c, e)
        grads = torch.autograd.grad(y, (x, st, w, mw, mb), gold.t(f"{t}.gy").double())
        for got, n in zip(grads, ("gx", "gstyle", "gw", "gmw", "gmb")):
            e = rel_err(got, gold.t(f"{t}.{n}"))
            print(t, n, e)
            assert e < GTOL, (c, n, e)
