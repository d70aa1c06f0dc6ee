"""Outputs of every forward-family convolution kernel pinned to what the library gave BEFORE its epilogue was rewritten on the
shared rules of csrc/conv_epilogue.hpp (the f32 rule, the bf16 rule, the bf16 tile epilogue, the row table).

The rewrite alters no value: every site calls the same roundings in the same order as the text it replaces.
tests/golden/conv_epilogue_pinned.npz (tests/golden/make_golden_conv_epilogue_pinned.py, run on the parent commit's
library) holds, per output tensor of every case below, its shape, the SHA-256 of its bytes and its first 16 values; the
inputs are re-made here from seeds on the CPU.  Every case uses the fullest epilogue its kernel admits -- per-sample output
scale, bias, leaky-ReLU with act_gain != 1, residual with resid_gain != 1 -- and, where the kernel admits accumulation, a
second run that adds into a prefilled y.  Each case first asserts, from the plan and the library's ``*_supported`` exports
(restating csrc's dispatch rules where the library does not export them), that the intended kernel is the one that runs."""
import contextlib
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CL = torch.channels_last
BF = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "conv_epilogue_pinned.npz")
ALPHA, ACT_GAIN, RESID_GAIN = 0.2, 1.3, 0.6


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def _math(f32):
    """IDEAS_MATH=f32 for the duration: the f32 MFMA kernels instead of the split-bf16 ones (op/conv.py reads it at import)."""
    import ideas_amd.op.conv as CV
    from ideas_amd import _lib
    old = CV.MATH
    CV.MATH = _lib.F32 if f32 else old
    try:
        yield
    finally:
        CV.MATH = old


class _Rng:
    """CPU generator (the same stream on every machine); tensors go to the device afterwards."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def n(self, *s):
        return torch.randn(*s, generator=self.g)

    def u(self, *s):
        return torch.rand(*s, generator=self.g) + 0.5


def _cl(t, dtype=torch.float32):
    return t.to(dtype).cuda().contiguous(memory_format=CL)


def _sup(name, p, *more):
    from ideas_amd import _lib
    return bool(getattr(_lib.load(), name)(C.byref(p), *more))


def _pointwise(p):       # csrc/conv_direct.hip::is_pointwise
    return ((p.TY, p.TX, p.sy, p.sx, p.offy, p.offx, p.osy, p.osx, p.ooy, p.oox) == (1, 1, 1, 1, 0, 0, 1, 1, 0, 0)
            and (p.IH, p.IW) == (p.OH, p.OW) == (p.YH, p.YW))


def _b3_pw_shape(p, resid):      # csrc/conv_b3_pw.hip::ideas_b3_pw_ok for a launch without per-sample scales and without accumulation
    return (_pointwise(p) and not p.reflect and p.Cin % 16 == 0 and p.Cin >= 16 and p.Cout >= 16
            and (p.Cin <= 128 or (p.Cin % 128 == 0 and p.Cin <= 1024 and resid)))


def _s2img_shape(p):     # csrc/conv_b3_s2fir.hip::ideas_b3_s2img_ok under IDEAS_S2IMG_ALL=1, IDEAS_S2IMG_MIN_BLOCKS=1
    return ((p.TY, p.TX, p.sy, p.sx, p.offy, p.offx, p.reflect) == (3, 3, 2, 2, 0, 0, 0) and p.Cin % 16 == 0 and p.Cout % 4 == 0
            and p.OW >= 16 and p.OH >= 8)


def _bf16_pw_shape(p):   # csrc/conv_bf16_pw.hip::ideas_bf16_pw_ok for a launch with shared weights, no output scale, no accumulation
    return _pointwise(p) and not p.reflect and p.Cin in (32, 64, 128) and p.Cout % 8 == 0 and 8 <= p.Cout <= 256


def _bf16_img_tp(p):     # csrc/conv_bf16.hip::bf16_img_tp: patch width of the LDS-image kernel, 0 = not its geometry
    if (p.TY, p.TX, p.sy, p.sx, p.osy, p.osx, p.ooy, p.oox) != (3, 3, 1, 1, 1, 1, 0, 0) or (p.dy, p.offy, p.dx, p.offx) != (1, -1, 1, -1):
        return 0
    if (p.OH, p.OW) != (p.IH, p.IW) or (p.YH, p.YW) != (p.OH, p.OW) or p.Cin % 32 or p.Cout <= 32 or p.OW % 16:
        return 0
    tp = 64 if p.OW % 64 == 0 else 32 if p.OW % 32 == 0 else 16
    return tp if p.OH % (256 // tp) == 0 else 0


def _fwd(seed, shape, cout, k, stride, pad, gain, expect, *, dtype=torch.float32, mod=False, resid=True, reflect=False):
    """One forward launch through op/conv.py::launch_fwd with bias + leaky-ReLU * ACT_GAIN (+ per-sample scales, + residual);
    ``expect(p, with_resid)`` -> (is this the intended kernel, does it admit accumulation).  Outputs: y, and y accumulated into
    a prefilled tensor where admitted."""
    import ideas_amd.op.conv as CV
    from ideas_amd.op.conv_plan import ConvGeom, plan_fwd
    r = _Rng(seed)
    B, cin, H, W = shape
    x, w, b = _cl(r.n(*shape), dtype), _cl(r.n(cout, cin, k, k)), (r.n(cout) * 0.3).cuda()
    lin, lout = (r.u(B, cin).cuda(), r.u(B, cout).cuda()) if mod else (None, None)
    g = ConvGeom(k, k, stride, pad, reflect)
    L = plan_fwd(x.shape, w, g)
    yshape = (L.B, L.Cout, L.YH, L.YW)
    rs = _cl(r.n(*yshape), dtype) if resid else None
    prev = _cl(r.n(*yshape), dtype)
    outs = []
    admits_acc = expect(CV._params(L, gain, False, True, ALPHA, ACT_GAIN, RESID_GAIN), resid)[1]
    for acc in ((False, True) if admits_acc else (False,)):
        assert expect(CV._params(L, gain, acc, True, ALPHA, ACT_GAIN, RESID_GAIN), resid)[0], (shape, cout, k, acc)
        y = prev.clone() if acc else torch.empty(yshape, device="cuda", dtype=dtype, memory_format=CL)
        CV.launch_fwd(y, x, L, gain, lin, lout, b, rs, act=True, alpha=ALPHA, act_gain=ACT_GAIN, resid_gain=RESID_GAIN, accumulate=acc)
        outs.append(y)
    return outs


# ---- which kernel a launch_fwd call reaches (csrc/conv_igemm.hip::ideas_conv_igemm, conv_b3.hip::ideas_b3_fwd, conv_bf16.hip::ideas_bf16_fwd) -----
def _is_igemm_f32(p, resid):
    import ideas_amd.op.conv as CV
    from ideas_amd import _lib
    return CV.MATH == _lib.F32 and p.Cin % 4 == 0, True


def _is_b3_generic(p, resid):    # IDEAS_S2IMG_MIN_BLOCKS=0: not the LDS-image kernel; 3x3: not the flat 1x1 kernel
    import ideas_amd.op.conv as CV
    from ideas_amd import _lib
    return (CV.MATH == _lib.F32_B3 and _sup("ideas_b3_conv_supported", p) and p.TY * p.TX == 9 and os.environ.get("IDEAS_S2IMG_MIN_BLOCKS") == "0"
            and (p.B * p.OH * p.OW) % 128 != 0), True


def _is_b3_pw(p, resid):         # accumulation is the generic kernel's: the flat kernel declines it
    return _sup("ideas_b3_conv_supported", p) and _b3_pw_shape(p, resid) and p.Cin <= 128 and not p.accumulate, False


def _is_b3_pwk(p, resid):
    return _sup("ideas_b3_conv_supported", p) and _b3_pw_shape(p, resid) and p.Cin > 128 and not p.accumulate, False


def _is_s2img(p, resid):
    return _sup("ideas_b3_conv_supported", p) and _s2img_shape(p) and not p.accumulate, False


def _direct_kernel(p):
    """csrc/conv_direct.hip::conv_direct_impl without per-sample scales: the four VALU kernels in the order it tries them."""
    pw = _pointwise(p)
    if pw and p.Cout <= 8 and p.Cin >= 32:
        return "rowdot"
    if pw and p.Cin <= 4 and p.Cout % 4 == 0 and 16 <= p.Cout <= 1024:
        return "smallk_vec"
    if pw and p.Cin <= 8 and p.Cout <= 256:
        return "smallk"
    return "direct"


def _is_bf16_generic(p, resid):  # not the flat 1x1 kernel (3x3), not the LDS-image kernel (stride 2)
    return _sup("ideas_bf16_conv_supported", p, 1) and not _bf16_pw_shape(p) and _bf16_img_tp(p) == 0, True


def _is_bf16_img(p, resid):      # 16 x 16: the narrowest patch (TP = 16), one patch per image
    return _sup("ideas_bf16_conv_supported", p, 1) and _bf16_img_tp(p) == 16 and os.environ.get("IDEAS_BF16_IMG") != "0", True


def _is_bf16_pw(p, resid):
    return _sup("ideas_bf16_conv_supported", p, 0) and _bf16_pw_shape(p) and not p.accumulate and os.environ.get("IDEAS_BF16_PW") != "0", False


def _direct_f32(seed, shape, cout, k, kernel):
    """The VALU kernels behind ideas_conv_direct through the C ABI (launch_fwd sends f32 launches with Cin % 4 == 0 to the MFMA
    kernel, which leaves the row-dot kernel to the bf16 path and to this call)."""
    import ideas_amd.op.conv as CV
    from ideas_amd import _lib
    from ideas_amd.op.conv_plan import ConvGeom, plan_fwd
    r = _Rng(seed)
    x, w, b = _cl(r.n(*shape)), _cl(r.n(cout, shape[1], k, k)), (r.n(cout) * 0.3).cuda()
    L = plan_fwd(x.shape, w, ConvGeom(k, k, 1, k // 2, False))
    yshape = (L.B, L.Cout, L.YH, L.YW)
    rs, prev = _cl(r.n(*yshape)), _cl(r.n(*yshape))
    outs = []
    for acc in (False, True):
        p = CV._params(L, 0.21, acc, True, ALPHA, ACT_GAIN, RESID_GAIN)
        assert _direct_kernel(p) == kernel
        y = prev.clone() if acc else torch.empty(yshape, device="cuda", memory_format=CL)
        rc = _lib.load().ideas_conv_direct(_lib.ptr(y), _lib.ptr(x), _lib.ptr(L.wmat), None, None, _lib.ptr(b), _lib.ptr(rs), C.byref(p),
                                           _lib.F32, _lib.stream_ptr())
        _lib.check(rc, "ideas_conv_direct")
        outs.append(y)
    return outs


def _direct_bf16(seed, shape, cout, k, kernel):
    def expect(p, resid):
        # op/conv.py::launch_fwd, bf16: no MFMA kernel for the geometry, and the VALU kernels are its declared bf16 path
        return _sup("ideas_bf16_direct_supported", p) and not _sup("ideas_bf16_conv_supported", p, 0) and _direct_kernel(p) == kernel, True
    return _fwd(seed, shape, cout, k, 1, 0, 0.21, expect, dtype=BF)


def _direct_modulated(seed, dtype):
    """conv_direct_kernel with everything on: 3x3, Cin = 3, per-sample scales (only this kernel of the file takes them)."""
    import ideas_amd.op.conv as CV
    from ideas_amd import _lib
    from ideas_amd.op.conv_plan import ConvGeom, plan_fwd
    r = _Rng(seed)
    x, w, b = _cl(r.n(2, 3, 7, 9), dtype), _cl(r.n(8, 3, 3, 3)), (r.n(8) * 0.3).cuda()
    lin, lout = r.u(2, 3).cuda(), r.u(2, 8).cuda()
    L = plan_fwd(x.shape, w, ConvGeom(3, 3, 1, 1, False))
    yshape = (L.B, L.Cout, L.YH, L.YW)
    rs, prev = _cl(r.n(*yshape), dtype), _cl(r.n(*yshape), dtype)
    outs = []
    for acc in (False, True):
        p = CV._params(L, 0.19, acc, True, ALPHA, ACT_GAIN, RESID_GAIN)
        assert _direct_kernel(p) == "direct" and p.Cin == 3
        y = prev.clone() if acc else torch.empty(yshape, device="cuda", dtype=dtype, memory_format=CL)
        rc = _lib.load().ideas_conv_direct(_lib.ptr(y), _lib.ptr(x), _lib.ptr(L.wmat), _lib.ptr(lin), _lib.ptr(lout), _lib.ptr(b), _lib.ptr(rs),
                                           C.byref(p), _lib.BF16 if dtype == BF else _lib.F32, _lib.stream_ptr())
        _lib.check(rc, "ideas_conv_direct")
        outs.append(y)
    return outs


def _s2fir(mod):
    """conv_b3_s2fir_kernel MODE 0: Blur (pad 2, 2) + 3x3 / stride 2, 16 -> 64 channels, 16 x 32 -> 17 x 33 -> 8 x 16, with bias,
    activation and the residual (the raw launcher fixes resid_gain at 1; no accumulation in this kernel)."""
    import ideas_amd.op.conv as CV
    from ideas_amd.model import make_kernel
    r = _Rng(141 + mod)
    x, w, b = _cl(r.n(1, 16, 16, 32)), _cl(r.n(64, 16, 3, 3)), (r.n(64) * 0.3).cuda()
    lin, lout = (r.u(1, 16).cuda(), r.u(1, 64).cuda()) if mod else (None, None)
    rs = _cl(r.n(1, 64, 8, 16))
    fir = make_kernel((1, 3, 3, 1)).cuda()
    assert CV.blur_conv_s2_ok(x, w, fir, (2, 2))
    y, _ = CV.blur_conv_s2_raw(x, w, fir, (2, 2), 0.08, bias=b, act=True, act_gain=ACT_GAIN, alpha=ALPHA, resid=rs, lin=lin, lout=lout)
    assert tuple(y.shape) == (1, 64, 8, 16)
    return [y]


def _tphase(cin, cout, h, w_, B, st16):
    """conv_b3_tphase_kernel, modulated (the scale piece of the rule only: gain, out_scale), both store forms."""
    import ideas_amd.op.conv as CV
    from ideas_amd import _lib
    from ideas_amd.op.conv_plan import ConvGeom, convT_out_size, plan_dgrad
    r = _Rng(123 + cin + cout + h)
    x, w = _cl(r.n(B, cin, h, w_)), _cl(r.n(cin, cout, 3, 3))
    lin, lout = r.u(B, cin).cuda(), r.u(B, cout).cuda()
    g = ConvGeom(3, 3, 2, 0, False)
    out_hw = convT_out_size(h, w_, g)
    launches, need_zero = plan_dgrad(x.shape, w, g, out_hw)
    assert len(launches) == 4 and not need_zero and all(_sup("ideas_b3_conv_supported", CV._params(L, 0.05)) for L in launches)
    # csrc/conv_b3_tphase.hip::tphase_match: this geometry with Cin % 16 == 0 and Cout > 64
    assert cin % 16 == 0 and cout > 64 and out_hw == (2 * h + 1, 2 * w_ + 1)
    y = CV.conv_dgrad_raw(x, w, g, out_hw, 0.05, lin=lin, lout=lout)
    fn = _lib.load().ideas_b3_tphase_store16
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    assert int(fn(y.data_ptr(), cout)) == int(st16)
    return [y]


def _bf16_multi(cin, cout, h, w_, B):
    """conv_bf16_multi_kernel: the four parity phases of a modulated 3x3 / stride-2 / pad-0 transposed conv on bf16 activations in one
    grid.  The kernel has no bias, activation, residual or accumulation (ideas_conv_igemm_multi declines them): gain and the
    per-sample output scale are its whole epilogue, in its own arithmetic form (csrc/conv_epilogue.hpp::epi_bf16, BIAS = false)."""
    import ideas_amd.op.conv as CV
    from ideas_amd.op.conv_plan import ConvGeom, convT_out_size, plan_dgrad
    r = _Rng(131 + cin + cout + h)
    x, w = _cl(r.n(B, cin, h, w_), BF), _cl(r.n(cin, cout, 3, 3))
    lin, lout = r.u(B, cin).cuda(), r.u(B, cout).cuda()
    g = ConvGeom(3, 3, 2, 0, False)
    out_hw = convT_out_size(h, w_, g)
    launches, need_zero = plan_dgrad(x.shape, w, g, out_hw)
    # op/conv.py::launch_multi takes 2-4 launches that the bf16 MFMA family covers, all of them, as one ideas_conv_igemm_multi call
    assert CV.B3_MULTI and len(launches) == 4 and not need_zero
    assert all(_sup("ideas_bf16_conv_supported", CV._params(L, 0.05), 1) for L in launches)
    y = CV.conv_dgrad_raw(x, w, g, out_hw, 0.05, lin=lin, lout=lout)
    assert y.dtype == BF and tuple(y.shape) == (B, cout, 2 * h + 1, 2 * w_ + 1)
    return [y]


def _wino(seed, shape, cout, f32, vec, accumulate):
    """The generic Winograd tail (wino_finish4; IDEAS_B3_WINO_EPI=0 turns the branch-free tails off) of the split-bf16 kernels, or
    conv3x3_wino_kernel (f32): modulated, bias, activation, residual; ``vec``: the 16-byte branch (Cout % 4 == 0 and 16-byte
    aligned operands), else the element-wise one, reached with a bias that is only 4-byte aligned."""
    import ideas_amd.op.conv as CV
    from ideas_amd import _lib
    from ideas_amd.op.conv_plan import ConvGeom, plan_fwd
    r = _Rng(seed)
    B, cin, H, W = shape
    x, w, b = _cl(r.n(*shape)), _cl(r.n(cout, cin, 3, 3)), (r.n(cout + 1) * 0.3).cuda()[0 if vec else 1:][:cout]
    lin, lout = r.u(B, cin).cuda(), r.u(B, cout).cuda()
    rs, prev = _cl(r.n(B, cout, H, W)), _cl(r.n(B, cout, H, W))
    g = ConvGeom(3, 3, 1, 1, False)
    p0 = CV._params(plan_fwd(x.shape, w, g), 0.06)
    # csrc/conv_b3_wino.hip::wino_vec_ok
    assert (cout % 4 == 0 and all(t.data_ptr() % 16 == 0 for t in (prev, rs, lout, b))) == vec and b.data_ptr() % 4 == 0
    if f32:
        assert CV._wino_ok(g, cin, W) and cin % 8 == 0 and W % 2 == 0
        u, dt = CV.wino_weights(w.permute(0, 2, 3, 1)), _lib.F32
    else:
        assert CV._b3_wino_ok(g, cin, cout, W) and _sup("ideas_b3_wino_supported", p0) and os.environ.get("IDEAS_B3_WINO_EPI") == "0"
        u, dt = CV.b3_wino_planes(w, False), _lib.F32_B3
    outs = []
    for acc in ((False, True) if accumulate else (False,)):
        y = prev.clone() if acc else torch.empty((B, cout, H, W), device="cuda", memory_format=CL)
        p = _lib.ConvParams(B, H, W, cin, H, W, cout, H, W, 3, 3, 1, 1, 1, 1, -1, -1, 1, 1, 0, 0, 0, 1, ALPHA, ACT_GAIN, RESID_GAIN, int(acc), 0.06)
        rc = _lib.load().ideas_conv3x3_wino(_lib.ptr(y), _lib.ptr(x), _lib.ptr(u), _lib.ptr(lin), _lib.ptr(lout), _lib.ptr(b), _lib.ptr(rs),
                                            C.byref(p), dt, _lib.stream_ptr())
        _lib.check(rc, "ideas_conv3x3_wino")
        outs.append(y)
    return outs


_NO_S2IMG = {"IDEAS_S2IMG_MIN_BLOCKS": "0"}
_S2IMG = {"IDEAS_S2IMG_ALL": "1", "IDEAS_S2IMG_MIN_BLOCKS": "1"}
_TPHASE = {"IDEAS_B3_TPHASE": "1", "IDEAS_B3_TPHASE_STORE": None}
_WINO_GENERIC = {"IDEAS_B3_WINO_EPI": "0", "IDEAS_B3_WINO2D": None, "IDEAS_B3_WINO_N256": None}
GENERIC = ((1, 16, 9, 11), 80, 3, 2, 0)     # 3x3 / stride 2 / no padding, 16 -> 80 channels, 9 x 11 -> 4 x 5: 20 rows of a 128-row tile, ragged N
# name -> (environment, f32 math path, thunk returning the output tensors)
CASES = {
    "igemm_f32": ({}, True, lambda: _fwd(201, *GENERIC, 0.07, _is_igemm_f32, mod=True)),
    "b3_generic": (_NO_S2IMG, False, lambda: _fwd(202, *GENERIC, 0.07, _is_b3_generic, mod=True)),
    "b3_pw_ragged": ({"IDEAS_B3_PW": None}, False, lambda: _fwd(203, (3, 32, 9, 14), 64, 1, 1, 0, 0.11, _is_b3_pw)),
    "b3_pw_full": ({"IDEAS_B3_PW": None}, False, lambda: _fwd(204, (2, 64, 16, 16), 128, 1, 1, 0, 0.11, _is_b3_pw)),
    "b3_pwk_ragged": ({"IDEAS_B3_PW": None}, False, lambda: _fwd(205, (3, 256, 9, 14), 64, 1, 1, 0, 0.11, _is_b3_pwk)),
    "b3_pwk_full": ({"IDEAS_B3_PW": None}, False, lambda: _fwd(206, (2, 256, 16, 16), 128, 1, 1, 0, 0.11, _is_b3_pwk)),
    "s2fir_plain": ({"IDEAS_S2FIR_CFG": None}, False, lambda: _s2fir(0)),
    "s2fir_mod": ({"IDEAS_S2FIR_CFG": None}, False, lambda: _s2fir(1)),
    "s2img_plain": (_S2IMG, False, lambda: _fwd(207, (1, 16, 17, 33), 64, 3, 2, 0, 0.08, _is_s2img)),
    "s2img_mod": (_S2IMG, False, lambda: _fwd(208, (1, 16, 17, 33), 64, 3, 2, 0, 0.08, _is_s2img, mod=True)),
    "s2img_ba_row": (_S2IMG, False, lambda: _fwd(209, (2, 64, 17, 33), 256, 3, 2, 0, 0.05, _is_s2img)),
    "s2img_mod_row": (_S2IMG, False, lambda: _fwd(210, (1, 128, 65, 65), 128, 3, 2, 0, 0.05, _is_s2img, mod=True)),
    "tphase_store16": (_TPHASE, False, lambda: _tphase(16, 128, 4, 16, 2, True)),
    "tphase_store4": (dict(_TPHASE, IDEAS_B3_TPHASE_STORE="0"), False, lambda: _tphase(16, 128, 4, 16, 2, False)),
    "tphase_ragged_store16": (_TPHASE, False, lambda: _tphase(32, 192, 5, 18, 2, True)),
    "wino_b3_vec_acc": (_WINO_GENERIC, False, lambda: _wino(211, (2, 32, 8, 16), 128, False, True, True)),
    "wino_b3_elementwise": (_WINO_GENERIC, False, lambda: _wino(212, (1, 32, 8, 14), 72, False, False, False)),
    "wino_b3_small_tile_acc": (_WINO_GENERIC, False, lambda: _wino(213, (1, 16, 6, 10), 36, False, True, True)),
    "wino_f32": ({}, True, lambda: _wino(214, (1, 16, 6, 10), 72, True, True, True)),
    "direct_f32": ({}, True, lambda: _direct_modulated(215, torch.float32)),
    "direct_bf16": ({}, False, lambda: _direct_modulated(216, BF)),
    "smallk_f32": ({}, True, lambda: _direct_f32(217, (2, 3, 9, 7), 6, 1, "smallk")),
    "smallk_bf16": ({}, False, lambda: _direct_bf16(218, (2, 3, 9, 7), 6, 1, "smallk")),
    "smallk_vec_f32": ({}, True, lambda: _direct_f32(219, (2, 3, 9, 7), 32, 1, "smallk_vec")),
    "smallk_vec_bf16": ({}, False, lambda: _direct_bf16(220, (2, 3, 9, 7), 32, 1, "smallk_vec")),
    "rowdot_f32": ({}, True, lambda: _direct_f32(221, (2, 64, 9, 7), 3, 1, "rowdot")),
    "rowdot_bf16": ({}, False, lambda: _direct_bf16(222, (2, 64, 9, 7), 3, 1, "rowdot")),
    "bf16_wide": ({}, False, lambda: _fwd(223, (2, 32, 9, 11), 80, 3, 2, 0, 0.07, _is_bf16_generic, dtype=BF, mod=True)),
    "bf16_narrow": ({}, False, lambda: _fwd(224, (2, 32, 9, 11), 76, 3, 2, 0, 0.07, _is_bf16_generic, dtype=BF, mod=True)),
    "bf16_img": ({"IDEAS_BF16_IMG": None}, False, lambda: _fwd(225, (2, 32, 16, 16), 64, 3, 1, 1, 0.06, _is_bf16_img, dtype=BF, mod=True)),
    "bf16_multi_mod": ({}, False, lambda: _bf16_multi(32, 128, 4, 16, 2)),
    "bf16_multi_mod_narrow": ({}, False, lambda: _bf16_multi(32, 36, 5, 9, 2)),
    "bf16_pw": ({"IDEAS_BF16_PW": None}, False, lambda: _fwd(226, (3, 32, 9, 14), 64, 1, 1, 0, 0.11, _is_bf16_pw, dtype=BF)),
}


def run_case(name):
    """[(shape, sha256 hex, first 16 values as float32)] of the case's outputs, in their memory order (bf16 hashed as stored)."""
    env, f32, thunk = CASES[name]
    with _env(**env), _math(f32):
        outs = thunk()
        torch.cuda.synchronize()
    res = []
    for t in outs:
        t = t.detach().permute(0, 2, 3, 1).contiguous()
        a = t.float().cpu().numpy()
        assert np.isfinite(a).all() and float(np.abs(a).max()) > 0, name
        raw = (t.view(torch.int16) if t.dtype == BF else t).cpu().numpy()
        res.append((tuple(a.shape), hashlib.sha256(raw.tobytes()).hexdigest(), a.reshape(-1)[:16].astype(np.float32).copy()))
    return res


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _check(name, got, golden):
    assert int(golden[name + "/n"]) == len(got)
    for i, (shape, sha, head) in enumerate(got):
        k = "%s/%d" % (name, i)
        assert tuple(golden[k + "/shape"]) == shape, k
        assert np.array_equal(golden[k + "/head"], head), (k, golden[k + "/head"], head)
        assert bytes(golden[k + "/sha256"]).hex() == sha, k


@pytest.mark.parametrize("name", sorted(CASES))
def test_conv_epilogue_outputs_are_bitwise_the_pinned_ones(name, golden):
    _check(name, run_case(name), golden)

