"""Outputs of the split-bf16 ("b3") kernel families pinned to what the library gave BEFORE their staging code was rewritten
with single-instruction f32 helpers (csrc/b3.hpp) and before conv_b3_tphase_kernel got its 16-byte stores.

Neither change alters a value: the helpers compute the same IEEE operations one lane-element at a time, the new epilogue
applies the same roundings in the same order.  tests/golden/b3_pinned.npz (tests/golden/make_golden_b3_pinned.py, run on
the parent commit's library) holds, per output tensor of every case below, its shape, the SHA-256 of its bytes and its
first 16 values; the inputs are re-made here from seeds on the CPU.  One case per family at the smallest shape its
dispatch admits, plain and modulated where the family has both; each case first asserts from the plan that the intended
kernel is the one that runs (the predicates below restate csrc's dispatch rules where the library does not export them).
The weight-gradient cases have B * OH = 16 and OW = 16, a single block per tile, so that the f32 atomics add into zeros
exactly once and the result does not depend on the run."""
import contextlib
import ctypes as C
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CL = torch.channels_last
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "b3_pinned.npz")


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


class _Rng:
    """CPU generator (the same stream on every machine); tensors go to the device afterwards."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def n(self, *s):
        return torch.randn(*s, generator=self.g)

    def u(self, *s):
        return torch.rand(*s, generator=self.g) + 0.5


def _cl(t):
    return t.cuda().contiguous(memory_format=CL)


def _sup(name, p):
    from ideas_amd import _lib
    return bool(getattr(_lib.load(), name)(C.byref(p)))


# ---- the cases: name -> (environment, thunk returning the output tensors) --------------------------------------------------------

def _generic(mod):
    """conv_b3_kernel: 3x3 / stride 2 / no padding, 16 -> 80 channels, 9 x 11 -> 4 x 5: M = 20 of a 128-pixel tile, ragged N."""
    import ideas_amd.op.conv as CV
    from ideas_amd.op.conv_plan import ConvGeom, plan_fwd
    r = _Rng(11 + mod)
    x, w = _cl(r.n(1, 16, 9, 11)), _cl(r.n(80, 16, 3, 3))
    lin, lout = (r.u(1, 16).cuda(), r.u(1, 80).cuda()) if mod else (None, None)
    g = ConvGeom(3, 3, 2, 0, False)
    p = CV._params(plan_fwd(x.shape, w, g), 0.07)
    assert _sup("ideas_b3_conv_supported", p) and p.TY * p.TX == 9      # not the flat 1x1 kernel; IDEAS_S2IMG_MIN_BLOCKS=0: not MODE 1
    assert (p.B * p.OH * p.OW) % 128 != 0
    return [CV.conv_fwd_raw(x, w, g, 0.07, lin=lin, lout=lout)]


def _transposed(mod, cin, cout, h, w_, B, expect_tphase):
    """The four parity phases of a 3x3 / stride-2 / pad-0 transposed conv: conv_b3_multi_kernel (Cout <= 64) or conv_b3_tphase_kernel."""
    import ideas_amd.op.conv as CV
    from ideas_amd.op.conv_plan import ConvGeom, convT_out_size, plan_dgrad
    r = _Rng(23 + mod + cin + cout + h)
    x, w = _cl(r.n(B, cin, h, w_)), _cl(r.n(cin, cout, 3, 3))
    lin, lout = (r.u(B, cin).cuda(), r.u(B, cout).cuda()) if mod else (None, None)
    g = ConvGeom(3, 3, 2, 0, False)
    out_hw = convT_out_size(h, w_, g)
    launches, need_zero = plan_dgrad(x.shape, w, g, out_hw)
    assert len(launches) == 4 and not need_zero
    assert all(_sup("ideas_b3_conv_supported", CV._params(L, 0.05)) for L in launches)
    assert sorted((L.TY, L.TX) for L in launches) == [(1, 1), (1, 2), (2, 1), (2, 2)]
    # csrc/conv_b3_tphase.hip::tphase_match: this geometry with Cin % 16 == 0 and Cout > 64 (IDEAS_B3_TPHASE=1: plain launches too)
    assert (cin % 16 == 0 and cout > 64 and out_hw == (2 * h + 1, 2 * w_ + 1)) == expect_tphase
    return [CV.conv_dgrad_raw(x, w, g, out_hw, 0.05, lin=lin, lout=lout)]


def _wino2d(mod, cout, want_n256):
    """conv_b3_wino2d_kernel: 32 -> 128 (NB = 2) / 256 (NB = 4) channels on 8 x 16 (8 pair columns, one patch)."""
    import ideas_amd.op.conv as CV
    from ideas_amd import _lib
    from ideas_amd.op.conv_plan import ConvGeom, plan_fwd
    r = _Rng(37 + mod + cout)
    B, cin, H, W = 1, 32, 8, 16
    x, w = _cl(r.n(B, cin, H, W)), _cl(r.n(cout, cin, 3, 3))
    lin, lout = (r.u(B, cin).cuda(), r.u(B, cout).cuda()) if mod else (None, None)
    g = ConvGeom(3, 3, 1, 1, False)
    assert CV._b3_wino_ok(g, cin, cout, W) and _sup("ideas_b3_wino_supported", CV._params(plan_fwd(x.shape, w, g), 0.06))
    # csrc/conv_b3_wino.hip::wino_choose: the row-sharing kernel needs the wide tile and an image that divides into its patches
    w2 = W // 2
    tp = 32 if w2 % 32 == 0 else 16 if w2 % 16 == 0 else 8 if w2 % 8 == 0 else 0
    assert cin % 32 == 0 and cout > 64 and tp and H % (64 // tp) == 0
    fn = _lib.load().ideas_b3_wino_n256_tiles
    fn.restype, fn.argtypes = C.c_int64, [C.c_int] * 5
    assert (int(fn(B, H, W, cin, cout)) > 0) == want_n256
    return [CV.conv_fwd_raw(x, w, g, 0.06, lin=lin, lout=lout)]


def _s2fir(mod, want_xb):
    """conv_b3_s2fir_kernel with its FIR: Blur (pad 2, 2) + 3x3 / stride 2, 16 -> 64 channels, 16 x 32 -> 17 x 33 -> 8 x 16."""
    import ideas_amd.op.conv as CV
    from ideas_amd.model import make_kernel
    r = _Rng(41 + mod)
    x, w = _cl(r.n(1, 16, 16, 32)), _cl(r.n(64, 16, 3, 3))
    lin, lout = (r.u(1, 16).cuda(), r.u(1, 64).cuda()) if mod else (None, None)
    fir = make_kernel((1, 3, 3, 1)).cuda()
    assert CV.blur_conv_s2_ok(x, w, fir, (2, 2), want_xb=want_xb)
    y, xb = CV.blur_conv_s2_raw(x, w, fir, (2, 2), 0.08, want_xb=want_xb, lin=lin, lout=lout)
    assert (xb is not None) == want_xb
    return [y] + ([xb] if want_xb else [])


def _s2img(mod):
    """conv_b3_s2fir_kernel, MODE 1 (no FIR): 3x3 / stride 2 / no padding, 16 -> 64 channels, 17 x 33 -> 8 x 16."""
    import ideas_amd.op.conv as CV
    from ideas_amd.op.conv_plan import ConvGeom, plan_fwd
    r = _Rng(43 + mod)
    x, w = _cl(r.n(1, 16, 17, 33)), _cl(r.n(64, 16, 3, 3))
    lin, lout = (r.u(1, 16).cuda(), r.u(1, 64).cuda()) if mod else (None, None)
    g = ConvGeom(3, 3, 2, 0, False)
    p = CV._params(plan_fwd(x.shape, w, g), 0.08)
    # csrc/conv_b3_s2fir.hip::ideas_b3_s2img_ok under IDEAS_S2IMG_ALL=1, IDEAS_S2IMG_MIN_BLOCKS=1
    assert (p.TY, p.TX, p.sy, p.offy, p.reflect) == (3, 3, 2, 0, 0) and p.Cin % 16 == 0 and p.Cout % 4 == 0 and p.OW >= 16 and p.OH >= 8
    return [CV.conv_fwd_raw(x, w, g, 0.08, lin=lin, lout=lout)]


def _pw():
    """conv_b3_pw_kernel: 1x1, 16 -> 16 channels on 4 x 4."""
    import ideas_amd.op.conv as CV
    from ideas_amd.op.conv_plan import ConvGeom, plan_fwd
    r = _Rng(47)
    x, w, b = _cl(r.n(1, 16, 4, 4)), _cl(r.n(16, 16, 1, 1)), r.n(16).cuda()
    g = ConvGeom(1, 1, 1, 0, False)
    p = CV._params(plan_fwd(x.shape, w, g), 0.2)
    # csrc/conv_b3_pw.hip::ideas_b3_pw_ok: single tap, dense, no per-sample scales, Cin % 16 == 0 up to 128, Cout >= 16
    assert _sup("ideas_b3_conv_supported", p) and (p.TY, p.TX, p.sy) == (1, 1, 1) and p.Cin % 16 == 0 and 16 <= p.Cin <= 128 and p.Cout >= 16
    return [CV.conv_fwd_raw(x, w, g, 0.2, bias=b, act=True, act_gain=math.sqrt(2))]


def _wgrad(mod, stride, cin, tap_fused):
    """conv_b3_wgrad3_kernel<stride> / conv_b3_wgrad_kernel (IDEAS_B3_WGRAD3=0): B * OH = 16, OW = 16, one block per tile."""
    import ideas_amd.op.conv as CV
    from ideas_amd.op.conv_plan import ConvGeom, plan_wgrad
    r = _Rng(53 + mod + stride + cin)
    cout = 64
    g = ConvGeom(3, 3, stride, 1 if stride == 1 else 0, False)
    ih, iw = (16, 16) if stride == 1 else (33, 33)
    x, gy = _cl(r.n(1, cin, ih, iw)), _cl(r.n(1, cout, 16, 16))
    lin, lout = (r.u(1, cin).cuda(), r.u(1, cout).cuda()) if mod else (None, None)
    p = CV._params(plan_wgrad(x.shape, gy.shape, g), 0.03)
    assert (p.OH, p.OW) == (16, 16) and _sup("ideas_b3_wgrad_supported", p)
    assert _sup("ideas_b3_wgrad3_supported", p)                          # (the shape; the switch keeps the generic case off it)
    assert (os.environ.get("IDEAS_B3_WGRAD3") != "0") == tap_fused
    return [CV.conv_wgrad_raw(gy, x, g, (cout, cin, 3, 3), 0.03, lin=lin, lout=lout)]


_NO_S2IMG = {"IDEAS_S2IMG_MIN_BLOCKS": "0"}
_S2IMG = {"IDEAS_S2IMG_ALL": "1", "IDEAS_S2IMG_MIN_BLOCKS": "1"}
CASES = {}
for _m, _tag in ((0, "plain"), (1, "mod")):
    CASES["generic_" + _tag] = (_NO_S2IMG, lambda m=_m: _generic(m))
    CASES["multi_" + _tag] = ({"IDEAS_B3_TPHASE": "1"}, lambda m=_m: _transposed(m, 16, 32, 4, 5, 1, False))
    CASES["tphase_" + _tag] = ({"IDEAS_B3_TPHASE": "1"}, lambda m=_m: _transposed(m, 16, 128, 4, 16, 2, True))
    CASES["tphase_ragged_" + _tag] = ({"IDEAS_B3_TPHASE": "1"}, lambda m=_m: _transposed(m, 32, 192, 5, 18, 2, True))
    CASES["wino2d_nb2_" + _tag] = ({"IDEAS_B3_WINO2D": None, "IDEAS_B3_WINO_N256": "0"}, lambda m=_m: _wino2d(m, 128, False))
    CASES["wino2d_nb4_" + _tag] = ({"IDEAS_B3_WINO2D": None, "IDEAS_B3_WINO_N256": "1"}, lambda m=_m: _wino2d(m, 256, True))
    CASES["s2fir_" + _tag] = ({"IDEAS_S2FIR_CFG": None}, lambda m=_m: _s2fir(m, False))
    CASES["s2fir_xb_" + _tag] = ({"IDEAS_S2FIR_CFG": None}, lambda m=_m: _s2fir(m, True))
    CASES["s2img_" + _tag] = (_S2IMG, lambda m=_m: _s2img(m))
    CASES["wgrad3_s1_" + _tag] = ({"IDEAS_B3_WGRAD3": None}, lambda m=_m: _wgrad(m, 1, 64, True))
    CASES["wgrad3_s2_" + _tag] = ({"IDEAS_B3_WGRAD3": None, "IDEAS_B3_WGRAD3_S2": None}, lambda m=_m: _wgrad(m, 2, 64, True))
    CASES["wgrad_" + _tag] = ({"IDEAS_B3_WGRAD3": "0"}, lambda m=_m: _wgrad(m, 1, 256, False))
CASES["pw"] = ({"IDEAS_B3_PW": None}, _pw)
S2FIR_CASES = [k for k in CASES if k.startswith(("s2fir_", "s2img_"))]      # also run on libideas_hip_dppb.so


def run_case(name):
    """[(shape, sha256 hex, first 16 values as float32)] of the case's outputs, in their memory order."""
    env, thunk = CASES[name]
    with _env(**env):
        outs = thunk()
        torch.cuda.synchronize()
    res = []
    for t in outs:
        a = t.detach().permute(0, 2, 3, 1).contiguous().cpu().numpy() if t.dim() == 4 else t.detach().cpu().numpy()
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
        res.append((tuple(a.shape), hashlib.sha256(a.tobytes()).hexdigest(), a.reshape(-1)[:16].copy()))
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
def test_b3_outputs_are_bitwise_the_pinned_ones(name, golden):
    _check(name, run_case(name), golden)


def test_b3_s2fir_outputs_are_pinned_on_the_dpp_builtin_build_too(golden):
    """The Blur + stride-2 cases on libideas_hip_dppb.so (child process: the library is chosen at import)."""
    from ideas_amd import _lib
    lib = os.path.join(os.path.dirname(os.path.abspath(_lib.LIB_PATH)), "libideas_hip_dppb.so")
    assert os.path.exists(lib), "make -C ideas_amd/csrc builds libideas_hip_dppb.so next to libideas_hip.so"
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + S2FIR_CASES, env=dict(os.environ, IDEAS_HIP_LIB=lib),
                       capture_output=True, text=True, timeout=600, cwd=os.path.dirname(HERE))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(got) == sorted(S2FIR_CASES)
    for name, outs in got.items():
        _check(name, [(tuple(s), h, np.array(v, dtype=np.float32)) for s, h, v in outs], golden)


if __name__ == "__main__":          # python tests/test_b3_pinned_gpu.py CASE...: one JSON line {case: [[shape, sha256, head], ...]}
    sys.path.insert(0, os.path.dirname(HERE))
    out = {n: [[list(s), h, [float(v) for v in head]] for s, h, head in run_case(n)] for n in sys.argv[1:]}
    print(json.dumps(out))
