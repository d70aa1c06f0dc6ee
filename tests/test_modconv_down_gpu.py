"""GPU parity of the downsampling ModulatedConv2d (stylegan2/model.py:181-277, downsample branch: Blur, then the stride-2
``groups=batch`` conv of per-sample weights) on the HIP path: one launch of csrc/conv_b3_s2fir.hip with per-sample scales where the
dispatch admits the shape, the blur kernel + the scaled stride-2 conv elsewhere.

The oracle has no such layer; the reference here is tests/modconv_down_ref.py, the f64 restatement that
tests/test_modconv_down.py pins to the reference's own recorded output on the CPU.  Bounds: ``rel_err`` with TOL / GTOL of
tests/test_ops_gpu.py::test_modconv_golden."""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import Golden, rel_err
import modconv_down_ref as R

pytestmark = pytest.mark.gpu
CL = torch.channels_last
TOL, GTOL = 1e-5, 1e-4
FIR = (1, 3, 3, 1)
# (B, Cin, Cout, H, fused, min_blocks): `fused` = the fused launch is dispatched for the shape (with a weight gradient pending) at the
# workgroup threshold `min_blocks` (None: the default of op.conv.BLUR_CONV_MOD_MIN_BLOCKS, 512).  The three small shapes have 32, 16
# and 8 workgroups: the tests lower the threshold for them, as tests/test_ops_gpu.py does for the unmodulated kernel.
FUSED_CASES = [(4, 64, 128, 64), (2, 128, 256, 64), (2, 512, 512, 32)]
DEFAULT_CASES = [(64, 64, 128, 64, True, None),       # 512 workgroups: dispatched as shipped
                 (4, 64, 128, 64, False, None)]       # 32 workgroups: the shipped threshold keeps the chain
CHAIN_CASES = [(2, 24, 32, 17),          # Cin % 16 != 0, odd size
               (2, 64, 64, 33),          # odd size: the blurred size is 34 != 2 OH + 1, the side output would be incomplete
               (3, 32, 48, 16)]          # 8 x 8 output pixels: below the kernel's 8 x 16 patch
RANDOM_CASES = [c + (True, 0) for c in FUSED_CASES] + [c + (False, 0) for c in CHAIN_CASES] + DEFAULT_CASES


def _min_blocks(monkeypatch, n):
    from ideas_amd.op import conv as convmod
    if n is None:
        assert convmod.BLUR_CONV_MOD_MIN_BLOCKS == convmod.BLUR_CONV_MIN_BLOCKS == 512
    else:
        monkeypatch.setattr(convmod, "BLUR_CONV_MOD_MIN_BLOCKS", n)


def dev(t, cl=False):
    t = t.detach().cuda()
    if cl and t.dim() == 4:
        t = t.contiguous(memory_format=CL)
    return t


@pytest.fixture(scope="module")
def gold():
    return Golden("modconv_down.npz")


class _Count:
    """Counts the calls of the fused launcher (op.conv.blur_conv_s2_raw, looked up through the module at call time by
    op.modulated_conv): a silent fall-back to the chain cannot pass for the fused kernel, nor the other way round."""

    def __init__(self, monkeypatch):
        from ideas_amd.op import conv as convmod
        self.n, self.mod = 0, 0
        orig = convmod.blur_conv_s2_raw

        def counted(*a, **k):
            self.n += 1
            self.mod += int(k.get("lin") is not None)
            return orig(*a, **k)
        monkeypatch.setattr(convmod, "blur_conv_s2_raw", counted)


def _b3():
    from ideas_amd import _lib
    from ideas_amd.op import conv as convmod
    return convmod.MATH == _lib.F32_B3


# ------------------------------------------------------------------------------------------------- golden
def test_golden(gold, monkeypatch):
    from ideas_amd.model import ModulatedConv2d
    meta = gold.json("meta")
    cnt = _Count(monkeypatch)
    for c in meta["cases"]:
        t = f"down{c['i']}"
        mod = ModulatedConv2d(c["cin"], c["cout"], c["k"], meta["style_dim"], demodulate=c["demodulate"], downsample=True).cuda()
        mod.load_state_dict({"weight": gold.t(f"{t}.w"), "blur.kernel": gold.t(f"{t}.fir"), "modulation.weight": gold.t(f"{t}.mw"),
                             "modulation.bias": gold.t(f"{t}.mb")}, strict=True)
        x = dev(gold.t(f"{t}.x"), True).requires_grad_(True)
        st = dev(gold.t(f"{t}.style")).requires_grad_(True)
        y = mod(x, st)
        assert tuple(y.shape) == tuple(gold.t(f"{t}.y").shape)
        e = rel_err(y, gold.t(f"{t}.y"))
        print(t, "y", e)
        assert e < TOL, (c, e)
        grads = torch.autograd.grad(y, (x, st, mod.weight, mod.modulation.weight, mod.modulation.bias), dev(gold.t(f"{t}.gy"), True))
        for got, n in zip(grads, ("gx", "gstyle", "gw", "gmw", "gmb")):
            e = rel_err(got, gold.t(f"{t}.{n}"))
            print(t, n, e)
            assert e < GTOL, (c, n, e)
    assert cnt.n == 0          # (fixture sizes: all below the fused kernel's 8 x 16 output patch)


# ------------------------------------------------------------------------------------------------- random shapes vs f64
def _layer_and_ref(case, style_dim=64, demodulate=True):
    from ideas_amd.model import ModulatedConv2d
    B, ci, co, H = case[:4]
    torch.manual_seed(sum(case[:4]))
    mod = ModulatedConv2d(ci, co, 3, style_dim, demodulate=demodulate, downsample=True)
    x = torch.randn(B, ci, H, H, dtype=torch.float64).requires_grad_(True)
    st = torch.randn(B, style_dim, dtype=torch.float64).requires_grad_(True)
    P = [p.detach().double().requires_grad_(True) for p in (mod.weight, mod.modulation.weight, mod.modulation.bias)]
    return mod, x, st, P


@pytest.mark.parametrize("case", RANDOM_CASES)
def test_random_vs_f64(case, monkeypatch):
    B, ci, co, H, fused, min_blocks = case
    _min_blocks(monkeypatch, min_blocks)
    mod, x, st, P = _layer_and_ref(case)
    y = R.modconv_down(x, st, *P, mod.blur.kernel.double())
    gy = torch.randn_like(y)
    ref = torch.autograd.grad(y, [x, st] + P, gy)
    mod = mod.cuda()
    xd, sd = dev(x.float(), True).requires_grad_(True), dev(st.float()).requires_grad_(True)
    cnt = _Count(monkeypatch)
    yd = mod(xd, sd)
    assert (cnt.n, cnt.mod) == ((1, 1) if (fused and _b3()) else (0, 0)), ("path", case, cnt.n, cnt.mod)
    e = rel_err(yd, y)
    print(case, "y", e)
    assert e < TOL, (case, e)
    got = torch.autograd.grad(yd, (xd, sd, mod.weight, mod.modulation.weight, mod.modulation.bias), dev(gy.float(), True))
    for a, b, n in zip(got, ref, ("gx", "gstyle", "gw", "gmw", "gmb")):
        e = rel_err(a, b)
        print(case, n, e)
        assert e < GTOL, (n, case, e)


def test_kernel_1x1_and_no_demodulation_vs_f64(monkeypatch):
    """The branches the fused kernel does not take at any size: a 1x1 kernel (decimating FIR + unstrided 1x1 conv) and
    demodulate=False (no out_scale: the fused launch with in_scale alone)."""
    from ideas_amd.model import ModulatedConv2d
    _min_blocks(monkeypatch, 0)
    for ci, co, k, H, demod, fused in ((64, 96, 1, 32, True, False), (64, 128, 3, 64, False, True), (32, 20, 1, 15, False, False)):
        torch.manual_seed(ci + co + k + H)
        mod = ModulatedConv2d(ci, co, k, 32, demodulate=demod, downsample=True)
        x = torch.randn(2, ci, H, H, dtype=torch.float64).requires_grad_(True)
        st = torch.randn(2, 32, dtype=torch.float64).requires_grad_(True)
        P = [p.detach().double().requires_grad_(True) for p in (mod.weight, mod.modulation.weight, mod.modulation.bias)]
        y = R.modconv_down(x, st, *P, mod.blur.kernel.double(), demodulate=demod)
        gy = torch.randn_like(y)
        ref = torch.autograd.grad(y, [x, st] + P, gy)
        mod = mod.cuda()
        xd, sd = dev(x.float(), True).requires_grad_(True), dev(st.float()).requires_grad_(True)
        with monkeypatch.context() as mp:
            cnt = _Count(mp)
            yd = mod(xd, sd)
        assert cnt.n == int(fused and _b3()), (ci, co, k, H, cnt.n)
        assert rel_err(yd, y) < TOL, (ci, co, k, H, rel_err(yd, y))
        got = torch.autograd.grad(yd, (xd, sd, mod.weight, mod.modulation.weight, mod.modulation.bias), dev(gy.float(), True))
        for a, b, n in zip(got, ref, ("gx", "gstyle", "gw", "gmw", "gmb")):
            assert rel_err(a, b) < GTOL, (n, ci, co, k, H, rel_err(a, b))


# ------------------------------------------------------------------------------------------------- fused launch vs the chain
def _raw_inputs(case):
    from ideas_amd.model import make_kernel
    B, ci, co, H = case
    torch.manual_seed(sum(case))
    x = torch.randn(B, ci, H, H, dtype=torch.float64) * (torch.rand(B, ci, 1, 1, dtype=torch.float64) * 3 + 0.1)
    w = torch.randn(co, ci, 3, 3, dtype=torch.float64)
    s = torch.rand(B, ci, dtype=torch.float64) + 0.5
    d = torch.rand(B, co, dtype=torch.float64) + 0.5
    return x, w, s, d, make_kernel(FIR)


# (case, the chain's conv kernel)
CHAIN_EQ_CASES = [((4, 64, 128, 64), "conv_b3_kernel"), ((2, 128, 256, 64), "s2img")]


@pytest.mark.parametrize("case,chain_kernel", CHAIN_EQ_CASES)
def test_fused_equals_chain(case, chain_kernel, monkeypatch):
    """The fused launch against upfirdn2d -> conv_fwd_raw(stride 2, lin=s, lout=d) on the same device.  The side output is BITWISE
    the stand-alone blur (and unscaled).  y: the staged operand is bitwise the chain's (s * blur(x), one rounding), and both of the
    chain's conv kernels -- the generic conv_b3_kernel (Cout <= 128) and the same LDS-image kernel without the FIR (Cout > 128 and
    enough blocks; forced here for a small shape with IDEAS_S2IMG_MIN_BLOCKS=1) -- turn out to add the products in the fused
    kernel's order: on an MI355X this test's own figures (printed below, `-s`) were fused vs chain 0.0 in both cases, and both
    7.4e-7 resp. 1.1e-6 from f64 -- so equality is what is asserted."""
    if not _b3():
        pytest.skip("IDEAS_MATH=f32: the fused kernel is never dispatched, there is nothing to compare")
    from ideas_amd.op import conv as convmod
    from ideas_amd.op.conv_plan import ConvGeom
    from ideas_amd.op.upfirdn2d import upfirdn2d_raw
    B, ci, co, H = case
    x, w, s, d, fir = _raw_inputs(case)
    gain = 1 / math.sqrt(9 * ci)
    y64 = F.conv2d(R.blur(x, fir.double(), (2, 2)) * s[:, :, None, None], w, stride=2) * gain * d[:, :, None, None]
    xd, wd, sd, dd, fd = dev(x.float(), True), dev(w.float(), True), dev(s.float()), dev(d.float()), fir.cuda()
    monkeypatch.setenv("IDEAS_S2IMG_MIN_BLOCKS", "1" if chain_kernel == "s2img" else "0")
    assert convmod.blur_conv_s2_ok(xd, wd, fd, (2, 2), want_xb=True)
    yf, xbf = convmod.blur_conv_s2_raw(xd, wd, fd, (2, 2), gain, want_xb=True, lin=sd, lout=dd)
    xbc = upfirdn2d_raw(xd, fd, (1, 1), (1, 1), (2, 2, 2, 2), (H + 1, H + 1), flip=True)
    yc = convmod.conv_fwd_raw(xbc, wd, ConvGeom(3, 3, 2, 0, False), gain, lin=sd, lout=dd)
    assert torch.equal(xbf, xbc), float((xbf - xbc).abs().max())
    yf0, _ = convmod.blur_conv_s2_raw(xd, wd, fd, (2, 2), gain, lin=sd, lout=dd)          # without the side output: the same y
    assert torch.equal(yf0, yf)
    ef, ec, same = rel_err(yf, y64), rel_err(yc, y64), bool(torch.equal(yf, yc))
    print(case, chain_kernel, "fused vs f64", ef, "chain vs f64", ec, "bitwise", same, "fused vs chain", rel_err(yf, yc))
    assert ef < TOL and ec < TOL
    assert same, (case, rel_err(yf, yc))


def test_null_scales_are_the_unmodulated_kernel():
    """ideas_b3_blur_conv_s2_mod with both scales NULL == ideas_b3_blur_conv_s2, through the C ABI, y and side output."""
    import ctypes as C
    from ideas_amd import _lib
    from ideas_amd.op import conv as convmod
    if not _b3():
        pytest.skip("IDEAS_MATH=f32: the fused kernel is never dispatched, there is nothing to compare")
    case = (2, 64, 128, 64)
    B, ci, co, H = case
    x, w, _, _, fir = _raw_inputs(case)
    xd, wd, fd = dev(x.float(), True), dev(w.float(), True), fir.cuda()
    bias = torch.randn(co, device="cuda") * 0.3
    L = convmod._blur_conv_plan(tuple(xd.shape), wd, fd, (2, 2))[0]
    p = convmod._params(L, 0.05, False, True, 0.2, math.sqrt(2), 1.0)
    kh, kv = convmod.fir_factors(fd)
    planes = convmod.b3_planes(L)
    outs = []
    for modulated in (False, True):
        y = torch.empty((B, co, L.OH, L.OW), device="cuda", memory_format=CL)
        xb = torch.empty((B, ci, H + 1, H + 1), device="cuda", memory_format=CL)
        if modulated:
            rc = _lib.load().ideas_b3_blur_conv_s2_mod(_lib.ptr(y), _lib.ptr(xb), _lib.ptr(xd), _lib.ptr(planes), kh, kv, None, None,
                                                       _lib.ptr(bias), None, C.byref(p), H, H, 2, _lib.stream_ptr())
        else:
            rc = _lib.load().ideas_b3_blur_conv_s2(_lib.ptr(y), _lib.ptr(xb), _lib.ptr(xd), _lib.ptr(planes), kh, kv, _lib.ptr(bias), None,
                                                   C.byref(p), H, H, 2, _lib.stream_ptr())
        _lib.check(rc, "ideas_b3_blur_conv_s2[_mod]")
        outs.append((y, xb))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # ... and all-ones scales multiply by exactly 1: the modulated instantiation gives the same bits
    one_i, one_o = torch.ones(B, ci, device="cuda"), torch.ones(B, co, device="cuda")
    y1, xb1 = convmod.blur_conv_s2_raw(xd, wd, fd, (2, 2), 0.05, bias=bias, act=True, act_gain=math.sqrt(2), want_xb=True, lin=one_i, lout=one_o)
    assert torch.equal(y1, outs[0][0]) and torch.equal(xb1, outs[0][1])


# ------------------------------------------------------------------------------------------------- fused activation
@pytest.mark.parametrize("case", [(4, 64, 128, 64, True), (2, 64, 64, 33, False), (2, 32, 40, 20, False)])
def test_fused_activation_equals_unfused(case, monkeypatch):
    import ideas_amd.op as op
    B, ci, co, H, fused = case
    _min_blocks(monkeypatch, 0)
    mod, x, st, P = _layer_and_ref(case)
    mod = mod.cuda()
    torch.manual_seed(1 + sum(case[:4]))
    b = (torch.randn(co, device="cuda") * 0.3).requires_grad_(True)
    s0 = mod.modulation(dev(st.float())).detach()
    outs = []
    cnt = _Count(monkeypatch)
    for fuse in (True, False):
        xd, sd = dev(x.float(), True).requires_grad_(True), s0.clone().requires_grad_(True)
        kw = dict(demodulate=True, downsample=True, fir=mod.blur.kernel)
        if fuse:
            y = op.modulated_conv2d(xd, mod.weight, sd, act_bias=b, **kw)
        else:
            y = op.fused_leaky_relu(op.modulated_conv2d(xd, mod.weight, sd, **kw), b)
        if not outs:
            torch.manual_seed(2)
            gy = torch.randn_like(y)
        outs.append((y, torch.autograd.grad(y, (xd, sd, mod.weight, b), gy)))
    assert cnt.n == (2 if (fused and _b3()) else 0)
    assert torch.equal(outs[0][0], outs[1][0]), float((outs[0][0] - outs[1][0]).abs().max())
    for a, r, n in zip(outs[0][1], outs[1][1], ("gx", "gs", "gw", "gb")):
        assert rel_err(a, r) < GTOL, (n, case, rel_err(a, r))
    # ... and the fused form against f64
    sr = R.styles(st, P[1], P[2])
    y64 = F.leaky_relu(R.modconv_down_s(x, sr, P[0][0], mod.blur.kernel.double().cpu()) + b.detach().double().cpu().view(1, -1, 1, 1), 0.2) * 2 ** 0.5
    assert rel_err(outs[0][0], y64) < TOL, rel_err(outs[0][0], y64)


# ------------------------------------------------------------------------------------------------- frozen inputs
@pytest.mark.parametrize("case", [(4, 64, 128, 64), (2, 24, 32, 17)])
def test_frozen_weight_and_frozen_input(case, monkeypatch):
    B, ci, co, H = case
    _min_blocks(monkeypatch, 0)
    mod, x, st, P = _layer_and_ref(case)
    mod = mod.cuda()
    sd = dev(st.float()).requires_grad_(True)

    def blurred_saved(y):
        """Saved tensors of the conv node of the blurred tensor's shape [B, Cin, H + 1, H + 1]."""
        fn = y.grad_fn
        assert type(fn).__name__ == "_ModConvBackward", type(fn).__name__
        return [t for t in fn.saved_tensors if t.dim() == 4 and tuple(t.shape) == (B, ci, H + 1, H + 1)]

    # everything trainable: the blurred tensor is kept for the weight gradient
    xd = dev(x.float(), True).requires_grad_(True)
    y = mod(xd, sd)
    assert len(blurred_saved(y)) == 1
    full = torch.autograd.grad(y.sum(), (xd, sd, mod.weight))
    # frozen weight: no blurred tensor anywhere, the other gradients unchanged
    mod.weight.requires_grad_(False)
    y = mod(xd, sd)
    assert blurred_saved(y) == []
    gx, gs = torch.autograd.grad(y.sum(), (xd, sd))
    assert rel_err(gx, full[0]) < GTOL and rel_err(gs, full[1]) < GTOL
    with pytest.raises(RuntimeError):
        torch.autograd.grad(mod(xd, sd).sum(), mod.weight)
    # frozen input and style: only the weight gradient
    mod.weight.requires_grad_(True)
    for p in mod.modulation.parameters():
        p.requires_grad_(False)
    y = mod(dev(x.float(), True), dev(st.float()))
    (gw,) = torch.autograd.grad(y.sum(), mod.weight)
    assert rel_err(gw, full[2]) < GTOL
    # nothing trainable: no graph at all
    mod.weight.requires_grad_(False)
    assert mod(dev(x.float(), True), dev(st.float())).grad_fn is None


# ------------------------------------------------------------------------------------------------- second order
@pytest.mark.parametrize("case", [(2, 32, 48, 16, 3), (2, 64, 128, 64, 3), (2, 16, 24, 12, 1)])
def test_second_order_through_the_composite(case):
    """second_order(): autograd.grad(create_graph=True) w.r.t. style and input, then a second backward, against the f64
    restatement's double backward.  Bounds of tests/test_nets_gpu.py::test_path_length_regulariser_second_order_through_modconv:
    TOL for the output, 1e-4 for the first-order quantities, 2e-3 for the gradients of the penalty."""
    from ideas_amd.model import ModulatedConv2d
    from ideas_amd.op.modulated_conv import second_order
    B, ci, co, H, k = case
    torch.manual_seed(sum(case))
    mod = ModulatedConv2d(ci, co, k, 32, downsample=True)
    x = torch.randn(B, ci, H, H, dtype=torch.float64).requires_grad_(True)
    st = torch.randn(B, 32, dtype=torch.float64).requires_grad_(True)
    P = [p.detach().double().requires_grad_(True) for p in (mod.weight, mod.modulation.weight, mod.modulation.bias)]

    def penalty(y, x_, st_, params, noise):
        g_st, g_x = torch.autograd.grad((y * noise).sum(), (st_, x_), create_graph=True)
        pen = g_st.pow(2).sum(1).sqrt().mean() + g_x.pow(2).mean()
        return g_st, g_x, pen, torch.autograd.grad(pen, [x_, st_] + list(params))
    y = R.modconv_down(x, st, *P, mod.blur.kernel.double())
    noise = torch.randn_like(y)
    g_st, g_x, pen, ref = penalty(y, x, st, P, noise)
    mod = mod.cuda()
    xd, sd = dev(x.float(), True).requires_grad_(True), dev(st.float()).requires_grad_(True)
    with second_order():
        yd = mod(xd, sd)
        g_std, g_xd, pend, got = penalty(yd, xd, sd, [mod.weight, mod.modulation.weight, mod.modulation.bias], dev(noise.float(), True))
    assert rel_err(yd, y) < TOL
    assert rel_err(g_std, g_st) < 1e-4 and rel_err(g_xd, g_x) < 1e-4
    assert abs(float(pend) - float(pen)) <= 1e-4 * abs(float(pen)) + 1e-12
    for a, b, n in zip(got, ref, ("x", "style", "w", "mw", "mb")):
        assert rel_err(a, b) < 2e-3, (n, case, rel_err(a, b))


# ------------------------------------------------------------------------------------------------- bf16 activations
@pytest.mark.parametrize("case", [(2, 64, 128, 64), (3, 32, 96, 24), (2, 128, 160, 32)])
def test_bf16_mode_runs_the_chain(case, monkeypatch):
    """Under the bf16 precision switch the layer runs forward and backward through the chain (bf16 blur, bf16 scaled stride-2 conv):
    the bounds of tests/test_bf16_gpu.py::test_modconv_bf16_vs_f64 for the same-resolution modulated conv, against f64 on the
    bf16-rounded input."""
    import ideas_amd.op as op
    from ideas_amd import precision
    from ideas_amd.model import make_kernel
    BF = torch.bfloat16
    B, ci, co, H = case
    torch.manual_seed(sum(case))
    x = torch.randn(B, ci, H, H, dtype=torch.float64).float().to(BF).double().requires_grad_(True)
    w = torch.randn(1, co, ci, 3, 3, dtype=torch.float64).requires_grad_(True)
    st = (torch.randn(B, ci, dtype=torch.float64) * 0.3 + 1).requires_grad_(True)
    fir = make_kernel(FIR)
    y = R.modconv_down_s(x, st, w[0], fir.double())
    gy = torch.randn_like(y).float().to(BF).double()
    gx, gw, gs = torch.autograd.grad(y, (x, w, st), gy)
    xd = dev(x, True).to(BF).requires_grad_(True)
    wd, sd = dev(w.float()).requires_grad_(True), dev(st.float()).requires_grad_(True)
    cnt = _Count(monkeypatch)
    with precision.activations(BF):
        yd = op.modulated_conv2d(xd, wd, sd, demodulate=True, downsample=True, fir=fir.cuda())
        assert yd.dtype == BF and cnt.n == 0
        assert rel_err(yd, y) < 1.5e-2, ("y", case, rel_err(yd, y))
        gxd, gwd, gsd = torch.autograd.grad(yd, (xd, wd, sd), dev(gy, True).to(BF))
    assert rel_err(gxd, gx) < 2e-2, ("gx", case, rel_err(gxd, gx))
    assert rel_err(gwd, gw) < 2e-2, ("gw", case, rel_err(gwd, gw))
    cos = F.cosine_similarity(gsd.double().cpu().flatten(), gs.flatten(), dim=0)
    assert float(cos) > 0.98, ("gs", case, float(cos))


# ------------------------------------------------------------------------------------------------- the other builds
def _rerun(env_extra, n_expected):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
                        "test_golden or test_random_vs_f64"], env=env, capture_output=True, text=True, timeout=1200,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert "%d passed" % n_expected in r.stdout, r.stdout[-500:]


def test_f32_math_runs_the_chain_everywhere():
    """IDEAS_MATH=f32 (the f32 matrix instruction): no fused launch; golden and random cases once more in a child process (the
    switch is read at import)."""
    _rerun({"IDEAS_MATH": "f32"}, 1 + len(RANDOM_CASES))


def test_dpp_builtin_build_covers_the_modulated_instantiations():
    """libideas_hip_dppb.so (-DS2FIR_DPP_BUILTIN=1: the producer's taps from the compiler's builtin instead of the inline assembly):
    golden and random cases in a child process, as tests/test_ops_gpu.py does for the unmodulated kernel."""
    from ideas_amd import _lib
    lib = os.path.join(os.path.dirname(os.path.abspath(_lib.LIB_PATH)), "libideas_hip_dppb.so")
    assert os.path.exists(lib), "make -C ideas_amd/csrc builds libideas_hip_dppb.so next to libideas_hip.so"
    _rerun({"IDEAS_HIP_LIB": lib}, 1 + len(RANDOM_CASES))
