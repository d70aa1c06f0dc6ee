"""float16 / float64 and any-size FIRs through fused_leaky_relu, upfirdn2d and the modules built only on them.

Yardstick: oracle.torch_ref in float64 on the CPU (the one full-size bias-gradient check sums its f64 reference with torch on the
device, 268M elements being too many for the CPU here)."""
import numpy as np
import pytest
import torch

import oracle.torch_ref as O

pytestmark = pytest.mark.gpu
CL = torch.channels_last
H = torch.float16
D = torch.float64
A32 = float(np.float32(0.2))              # what the f32 `alpha` / `scale` arguments of the C ABI carry
S32 = float(np.float32(2 ** 0.5))


@pytest.fixture(scope="module")
def ops():
    import ideas_amd.op as op
    return op


def dev(t, cl=False, dtype=None):
    t = t.detach().cuda()
    if dtype is not None:
        t = t.to(dtype)
    if cl and t.dim() == 4:
        t = t.contiguous(memory_format=CL)
    return t


def half_exact(t):
    """Round to half and back: inputs both sides see exactly."""
    return t.to(H).to(D)


def check_half(got, ref, what=""):
    """got: f16; ref: f64 value of the same computation.  Every element within one half ulp of ref, >= 99.9 % of them equal to
    ref rounded to half (f32 accumulation, one rounding at the store)."""
    assert got.dtype == H, (what, got.dtype)
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    _, e = torch.frexp(ref)
    ulp = torch.pow(2.0, torch.clamp(e.double() - 11, min=-24))
    err = (got - ref).abs()
    bad = err > ulp
    assert not bool(bad.any()), (what, int(bad.sum()), float((err / ulp).max()))
    exact = float((got == ref.to(H).double()).double().mean())
    assert exact >= 0.999, (what, exact)


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    d = float(b.abs().max())
    return float((a - b).abs().max()) / (d if d > 0 else 1.0)


def away_from_kink(shape, c, cl=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    b = torch.randn(c, dtype=D, generator=g) * 0.3
    v = torch.randn(*shape, dtype=D, generator=g)
    v = torch.sign(v) * (v.abs() + 0.05)
    x = v - b.view([1, -1] + [1] * (len(shape) - 2))
    return x, b


# ------------------------------------------------------------------------------------------------ float64: fused_leaky_relu
@pytest.mark.parametrize("shape,cl", [((2, 12, 9, 7), False), ((2, 12, 9, 7), True), ((3, 16, 8, 8), True), ((5, 33), False),
                                      ((2, 5, 3, 3), False), ((2, 5, 3, 3), True)])
@pytest.mark.parametrize("with_bias", [True, False])
def test_fused_leaky_relu_f64_bitwise_and_grads(ops, shape, cl, with_bias):
    torch.manual_seed(sum(shape))
    x = torch.randn(*shape, dtype=D).requires_grad_(True)
    b = (torch.randn(shape[1], dtype=D) if with_bias else None)
    bb = b.clone().requires_grad_(True) if with_bias else None
    y = O.fused_leaky_relu(x, bb, A32, S32)
    g = torch.randn_like(y)
    grads = torch.autograd.grad(y, [x] + ([bb] if with_bias else []), g)
    xd = dev(x, cl).requires_grad_(True)
    bd = dev(b).requires_grad_(True) if with_bias else None
    yd = ops.fused_leaky_relu(xd, bd, 0.2, 2 ** 0.5)
    assert yd.dtype == D and torch.equal(yd.cpu(), y.detach()), float((yd.cpu() - y).abs().max())
    if cl and len(shape) == 4:
        assert yd.is_contiguous(memory_format=CL)
    gd = torch.autograd.grad(yd, [xd] + ([bd] if with_bias else []), dev(g, cl))
    assert rel_err(gd[0], grads[0]) <= 1e-15
    if with_bias:
        assert gd[1].dtype == D
        assert float((gd[1].cpu() - grads[1]).abs().max()) <= 1e-13 * float(g.abs().sum())


@pytest.mark.parametrize("cl", [False, True])
def test_fused_leaky_relu_f64_gradcheck(ops, cl):
    x, b = away_from_kink((2, 3, 4, 5), 3, cl, seed=1)
    xd = dev(x, cl).requires_grad_(True)
    bd = dev(b).requires_grad_(True)
    fn = lambda a, c: ops.fused_leaky_relu(a, c)          # noqa: E731
    assert torch.autograd.gradcheck(fn, (xd, bd))
    assert torch.autograd.gradgradcheck(fn, (xd, bd))


# ------------------------------------------------------------------------------------------------ float64: upfirdn2d
FIR_CASES = [  # (shape, fir taps / shape, up, down, pad)
    ((2, 3, 11, 9), (1, 3, 3, 1), 1, 1, (2, 1)),
    ((2, 3, 11, 9), (1, 3, 3, 1), 2, 1, (2, 1)),
    ((2, 3, 12, 10), (1, 3, 3, 1), 1, 2, (1, 1)),
    ((2, 3, 7, 8), (1, 3, 3, 1), 2, 2, (2, 2)),
    ((2, 3, 11, 9), (1, 3, 3, 1), 1, 1, (-1, 2)),
    ((2, 3, 11, 9), (1, 3, 3, 1), 2, 1, (0, -1)),
    ((2, 3, 11, 9), "asym4x3", 1, 1, (1, 2)),
    ((1, 4, 20, 18), "rand9x9", 1, 1, (4, 4)),
    ((1, 4, 16, 15), "rand12x12", 2, 1, (6, 5)),
    ((1, 4, 16, 40), "rand1x17", 1, 2, (8, 8)),
    ((1, 2, 40, 36), "rand32x32", 1, 1, (16, 15)),
]


def make_fir(spec, seed=0):
    g = torch.Generator().manual_seed(seed)
    if isinstance(spec, tuple):
        return O.make_kernel(spec).double()
    if spec == "asym4x3":
        return torch.randn(4, 3, dtype=D, generator=g)
    kh, kw = (int(v) for v in spec[4:].split("x"))
    return torch.randn(kh, kw, dtype=D, generator=g) / (kh * kw) ** 0.5


def oracle_upfirdn2d(x, k, up, down, pad):
    """O.upfirdn2d with an FIR of any shape (the oracle restates the op with conv2d, which takes any kh x kw)."""
    return O.upfirdn2d(x, k, up=up, down=down, pad=pad)


@pytest.mark.parametrize("case", FIR_CASES, ids=[f"{c[1]}-u{c[2]}d{c[3]}p{c[4]}" for c in FIR_CASES])
@pytest.mark.parametrize("cl", [False, True])
def test_upfirdn2d_f64_vs_oracle(ops, case, cl):
    shape, spec, up, down, pad = case
    torch.manual_seed(sum(shape))
    k = make_fir(spec)
    x = torch.randn(*shape, dtype=D).requires_grad_(True)
    y = oracle_upfirdn2d(x, k, up, down, pad)
    g = torch.randn_like(y)
    (gx,) = torch.autograd.grad(y, x, g)
    xd = dev(x, cl).requires_grad_(True)
    yd = ops.upfirdn2d(xd, dev(k), up=up, down=down, pad=pad)
    assert yd.dtype == D and yd.shape == y.shape
    assert yd.is_contiguous(memory_format=CL) if cl else yd.is_contiguous()
    assert float((yd.cpu() - y).abs().max()) <= 1e-13 * float(y.abs().max())
    (gxd,) = torch.autograd.grad(yd, xd, dev(g, cl))
    assert float((gxd.cpu() - gx).abs().max()) <= 1e-13 * float(gx.abs().max())


GC_CASES = [((1, 2, 5, 6), (1, 3, 3, 1), 1, 1, (2, 1)), ((1, 2, 5, 6), (1, 3, 3, 1), 1, 1, (1, 1)),
            ((1, 2, 5, 6), (1, 3, 3, 1), 1, 1, (2, 2)), ((1, 2, 5, 6), (1, 3, 3, 1), 1, 1, (1, 2)),
            ((1, 2, 4, 5), (1, 3, 3, 1), 2, 1, (2, 1)), ((1, 2, 6, 7), (1, 3, 3, 1), 1, 2, (1, 1)),
            ((1, 2, 7, 6), "rand9x9", 1, 1, (4, 4))]


@pytest.mark.parametrize("case", GC_CASES, ids=[f"{c[1]}-u{c[2]}d{c[3]}p{c[4]}" for c in GC_CASES])
@pytest.mark.parametrize("cl", [False, True])
def test_upfirdn2d_f64_gradcheck(ops, case, cl):
    shape, spec, up, down, pad = case
    torch.manual_seed(7)
    k = dev(make_fir(spec, seed=3))
    xd = dev(torch.randn(*shape, dtype=D), cl).requires_grad_(True)
    fn = lambda a: ops.upfirdn2d(a, k, up=up, down=down, pad=pad)          # noqa: E731
    assert torch.autograd.gradcheck(fn, (xd,))
    assert torch.autograd.gradgradcheck(fn, (xd,))


def test_modules_f64_gradcheck():
    from ideas_amd.model import Blur, FusedLeakyReLU, ScaledLeakyReLU
    blur = Blur((1, 3, 3, 1), pad=(2, 1), upsample_factor=2).cuda().double()
    assert blur.kernel.dtype == D
    xb = dev(torch.randn(1, 3, 5, 6, dtype=D), True).requires_grad_(True)
    assert torch.autograd.gradcheck(blur, (xb,)) and torch.autograd.gradgradcheck(blur, (xb,))
    act = FusedLeakyReLU(3).cuda().double()
    x, b = away_from_kink((1, 3, 4, 5), 3, seed=5)
    with torch.no_grad():
        act.bias.copy_(dev(b))
    assert act.bias.dtype == D
    xd = dev(x).requires_grad_(True)
    assert torch.autograd.gradcheck(act, (xd,)) and torch.autograd.gradgradcheck(act, (xd,))
    (gb,) = torch.autograd.grad(act(xd).sum(), act.bias)
    assert gb.dtype == D
    sl = ScaledLeakyReLU(0.2)
    xs = dev(torch.sign(torch.randn(2, 3, 4, 4, dtype=D)) * (torch.rand(2, 3, 4, 4, dtype=D) + 0.05)).requires_grad_(True)
    assert torch.autograd.gradcheck(sl, (xs,)) and torch.autograd.gradgradcheck(sl, (xs,))


# ------------------------------------------------------------------------------------------------ float16
@pytest.mark.parametrize("shape,cl", [((2, 16, 9, 7), True), ((2, 12, 9, 7), True), ((2, 16, 9, 8), False), ((2, 5, 9, 7), False),
                                      ((3, 40), False), ((4, 3, 17, 5), True)])
def test_fused_leaky_relu_f16(ops, shape, cl):
    torch.manual_seed(sum(shape))
    x = half_exact(torch.randn(*shape, dtype=D) * 4)
    b = half_exact(torch.randn(shape[1], dtype=D))
    g = half_exact(torch.randn(*shape, dtype=D))
    bf = b.float().double()                                   # the kernel adds an f32 bias
    y = O.fused_leaky_relu(x, bf, A32, S32)
    xd = dev(x, cl, H).requires_grad_(True)
    bd = dev(b, dtype=H).requires_grad_(True)
    yd = ops.fused_leaky_relu(xd, bd, 0.2, 2 ** 0.5)
    check_half(yd, y, "y")
    if cl and len(shape) == 4:
        assert yd.is_contiguous(memory_format=CL)
    gxd, gbd = torch.autograd.grad(yd, [xd, bd], dev(g, cl, H))
    out_h = yd.detach().cpu().double()                      # the backward's mask is the sign of the stored half output
    gx = torch.where(out_h > 0, g, g * A32) * S32
    check_half(gxd, gx, "gx")
    assert gbd.dtype == H
    gb = gx.sum(dim=[0] + list(range(2, len(shape))))
    assert float((gbd.cpu().double() - gb).abs().max()) <= 1e-5 * float(g.abs().sum()) + float(gb.abs().max()) * 2 ** -11


F16_FIR_CASES = [  # (shape, spec, up, down, pad, cl)
    ((2, 16, 33, 31), (1, 3, 3, 1), 1, 1, (2, 1), True),     # 4x4 unit, C % 8 == 0: blur4 8-channel kernel
    ((2, 64, 17, 17), (1, 3, 3, 1), 1, 1, (1, 1), True),
    ((2, 16, 32, 30), (1, 3, 3, 1), 1, 2, (1, 1), True),     # down-2
    ((2, 24, 33, 31), (1, 3, 3, 1), 1, 2, (2, 2), True),
    ((2, 16, 17, 15), (1, 3, 3, 1), 2, 1, (2, 2), True),     # up-2
    ((2, 8, 5, 7), (1, 3, 3, 1), 2, 1, (3, 2), True),
    ((2, 12, 17, 15), (1, 3, 3, 1), 1, 1, (2, 1), True),     # C % 8 != 0: generic
    ((2, 12, 17, 15), (1, 3, 3, 1), 2, 1, (2, 1), True),
    ((2, 5, 33, 70), (1, 3, 3, 1), 1, 1, (2, 1), False),     # NCHW: the LDS tile kernel
    ((2, 5, 17, 15), (1, 3, 3, 1), 2, 1, (2, 1), False),
    ((1, 8, 20, 19), "rand12x12", 1, 1, (6, 5), True),       # large FIR
    ((1, 8, 20, 19), "rand12x12", 1, 1, (6, 5), False),
]


@pytest.mark.parametrize("case", F16_FIR_CASES, ids=[f"C{c[0][1]}-{c[1]}-u{c[2]}d{c[3]}-cl{int(c[5])}" for c in F16_FIR_CASES])
def test_upfirdn2d_f16(ops, case):
    shape, spec, up, down, pad, cl = case
    torch.manual_seed(sum(shape))
    k = make_fir(spec).float().double()                       # the kernel's FIR is f32
    x = half_exact(torch.randn(*shape, dtype=D))
    y = oracle_upfirdn2d(x, k, up, down, pad)
    g = half_exact(torch.randn_like(y))
    xr = x.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(oracle_upfirdn2d(xr, k, up, down, pad), xr, g)
    xd = dev(x, cl, H).requires_grad_(True)
    yd = ops.upfirdn2d(xd, dev(k.float()), up=up, down=down, pad=pad)
    assert yd.is_contiguous(memory_format=CL) if cl else yd.is_contiguous()
    check_half(yd, y, "y")
    (gxd,) = torch.autograd.grad(yd, xd, dev(g, cl, H))
    check_half(gxd, gx, "gx")


def test_fused_leaky_relu_f16_full_size_bias_grad(ops):
    torch.manual_seed(0)
    shape = (32, 128, 256, 256)
    xd = torch.randn(shape, device="cuda", dtype=H).contiguous(memory_format=CL).requires_grad_(True)
    bd = (torch.randn(128, device="cuda") * 0.1).to(H).requires_grad_(True)
    yd = ops.fused_leaky_relu(xd, bd)
    g = torch.randn(shape, device="cuda", dtype=H).contiguous(memory_format=CL)
    gxd, gbd = torch.autograd.grad(yd, [xd, bd], g)
    assert gbd.dtype == H and gxd.is_contiguous(memory_format=CL)
    with torch.no_grad():
        g64 = g.double()
        gx = torch.where(yd.double() > 0, g64, g64 * A32) * S32
        gb = gx.sum(dim=(0, 2, 3))
        tol = 1e-5 * float(g64.abs().sum(dim=(0, 2, 3)).max())
        del gx, g64
    err = (gbd.double() - gb).abs() - gb.abs() * 2 ** -11          # (the f32 sum is rounded to half once at the end)
    assert float(err.max()) <= tol, (float(err.max()), tol)


def test_modules_f16(ops):
    from ideas_amd.model import Blur, FusedLeakyReLU, ScaledLeakyReLU
    for cl in (False, True):
        blur = Blur((1, 3, 3, 1), pad=(2, 1)).cuda().half()
        act = FusedLeakyReLU(16).cuda().half()
        x = dev(torch.randn(2, 16, 12, 12), cl, H).requires_grad_(True)
        y = act(blur(x))
        assert y.dtype == H and (y.is_contiguous(memory_format=CL) if cl else y.is_contiguous())
        gx, gb = torch.autograd.grad(y.square().sum(), [x, act.bias], create_graph=True)
        assert gx.dtype == H and gb.dtype == H
        (ggx,) = torch.autograd.grad(gx.float().sum() + gb.float().sum(), x)
        assert ggx.dtype == H and bool(torch.isfinite(ggx).all())
        y2 = ScaledLeakyReLU()(x)
        assert y2.dtype == H
        (g2,) = torch.autograd.grad(y2.sum(), x)
        assert g2.dtype == H


# ------------------------------------------------------------------------------------------------ large FIR in f32 / bf16
@pytest.mark.parametrize("spec,pad", [("rand9x9", (4, 4)), ("rand16x16", (8, 7))])
@pytest.mark.parametrize("cl", [False, True])
def test_upfirdn2d_large_fir_f32(ops, spec, pad, cl):
    torch.manual_seed(11)
    k = make_fir(spec).float().double()
    x = torch.randn(2, 8, 21, 19, dtype=D).float().double()
    y = oracle_upfirdn2d(x, k, 1, 1, pad)
    yd = ops.upfirdn2d(dev(x, cl, torch.float32), dev(k.float()), pad=pad)
    assert rel_err(yd, y) < 1e-5
    y2 = oracle_upfirdn2d(x, k, 2, 1, pad)
    yd2 = ops.upfirdn2d(dev(x, cl, torch.float32), dev(k.float()), up=2, pad=pad)
    assert rel_err(yd2, y2) < 1e-5


@pytest.mark.parametrize("spec,pad", [("rand9x9", (4, 4)), ("rand16x16", (8, 7))])
def test_upfirdn2d_large_fir_bf16(ops, spec, pad):
    torch.manual_seed(12)
    k = make_fir(spec).float().double()
    x = torch.randn(2, 16, 21, 19, dtype=D).float().to(torch.bfloat16).double()
    y = oracle_upfirdn2d(x, k, 1, 1, pad)
    yd = ops.upfirdn2d(dev(x, True, torch.bfloat16), dev(k.float()), pad=pad)
    assert yd.dtype == torch.bfloat16
    got = yd.double().cpu()
    bound = y.abs() * 2.0 ** -8 + 1e-3 * float(y.abs().max()) + 1e-30
    assert not bool(((got - y).abs() > bound).any()), float((got - y).abs().max())


# ------------------------------------------------------------------------------------------------ guard
def test_convolutions_keep_their_dtypes(ops):
    """The conv family is out of scope: op.conv2d keeps casting its input to the activation dtype (f32 here) as before, and its
    kernel boundary still refuses half."""
    from ideas_amd.op import conv
    x = torch.randn(1, 8, 8, 8, device="cuda", dtype=H)
    y = ops.conv2d(x, torch.randn(8, 8, 3, 3, device="cuda"), padding=1)
    assert y.dtype == torch.float32
    with pytest.raises(RuntimeError, match="only float32 and bfloat16"):
        conv._nhwc(x)
