"""op.affine_warp / op.color_affine (csrc/augment.hip) and ideas_amd.non_leaking on the device, against exact answers, float64
F.grid_sample on the CPU and the reference's own runs stored in tests/golden/non_leaking.npz."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import Golden, rel_err
from test_bf16_gpu import close_bf16

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last
BF = torch.bfloat16
TOL, GTOL = 1e-5, 1e-4            # forward / gradient, of the largest element


@pytest.fixture(scope="module")
def gold():
    return Golden("non_leaking.npz")


@pytest.fixture(scope="module")
def op():
    import ideas_amd.op as op
    return op


@pytest.fixture(scope="module")
def NL():
    import ideas_amd.non_leaking as NL
    return NL


def fmt(t, layout):
    return t.contiguous(memory_format=CL) if layout == "nhwc" else t.contiguous()


def keeps_format(y, layout):
    return y.is_contiguous(memory_format=CL) if layout == "nhwc" else y.is_contiguous()


def thetas(rows, b=2):
    return torch.tensor(rows, dtype=torch.float32).view(1, 6).repeat(b, 1).to(DEV)


# ------------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
@pytest.mark.parametrize("c", (1, 3, 4, 8))
def test_affine_warp_exact_cases(op, c, layout):
    _exact_cases(op, c, layout, torch.float32)


@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
@pytest.mark.parametrize("c", (1, 3, 4, 8))
def test_affine_warp_exact_cases_bf16(op, c, layout):
    """NHWC: C = 4 (f32 would vectorise), 3 and 1 run the bf16 element kernel, C = 8 the 8-wide one."""
    _exact_cases(op, c, layout, BF)


def _exact_cases(op, c, layout, dtype):
    gen = torch.Generator().manual_seed(10 + c)
    x = torch.randn(2, c, 9, 7, generator=gen).to(dtype)            # H = 9, W = 7
    xd = fmt(x.to(DEV), layout)
    H, W = 9, 7

    y = op.affine_warp(xd, thetas([1, 0, 0, 0, 1, 0]), (H, W))
    assert y.dtype == dtype and keeps_format(y, layout) and torch.equal(y.cpu(), x), "identity"

    # sx = ox + 2, sy = oy - 3: y[oy, ox] = x[oy - 3, ox + 2], zeros shifted in
    y = op.affine_warp(xd, thetas([1, 0, 2, 0, 1, -3]), (H, W))
    want = torch.zeros_like(x)
    want[:, :, 3:, :W - 2] = x[:, :, :H - 3, 2:]
    assert torch.equal(y.cpu(), want), "integer translation"

    # 90 degrees: sx = oy, sy = H - 1 - ox -> y[oy, ox] = x[H - 1 - ox, oy], output 7 x 9
    y = op.affine_warp(xd, thetas([0, 1, 0, -1, 0, H - 1]), (W, H))
    assert y.shape == (2, c, W, H) and torch.equal(y.cpu(), x.flip(2).transpose(2, 3)), "90-degree rotation"

    y = op.affine_warp(xd, thetas([1, 0, W + 5, 0, 1, 0]), (H, W))
    assert torch.equal(y.cpu(), torch.zeros_like(x)), "every sample outside"

    # sx = ox - 0.5: exactly half of each neighbour, a zero past the left edge; in f32 from the operands, one rounding at the store
    y = op.affine_warp(xd, thetas([1, 0, -0.5, 0, 1, 0]), (H, W))
    left = torch.cat((torch.zeros(2, c, H, 1), x[..., :-1].float()), -1)
    assert torch.equal(y.cpu(), (0.5 * (left + x.float())).to(dtype)), "half-pixel shift"


@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
def test_affine_warp_boundary_positions_are_exact(op, layout):
    """Positions on the two limits of (-1, W) x (-1, H) and a quarter-pixel shift of small integers, along x and along y."""
    H, W = 9, 7
    gen = torch.Generator().manual_seed(20)
    x = torch.randn(2, 4, H, W, generator=gen)
    xi = torch.randint(-8, 9, (2, 4, H, W), generator=gen).float()
    warp = lambda t, row: op.affine_warp(fmt(t.to(DEV), layout), thetas(row), (H, W)).cpu()
    zeros = torch.zeros_like(x)

    want = zeros.clone()                                            # sx = ox - 1: the tap of ox = 0 at exactly -1 is outside
    want[..., 1:] = x[..., :-1]
    assert torch.equal(warp(x, [1, 0, -1, 0, 1, 0]), want), "x: tap at -1"
    want = zeros.clone()                                            # sx = ox + W - 1: only ox = 0 is inside, at exactly W - 1
    want[..., 0] = x[..., W - 1]
    assert torch.equal(warp(x, [1, 0, W - 1, 0, 1, 0]), want), "x: tap at W - 1"
    right = torch.cat((xi[..., 1:], torch.zeros(2, 4, H, 1)), -1)   # sx = ox + 0.25: 3/4 of x[ox], 1/4 of x[ox + 1] (zero past W - 1)
    want = 0.75 * xi + 0.25 * right
    assert torch.equal(want[..., W - 1], 0.75 * xi[..., W - 1])
    assert torch.equal(warp(xi, [1, 0, 0.25, 0, 1, 0]), want), "x: quarter pixel"

    want = zeros.clone()
    want[:, :, 1:] = x[:, :, :-1]
    assert torch.equal(warp(x, [1, 0, 0, 0, 1, -1]), want), "y: tap at -1"
    want = zeros.clone()
    want[:, :, 0] = x[:, :, H - 1]
    assert torch.equal(warp(x, [1, 0, 0, 0, 1, H - 1]), want), "y: tap at H - 1"
    below = torch.cat((xi[:, :, 1:], torch.zeros(2, 4, 1, W)), 2)
    want = 0.75 * xi + 0.25 * below
    assert torch.equal(want[:, :, H - 1], 0.75 * xi[:, :, H - 1])
    assert torch.equal(warp(xi, [1, 0, 0, 0, 1, 0.25]), want), "y: quarter pixel"


# ------------------------------------------------------------------------------------------------- general thetas
def general_theta(b, gen, hw, out_hw):
    """Rotation, anisotropic scale and a fractional shift about the centres; the corners of the output fall outside the input."""
    rows = []
    for i in range(b):
        ang = float(torch.rand(1, generator=gen)) * 2 * math.pi
        s_x, s_y = 0.8 + 0.7 * float(torch.rand(1, generator=gen)), 0.9 + 0.8 * float(torch.rand(1, generator=gen))
        s_x, s_y = s_x * hw[1] / out_hw[1], s_y * hw[0] / out_hw[0]
        d_x, d_y = (torch.rand(2, generator=gen) * 3 - 1.5).tolist()
        a, b_, c, d = math.cos(ang) * s_x, -math.sin(ang) * s_y, math.sin(ang) * s_x, math.cos(ang) * s_y
        cx, cy, ocx, ocy = (hw[1] - 1) / 2, (hw[0] - 1) / 2, (out_hw[1] - 1) / 2, (out_hw[0] - 1) / 2
        rows.append([a, b_, cx + d_x - a * ocx - b_ * ocy, c, d, cy + d_y - c * ocx - d * ocy])
    return torch.tensor(rows, dtype=torch.float32)


def grid_sample_f64(x, theta, out_hw):
    """float64 F.grid_sample on the CPU from the same f32 theta."""
    from ideas_amd.op.augment import affine_warp_composition
    return affine_warp_composition(x.double(), theta.double(), out_hw)


GENERAL = (((2, 3, 16, 16), (21, 19)), ((1, 8, 33, 5), (9, 40)))
_general_cache = {}


def general_case(i):
    """(x, theta, cot, reference output, reference input gradient), computed once per shape."""
    if i not in _general_cache:
        shape, out_hw = GENERAL[i]
        gen = torch.Generator().manual_seed(40 + i)
        x = torch.randn(*shape, generator=gen)
        theta = general_theta(shape[0], gen, shape[2:], out_hw)
        cot = torch.randn(shape[0], shape[1], *out_hw, generator=gen)
        x64 = x.double().requires_grad_(True)
        y64 = grid_sample_f64(x64, theta, out_hw)
        (g64,) = torch.autograd.grad((y64 * cot.double()).sum(), x64)
        outside = float((y64.detach() == 0).double().mean())
        assert 0.02 < outside < 0.9, outside                 # some samples fall outside, most do not
        _general_cache[i] = (x, theta, cot, y64.detach(), g64)
    return _general_cache[i]


@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
@pytest.mark.parametrize("case", range(len(GENERAL)))
def test_affine_warp_general_f32(op, case, layout):
    x, theta, cot, y64, g64 = general_case(case)
    out_hw = GENERAL[case][1]
    xd = fmt(x.to(DEV), layout).requires_grad_(True)
    y = op.affine_warp(xd, theta.to(DEV), out_hw)
    assert keeps_format(y, layout)
    (gx,) = torch.autograd.grad((y * cot.to(DEV)).sum(), xd)
    ey, eg = rel_err(y, y64), rel_err(gx, g64)
    print(f"affine_warp f32 {layout} {tuple(x.shape)} -> {out_hw}: y {ey:.2e}  gx {eg:.2e}")
    assert ey <= TOL and eg <= GTOL
    # adjoint identity on the device's own numbers: <warp(x), g> == <x, warp_bwd(g)>
    lhs = float((y.detach().double() * cot.to(DEV).double()).sum())
    rhs = float((xd.detach().double() * gx.double()).sum())
    scale = float((y.detach().double() * cot.to(DEV).double()).abs().sum())
    print(f"  adjoint: |{lhs:.6f} - {rhs:.6f}| = {abs(lhs - rhs):.2e}  vs 1e-5 * {scale:.3f}")
    assert abs(lhs - rhs) <= 1e-5 * scale


@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
@pytest.mark.parametrize("case", range(len(GENERAL)))
def test_affine_warp_general_bf16(op, case, layout):
    x, theta, cot, _, _ = general_case(case)
    out_hw = GENERAL[case][1]
    xb, cb = x.bfloat16(), cot.bfloat16()
    x64 = xb.double().requires_grad_(True)                   # the reference on the rounded operands
    y64 = grid_sample_f64(x64, theta, out_hw)
    (g64,) = torch.autograd.grad((y64 * cb.double()).sum(), x64)
    xd = fmt(xb.to(DEV), layout).requires_grad_(True)
    y = op.affine_warp(xd, theta.to(DEV), out_hw)
    assert y.dtype == torch.bfloat16 and keeps_format(y, layout)
    (gx,) = torch.autograd.grad(y, xd, fmt(cb.to(DEV), layout))
    assert gx.dtype == torch.bfloat16
    close_bf16(y, y64, "y")
    close_bf16(gx, g64, "gx")


# ------------------------------------------------------------------------------------------------- hostile thetas
HOSTILE = {"nan coefficient": [1, float("nan"), 0, 0, 1, 0], "inf offset": [1, 0, float("inf"), 0, 1, 0],
           "1e30 scale": [1e30, 0, 1e30, 0, 1e30, 1e30], "-1e30 offset": [1, 0, -1e30, 0, 1, 0]}


@pytest.mark.parametrize("dtype", (torch.float32, BF), ids=("f32", "bf16"))
@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
@pytest.mark.parametrize("c", (4, 8))
def test_affine_warp_hostile_theta_zeroes_its_sample_only(op, c, layout, dtype):
    """Sample 1 of three carries a theta that is not finite or whose positions overflow an int: its output and its input gradient
    are exactly zero, and the neighbours are what they are beside an ordinary sample."""
    H, W = 9, 7
    gen = torch.Generator().manual_seed(30 + c)
    x = torch.randn(3, c, H, W, generator=gen).to(dtype)
    cot = torch.randn(3, c, H, W, generator=gen).to(dtype)
    theta = general_theta(3, gen, (H, W), (H, W))
    x64 = x[[0, 2]].double().requires_grad_(True)
    y64 = grid_sample_f64(x64, theta[[0, 2]], (H, W))
    (g64,) = torch.autograd.grad((y64 * cot[[0, 2]].double()).sum(), x64)
    plain = op.affine_warp(fmt(x.to(DEV), layout), theta.to(DEV), (H, W))
    for name, row in HOSTILE.items():
        th = theta.clone()
        th[1] = torch.tensor(row)
        xd = fmt(x.to(DEV), layout).requires_grad_(True)
        y = op.affine_warp(xd, th.to(DEV), (H, W))
        (gx,) = torch.autograd.grad(y, xd, fmt(cot.to(DEV), layout))
        assert float(y[1].abs().max()) == 0.0 and not bool(torch.isnan(y[1]).any()), name
        assert torch.equal(y[[0, 2]], plain[[0, 2]]), name
        assert float(gx[1].abs().max()) == 0.0 and not bool(torch.isnan(gx[1]).any()), name
        if dtype == BF:
            close_bf16(gx[[0, 2]], g64, name + " gx")
        else:
            e = rel_err(gx[[0, 2]], g64)
            print(f"hostile theta ({name}) f32 {layout} C = {c}: gx of the neighbours {e:.2e}")
            assert e <= GTOL, name


# ------------------------------------------------------------------------------------------------- loaded atomics
def _scale_theta(b, scale, offsets):
    return torch.tensor([[scale, 0, offsets[i][0], 0, scale, offsets[i][1]] for i in range(b)], dtype=torch.float32)


# (input shape, output size, theta): 96 x 96 outputs inside an 8 x 8 image -- about 144 land on each input pixel; 16 x 16 outputs
# four pixels apart in a 64 x 64 image -- every tap is its input pixel's only contribution and three quarters get none
ATOMIC = {"minify": ((2, 4, 8, 8), (96, 96), _scale_theta(2, 6.5 / 95, ((0.25, 0.25), (0.125, 0.375)))),
          "magnify": ((2, 8, 64, 64), (16, 16), _scale_theta(2, 4.0, ((0.5, 0.25), (1.25, 2.75))))}
_atomic_cache = {}


def atomic_case(name, dtype):
    """(x, theta, cot, reference output, reference input gradient) on operands rounded to ``dtype``, computed once."""
    if (name, dtype) not in _atomic_cache:
        shape, out_hw, theta = ATOMIC[name]
        gen = torch.Generator().manual_seed(50 + len(name))
        x = torch.randn(*shape, generator=gen).to(dtype)
        cot = torch.randn(shape[0], shape[1], *out_hw, generator=gen).to(dtype)
        x64 = x.double().requires_grad_(True)
        y64 = grid_sample_f64(x64, theta, out_hw)
        (g64,) = torch.autograd.grad((y64 * cot.double()).sum(), x64)
        outside = float((y64.detach() == 0).double().mean())
        assert outside == 0 if name == "minify" else outside < 0.9, outside
        if name == "magnify":
            assert float((g64 == 0).double().mean()) > 0.7
        _atomic_cache[(name, dtype)] = (x, theta, cot, y64.detach(), g64)
    return _atomic_cache[(name, dtype)]


@pytest.mark.parametrize("dtype", (torch.float32, BF), ids=("f32", "bf16"))
@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
@pytest.mark.parametrize("name", tuple(ATOMIC))
def test_affine_warp_backward_under_atomic_load(op, name, layout, dtype):
    x, theta, cot, y64, g64 = atomic_case(name, dtype)
    out_hw = ATOMIC[name][1]
    xd = fmt(x.to(DEV), layout).requires_grad_(True)
    y = op.affine_warp(xd, theta.to(DEV), out_hw)
    assert y.dtype == dtype and keeps_format(y, layout)
    (gx,) = torch.autograd.grad(y, xd, fmt(cot.to(DEV), layout))
    if dtype == BF:
        close_bf16(y, y64, "y")
        close_bf16(gx, g64, "gx")
    else:
        ey, eg = rel_err(y, y64), rel_err(gx, g64)
        print(f"affine_warp {name} f32 {layout}: y {ey:.2e}  gx {eg:.2e}")
        assert ey <= TOL and eg <= GTOL
        lhs = float((y.detach().double() * cot.to(DEV).double()).sum())
        rhs = float((xd.detach().double() * gx.double()).sum())
        scale = float((y.detach().double() * cot.to(DEV).double()).abs().sum())
        print(f"  adjoint: |{lhs:.6f} - {rhs:.6f}| = {abs(lhs - rhs):.2e}  vs 1e-5 * {scale:.3f}")
        assert abs(lhs - rhs) <= 1e-5 * scale
    if name == "magnify":
        assert float(gx.cpu()[g64 == 0].abs().max()) == 0.0


@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
def test_affine_warp_bwd_accumulates_without_clear(op, layout):
    """ideas_affine_warp_bwd(clear = 0) adds to what gx holds; clear = 1 on the same buffer then gives the plain result, bitwise
    where an input pixel has at most one contribution (everywhere in the magnification case)."""
    from ideas_amd import _lib
    x, theta, cot, _, g64 = atomic_case("magnify", torch.float32)
    (b, c, h, w), (oh, ow) = ATOMIC["magnify"][0], ATOMIC["magnify"][1]
    xd = fmt(x.to(DEV), layout).requires_grad_(True)
    gy, th = fmt(cot.to(DEV), layout), theta.to(DEV)
    (plain,) = torch.autograd.grad(op.affine_warp(xd, th, (oh, ow)), xd, gy)
    prefill = fmt(torch.randn(b, c, h, w, generator=torch.Generator().manual_seed(51)).to(DEV), layout)
    buf = prefill.clone(memory_format=torch.preserve_format)
    assert keeps_format(buf, layout)
    call = lambda clear: _lib.load().ideas_affine_warp_bwd(_lib.ptr(buf), _lib.ptr(gy), _lib.ptr(th), b, c, h, w, oh, ow, clear,
                                                           _lib.NHWC if layout == "nhwc" else _lib.NCHW, _lib.F32, _lib.stream_ptr())
    assert call(0) == 0
    want = prefill.double() + plain.double()
    e = float((buf.double() - want).abs().max()) / float(want.abs().max())
    print(f"affine_warp_bwd clear = 0 {layout}: {e:.2e}")
    assert e <= GTOL
    assert torch.equal(buf[(g64 == 0).to(DEV)], prefill[(g64 == 0).to(DEV)])       # untouched where nothing lands
    assert call(1) == 0
    assert torch.equal(buf, plain)


def test_affine_warp_fallback_dtypes_and_second_order(op):
    """f64 / f16 tensors and a graph built inside second_order() take the grid_sample composition."""
    from ideas_amd.op.modulated_conv import second_order
    x, theta, cot, y64, g64 = general_case(0)
    out_hw = GENERAL[0][1]
    xd = x.double().to(DEV).requires_grad_(True)
    y = op.affine_warp(xd, theta.to(DEV), out_hw)
    (gx,) = torch.autograd.grad((y * cot.double().to(DEV)).sum(), xd)
    assert y.dtype == torch.float64 and rel_err(y, y64) <= 1e-12 and rel_err(gx, g64) <= 1e-12
    yh = op.affine_warp(x.half().to(DEV), theta.to(DEV), out_hw)
    assert yh.dtype == torch.float16 and rel_err(yh, y64) <= 2e-2          # an f16 grid: positions to ~1e-2 pixel
    xs = x.to(DEV).requires_grad_(True)
    with second_order():
        ys = op.affine_warp(xs, theta.to(DEV), out_hw)
        (g1,) = torch.autograd.grad((ys * cot.to(DEV)).sum(), xs, create_graph=True)
    assert rel_err(ys, y64) <= TOL and rel_err(g1, g64) <= GTOL


# ------------------------------------------------------------------------------------------------- colour
def color_ref(x, m, cot):
    x64 = x.double().requires_grad_(True)
    m64 = m.double().reshape(-1, 3, 4)
    y64 = torch.einsum("bij,bjhw->bihw", m64[:, :, :3], x64) + m64[:, :, 3].reshape(-1, 3, 1, 1)
    (g64,) = torch.autograd.grad((y64 * cot.double()).sum(), x64)
    return y64.detach(), g64


def color_cases(gold):
    gen = torch.Generator().manual_seed(60)
    yield "col", gold.t("col/x").float(), gold.t("col/C")[:, :3, :].contiguous(), gold.t("col/cot")
    yield "1x1", torch.randn(2, 3, 1, 1, generator=gen), torch.randn(2, 3, 4, generator=gen), torch.randn(2, 3, 1, 1, generator=gen)


@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
def test_color_affine_f32(op, gold, layout):
    for tag, x, m, cot in color_cases(gold):
        y64, g64 = color_ref(x, m, cot)
        xd = fmt(x.to(DEV), layout).requires_grad_(True)
        y = op.color_affine(xd, m.to(DEV))
        assert keeps_format(y, layout)
        (gx,) = torch.autograd.grad((y * cot.to(DEV)).sum(), xd)
        ey, eg = rel_err(y, y64), rel_err(gx, g64)
        print(f"color_affine f32 {layout} {tag}: y {ey:.2e}  gx {eg:.2e}")
        assert ey <= TOL and eg <= GTOL
        y12 = op.color_affine(xd.detach(), m.reshape(-1, 12).to(DEV))
        assert torch.equal(y12, y.detach())


def test_color_affine_bf16(op, gold):
    for tag, x, m, cot in color_cases(gold):
        xb, cb = x.bfloat16(), cot.bfloat16()
        y64, g64 = color_ref(xb, m, cb)
        for layout in ("nchw", "nhwc"):
            xd = fmt(xb.to(DEV), layout).requires_grad_(True)
            y = op.color_affine(xd, m.to(DEV))
            (gx,) = torch.autograd.grad(y, xd, fmt(cb.to(DEV), layout))
            assert y.dtype == gx.dtype == torch.bfloat16
            close_bf16(y, y64, f"{tag} y")
            close_bf16(gx, g64, f"{tag} gx")


def test_color_affine_fallback_f64(op, gold):
    _, x, m, cot = next(color_cases(gold))
    y64, g64 = color_ref(gold.t("col/x"), m, cot)
    xd = gold.t("col/x").to(DEV).requires_grad_(True)
    y = op.color_affine(xd, m.to(DEV))
    (gx,) = torch.autograd.grad((y * cot.double().to(DEV)).sum(), xd)
    assert y.dtype == torch.float64 and rel_err(y, y64) <= 1e-12 and rel_err(gx, g64) <= 1e-12


# ------------------------------------------------------------------------------------------------- the module against the reference
def check_against_reference(gold, tag, fn, x64):
    """fn(x) on the device in f32 (x rounded from the stored f64 input) against the reference's f64 output and input gradient.
    Bounds: max(1e-5, 4 * f32_dev) / max(1e-4, 4 * f32_dev), f32_dev = the deviation of the reference's OWN f32 run for this case
    and quantity; the factor 4 allows for our different, equally valid, order of f32 operations."""
    dev_y, dev_g = gold.t(tag + "/f32_dev").tolist()
    x = x64.float().to(DEV).requires_grad_(True)
    y = fn(x)
    ref = gold.t(tag + "/y")
    assert y.shape == ref.shape
    (gx,) = torch.autograd.grad((y * gold.t(tag + "/cot").to(DEV)).sum(), x)
    ey, eg = rel_err(y, ref), rel_err(gx, gold.t(tag + "/gx"))
    by, bg = max(1e-5, 4 * dev_y), max(1e-4, 4 * dev_g)
    print(f"{tag}: y {ey:.2e} (bound {by:.2e}, reference's f32 run {dev_y:.2e})  gx {eg:.2e} (bound {bg:.2e}, reference's f32 run {dev_g:.2e})")
    assert ey <= by and eg <= bg


@pytest.mark.parametrize("tag", ("aff16", "aff24x20", "aff32", "aff32_c5"))
def test_random_apply_affine_matches_reference(gold, NL, tag):
    G = gold.t(tag + "/G")

    def fn(x):
        y, G_out = NL.random_apply_affine(x, 1.0, G)
        assert G_out is G
        return y
    check_against_reference(gold, tag, fn, gold.t(tag + "/x"))


def test_random_apply_color_matches_reference(gold, NL):
    C = gold.t("col/C")
    check_against_reference(gold, "col", lambda x: NL.random_apply_color(x, 1.0, C)[0], gold.t("col/x"))


def test_augment_matches_reference(gold, NL):
    G, C = gold.t("aff32/G"), gold.t("aug32/C")

    def fn(x):
        y, (G_out, C_out) = NL.augment(x, 1.0, (G, C))
        assert G_out is G and C_out is C
        return y
    check_against_reference(gold, "aug32", fn, gold.t("aff32/x"))


# ------------------------------------------------------------------------------------------------- sampling paths
def test_augment_samples_its_matrices(NL):
    gen = torch.Generator().manual_seed(70)
    x = torch.randn(4, 3, 32, 32, generator=gen).to(DEV)
    # what the seed predicts: sample_affine draws until a reflect pad exists, then sample_color
    torch.manual_seed(5)
    while True:
        G = NL.sample_affine(0.6, 4, 32, 32)
        if max(NL.get_padding(torch.inverse(G), 32, 32)) + 6 < 32:
            break
    C = NL.sample_color(0.6, 4)
    torch.manual_seed(5)
    y, (G2, C2) = NL.augment(x, 0.6)
    assert y.shape == (4, 3, 32, 32) and y.device.type == "cuda" and bool(torch.isfinite(y).all())
    assert torch.equal(G2, G) and torch.equal(C2, C)


def test_augment_p0_runs_the_whole_pipeline(NL):
    gen = torch.Generator().manual_seed(71)
    x = torch.randn(2, 3, 32, 32, generator=gen).to(DEV)
    y, (G, C) = NL.augment(x, 0)
    assert y.shape == x.shape and bool(torch.isfinite(y).all())
    assert torch.equal(G, torch.eye(3).expand(2, 3, 3)) and torch.equal(C, torch.eye(4).expand(2, 4, 4))
    # (identity matrices do not give the image back: the reference's grid, linspace end points under align_corners=False, steps
    # by w2 / (w2 - 1) pixels of the 2x image, and warp_theta reproduces that grid)
