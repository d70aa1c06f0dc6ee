"""GPU parity of the StyleGAN2 generator side: ``op.noise_bias_act`` (forward and the one-pass backward) against an f64 restatement on
the same rounded operands, and ``StyledConv`` / ``ToRGB`` / ``Upsample`` / ``Downsample`` / ``Generator`` against what the reference's
classes computed (tests/golden/stylegan2_gen.npz).  Tolerances: DESIGN.md "Tolerances" (1e-5 forward, 1e-4 gradients, of the largest
element), the network bounds of tests/test_stylegan2_disc_gpu.py, the bf16 bounds of tests/test_bf16_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

from conftest import Golden, rel_err
from test_bf16_gpu import close_bf16

pytestmark = pytest.mark.gpu
CL = torch.channels_last
BF = torch.bfloat16
TOL, GTOL = 1e-5, 1e-4
SLOPE, SCALE = 0.2, 2 ** 0.5

# (B, C, H, W, noise batch): vector and scalar (C = 5, 3) channel paths, both noise forms, more than 64 vectors per pixel (512), and
# enough pixels for many blocks (the partials and the fill kernel)
OP_CASES = [(2, 8, 9, 9, 2), (2, 12, 9, 9, 1), (1, 5, 4, 4, 1), (3, 3, 8, 8, 3), (2, 512, 4, 4, 2), (2, 64, 33, 33, 2)]
_ids = lambda c: "x".join(map(str, c))


@pytest.fixture(scope="module")
def gold():
    return Golden("stylegan2_gen.npz")


def _operands(case, dtype):
    """x, noise, nw, bias, gy as the kernels see them (x / gy rounded to ``dtype``), in f64 on the CPU.  Elements whose
    pre-activation would land within 1e-3 of zero are moved away from it: the f32 and the f64 evaluation must agree on the sign."""
    b, c, h, w, nb = case
    g = torch.Generator().manual_seed(11 + sum(case))
    rnd = lambda *s: torch.randn(*s, generator=g)
    x, gy = rnd(b, c, h, w).to(dtype).double(), rnd(b, c, h, w).to(dtype).double()
    nz, nw, bias = rnd(nb, 1, h, w).double(), rnd(1).double(), rnd(c).double()
    pre = x + nw * nz + bias.view(1, c, 1, 1)
    x = torch.where(pre.abs() < 1e-3, x + 0.25, x).to(dtype).double()
    assert float((x + nw * nz + bias.view(1, c, 1, 1)).abs().min()) > 1e-4
    return x, nz, nw, bias, gy


def _ref(x, nz, nw, bias, gy):
    c = x.shape[1]
    pre = x + nw * nz + bias.view(1, c, 1, 1)
    out = torch.where(pre > 0, pre, pre * SLOPE) * SCALE
    gpre = gy * SCALE * torch.where(out > 0, 1.0, SLOPE)
    gn = nw * gpre.sum(1, keepdim=True)
    if nz.shape[0] == 1:
        gn = gn.sum(0, keepdim=True)
    return dict(out=out, gx=gpre, gb=gpre.sum((0, 2, 3)), gnw=(gpre * nz).sum(), gnw_abs=(gpre * nz).abs().sum(), gn=gn)


def _run(ops, dtype, fmt, nw=None, noise_grad=True, bias_grad=True):
    """out and the gradients of the op on the device; a gradient that is not asked for (``noise_grad`` / ``bias_grad``) is None."""
    import ideas_amd.op as op
    x64, nz64, nw64, b64, gy64 = ops
    x = x64.to(dtype).cuda().contiguous(memory_format=fmt).requires_grad_(True)
    nz = nz64.float().cuda().requires_grad_(noise_grad)
    nwt = (nw64 if nw is None else nw).float().cuda().requires_grad_(True)
    bias = b64.float().cuda().requires_grad_(bias_grad)
    out = op.noise_bias_act(x, nz, nwt, bias, SLOPE, SCALE)
    leaves = {"gx": x, "gnw": nwt}
    if noise_grad:
        leaves["gn"] = nz
    if bias_grad:
        leaves["gb"] = bias
    grads = torch.autograd.grad(out, list(leaves.values()), gy64.to(dtype).cuda().contiguous(memory_format=fmt))
    res = dict(out=out.detach(), gn=None, gb=None)
    res.update(zip(leaves, grads))
    return res


# Shapes past the grid caps (4096 blocks forward, NOISE_ACT_MAX_PARTIALS backward), so that a block takes its pixel loop more than
# once, at both ends of the lane-group size: G = 64 (f32: 33 vectors of 4; bf16: 132 % 8 != 0, the scalar path with 132 elements
# over 64 lanes, unevenly) and G = 4 (three scalar channels; a [1, 1, H, W] noise against B = 5: the fold through the workspace)
MULTI_TRIP = (1, 132, 257, 257, 1)
MULTI_TRIP_CASES = [MULTI_TRIP, (5, 3, 512, 512, 1)]
# more than 64 vectors a pixel with lanes that carry different counts: 129 vectors of 4 f32 / of 8 bf16 (lane 0 three, the rest
# two), 70 scalar elements (lanes 0..5 two, the rest one); each shape runs in both dtypes (516 bf16 and 70 are scalar paths)
UNEVEN_CASES = [(2, 516, 3, 3, 2), (2, 1032, 3, 3, 2), (2, 70, 5, 5, 1)]


def _trips(case, dtype):
    """(forward, backward) passes of a block through its pixel loop, from the split csrc/noise_act.hip documents: L vectors of 4
    f32 / 8 bf16 elements (elements when C is no multiple), G = the power of two >= min(L, 64) lanes a pixel, 256 / G pixels a block,
    4 in flight; at most 4096 blocks forward and NOISE_ACT_MAX_PARTIALS backward."""
    from ideas_amd import _lib
    b, c, h, w, nb = case
    vw = 8 if dtype == BF else 4
    vectors = c // vw if c % vw == 0 else c
    g = 1
    while g < vectors and g < 64:
        g *= 2
    per_block, npix = (256 // g) * 4, b * h * w
    trips = lambda cap: -(-npix // (min(-(-npix // per_block), cap) * per_block))
    return trips(4096), trips(_lib.NOISE_ACT_MAX_PARTIALS)


_case_cache = {}


def _case(case, dtype):
    """(operands, f64 reference) of a case, computed once."""
    if (case, dtype) not in _case_cache:
        ops = _operands(case, dtype)
        _case_cache[(case, dtype)] = (ops, _ref(*ops))
    return _case_cache[(case, dtype)]


def _check_f32_side(case, got, ref):
    """The f32 results of either activation dtype: bias, noise-weight and noise gradients."""
    e = rel_err(got["gb"], ref["gb"])
    print(case, "gbias", e)
    assert e < GTOL, (case, e)
    e = rel_err(got["gn"], ref["gn"])
    print(case, "gnoise", e)
    assert e < GTOL, (case, e)
    d, bound = abs(float(got["gnw"]) - float(ref["gnw"])), 1e-5 * float(ref["gnw_abs"])
    print(case, "gnw |got - ref|", d, "bound", bound)
    assert d <= bound, (case, d, bound)


def _check_f32(case, fmt):
    b, c, h, w, nb = case
    ops, ref = _case(case, torch.float32)
    got = _run(ops, torch.float32, fmt)
    assert tuple(got["out"].shape) == (b, c, h, w) and got["out"].dtype == torch.float32 and got["out"].is_contiguous(memory_format=CL)
    assert tuple(got["gn"].shape) == (nb, 1, h, w) and tuple(got["gnw"].shape) == (1,) and tuple(got["gb"].shape) == (c,)
    e = rel_err(got["out"], ref["out"])
    print(case, "out", e)
    assert e < TOL, (case, e)
    e = rel_err(got["gx"], ref["gx"])
    print(case, "gx", e)
    assert e < GTOL, (case, e)
    _check_f32_side(case, got, ref)


def _check_bf16(case):
    """bf16 tensors, channels_last: f32 arithmetic, one rounding to bf16 at each store; the f32 side results keep the f32 bounds."""
    ops, ref = _case(case, BF)
    got = _run(ops, BF, CL)
    assert got["out"].dtype == BF and got["gx"].dtype == BF and got["gn"].dtype == torch.float32
    close_bf16(got["out"], ref["out"], "out")
    # the kernel's mask is the sign of the STORED bf16 output, which is the sign of the pre-activation
    close_bf16(got["gx"], ref["gx"], "gx")
    _check_f32_side(case, got, ref)


@pytest.mark.parametrize("fmt", [torch.contiguous_format, CL], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("case", OP_CASES, ids=_ids)
def test_op_f32_vs_f64_restatement(case, fmt):
    _check_f32(case, fmt)


@pytest.mark.parametrize("case", OP_CASES, ids=_ids)
def test_op_bf16_vs_f64_on_the_same_operands(case):
    _check_bf16(case)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", MULTI_TRIP_CASES, ids=_ids)
def test_op_multi_trip_vs_f64(case, dtype):
    """Capped grids: the grid-stride loops of both kernels, the shared trip count of the backward and a partial last trip."""
    fwd, bwd = _trips(case, dtype)
    print(case, dtype, "trips forward", fwd, "backward", bwd)
    assert fwd >= 2 and bwd >= 2, (fwd, bwd)
    if dtype == BF:
        _check_bf16(case)
    else:
        _check_f32(case, CL)


@pytest.mark.parametrize("fmt", [torch.contiguous_format, CL], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("case", UNEVEN_CASES, ids=_ids)
def test_op_f32_uneven_lanes_above_64_vectors(case, fmt):
    _check_f32(case, fmt)


@pytest.mark.parametrize("case", UNEVEN_CASES, ids=_ids)
def test_op_bf16_uneven_lanes_above_64_vectors(case):
    _check_bf16(case)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [(2, 64, 33, 33, 2), MULTI_TRIP], ids=_ids)
def test_backward_without_noise_or_bias_gradient(case, dtype):
    """What training runs: the noise is drawn or a buffer (no noise gradient: the kernel variant that never reads the noise weight)
    and, for a frozen bias, no bias gradient.  Everything else is the full run's bits; gbias (float atomics) keeps its bound."""
    ops, ref = _case(case, dtype)
    full = _run(ops, dtype, CL)
    got = _run(ops, dtype, CL, noise_grad=False)
    assert got["gn"] is None
    for k in ("out", "gx", "gnw"):
        assert torch.equal(got[k], full[k]), ("no noise gradient", k)
    e = rel_err(got["gb"], ref["gb"])
    print(case, dtype, "gbias without the noise gradient", e)
    assert e < GTOL, (case, e)
    got = _run(ops, dtype, CL, bias_grad=False)
    assert got["gb"] is None
    for k in ("out", "gx", "gnw", "gn"):
        assert torch.equal(got[k], full[k]), ("no bias gradient", k)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [(2, 8, 9, 9, 2), (1, 5, 4, 4, 1), (2, 64, 33, 33, 2), MULTI_TRIP], ids=_ids)
def test_zero_noise_weight_is_fused_leaky_relu_bit_for_bit(case, dtype):
    import ideas_amd.op as op
    ops, _ = _case(case, dtype)
    got = _run(ops, dtype, CL, nw=torch.zeros(1, dtype=torch.float64))
    x = ops[0].to(dtype).cuda().contiguous(memory_format=CL)
    want = op.fused_leaky_relu(x, ops[3].float().cuda(), SLOPE, SCALE)
    assert torch.equal(got["out"], want)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [(2, 64, 33, 33, 2), (2, 12, 9, 9, 1), MULTI_TRIP], ids=_ids)
def test_two_runs_are_bitwise_equal(case, dtype):
    ops, _ = _case(case, dtype)
    a, b = _run(ops, dtype, CL), _run(ops, dtype, CL)
    for k in ("out", "gx", "gnw", "gn"):
        assert torch.equal(a[k], b[k]), k


def test_second_order_runs_the_composition_and_is_refused_elsewhere():
    import ideas_amd.op as op
    from ideas_amd.op.modulated_conv import second_order
    case = (2, 8, 9, 9, 2)
    ops = _operands(case, torch.float32)
    first = _run(ops, torch.float32, CL)
    leaves = lambda: (ops[0].float().cuda().contiguous(memory_format=CL).requires_grad_(True), ops[1].float().cuda().requires_grad_(True),
                      ops[2].float().cuda().requires_grad_(True), ops[3].float().cuda().requires_grad_(True),
                      ops[4].float().cuda().contiguous(memory_format=CL).requires_grad_(True))
    x, nz, nw, bias, gy = leaves()
    with pytest.raises(RuntimeError):
        (gx,) = torch.autograd.grad(op.noise_bias_act(x, nz, nw, bias, SLOPE, SCALE), x, gy, create_graph=True)
        torch.autograd.grad(gx.sum(), gy)
    x, nz, nw, bias, gy = leaves()
    with second_order():
        out = op.noise_bias_act(x, nz, nw, bias, SLOPE, SCALE)
        gx, gn, gnw, gb = torch.autograd.grad(out, (x, nz, nw, bias), gy, create_graph=True)
        (ggy,) = torch.autograd.grad((gx * x.detach()).sum(), gy)
    ref = _ref(*ops)
    assert rel_err(out, first["out"]) < TOL and rel_err(gx, first["gx"]) < GTOL
    assert rel_err(gn, first["gn"]) < GTOL and rel_err(gb, first["gb"]) < GTOL
    assert abs(float(gnw.detach()) - float(first["gnw"])) <= 1e-5 * float(ref["gnw_abs"])
    want = ops[0] * SCALE * torch.where(ref["out"] > 0, 1.0, SLOPE)               # d(sum(gx * x)) / d gy
    e = rel_err(ggy, want)
    print("second order d(gx . x)/d gy", e)
    assert e < GTOL, e


def test_noise_injection_draws_its_noise():
    """noise=None on [2, 4, 64, 64] with weight = 1 and a zero image: n = out - image is the drawn [B, 1, H, W] field.  Bounds: five
    sigma for N = 8192 normal samples."""
    from ideas_amd.model import NoiseInjection
    m = NoiseInjection().cuda()
    with torch.no_grad():
        m.weight.fill_(1.0)
    image = torch.zeros(2, 4, 64, 64, device="cuda")
    torch.manual_seed(123)
    n = m(image) - image
    assert tuple(n.shape) == (2, 4, 64, 64) and n.device == image.device
    assert torch.equal(n, n[:, :1].expand_as(n))
    field = n[:, 0].double()
    mean, std = float(field.mean()), float(field.std())
    print("drawn noise: mean %.4f, std %.4f" % (mean, std))
    assert abs(mean) < 5 / 8192 ** 0.5
    assert abs(std - 1) < 5 / (2 * 8192) ** 0.5
    assert not torch.equal(m(image), n)


# ------------------------------------------------------------------------------------------------- layers
def _load(gold, tag, m):
    pre = f"{tag}/sd/"
    m.load_state_dict({k[len(pre):]: gold.t(k) for k in gold.keys() if k.startswith(pre)}, strict=True)
    return m.cuda()


def _layer_check(gold, tag, m, inputs):
    """``inputs``: names of the golden's leaves, in the order of the module's forward."""
    leaves = [gold.t(f"{tag}/{k}").cuda() for k in inputs]
    leaves = [(t.contiguous(memory_format=CL) if t.dim() == 4 else t).requires_grad_(True) for t in leaves]
    y = m(*leaves)
    ref = gold.t(f"{tag}/y")
    assert tuple(y.shape) == tuple(ref.shape)
    e = rel_err(y, ref)
    print(tag, "y", e)
    assert e < TOL, (tag, e)
    names = [n for n, _ in m.named_parameters()]
    grads = torch.autograd.grad(y, leaves + [p for _, p in m.named_parameters()], gold.t(f"{tag}/cot").cuda())
    for k, g in zip(inputs, grads):
        e = rel_err(g, gold.t(f"{tag}/g_{k}"))
        print(tag, "g", k, e)
        assert e < GTOL, (tag, k, e)
    for n, g in zip(names, grads[len(leaves):]):
        ref_g = gold.t(f"{tag}/g/{n}")
        assert tuple(g.shape) == tuple(ref_g.shape), (tag, n)
        e = rel_err(g, ref_g)
        print(tag, n, e)
        assert e < GTOL, (tag, n, e)
    return y.detach(), [g.detach() for g in grads]


def _styled(gold, c):
    from ideas_amd.model import StyledConv
    return _load(gold, c["tag"], StyledConv(c["cin"], c["cout"], 3, 16, upsample=c["upsample"]))


@pytest.mark.parametrize("i", [0, 1, 2], ids=["same", "up", "c5"])
def test_styled_conv_vs_reference(gold, i):
    c = gold.json("meta")["sc"][i]
    y, _ = _layer_check(gold, c["tag"], _styled(gold, c), ("x", "style", "noise"))
    assert list(y.shape[2:]) == [c["out_hw"]] * 2


@pytest.mark.parametrize("i", [0, 1, 2], ids=["same", "up", "c5"])
def test_styled_conv_bf16_vs_its_f32_path(gold, i):
    """bf16 activations against the f32 HIP result on the same weights, with the network bound of tests/test_bf16_gpu.py: outputs
    within 4e-2 of the largest, gradient cosine > 0.99 overall and > 0.9 per tensor."""
    from ideas_amd import precision
    c = gold.json("meta")["sc"][i]
    m = _styled(gold, c)
    tag = c["tag"]
    x = gold.t(f"{tag}/x").cuda().contiguous(memory_format=CL).requires_grad_(True)
    style, noise = gold.t(f"{tag}/style").cuda().requires_grad_(True), gold.t(f"{tag}/noise").cuda().requires_grad_(True)
    cot = gold.t(f"{tag}/cot").cuda()

    def run():
        y = m(x, style, noise=noise)
        return y, torch.autograd.grad(y.float(), [x, style, noise] + list(m.parameters()), cot)
    ref, gref = run()
    with precision.activations(BF):
        got, ggot = run()
    assert got.dtype == BF
    e = rel_err(got, ref)
    assert e < 4e-2, e
    flat = lambda gs: torch.cat([g_.flatten().double() for g_ in gs])
    cos = float(F.cosine_similarity(flat(ggot), flat(gref), dim=0))
    worst = min(float(F.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0))
                for a, b in zip(ggot, gref) if float(b.abs().max()) > 1e-6 and b.numel() > 64)
    print(tag, "bf16 vs f32 path: y %.2e, gradient cosine %.5f (worst tensor %.4f)" % (e, cos, worst))
    assert cos > 0.99 and worst > 0.9, (cos, worst)


def test_to_rgb_vs_reference(gold):
    from ideas_amd.model import ToRGB
    for c in gold.json("meta")["rgb"]:
        m = _load(gold, c["tag"], ToRGB(8, 16, upsample=c["upsample"]))
        y, _ = _layer_check(gold, c["tag"], m, ("x", "style", "skip") if c["upsample"] else ("x", "style"))
        assert tuple(y.shape) == (2, 3, 18, 18)


def test_upsample_downsample_pixel_norm_vs_reference(gold):
    from ideas_amd.model import Downsample, PixelNorm, Upsample
    meta = gold.json("meta")
    for tag, m in (("up", Upsample([1, 3, 3, 1])), ("down", Downsample([1, 3, 3, 1]))):
        y, _ = _layer_check(gold, tag, m.cuda(), ("x",))
        assert list(y.shape[2:]) == meta[tag]["out_hw"]
    _layer_check(gold, "pn", PixelNorm(), ("x",))


# ------------------------------------------------------------------------------------------------- generator
def _generator(gold, size):
    from ideas_amd.model import Generator
    init = gold.json("meta")["init"]
    torch.manual_seed(init["seed"])
    net = Generator(size, init["style_dim"], init["n_mlp"])
    pre = f"gen{size}/fill/"
    fill = {k[len(pre):]: gold.t(k) for k in gold.keys() if k.startswith(pre)}
    named = dict(net.named_parameters())
    assert set(fill) == {n for n in named if n.endswith("bias") or n.endswith("noise.weight")}
    with torch.no_grad():
        for n, v in fill.items():
            named[n].copy_(v)
    return net.cuda()


@pytest.fixture(scope="module")
def gen8(gold):
    return _generator(gold, 8)


def _noises(gold, size, net):
    return [gold.t(f"gen{size}/noise{i}").cuda() for i in range(net.num_layers)]


def _gen_check(gold, tag, net, kwargs, n_styles=1):
    params = list(net.parameters())
    zs = [gold.t(f"{tag}/z{i}").cuda().requires_grad_(True) for i in range(n_styles)]
    image, latent = net(zs, return_latents=True, **kwargs)
    ref = gold.t(f"{tag}/y")
    assert image.dtype == torch.float32 and tuple(image.shape) == tuple(ref.shape) == (2, 3, net.size, net.size)
    e = rel_err(image, ref)
    print(tag, "image", e)
    assert e < TOL, (tag, e)
    ref_l = gold.t(f"{tag}/latent")
    assert tuple(latent.shape) == tuple(ref_l.shape) == (2, net.n_latent, net.style_dim)
    e = rel_err(latent, ref_l)
    print(tag, "latent", e)
    assert e < TOL, (tag, e)
    grads = torch.autograd.grad((image * gold.t(f"{tag}/cot").cuda()).sum(), zs + params, allow_unused=True)
    for i in range(n_styles):
        e = rel_err(grads[i], gold.t(f"{tag}/g_z{i}"))
        print(tag, "dz%d" % i, e)
        assert e < GTOL, (tag, i, e)
    norms = torch.tensor([0.0 if q is None else float(q.norm()) for q in grads[n_styles:]], dtype=torch.float64)
    want = gold.t(f"{tag}/gparam_norms")
    print(tag, "gparam norms, worst relative", float(((norms - want).abs() / want.clamp_min(1e-30))[want > 0].max()))
    assert torch.allclose(norms, want, rtol=5e-4, atol=1e-6), tag


def test_generator8_vs_reference(gold, gen8):
    _gen_check(gold, "gen8", gen8, dict(noise=_noises(gold, 8, gen8)))


def test_generator16_vs_reference(gold):
    net = _generator(gold, 16)
    _gen_check(gold, "gen16", net, dict(noise=_noises(gold, 16, net)))


@pytest.mark.parametrize("tag", ["gen8_bufs", "gen8_mix", "gen8_trunc", "gen8_wlat"])
def test_generator8_settings_vs_reference(gold, gen8, tag):
    kwargs = dict(randomize_noise=False)
    if tag == "gen8_mix":
        kwargs["inject_index"] = 2
    if tag == "gen8_trunc":
        kwargs.update(truncation=0.7, truncation_latent=gold.t("gen8_trunc/truncation_latent").cuda())
    if tag == "gen8_wlat":
        kwargs["input_is_latent"] = True
    _gen_check(gold, tag, gen8, kwargs, n_styles=2 if tag == "gen8_mix" else 1)


def test_path_length_vs_reference(gold, gen8):
    from ideas_amd.op.modulated_conv import second_order
    from ideas_amd.train_step import g_path_regularize
    net = gen8
    params = list(net.parameters())
    lat = gold.t("gen8_path/latent").cuda().requires_grad_(True)
    with second_order():
        image, _ = net([lat], input_is_latent=True, noise=_noises(gold, 8, net))
        e = rel_err(image, gold.t("gen8_path/image"))
        print("path length: image", e)
        assert e < TOL, e
        pen, mean, lengths = g_path_regularize(image, lat, torch.zeros((), device="cuda"), noise=gold.t("gen8_path/img_noise").cuda())
        gr = torch.autograd.grad(pen, params, allow_unused=True)
    ref = float(gold.t("gen8_path/penalty"))
    print("path length: penalty", float(pen), ref, "mean", float(mean), float(gold.t("gen8_path/mean")))
    assert abs(float(pen) - ref) <= 2e-4 * abs(ref), (float(pen), ref)
    e = rel_err(lengths, gold.t("gen8_path/lengths"))
    print("path length: lengths", e)
    assert e < GTOL, e
    norms = torch.tensor([0.0 if q is None else float(q.norm()) for q in gr], dtype=torch.float64)
    want = gold.t("gen8_path/gparam_norms")
    print("path length: gparam norms, worst relative", float(((norms - want).abs() / want.clamp_min(1e-30))[want > 0].max()))
    assert torch.allclose(norms, want, rtol=2e-3, atol=1e-8)


def test_generator_consistency(gen8):
    from ideas_amd.model import Generator, NoiseInjection
    torch.manual_seed(9)
    ml = gen8.mean_latent(64)
    assert tuple(ml.shape) == (1, 32) and bool(torch.isfinite(ml).all())
    assert tuple(gen8.get_latent(torch.randn(3, 32, device="cuda")).shape) == (3, 32)
    noises = gen8.make_noise()
    assert [tuple(n.shape) for n in noises] == [tuple(b.shape) for b in gen8.noises.buffers()]
    assert all(n.is_cuda for n in noises)
    net = Generator(16, 32, 2).cuda()
    with torch.no_grad():
        for m in net.modules():                       # at its initial zero the noise never reaches the image
            if isinstance(m, NoiseInjection):
                m.weight.fill_(0.5)
    z = torch.randn(2, 32, device="cuda")
    image, latent = net([z], randomize_noise=True)
    assert latent is None and tuple(image.shape) == (2, 3, 16, 16) and image.dtype == torch.float32 and bool(torch.isfinite(image).all())
    image2, _ = net([z], randomize_noise=True)
    assert not torch.equal(image, image2)             # fresh noise in every call
    grads = torch.autograd.grad(image.square().mean(), list(net.parameters()))
    for (n, _), g in zip(net.named_parameters(), grads):
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, n
