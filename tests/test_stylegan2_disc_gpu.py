"""GPU parity of the StyleGAN2 discriminator side: ``op.minibatch_stddev`` (forward, backward, backward of the backward) against the
f64 restatement tests/mbstd_ref.py (pinned to the reference in tests/test_stylegan2_disc.py) and against the reference's own
captured block output, and ``ConvLayer`` / ``ResBlock`` / ``Discriminator`` against what the reference's classes computed
(tests/golden/stylegan2_disc.npz).  Tolerances: DESIGN.md "Tolerances" (1e-5 forward, 1e-4 gradients, of the largest element), the
network bounds of tests/test_nets_gpu.py, the bf16 bounds of tests/test_bf16_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

from conftest import Golden, rel_err
import mbstd_ref as R
from test_bf16_gpu import close_bf16

pytestmark = pytest.mark.gpu
CL = torch.channels_last
BF = torch.bfloat16
TOL, GTOL = 1e-5, 1e-4

OP_CASES = [(4, 8, 4, 4, 1), (8, 12, 4, 4, 1), (2, 8, 4, 4, 1), (3, 4, 2, 2, 1), (1, 8, 4, 4, 1), (8, 12, 3, 5, 2), (4, 5, 4, 4, 1),
            (8, 512, 4, 4, 1)]
# (case, group) with more than four samples in a group: the kernels instantiated for up to 16 register-held samples, with G = 8,
# an odd G (5), G = min(B, group) = 6 and the maximum 16
GROUP_CASES = [((8, 12, 4, 4, 1), 8), ((16, 8, 3, 5, 2), 8), ((10, 6, 2, 2, 1), 5), ((6, 4, 2, 2, 1), 8), ((16, 8, 4, 4, 1), 16)]
# K = 260 * 81 = 21060 columns: more than MBSTD_MAX_PARTIALS blocks of 256, so a block walks its column loop twice (the second
# trip partial) and the fill kernel adds all the partials
CAPPED_CASE = (4, 260, 9, 9, 1)
_ids = lambda c: "x".join(map(str, c))
_gids = lambda cg: _ids(cg[0]) + "-g%d" % cg[1]


@pytest.fixture(scope="module")
def gold():
    return Golden("stylegan2_disc.npz")


def _operands(case, dtype, offset=0.0):
    """x, gout, v as the kernels see them (rounded to ``dtype``), in f64 on the CPU; ``offset`` is added to x before the rounding."""
    b, c, h, w, feat = case
    g = torch.Generator().manual_seed(7 + sum(case))
    rnd = lambda *s: torch.randn(*s, generator=g)
    return (rnd(b, c, h, w) + offset).to(dtype).double(), rnd(b, c + feat, h, w).to(dtype).double(), rnd(b, c, h, w).to(dtype).double()


def _run(case, x64, gout64, v64, dtype, fmt, second=True, group=4):
    """out, gx, (dgout, dx) of the op on the device."""
    import ideas_amd.op as op
    feat = case[4]
    x = x64.to(dtype).cuda().contiguous(memory_format=fmt).requires_grad_(True)
    gout = gout64.to(dtype).cuda().contiguous(memory_format=CL).requires_grad_(True)
    out = op.minibatch_stddev(x, group, feat)
    (gx,) = torch.autograd.grad(out, x, gout, create_graph=True)
    if not second:
        return x, out, gx, None, None
    dgout, dx = torch.autograd.grad(gx, (gout, x), v64.to(dtype).cuda().contiguous(memory_format=CL))
    return x, out, gx, dgout, dx


def _trips(case):
    """Passes of a block through its column loop: ceil(K / 256) blocks, at most MBSTD_MAX_PARTIALS, 256 columns a pass."""
    from ideas_amd import _lib
    b, c, h, w, feat = case
    k = (c // feat) * h * w
    nblk = min(-(-k // 256), _lib.MBSTD_MAX_PARTIALS)
    return -(-k // (nblk * 256))


def _check_f32(case, fmt, group=4, ops=None):
    b, c, h, w, feat = case
    x64, gout64, v64 = ops if ops is not None else _operands(case, torch.float32)
    x, out, gx, dgout, dx = _run(case, x64, gout64, v64, torch.float32, fmt, group=group)
    assert tuple(out.shape) == (b, c + feat, h, w) and out.dtype == torch.float32 and out.is_contiguous(memory_format=CL)
    assert torch.equal(out[:, :c], x.detach())                                   # the copy part is bit-exact
    ref = R.minibatch_stddev(x64, group, feat)
    e = rel_err(out[:, c:], ref[:, c:])
    print(case, group, "statistic", e)
    assert e < TOL, (case, e)
    e = rel_err(gx, R.backward(x64, gout64, group, feat))
    print(case, group, "gx", e)
    assert e < GTOL, (case, e)
    ref_dgout, ref_dx = R.backward2(x64, gout64, v64, group, feat)
    assert torch.equal(dgout[:, :c], v64.float().cuda())
    e = rel_err(dgout[:, c:], ref_dgout[:, c:])
    print(case, group, "d gout statistic channel", e)
    assert e < GTOL, (case, e)
    if b > 1:
        e = rel_err(dx, ref_dx)
        print(case, group, "d x", e)
        assert e < GTOL, (case, e)
    else:
        assert float(dx.abs().max()) == 0.0


def _check_bf16(case, group=4):
    """bf16 tensors, channels_last: statistics in f32, one rounding to bf16 at each store (the op bound of tests/test_bf16_gpu.py)."""
    b, c, h, w, feat = case
    x64, gout64, v64 = _operands(case, BF)
    x, out, gx, dgout, dx = _run(case, x64, gout64, v64, BF, CL, group=group)
    assert out.dtype == BF and gx.dtype == BF and dx.dtype == BF
    assert torch.equal(out[:, :c], x.detach())
    close_bf16(out[:, c:], R.minibatch_stddev(x64, group, feat)[:, c:], "statistic")
    close_bf16(gx, R.backward(x64, gout64, group, feat), "gx")
    ref_dgout, ref_dx = R.backward2(x64, gout64, v64, group, feat)
    assert torch.equal(dgout[:, :c].double().cpu(), v64)
    close_bf16(dgout[:, c:], ref_dgout[:, c:], "d gout statistic channel")
    close_bf16(dx, ref_dx, "d x")


@pytest.mark.parametrize("fmt", [torch.contiguous_format, CL], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("case", OP_CASES, ids=_ids)
def test_op_f32_vs_f64_restatement(case, fmt):
    _check_f32(case, fmt)


@pytest.mark.parametrize("case", OP_CASES, ids=_ids)
def test_op_bf16_vs_f64_on_the_same_operands(case):
    _check_bf16(case)


@pytest.mark.parametrize("fmt", [torch.contiguous_format, CL], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("cg", GROUP_CASES, ids=_gids)
def test_op_f32_groups_above_four(cg, fmt):
    """G in 5..16: all three orders against the restatement called with the same group."""
    _check_f32(cg[0], fmt, group=cg[1])


@pytest.mark.parametrize("cg", GROUP_CASES, ids=_gids)
def test_op_bf16_groups_above_four(cg):
    _check_bf16(cg[0], group=cg[1])


@pytest.mark.parametrize("fmt", [torch.contiguous_format, CL], ids=["nchw", "nhwc"])
def test_op_f32_capped_grid_walks_the_column_loop_twice(fmt):
    assert _trips(CAPPED_CASE) >= 2
    _check_f32(CAPPED_CASE, fmt)


def test_op_bf16_capped_grid_walks_the_column_loop_twice():
    assert _trips(CAPPED_CASE) >= 2
    _check_bf16(CAPPED_CASE)


@pytest.mark.parametrize("fmt", [torch.contiguous_format, CL], ids=["nchw", "nhwc"])
def test_op_f32_large_mean_does_not_cancel(fmt):
    """x = 100 + randn: var = E[x^2] - mean^2 in f32 loses 1e4 * 6e-8 of 1e4 against a variance of 1, and f32 centring comes back
    multiplied by |x| sd / eps in the double backward (csrc/minibatch_stddev.hip::column_stats).  The usual bounds hold only for
    two-pass statistics in double."""
    case = (4, 8, 4, 4, 1)
    ops = _operands(case, torch.float32, offset=100.0)
    assert float(ops[0].mean()) > 99
    _check_f32(case, fmt, ops=ops)


@pytest.mark.parametrize("case,dtype", [((4, 8, 4, 4, 1), torch.float32), ((4, 8, 4, 4, 1), BF), ((3, 4, 2, 2, 1), torch.float32)],
                         ids=["4x8x4x4x1-f32", "4x8x4x4x1-bf16", "3x4x2x2x1-f32"])
def test_identical_samples_give_sqrt_eps_with_a_group(case, dtype):
    """Zero variance with G > 1 (G = 3: sum / 3 is inexact): the statistic is sqrt(eps), u = 0 leaves gx = gout[:, :C], and the
    double backward is a (v - mean_g v) / sd with sd = 1e-4: values in the hundreds."""
    b, c, h, w, feat = case
    x64, gout64, v64 = _operands(case, dtype)
    x64 = x64[:1].expand(b, c, h, w).contiguous()
    x, out, gx, dgout, dx = _run(case, x64, gout64, v64, dtype, CL)
    assert torch.equal(out[:, :c], x.detach())
    if dtype == BF:       # the f32 value rounded once at the store: 1e-4 is 209.7 steps of 2^-21, nowhere near a tie
        assert torch.equal(out[:, c:].cpu(), torch.full((b, 1, h, w), 1e-4).to(BF))
    else:
        assert torch.allclose(out[:, c:].cpu(), torch.full((b, 1, h, w), 1e-4), rtol=1e-6, atol=0)
    e = rel_err(gx, gout64[:, :c])
    print(case, dtype, "gx vs gout[:, :C]", e)
    assert e < GTOL, (case, e)
    ref_dgout, ref_dx = R.backward2(x64, gout64, v64, 4, feat)
    assert float(ref_dx.abs().max()) > 50
    if dtype == BF:
        close_bf16(dx, ref_dx, "d x")
    else:
        e = rel_err(dx, ref_dx)
        print(case, dtype, "d x", e, "largest", float(ref_dx.abs().max()))
        assert e < GTOL, (case, e)


def test_group_of_seventeen_is_refused_and_writes_nothing():
    """B = 17 with group 32 is G = 17, one more than the kernels hold in registers: the op raises, and each C entry point returns an
    error without touching its outputs."""
    import ideas_amd.op as op
    from ideas_amd import _lib
    b, c, h, w, feat, group = 17, 4, 2, 2, 1, 32
    x = torch.randn(b, c, h, w, device="cuda").contiguous(memory_format=CL)
    with pytest.raises(RuntimeError):
        op.minibatch_stddev(x, group, feat)
    lib, p, s = _lib.load(), _lib.ptr, _lib.stream_ptr()
    sentinel = lambda *shape, dtype=torch.float32: torch.full(shape, -77.0, device="cuda", dtype=dtype)
    out, gx, dgout, dx = sentinel(b, h, w, c + feat), sentinel(b, h, w, c), sentinel(b, h, w, c + feat), sentinel(b, h, w, c)
    ws, a = sentinel(_lib.MBSTD_MAX_PARTIALS, dtype=torch.float64), sentinel(1)
    gout, v = torch.randn(b, h, w, c + feat, device="cuda"), torch.randn(b, h, w, c, device="cuda")
    assert lib.ideas_mbstd_fwd(p(out), p(ws), p(x), b, c, h, w, group, feat, 1e-8, _lib.F32, s) != 0
    assert lib.ideas_mbstd_bwd(p(gx), p(a), p(gout), p(x), b, c, h, w, group, feat, 1e-8, _lib.F32, s) != 0
    assert lib.ideas_mbstd_bwd2(p(dgout), p(dx), p(ws), p(v), p(x), p(a), b, c, h, w, group, feat, 1e-8, _lib.F32, s) != 0
    torch.cuda.synchronize()
    for t, name in ((out, "out"), (gx, "gx"), (dgout, "dgout"), (dx, "dx"), (ws, "workspace"), (a, "a")):
        assert bool((t == -77.0).all()), name


def test_single_sample_gives_sqrt_eps_and_no_extra_gradient():
    case = (1, 8, 4, 4, 1)
    x64, gout64, v64 = _operands(case, torch.float32)
    x, out, gx, dgout, dx = _run(case, x64, gout64, v64, torch.float32, CL)
    assert torch.allclose(out[:, 8:].cpu(), torch.full((1, 1, 4, 4), 1e-4), rtol=1e-6, atol=0)
    assert torch.equal(gx, gout64.float().cuda()[:, :8])                         # u = 0: the extra channel's gradient adds nothing
    assert float(dx.abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_two_runs_are_bitwise_equal(dtype):
    for case in ((8, 512, 4, 4, 1), CAPPED_CASE):
        ops = _operands(case, dtype)
        a = _run(case, *ops, dtype, CL)
        b = _run(case, *ops, dtype, CL)
        for u, v, name in zip(a[1:], b[1:], ("out", "gx", "dgout", "dx")):
            assert torch.equal(u, v), (case, name)


def test_third_order_request_raises():
    import ideas_amd.op as op
    case = (4, 8, 4, 4, 1)
    x64, gout64, v64 = _operands(case, torch.float32)
    x = x64.float().cuda().requires_grad_(True)
    gout = gout64.float().cuda().requires_grad_(True)
    (gx,) = torch.autograd.grad(op.minibatch_stddev(x), x, gout, create_graph=True)
    (dx,) = torch.autograd.grad(gx, x, v64.float().cuda(), create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(dx.sum(), x)


def test_op_reproduces_the_references_captured_block(gold):
    import ideas_amd.op as op
    for tag in ("disc8_b8", "disc8_b4", "mb_b3"):
        ref = gold.t(f"{tag}/mb_out").cuda()
        out = op.minibatch_stddev(ref[:, :512].contiguous())
        assert torch.equal(out[:, :512], ref[:, :512])
        e = rel_err(out[:, 512:], gold.t(f"{tag}/mb_stat64"))
        print(tag, "statistic vs the reference's expression in f64", e)
        assert e < TOL, (tag, e)
        assert rel_err(out[:, 512:], ref[:, 512:]) < TOL, tag


# ------------------------------------------------------------------------------------------------- layers
def _layer(gold, tag, m):
    pre = f"{tag}/sd/"
    m.load_state_dict({k[len(pre):]: gold.t(k) for k in gold.keys() if k.startswith(pre)}, strict=True)
    return m.cuda()


def _layer_check(gold, tag, m):
    x = gold.t(f"{tag}/x").cuda().contiguous(memory_format=CL).requires_grad_(True)
    y = m(x)
    ref = gold.t(f"{tag}/y")
    assert tuple(y.shape) == tuple(ref.shape)
    e = rel_err(y, ref)
    print(tag, "y", e)
    assert e < TOL, (tag, e)
    names = [n for n, _ in m.named_parameters()]
    grads = torch.autograd.grad(y, [x] + [p for _, p in m.named_parameters()], gold.t(f"{tag}/gy").cuda())
    e = rel_err(grads[0], gold.t(f"{tag}/gx"))
    print(tag, "gx", e)
    assert e < GTOL, (tag, e)
    for n, g in zip(names, grads[1:]):
        e = rel_err(g, gold.t(f"{tag}/g/{n}"))
        print(tag, n, e)
        assert e < GTOL, (tag, n, e)
    return y.detach(), [g.detach() for g in grads]


def test_conv_layers_vs_reference(gold):
    from ideas_amd.model import ConvLayer
    for c in gold.json("meta")["conv"]:
        m = ConvLayer(c["cin"], c["cout"], c["k"], downsample=c["downsample"], bias=c["bias"], activate=c["activate"])
        y, _ = _layer_check(gold, f"conv{c['i']}", _layer(gold, f"conv{c['i']}", m))
        assert list(y.shape[2:]) == c["out_hw"]


def test_res_block_vs_reference_on_both_body_routes(gold, monkeypatch):
    """Default dispatch (16 x 16 output pixels x 2 images: below BLUR_CONV_MIN_BLOCKS, the layer-by-layer body with the post_blur
    pairing), then with the threshold lowered so that the fused blur + stride-2 body (down_pair) runs; which one ran is asserted
    through down_pair_ok, and the two results agree within the same tolerances."""
    import ideas_amd.op.conv as cv
    from ideas_amd.model import ResBlock
    meta = gold.json("meta")["res"]
    m = _layer(gold, "res", ResBlock(meta["in_channel"], meta["out_channel"]))
    x = gold.t("res/x").cuda().contiguous(memory_format=CL)
    c1, c2, blur = m.conv1[0], m.conv2[1], m.conv2[0]
    ok = lambda: cv.down_pair_ok(x, c1.weight, c2.weight, blur.kernel, blur.pad, c1.padding)
    assert not ok()
    y0, g0 = _layer_check(gold, "res", m)
    monkeypatch.setattr(cv, "BLUR_CONV_MIN_BLOCKS", 1)
    assert ok() and m._fused_body() is not None
    y1, g1 = _layer_check(gold, "res", m)
    assert m._body_pair_ok(x)
    assert rel_err(y1, y0) < TOL
    for a, b in zip(g1, g0):
        assert rel_err(a, b) < GTOL


def _disc8(gold):
    from ideas_amd.model import Discriminator
    meta = gold.json("meta")
    torch.manual_seed(meta["init"]["seed"])
    net = Discriminator(8)
    pre = "disc8/bias/"
    biases = {k[len(pre):]: gold.t(k) for k in gold.keys() if k.startswith(pre)}
    named = dict(net.named_parameters())
    assert set(biases) == {n for n in named if n.endswith("bias")}
    with torch.no_grad():
        for n, b in biases.items():
            named[n].copy_(b)
    return net.cuda()


@pytest.fixture(scope="module")
def disc8(gold):
    return _disc8(gold)


@pytest.mark.parametrize("tag", ["disc8_b8", "disc8_b4"])
def test_discriminator_vs_reference(gold, disc8, tag):
    from ideas_amd.utils import d_r1_loss
    net = disc8
    params = list(net.parameters())
    x = gold.t(f"{tag}/x").cuda().contiguous(memory_format=CL).requires_grad_(True)
    logits = net(x)
    ref = gold.t(f"{tag}/logits")
    assert logits.dtype == torch.float32 and tuple(logits.shape) == tuple(ref.shape)
    e = rel_err(logits, ref)
    print(tag, "logits", e)
    assert e < TOL, (tag, e)
    grads = torch.autograd.grad(logits.sum(), [x] + params)
    e = rel_err(grads[0], gold.t(f"{tag}/gx"))
    print(tag, "gx", e)
    assert e < GTOL, (tag, e)
    norms = torch.tensor([float(q.norm()) for q in grads[1:]], dtype=torch.float64)
    print(tag, "gparam norms, worst relative", float(((norms - gold.t(f"{tag}/gparam_norms")).abs() / gold.t(f"{tag}/gparam_norms")).max()))
    assert torch.allclose(norms, gold.t(f"{tag}/gparam_norms"), rtol=5e-4, atol=1e-6), tag
    x2 = x.detach().clone().requires_grad_(True)
    r1 = d_r1_loss(net(x2), x2)
    r1_ref = float(gold.t(f"{tag}/r1"))
    print(tag, "r1", float(r1), r1_ref)
    assert abs(float(r1) - r1_ref) <= 2e-4 * abs(r1_ref), (tag, float(r1), r1_ref)
    gr = torch.autograd.grad(r1, params, allow_unused=True)
    n2 = torch.tensor([0.0 if q is None else float(q.norm()) for q in gr], dtype=torch.float64)
    ref2 = gold.t(f"{tag}/r1_gparam_norms")
    print(tag, "r1 gparam norms, worst relative", float(((n2 - ref2).abs() / ref2.clamp_min(1e-30)).max()))
    assert torch.allclose(n2, ref2, rtol=2e-3, atol=1e-8), tag


def test_discriminator_bf16_vs_its_f32_path(gold, disc8):
    """bf16 activations against the f32 HIP result on the same weights, with the network bound of tests/test_bf16_gpu.py
    (test_networks_bf16_vs_f32_path): outputs within 4e-2 of the largest, gradient cosine > 0.99 overall and > 0.9 per tensor."""
    from ideas_amd import precision
    net = disc8
    params = list(net.parameters())
    x = gold.t("disc8_b8/x").cuda().contiguous(memory_format=CL)

    def run():
        logits = net(x)
        return logits, torch.autograd.grad(logits.mean(), params)
    ref, gref = run()
    with precision.activations(BF):
        got, ggot = run()
    assert got.dtype == torch.float32
    e = rel_err(got, ref)
    assert e < 4e-2, e
    flat = lambda gs: torch.cat([g_.flatten().double() for g_ in gs])
    cos = float(F.cosine_similarity(flat(ggot), flat(gref), dim=0))
    worst = min(float(F.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0))
                for a, b in zip(ggot, gref) if float(b.abs().max()) > 1e-6 and b.numel() > 64)
    print("Discriminator(8) bf16 vs f32 path: logits %.2e, gradient cosine %.5f (worst tensor %.4f)" % (e, cos, worst))
    assert cos > 0.99 and worst > 0.9, (cos, worst)


def test_discriminator_16_runs_forward_backward_and_r1():
    """Two blocks, batch 4: finite results, and gradients reach every parameter -- of the logits and of the R1 penalty."""
    from ideas_amd.model import Discriminator
    from ideas_amd.utils import d_r1_loss
    torch.manual_seed(3)
    net = Discriminator(16).cuda()
    params = list(net.parameters())
    x = torch.randn(4, 3, 16, 16, device="cuda").requires_grad_(True)
    logits = net(x)
    assert tuple(logits.shape) == (4, 1) and bool(torch.isfinite(logits).all())
    grads = torch.autograd.grad(F.softplus(-logits).mean(), params)
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)
    r1 = d_r1_loss(net(x), x)
    assert bool(torch.isfinite(r1)) and float(r1) > 0
    gr = torch.autograd.grad(r1, params, allow_unused=True)
    named = [n for n, _ in net.named_parameters()]
    # weights, and the biases in front of the stddev block (the statistic depends on them smoothly), shape d logits / d x; the
    # biases behind it only move leaky-ReLU masks, and the last one nothing at all
    for n, g in zip(named, gr):
        if n.endswith("weight") or n.startswith("convs."):
            assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, n
        else:
            assert g is None or float(g.abs().max()) == 0.0, n
