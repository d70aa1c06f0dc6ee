"""Parameter gradients of the StyleGAN2 ``Generator`` / ``Discriminator`` as WHOLE TENSORS against the f64 restatement
tests/stylegan2_ref.py (pinned to the reference's goldens in tests/test_stylegan2_ref.py): first order, the R1 penalty and the
path-length penalty -- what a training step consumes.  The per-tensor norms of tests/test_stylegan2_gen_gpu.py / _disc_gpu.py cannot
see a sign flip, an in/out transposition, a tap flip or one wrong row (tests/test_stylegan2_ref.py::test_l2_err_sees_what_a_norm_cannot).

Network level (512 channels): for every parameter tensor ``l2_err(g_hip, g64, floor = 1e-3 max_k ||g64_k||) < 6e-3``, the small-tensor
rule and ``DIR_BOUNDS[0]`` of tests/test_nets_gpu.py.  Not tighter on purpose: with 65k-524k leaky-ReLU units a layer an f32 forward
may flip a few masks against f64 (one flip costs about 3e-3 in one tensor); the smallest structural error, one tap of one row, is
1.5e-2.  Where the f64 gradient is None or zero the HIP gradient is None or exactly zero.  The restatement evaluated in f32 on the
CPU is printed next to HIP: the noise floor of the comparison, not an assertion.

Mid-width chains (Cin % 16 == 0: the b3 MFMA kernels; Cout = 80: conv_b3_tphase_kernel; 5 -> 10: partial patches): their seeds leave
no leaky-ReLU unit within 1e-5 of zero (asserted on the CPU), so no mask can differ and the ELEMENTWISE contracts hold: outputs 1e-5,
first-order gradients 1e-4, second-order parameter gradients 2e-3 of the largest element."""
import pytest
import torch

from conftest import Golden, rel_err
import stylegan2_ref as R
import test_stylegan2_ref as C

pytestmark = pytest.mark.gpu
CL = torch.channels_last
TOL, GTOL, GTOL2 = 1e-5, 1e-4, 2e-3
DIR_BOUND = 6e-3
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def gold():
    return Golden("stylegan2_gen.npz")


@pytest.fixture(scope="module")
def dgold():
    return Golden("stylegan2_disc.npz")


@pytest.fixture(scope="module")
def gens(gold):
    """{size: Generator on the device}, built once; the restatement reads its weights through ``R.params_of``."""
    return {size: C.seeded_generator(gold, size).cuda() for size in (8, 16)}


@pytest.fixture(scope="module")
def discs(dgold):
    return {8: C.seeded_disc8(dgold).cuda(), 16: C.seeded_disc16().cuda()}


def _dev(t):
    t = t.float().cuda()
    return t.contiguous(memory_format=CL) if t.dim() == 4 else t


def _cast(v, dtype):
    if torch.is_tensor(v):
        return v.detach().to(dtype)
    if isinstance(v, (list, tuple)):
        return [_cast(u, dtype) for u in v]
    return v


def _is_zero(g):
    return g is None or float(g.abs().max()) == 0.0


def compare_whole(tag, net, g_hip, g64, g32):
    """The comparison rule of the module docstring over all parameters; prints HIP's and CPU-f32's error per tensor, then asserts."""
    names = [n for n, _ in net.named_parameters()]
    assert len(names) == len(g_hip) == len(g64) == len(g32)
    floor = 1e-3 * max(0.0 if g is None else float(g.norm()) for g in g64)
    assert floor > 0, tag
    rows, bad = [], []
    for n, gh, gr, gf in zip(names, g_hip, g64, g32):
        if _is_zero(gr):
            if not _is_zero(gh):
                bad.append((n, "f64 gradient is zero, HIP's is not", float(gh.abs().max())))
            continue
        if gh is None:
            bad.append((n, "no HIP gradient"))
            continue
        assert tuple(gh.shape) == tuple(gr.shape), (tag, n)
        e = R.l2_err(gh, gr, floor)
        e32 = float("nan") if gf is None else R.l2_err(gf, gr, floor)
        rows.append((e, e32, n))
        print("%-14s %-34s hip %.2e   cpu-f32 %.2e   |g64| %.3e" % (tag, n, e, e32, float(gr.norm())))
        if not e < DIR_BOUND:
            bad.append((n, e))
    worst = max(rows)
    print("%-14s WORST hip %.2e (%s), cpu-f32 there %.2e; worst cpu-f32 %.2e" % (tag, worst[0], worst[2], worst[1], max(r[1] for r in rows)))
    assert not bad, (tag, bad)
    return worst


# ------------------------------------------------------------------------------------------------- generator, first order
GEN_FIRST = {"gen8": (8, "gen8"), "gen16": (16, "gen16"), "gen8_mix": (8, "gen8_mix")}


def _ref_gen_first(net, size, zs, noise, cot, kw, dtype):
    P = R.params_of(net, dtype)
    image, _ = R.generator(P, size, _cast(zs, dtype), _cast(noise, dtype), **_cast(kw, dtype))
    return image.detach(), torch.autograd.grad((image * cot.to(dtype)).sum(), R.param_list(net, P), allow_unused=True)


@pytest.mark.parametrize("case", list(GEN_FIRST))
def test_generator_param_gradients_first_order(gold, gens, case, monkeypatch):
    """The goldens' z, noise and cotangent.  One 2-D z takes the shared ``styles_for`` path (one batched modulation launch, asserted),
    two styles with inject_index = 2 the per-layer path.  Worst tensor, l2_err of HIP / of the CPU-f32 restatement on
    that tensor (MI355X): gen8 5.0e-6 / 7.9e-7 (conv1.noise.weight), gen16 6.3e-6 / 5.2e-7 (convs.0.noise.weight), gen8_mix 1.9e-6 /
    9.0e-5 (convs.0.noise.weight); the CPU-f32 run's own worst tensors: 2.0e-6, 1.5e-6 and 3.4e-3 (a flipped leaky-ReLU mask)."""
    import ideas_amd.model as L
    size, tag = GEN_FIRST[case]
    net = gens[size]
    n_styles = 2 if case == "gen8_mix" else 1
    kw = dict(inject_index=2) if case == "gen8_mix" else {}
    zs = [gold.t(f"{tag}/z{i}") for i in range(n_styles)]
    noise = ([getattr(net.noises, f"noise_{i}").detach().cpu() for i in range(net.num_layers)] if case == "gen8_mix"
             else [gold.t(f"{tag}/noise{i}") for i in range(net.num_layers)])
    cot = gold.t(f"{tag}/cot")
    image64, g64 = _ref_gen_first(net, size, zs, noise, cot, kw, F64)
    _, g32 = _ref_gen_first(net, size, zs, noise, cot, kw, F32)
    batched = []
    make = L.styles_for._make
    monkeypatch.setattr(L.styles_for, "_make", lambda self: (batched.append(len(self.convs)), make(self))[1])
    image, latent = net([_dev(z) for z in zs], noise=[_dev(n) for n in noise], **kw)
    assert latent is None and batched == ([] if case == "gen8_mix" else [len(net._modconvs())]), batched
    e = rel_err(image, image64)
    print(case, "image", e)
    assert e < TOL, (case, e)
    g_hip = torch.autograd.grad((image * _dev(cot)).sum(), list(net.parameters()), allow_unused=True)
    compare_whole(case, net, g_hip, g64, g32)


# ------------------------------------------------------------------------------------------------- generator, path length
def _ref_gen_path(net, size, styles, noise, img_noise, kw, dtype):
    """The restatement's penalty of its OWN [B, n_latent, D] latent (a leaf when ``styles`` is one 3-D latent)."""
    P = R.params_of(net, dtype)
    styles = [s.requires_grad_(s.dim() == 3) for s in _cast(styles, dtype)]
    image, latent = R.generator(P, size, styles, _cast(noise, dtype), **_cast(kw, dtype))
    pen, mean, lengths = R.path_regularize(image, latent, torch.zeros((), dtype=dtype), img_noise.to(dtype))
    grads = torch.autograd.grad(pen, R.param_list(net, P), allow_unused=True)
    return image.detach(), float(pen.detach()), lengths.detach(), grads


def _check_path(tag, net, pen, lengths, image, params_grads, ref64, ref32):
    image64, pen64, len64, g64 = ref64
    e = rel_err(image, image64)
    print(tag, "image", e, "penalty", float(pen.detach()), pen64, "cpu-f32", ref32[1])
    assert e < TOL, (tag, e)
    assert abs(float(pen.detach()) - pen64) <= 2e-4 * abs(pen64), (tag, float(pen.detach()), pen64)
    e = rel_err(lengths, len64)
    print(tag, "lengths", e)
    assert e < GTOL, (tag, e)
    return compare_whole(tag, net, params_grads, g64, ref32[3])


@pytest.mark.parametrize("size", [8, 16])
def test_path_length_param_gradients_on_a_latent_leaf(gold, gens, size):
    """g_path_regularize on a [2, n_latent, 32] leaf (``input_is_latent=True``) inside ``second_order()``: size 8 on the golden's
    latent and image noise, size 16 on seeded ones.  Worst tensor, l2_err of HIP / of the CPU-f32 restatement on that
    tensor (MI355X): size 8 1.9e-6 / 8.7e-7 (convs.0.conv.modulation.bias), size 16 2.0e-6 / 8.3e-7 (conv1.conv.modulation.weight)."""
    from ideas_amd.op.modulated_conv import second_order
    from ideas_amd.train_step import g_path_regularize
    net = gens[size]
    noise = [gold.t(f"gen{size}/noise{i}") for i in range(net.num_layers)]
    if size == 8:
        lat, img_noise = gold.t("gen8_path/latent"), gold.t("gen8_path/img_noise")
    else:
        g = torch.Generator().manual_seed(1616)
        lat, img_noise = torch.randn(2, net.n_latent, 32, generator=g), torch.randn(2, 3, size, size, generator=g)
    kw = dict(input_is_latent=True)
    ref64 = _ref_gen_path(net, size, [lat], noise, img_noise, kw, F64)
    ref32 = _ref_gen_path(net, size, [lat], noise, img_noise, kw, F32)
    latd = _dev(lat).requires_grad_(True)
    with second_order():
        image, _ = net([latd], noise=[_dev(n) for n in noise], **kw)
        pen, _, lengths = g_path_regularize(image, latd, torch.zeros((), device="cuda"), noise=_dev(img_noise))
        gr = torch.autograd.grad(pen, list(net.parameters()), allow_unused=True)
    _check_path("path%d" % size, net, pen, lengths, image, gr, ref64, ref32)


@pytest.mark.parametrize("n_styles", [1, 2], ids=["one_z", "mixed"])
def test_path_length_the_way_the_training_step_calls_it(gold, gens, n_styles):
    """stylegan2/train.py:252-255: ``fake_img, latents = generator(noise, return_latents=True)`` then ``g_path_regularize(fake_img,
    latents, ...)``, with one z (mixing_noise: probability 0.1) and with two.  Before ``Generator.forward`` computed the image from the
    latent it returns, the one-z call raised "One of the differentiated Tensors appears to not have been used in the graph" (the
    pre-fix computation is replayed below and must still raise: that is why the shared path cannot serve this call).  Compared with
    the restatement's gradient through ITS [B, n_latent, D] latent, mapping network included.  Worst tensor,
    l2_err of HIP / of the CPU-f32 restatement on that tensor (MI355X): one z 1.9e-6 / 1.3e-6 (style.1.weight), mixed 1.8e-6 / 7.3e-7
    (convs.0.conv.modulation.weight)."""
    import ideas_amd.model as L
    from ideas_amd.op.modulated_conv import second_order
    from ideas_amd.train_step import g_path_regularize
    net = gens[8]
    tag = "gen8" if n_styles == 1 else "gen8_mix"
    zs = [gold.t(f"{tag}/z{i}") for i in range(n_styles)]
    noise = [gold.t(f"gen8/noise{i}") for i in range(net.num_layers)]
    img_noise = gold.t("gen8_path/img_noise")
    kw = dict(inject_index=2) if n_styles == 2 else {}
    ref64 = _ref_gen_path(net, 8, zs, noise, img_noise, kw, F64)
    ref32 = _ref_gen_path(net, 8, zs, noise, img_noise, kw, F32)
    noise_d = [_dev(n) for n in noise]
    if n_styles == 1:
        with second_order():
            shared = net.style(_dev(zs[0]))
            view = shared.unsqueeze(1).expand(-1, net.n_latent, -1)
            with L.styles_for(net._modconvs(), shared):
                old = net._synthesis(shared, lambda i: shared, noise_d)
            with pytest.raises(RuntimeError, match="not have been used in the graph"):
                torch.autograd.grad(old.sum(), view)
    with second_order():
        image, latents = net([_dev(z) for z in zs], return_latents=True, noise=noise_d, **kw)
        assert tuple(latents.shape) == (2, net.n_latent, 32)
        pen, _, lengths = g_path_regularize(image, latents, torch.zeros((), device="cuda"), noise=_dev(img_noise))
        gr = torch.autograd.grad(pen, list(net.parameters()), allow_unused=True)
    names = [n for n, _ in net.named_parameters()]
    assert all(g is not None for n, g in zip(names, gr) if n.startswith("style."))       # the penalty reaches the mapping network
    _check_path("train-path-%d" % n_styles, net, pen, lengths, image, gr, ref64, ref32)


def test_returned_latent_does_not_change_the_first_order_image(gold, gens):
    """The shared ``styles_for`` path stays for every call that cannot differentiate a returned latent -- no ``return_latents``, or no
    graph -- and yields the bits of the computation ``Generator.forward`` ran before (replayed here from its parts).  With
    ``return_latents=True`` under autograd the image is computed from the returned latent: the same image within the forward
    contract, the latent's own values unchanged, and d image / d latent exists per layer."""
    import ideas_amd.model as L
    net = gens[8]
    z = _dev(gold.t("gen8/z0"))
    noise = [_dev(gold.t(f"gen8/noise{i}")) for i in range(net.num_layers)]
    def replay():
        """What ``Generator.forward`` ran for one 2-D style before it looked at ``return_latents``."""
        shared = net.style(z)
        with L.styles_for(net._modconvs(), shared):
            return shared, net._synthesis(shared, lambda i: shared, noise)
    with torch.no_grad():
        _, old_ng = replay()
        plain_ng, none = net([z], noise=noise)
        lat_ng_image, lat_ng = net([z], return_latents=True, noise=noise)
    assert none is None and torch.equal(plain_ng, old_ng) and torch.equal(lat_ng_image, old_ng)
    shared, old = replay()                                             # under autograd
    plain, _ = net([z], noise=noise)                                   # no latent asked for: the first-order call
    assert plain.requires_grad and torch.equal(plain, old)
    image, latent = net([z], return_latents=True, noise=noise)
    assert torch.equal(latent, lat_ng) and torch.equal(latent, shared.unsqueeze(1).expand(-1, net.n_latent, -1))
    e = rel_err(image, old)
    print("image through the returned latent vs the shared path", e, "bitwise equal:", torch.equal(image, old))
    assert e < TOL, e
    (gl,) = torch.autograd.grad((image * _dev(gold.t("gen8/cot"))).sum(), latent)
    assert tuple(gl.shape) == tuple(latent.shape) and all(float(gl[:, i].abs().max()) > 0 for i in range(net.n_latent))
    # a latent that is itself a constant (no mapping network in the graph, nothing to differentiate) keeps the shared path
    w = shared.detach()
    img_w, lat_w = net([w], return_latents=True, input_is_latent=True, noise=noise)
    assert torch.equal(img_w, old) and torch.equal(lat_w[:, 0], w)


# ------------------------------------------------------------------------------------------------- discriminator
DISC = {"disc8_b8": (8, 8), "disc8_b4": (8, 4), "disc16_b4": (16, 4)}


def _ref_disc(net, size, x, dtype):
    P = R.params_of(net, dtype)
    params = R.param_list(net, P)
    x1 = x.to(dtype).requires_grad_(True)
    logits = R.discriminator(P, size, x1)
    g1 = torch.autograd.grad(logits.sum(), [x1] + params)
    x2 = x.to(dtype).requires_grad_(True)
    r1 = R.d_r1_loss(R.discriminator(P, size, x2), x2)
    g2 = torch.autograd.grad(r1, params, allow_unused=True)
    return logits.detach(), g1[0], g1[1:], float(r1.detach()), g2


@pytest.mark.parametrize("case", list(DISC))
def test_discriminator_param_gradients_first_order_and_r1(dgold, discs, case):
    """Every parameter's gradient of ``logits.sum()`` and of ``d_r1_loss``: Discriminator(8) at batch 8 (two stddev groups) and batch 4
    (one), Discriminator(16) at batch 4 (two ResBlocks; seeded weights and input).  Worst tensor, l2_err of HIP / of the
    CPU-f32 restatement on that tensor (MI355X), first order then R1: disc8_b8 1.3e-6 / 3.6e-7 and 1.2e-6 / 3.6e-7, disc8_b4 1.3e-6 /
    4.6e-7 and 1.4e-6 / 4.5e-7, disc16_b4 1.4e-6 / 1.7e-4 (convs.0.0.weight) and 3.1e-6 / 2.1e-4 (convs.0.1.bias): at 16 x 16 the f32
    CPU evaluation is the noisier of the two."""
    from ideas_amd.utils import d_r1_loss
    size, batch = DISC[case]
    net = discs[size]
    params = list(net.parameters())
    x = dgold.t(f"{case}/x") if size == 8 else torch.randn(batch, 3, 16, 16, generator=torch.Generator().manual_seed(1604))
    assert x.shape[0] == batch
    logits64, gx64, g64, r1_64, gr64 = _ref_disc(net, size, x, F64)
    _, _, g32, r1_32, gr32 = _ref_disc(net, size, x, F32)
    xd = _dev(x).requires_grad_(True)
    logits = net(xd)
    e = rel_err(logits, logits64)
    print(case, "logits", e)
    assert e < TOL, (case, e)
    grads = torch.autograd.grad(logits.sum(), [xd] + params)
    e = rel_err(grads[0], gx64)
    print(case, "gx", e)
    assert e < GTOL, (case, e)
    compare_whole(case, net, grads[1:], g64, g32)
    x2 = _dev(x).requires_grad_(True)
    r1 = d_r1_loss(net(x2), x2)
    print(case, "r1", float(r1.detach()), r1_64, "cpu-f32", r1_32)
    assert abs(float(r1.detach()) - r1_64) <= 2e-4 * abs(r1_64), (case, float(r1.detach()), r1_64)
    gr = torch.autograd.grad(r1, params, allow_unused=True)
    compare_whole(case + " r1", net, gr, gr64, gr32)


# ------------------------------------------------------------------------------------------------- chains without a mask flip
def _elementwise(tag, names, got, want, bound):
    bad = []
    for n, a, b in zip(names, got, want):
        if _is_zero(b):
            if not _is_zero(a):
                bad.append((n, "f64 gradient is zero, HIP's is not"))
            continue
        if a is None:
            bad.append((n, "no HIP gradient"))
            continue
        assert tuple(a.shape) == tuple(b.shape), (tag, n)
        e = rel_err(a, b)
        print("%-22s %-30s %.2e" % (tag, n, e))
        if not e < bound:
            bad.append((n, e))
    assert not bad, (tag, bound, bad)


@pytest.mark.parametrize("name", list(C.G_CHAINS))
def test_g_chain_elementwise_first_and_second_order(name):
    """StyledConv (up) -> StyledConv -> ToRGB with a skip.  First order: cotangents on both outputs, gradients of x, the latent, both
    noises, the skip and every parameter.  Second order: the path penalty of the RGB output with respect to the [2, 3, 16] latent
    leaf, inside ``second_order()``."""
    from ideas_amd.op.modulated_conv import second_order
    from ideas_amd.train_step import g_path_regularize
    m, ins, cots = C.g_chain_case(name)
    assert C.g_chain_fragile(name)[0] == 0
    keys = ("x", "lat", "n1", "n2", "skip")
    pnames = [n for n, _ in m.named_parameters()]

    def ref_leaves():
        return [ins[k].clone().requires_grad_(True) for k in keys]
    P = R.params_of(m)
    lv = ref_leaves()
    y64, rgb64 = C.g_chain_ref(P, *lv)
    g64 = torch.autograd.grad((y64 * cots["y"]).sum() + (rgb64 * cots["rgb"]).sum(), lv + R.param_list(m, P))
    lv2 = ref_leaves()
    _, rgb2 = C.g_chain_ref(P, *lv2)
    pen64, _, len64 = R.path_regularize(rgb2, lv2[1], torch.zeros((), dtype=F64), cots["img_noise"])
    gp64 = torch.autograd.grad(pen64, R.param_list(m, P), allow_unused=True)

    m = m.cuda()
    params = list(m.parameters())
    leaves = [_dev(ins[k]).requires_grad_(True) for k in keys]
    y, rgb = m(*leaves)
    for n, a, b in (("y", y, y64), ("rgb", rgb, rgb64)):
        e = rel_err(a, b)
        print(name, n, e)
        assert e < TOL, (name, n, e)
    grads = torch.autograd.grad((y * _dev(cots["y"])).sum() + (rgb * _dev(cots["rgb"])).sum(), leaves + params)
    _elementwise(name + " first order", list(keys) + pnames, grads, g64, GTOL)
    leaves = [_dev(ins[k]).requires_grad_(k == "lat") for k in keys]
    with second_order():
        _, rgb = m(*leaves)
        pen, _, lengths = g_path_regularize(rgb, leaves[1], torch.zeros((), device="cuda"), noise=_dev(cots["img_noise"]))
        gp = torch.autograd.grad(pen, params, allow_unused=True)
    e = rel_err(lengths, len64)
    print(name, "penalty", float(pen.detach()), float(pen64.detach()), "lengths", e)
    assert e < GTOL and abs(float(pen.detach()) - float(pen64.detach())) <= 2e-4 * abs(float(pen64.detach()))
    _elementwise(name + " path penalty", pnames, gp, gp64, GTOL2)


@pytest.mark.parametrize("route", ["default", "min_blocks_1"])
@pytest.mark.parametrize("name", list(C.D_CHAINS))
def test_d_chain_elementwise_first_order_and_r1(name, route, monkeypatch):
    """ConvLayer(3, 32, 1) -> ResBlock(32, 64) -> minibatch stddev -> ConvLayer(65, 64, 3), per-sample score (y * cot).sum((1, 2, 3)):
    first order and d_r1_loss, on the default dispatch and with BLUR_CONV_MIN_BLOCKS = 1.  Which body ran is asserted through
    down_pair_ok and a count of the calls of ``down_pair``: at 12 x 12 the 6 x 6 block output is below the fused kernel's 8 x 16
    output patch and the layer-by-layer body runs either way; at 16 x 32 the lowered threshold switches to the fused blur +
    stride-2 body."""
    import ideas_amd.models as M
    import ideas_amd.op.conv as cv
    from ideas_amd.utils import d_r1_loss
    m, x, cot = C.d_chain_case(name)
    assert C.d_chain_fragile(name)[0] == 0
    pnames = [n for n, _ in m.named_parameters()]
    P = R.params_of(m)
    score64 = lambda xx: (C.d_chain_ref(P, xx) * cot).sum((1, 2, 3))
    x1 = x.clone().requires_grad_(True)
    y64 = C.d_chain_ref(P, x1)
    g64 = torch.autograd.grad((y64 * cot).sum(), [x1] + R.param_list(m, P))
    x2 = x.clone().requires_grad_(True)
    r1_64 = R.d_r1_loss(score64(x2), x2)
    gr64 = torch.autograd.grad(r1_64, R.param_list(m, P), allow_unused=True)

    m = m.cuda()
    params = list(m.parameters())
    if route == "min_blocks_1":
        monkeypatch.setattr(cv, "BLUR_CONV_MIN_BLOCKS", 1)
    xd = _dev(x).requires_grad_(True)
    with torch.no_grad():
        h = m.stem(xd)
    c1, c2, blur = m.block.conv1[0], m.block.conv2[1], m.block.conv2[0]
    fused = cv.down_pair_ok(h, c1.weight, c2.weight, blur.kernel, blur.pad, c1.padding)
    assert fused == (route == "min_blocks_1" and name == "16x32"), (name, route, fused)
    pairs = []
    down_pair = M.down_pair
    monkeypatch.setattr(M, "down_pair", lambda *a, **k: (pairs.append(1), down_pair(*a, **k))[1])
    y = m(xd)
    assert (m.block._fused_body() is not None and m.block._body_pair_ok(h)) == fused
    assert len(pairs) == int(fused)
    e = rel_err(y, y64)
    print(name, route, "y", e)
    assert e < TOL, (name, route, e)
    cd = _dev(cot)
    grads = torch.autograd.grad((y * cd).sum(), [xd] + params)
    _elementwise("D %s %s first" % (name, route), ["x"] + pnames, grads, g64, GTOL)
    x2d = _dev(x).requires_grad_(True)
    r1 = d_r1_loss((m(x2d) * cd).sum((1, 2, 3)), x2d)
    assert len(pairs) == 2 * int(fused)
    print(name, route, "r1", float(r1.detach()), float(r1_64.detach()))
    assert abs(float(r1.detach()) - float(r1_64.detach())) <= 2e-4 * abs(float(r1_64.detach()))
    gr = torch.autograd.grad(r1, params, allow_unused=True)
    _elementwise("D %s %s r1" % (name, route), pnames, gr, gr64, GTOL2)
