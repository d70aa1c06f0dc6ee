"""Host-side pins of tests/stylegan2_ref.py, the f64 restatement that tests/test_stylegan2_grads_gpu.py holds the HIP networks to:

* against what the reference's ``Generator`` / ``Discriminator`` computed (tests/golden/stylegan2_gen.npz, stylegan2_disc.npz), with
  the bounds the GPU tests hold against the same goldens;
* ``l2_err`` on pure tensors: what the whole-tensor metric sees and a per-tensor norm does not;
* the mid-width chains of the GPU tests (defined here: modules, seeds, inputs) have NO leaky-ReLU unit within the forward contract
  (1e-5 of the site's largest value) of zero, so a kernel inside its contract cannot flip a mask and elementwise bounds hold.

No GPU: the modules are only constructed (for their seeded weights and state-dict keys), never run."""
import pytest
import torch
from torch import nn

from conftest import Golden, rel_err
import stylegan2_ref as R

TOL, GTOL = 1e-5, 1e-4
DIR_BOUND = 6e-3          # tests/test_nets_gpu.py::DIR_BOUNDS[0], the bound of tests/test_stylegan2_grads_gpu.py


@pytest.fixture(scope="module")
def gold():
    return Golden("stylegan2_gen.npz")


@pytest.fixture(scope="module")
def dgold():
    return Golden("stylegan2_disc.npz")


# ------------------------------------------------------------------------------------------------- seeded networks (CPU)
def seeded_generator(gold, size):
    """The seeded construction and fill of tests/test_stylegan2_gen_gpu.py::_generator, left on the CPU."""
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
    return net


def seeded_disc8(dgold):
    """tests/test_stylegan2_disc_gpu.py::_disc8, left on the CPU."""
    from ideas_amd.model import Discriminator
    torch.manual_seed(dgold.json("meta")["init"]["seed"])
    net = Discriminator(8)
    pre = "disc8/bias/"
    biases = {k[len(pre):]: dgold.t(k) for k in dgold.keys() if k.startswith(pre)}
    named = dict(net.named_parameters())
    assert set(biases) == {n for n in named if n.endswith("bias")}
    with torch.no_grad():
        for n, b in biases.items():
            named[n].copy_(b)
    return net


def seeded_disc16(seed=3):
    """``Discriminator(16)`` from ``seed``, every bias filled with seeded normal values (at zero a bias path is invisible)."""
    from ideas_amd.model import Discriminator
    torch.manual_seed(seed)
    net = Discriminator(16)
    fill_small(net, seed + 1)
    return net


def fill_small(m, seed):
    """Every ``*.bias`` and ``noise.weight`` <- seeded normal values (the fill of tests/golden/make_golden_stylegan2_gen.py)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("bias") or n.endswith("noise.weight"):
                p.copy_(torch.randn(p.shape, generator=g))


def gen_kwargs(gold, tag):
    """(keyword arguments of the settings case ``tag``, number of styles) -- tensors on the CPU."""
    kw = {}
    if tag == "gen8_mix":
        kw["inject_index"] = 2
    if tag == "gen8_trunc":
        kw.update(truncation=0.7, truncation_latent=gold.t("gen8_trunc/truncation_latent"))
    if tag == "gen8_wlat":
        kw["input_is_latent"] = True
    return kw, (2 if tag == "gen8_mix" else 1)


def gen_noise(gold, tag, P):
    """The per-layer noise of a golden case: stored fields for gen8 / gen16, the registered buffers for the settings cases."""
    n = 3 if tag.startswith("gen8") else 5
    if tag in ("gen8", "gen16"):
        return [gold.t(f"{tag}/noise{i}").to(P["input.input"].dtype) for i in range(n)]
    return [P[f"noises.noise_{i}"] for i in range(n)]


def to_dtype(kw, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in kw.items()}


# ------------------------------------------------------------------------------------------------- pins to the reference
def _norms(grads):
    return torch.tensor([0.0 if q is None else float(q.norm()) for q in grads], dtype=torch.float64)


@pytest.mark.parametrize("tag", ["gen8", "gen16", "gen8_bufs", "gen8_mix", "gen8_trunc", "gen8_wlat"])
def test_generator_restatement_vs_reference(gold, tag):
    size = 16 if tag == "gen16" else 8
    net = seeded_generator(gold, size)
    P = R.params_of(net)
    kw, n_styles = gen_kwargs(gold, tag)
    zs = [gold.t(f"{tag}/z{i}").double().requires_grad_(True) for i in range(n_styles)]
    image, latent = R.generator(P, size, zs, gen_noise(gold, tag, P), **to_dtype(kw, torch.float64))
    e = rel_err(image, gold.t(f"{tag}/y"))
    el = rel_err(latent, gold.t(f"{tag}/latent"))
    print(tag, "image", e, "latent", el)
    assert tuple(latent.shape) == (2, 2 * net.log_size - 2, 32)
    assert e < TOL and el < TOL, (tag, e, el)
    grads = torch.autograd.grad((image * gold.t(f"{tag}/cot").double()).sum(), zs + R.param_list(net, P), allow_unused=True)
    for i in range(n_styles):
        e = rel_err(grads[i], gold.t(f"{tag}/g_z{i}"))
        print(tag, "dz%d" % i, e)
        assert e < GTOL, (tag, i, e)
    assert torch.allclose(_norms(grads[n_styles:]), gold.t(f"{tag}/gparam_norms"), rtol=5e-4, atol=1e-6), tag


def test_path_length_restatement_vs_reference(gold):
    net = seeded_generator(gold, 8)
    P = R.params_of(net)
    lat = gold.t("gen8_path/latent").double().requires_grad_(True)
    image, latent = R.generator(P, 8, [lat], gen_noise(gold, "gen8", P), input_is_latent=True)
    assert latent is lat and rel_err(image, gold.t("gen8_path/image")) < TOL
    pen, mean, lengths = R.path_regularize(image, lat, torch.zeros((), dtype=torch.float64), gold.t("gen8_path/img_noise").double())
    ref, got = float(gold.t("gen8_path/penalty")), float(pen.detach())
    assert abs(got - ref) <= 2e-4 * abs(ref), (got, ref)
    assert abs(float(mean) - float(gold.t("gen8_path/mean"))) <= 2e-4 * abs(float(gold.t("gen8_path/mean")))
    e = rel_err(lengths, gold.t("gen8_path/lengths"))
    print("path length: penalty", got, ref, "lengths", e)
    assert e < GTOL, e
    gr = torch.autograd.grad(pen, R.param_list(net, P), allow_unused=True)
    assert torch.allclose(_norms(gr), gold.t("gen8_path/gparam_norms"), rtol=2e-3, atol=1e-8)


@pytest.mark.parametrize("tag", ["disc8_b8", "disc8_b4"])
def test_discriminator_restatement_vs_reference(dgold, tag):
    net = seeded_disc8(dgold)
    P = R.params_of(net)
    params = R.param_list(net, P)
    x = dgold.t(f"{tag}/x").double().requires_grad_(True)
    logits = R.discriminator(P, 8, x)
    e = rel_err(logits, dgold.t(f"{tag}/logits"))
    print(tag, "logits", e)
    assert tuple(logits.shape) == (x.shape[0], 1) and e < TOL, (tag, e)
    grads = torch.autograd.grad(logits.sum(), [x] + params)
    e = rel_err(grads[0], dgold.t(f"{tag}/gx"))
    print(tag, "gx", e)
    assert e < GTOL, (tag, e)
    assert torch.allclose(_norms(grads[1:]), dgold.t(f"{tag}/gparam_norms"), rtol=5e-4, atol=1e-6), tag
    x2 = x.detach().clone().requires_grad_(True)
    r1 = R.d_r1_loss(R.discriminator(P, 8, x2), x2)
    r1_ref, r1_got = float(dgold.t(f"{tag}/r1")), float(r1.detach())
    print(tag, "r1", r1_got, r1_ref)
    assert abs(r1_got - r1_ref) <= 2e-4 * abs(r1_ref), (tag, r1_got, r1_ref)
    gr = torch.autograd.grad(r1, params, allow_unused=True)
    assert torch.allclose(_norms(gr), dgold.t(f"{tag}/r1_gparam_norms"), rtol=2e-3, atol=1e-8), tag


# ------------------------------------------------------------------------------------------------- what l2_err adds to a norm
def test_l2_err_sees_what_a_norm_cannot():
    """A 512 x 512 x 3 x 3 gradient: a sign flip, an in/out transposition and a 180-degree tap flip leave the norm exactly where it
    was and are a relative error of at least 1 as tensors; one zeroed output-channel row (of 512: ~1e-3 of the norm) and one zeroed
    tap of one row (~1e-4) pass the norm check at the second-order rtol 2e-3 and miss the whole-tensor bound by a wide margin."""
    g = torch.randn(512, 512, 3, 3, generator=torch.Generator().manual_seed(1234), dtype=torch.float64)
    norm_ok = lambda a: torch.allclose(a.norm(), g.norm(), rtol=2e-3, atol=1e-8)
    assert R.l2_err(g, g) == 0.0 and R.l2_err(torch.zeros(3), torch.zeros(3)) == 0.0
    assert abs(R.l2_err(2 * g, g) - 1.0) < 1e-12 and R.l2_err(g, torch.zeros_like(g), floor=float(g.norm())) == 1.0
    for name, bad in (("sign", -g), ("transposed", g.transpose(0, 1)), ("taps flipped", g.flip(2, 3))):
        e = R.l2_err(bad, g)
        print(name, e)
        assert e >= 1.0 and norm_ok(bad), (name, e)
    row, tap = g.clone(), g.clone()
    row[17] = 0
    tap[17, :, 1, 2] = 0
    for name, bad in (("row", row), ("tap", tap)):
        e = R.l2_err(bad, g)
        print(name, e, float(bad.norm() / g.norm()) - 1)
        assert e > DIR_BOUND and norm_ok(bad), (name, e)


# ------------------------------------------------------------------------------------------------- the mid-width chains
class GChain(nn.Module):
    """One generator block: StyledConv (upsampling) -> StyledConv -> ToRGB with the upsampled skip; layer i reads ``lat[:, i]``."""

    def __init__(self, cin, cout):
        from ideas_amd.model import StyledConv, ToRGB
        super().__init__()
        self.up = StyledConv(cin, cout, 3, 16, upsample=True)
        self.conv = StyledConv(cout, cout, 3, 16)
        self.rgb = ToRGB(cout, 16)

    def forward(self, x, lat, n1, n2, skip):
        y = self.up(x, lat[:, 0], noise=n1)
        y = self.conv(y, lat[:, 1], noise=n2)
        return y, self.rgb(y, lat[:, 2], skip)


def g_chain_ref(P, x, lat, n1, n2, skip, record=None):
    y = R.styled_conv(P, "up", x, lat[:, 0], n1, upsample=True, record=record)
    y = R.styled_conv(P, "conv", y, lat[:, 1], n2, record=record)
    return y, R.to_rgb(P, "rgb", y, lat[:, 2], skip)


class DChain(nn.Module):
    """Stem -> ResBlock -> minibatch stddev -> 3x3 ConvLayer on the widened tensor."""

    def __init__(self, c0=32, c1=64):
        from ideas_amd.model import ConvLayer, ResBlock
        super().__init__()
        self.stem = ConvLayer(3, c0, 1)
        self.block = ResBlock(c0, c1)
        self.final = ConvLayer(c1 + 1, c1, 3)

    def forward(self, x):
        from ideas_amd.op import minibatch_stddev
        return self.final(minibatch_stddev(self.block(self.stem(x)), 4, 1))


def d_chain_ref(P, x, record=None):
    import mbstd_ref
    y = R.conv_layer_sg2(P, "stem", x, 1, record=record)
    y = R.res_block_sg2(P, "block", y, record=record)
    return R.conv_layer_sg2(P, "final", mbstd_ref.minibatch_stddev(y, 4, 1), 3, record=record)


# (cin, cout, h, seed): Cin % 16 == 0 puts both on the b3 MFMA kernels, Cout = 80 > 64 on conv_b3_tphase_kernel, 5 -> 10 gives
# partial patches.  The seeds are the first (searched on the CPU) with no unit within 1e-5 of its site's largest value.
G_CHAINS = {"64x32x8": (64, 32, 8, 7000), "32x80x5": (32, 80, 5, 7109)}
# (H, W, seed) of the D chain's x [4, 3, H, W].  12 x 12 is the smallest input with partial tiles in every layer; its 6 x 6 block output
# is below the 8 x 16 output patch of the fused blur + stride-2 body (op.conv._blur_conv_plan), which therefore never runs there,
# whatever BLUR_CONV_MIN_BLOCKS says.  16 x 32 is the smallest input at which that body can run: the case for the two body routes.
D_CHAINS = {"12x12": (12, 12, 7203), "16x32": (16, 32, 11278)}


def g_chain_case(name, seed=None):
    """(module on the CPU, f64 inputs dict) of a G chain."""
    cin, cout, h, s = G_CHAINS[name]
    seed = s if seed is None else seed
    torch.manual_seed(seed)
    m = GChain(cin, cout)
    fill_small(m, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    rn = lambda *shape: torch.randn(*shape, generator=g).double()
    ins = dict(x=rn(2, cin, h, h), lat=rn(2, 3, 16), n1=rn(2, 1, 2 * h, 2 * h), n2=rn(2, 1, 2 * h, 2 * h), skip=rn(2, 3, h, h))
    cots = dict(y=rn(2, cout, 2 * h, 2 * h), rgb=rn(2, 3, 2 * h, 2 * h), img_noise=rn(2, 3, 2 * h, 2 * h))
    return m, ins, cots


def d_chain_case(name, seed=None):
    """(module on the CPU, x [4, 3, H, W], cotangent of the [4, 64, H / 2, W / 2] output), f64."""
    h, w, s = D_CHAINS[name]
    seed = s if seed is None else seed
    torch.manual_seed(seed)
    m = DChain()
    fill_small(m, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    x = torch.randn(4, 3, h, w, generator=g).double()
    cot = torch.randn(4, 64, h // 2, w // 2, generator=g).double()
    return m, x, cot


def g_chain_fragile(name, seed=None, tol=TOL):
    m, ins, _ = g_chain_case(name, seed)
    record = []
    with torch.no_grad():
        g_chain_ref(R.params_of(m), ins["x"], ins["lat"], ins["n1"], ins["n2"], ins["skip"], record)
    return R.fragile(record, tol), record


def d_chain_fragile(name, seed=None, tol=TOL):
    m, x, _ = d_chain_case(name, seed)
    record = []
    with torch.no_grad():
        d_chain_ref(R.params_of(m), x, record)
    return R.fragile(record, tol), record


@pytest.mark.parametrize("name", list(G_CHAINS))
def test_g_chain_has_no_fragile_unit(name):
    n, record = g_chain_fragile(name)
    assert len(record) == 2 and sum(v.numel() for v in record) == 2 * 2 * G_CHAINS[name][1] * (2 * G_CHAINS[name][2]) ** 2
    print(name, "smallest |v| / max|v| per site", [float(v.abs().min() / v.abs().max()) for v in record])
    assert n == 0, n


@pytest.mark.parametrize("name", list(D_CHAINS))
def test_d_chain_has_no_fragile_unit(name):
    n, record = d_chain_fragile(name)
    h, w, _ = D_CHAINS[name]
    assert [tuple(v.shape) for v in record] == [(4, 32, h, w), (4, 32, h, w), (4, 64, h // 2, w // 2), (4, 64, h // 2, w // 2)]
    print("D chain", name, ": smallest |v| / max|v| per site", [float(v.abs().min() / v.abs().max()) for v in record])
    assert n == 0, n


def test_fragile_counts_units_near_zero():
    v = torch.tensor([[1.0, -2.0, 1e-7, 0.0], [4.0, -3e-5, 5e-5, 1.0]], dtype=torch.float64)
    assert R.fragile([v], 1e-5) == 3 and R.fragile([v, v[:1]], 1e-5) == 5 and R.fragile([v], 1e-9) == 1
    rec = []
    R._act(v, rec)
    R._act(v[0], None)
    assert len(rec) == 1 and torch.equal(rec[0], v)
