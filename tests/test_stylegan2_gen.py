"""Host-side checks of the StyleGAN2 generator side (stylegan2/model.py:14-72, 280-581): constructors / state dicts / seeded initial
values against the reference's (tests/golden/stylegan2_gen.npz, written by tests/golden/make_golden_stylegan2_gen.py), the C ABI of the
fused noise + bias + activation kernels, and the argument errors.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT, Golden

GEN_NAMES = ("PixelNorm", "Upsample", "Downsample", "NoiseInjection", "ConstantInput", "StyledConv", "ToRGB", "Generator")


@pytest.fixture(scope="module")
def gold():
    return Golden("stylegan2_gen.npz")


def _seeded(size, meta):
    from ideas_amd.model import Generator
    init = meta["init"]
    torch.manual_seed(init["seed"])
    return Generator(size, init["style_dim"], init["n_mlp"])


def test_layers_are_importable_from_the_layer_library():
    import ideas_amd.model as L
    import ideas_amd.stylegan2_gen as SG
    import ideas_amd.op as op
    for name in GEN_NAMES:
        assert getattr(L, name) is getattr(SG, name), name
    from ideas_amd.model import Generator, StyledConv, ToRGB            # noqa: F401
    assert L.StyledConv is not L.StyledConv_without_noise
    assert "noise_bias_act" in op.__all__ and callable(op.noise_bias_act)
    with pytest.raises(AttributeError):
        L.no_such_layer


@pytest.mark.parametrize("size", [8, 16])
def test_constructor_matches_the_reference(gold, size):
    meta = gold.json("meta")
    init = meta["init"]["sizes"][str(size)]
    net = _seeded(size, meta)
    sd = net.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == init["keys"]
    assert len(sd) == {8: 33, 16: 51}[size]
    assert [k for k, _ in net.named_parameters()] == init["param_keys"]          # creation order
    assert sum(p.numel() for p in net.parameters()) == init["n_params"]
    for k, v in sd.items():                                                      # same draws in the same order
        s, a = init["checksums"][k]
        assert abs(float(v.double().sum()) - s) <= 1e-9 * max(1.0, a), k
        assert abs(float(v.double().abs().sum()) - a) <= 1e-9 * max(1.0, a), k
    assert repr(net) == init["repr"]
    assert (net.n_latent, net.num_layers, net.log_size) == (init["n_latent"], init["num_layers"], init["log_size"])
    assert net.size == size and net.style_dim == 32 and net.channels[4] == 512 and net.channels[1024] == 32
    assert len(net.convs) == 2 * (net.log_size - 2) and len(net.to_rgbs) == net.log_size - 2 and len(net.upsamples) == 0
    assert [tuple(b.shape) for b in net.noises.buffers()] == [tuple(n.shape) for n in net.make_noise()]


def test_state_dict_keys_are_the_documented_ones(gold):
    keys = {k for k, _ in gold.json("meta")["init"]["sizes"]["8"]["keys"]}
    styled = lambda p: {f"{p}.conv.weight", f"{p}.conv.modulation.weight", f"{p}.conv.modulation.bias", f"{p}.noise.weight",
                        f"{p}.activate.bias"}
    rgb = lambda p: {f"{p}.conv.weight", f"{p}.conv.modulation.weight", f"{p}.conv.modulation.bias", f"{p}.bias"}
    want = ({"style.1.weight", "style.1.bias", "style.2.weight", "style.2.bias", "input.input", "convs.0.conv.blur.kernel",
             "to_rgbs.0.upsample.kernel", "noises.noise_0", "noises.noise_1", "noises.noise_2"}
            | styled("conv1") | styled("convs.0") | styled("convs.1") | rgb("to_rgb1") | rgb("to_rgbs.0"))
    assert keys == want


def test_reference_shaped_state_dict_loads_strict(gold):
    from ideas_amd.model import Generator, ModulatedConv2d
    keys = gold.json("meta")["init"]["sizes"]["8"]["keys"]
    g = torch.Generator().manual_seed(1)
    ref = {k: torch.randn(shape, generator=g) for k, shape in keys}              # NCHW-contiguous, as a reference checkpoint holds them
    net = Generator(8, 32, 2)
    res = net.load_state_dict(ref, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in net.state_dict().items():
        assert torch.equal(v, ref[k]), k
    n5 = 0
    for m in net.modules():                                                      # 5-D weights stay in the kernels' memory order
        if isinstance(m, ModulatedConv2d):
            w = m.weight
            assert w.dim() == 5
            w4 = w[0].transpose(0, 1) if m.upsample else w[0]
            assert w4.is_contiguous(memory_format=torch.channels_last), (m, w.stride())
            n5 += 1
    assert n5 == 5


def test_layer_signatures(gold):
    from ideas_amd.model import Downsample, StyledConv, ToRGB, Upsample
    meta = gold.json("meta")
    for c in meta["sc"]:
        m = StyledConv(c["cin"], c["cout"], 3, 16, upsample=c["upsample"])
        assert [n for n, _ in m.named_parameters()] == c["params"]
        assert [n for n, _ in m.named_children()] == ["conv", "noise", "activate"]
        assert set(m.state_dict()) == {k[len(f"{c['tag']}/sd/"):] for k in gold.keys() if k.startswith(f"{c['tag']}/sd/")}
        assert tuple(m.noise.weight.shape) == (1,) and float(m.noise.weight.detach()) == 0.0
    for c in meta["rgb"]:
        m = ToRGB(8, 16, upsample=c["upsample"])
        assert [n for n, _ in m.named_parameters()] == c["params"]
        assert hasattr(m, "upsample") == c["upsample"] and tuple(m.bias.shape) == (1, 3, 1, 1)
    for tag, cls in (("up", Upsample), ("down", Downsample)):
        m = cls([1, 3, 3, 1])
        assert list(m.pad) == meta[tag]["pad"] and m.factor == 2
        assert torch.allclose(m.kernel, torch.tensor(meta[tag]["kernel"]), rtol=0, atol=1e-7)


def test_pixel_norm_and_constant_input_on_the_cpu(gold):
    from ideas_amd.model import ConstantInput, PixelNorm
    x = gold.t("pn/x").requires_grad_(True)
    y = PixelNorm()(x)
    assert torch.allclose(y, gold.t("pn/y"), rtol=1e-6, atol=1e-7)
    (gx,) = torch.autograd.grad(y, x, gold.t("pn/cot"))
    assert torch.allclose(gx, gold.t("pn/g_x"), rtol=1e-5, atol=1e-6)
    c = ConstantInput(6)
    out = c(torch.zeros(3, 32))
    assert tuple(out.shape) == (3, 6, 4, 4) and out.data_ptr() == c.input.data_ptr()          # expanded, not copied
    assert torch.equal(out[2], c.input[0])


def test_path_regularize_takes_3d_latents():
    """[B, n_latent, D]: sum over the last axis, mean over the latent axis (stylegan2/train.py:92); [B, D] as before."""
    from ideas_amd.train_step import g_path_regularize
    g = torch.Generator().manual_seed(5)
    a = torch.randn(3 * 8 * 8, 4 * 6, generator=g, dtype=torch.float64)
    noise = torch.randn(2, 3, 8, 8, generator=g, dtype=torch.float64)
    lat = torch.randn(2, 4, 6, generator=g, dtype=torch.float64, requires_grad=True)
    img = (lat.reshape(2, 24) @ a.t()).reshape(2, 3, 8, 8)
    pen, mean, lengths = g_path_regularize(img, lat, torch.tensor(0.0, dtype=torch.float64), noise=noise)
    grad = ((noise / 8.0).reshape(2, -1) @ a).reshape(2, 4, 6)
    want = grad.pow(2).sum(2).mean(1).sqrt()
    assert tuple(lengths.shape) == (2,) and torch.allclose(lengths, want, rtol=1e-12)
    assert torch.allclose(mean, 0.01 * want.mean(), rtol=1e-12)
    assert torch.allclose(pen, (want - 0.01 * want.mean()).pow(2).mean(), rtol=1e-12)
    lat2 = lat.detach().reshape(2, 24).requires_grad_(True)
    _, _, l2 = g_path_regularize((lat2 @ a.t()).reshape(2, 3, 8, 8), lat2, torch.tensor(0.0, dtype=torch.float64), noise=noise)
    assert torch.allclose(l2, grad.reshape(2, 24).pow(2).sum(1).sqrt(), rtol=1e-12)


# ------------------------------------------------------------------------------------------------- C ABI and errors
ENTRY_POINTS = ("ideas_noise_bias_act", "ideas_noise_bias_act_bwd")


def test_c_abi_declares_and_exports_the_kernels():
    from ideas_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ideas_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 4 and _lib.load().ideas_abi_version() == 4        # additive within ABI 4
    assert int(re.search(r"#define\s+IDEAS_NOISE_ACT_MAX_PARTIALS\s+(\d+)", hdr).group(1)) == _lib.NOISE_ACT_MAX_PARTIALS
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in doc for name in ENTRY_POINTS)


def test_c_abi_argument_checks_run_before_any_launch():
    """NULL pointers, non-positive sizes, dtypes without a kernel and a noise batch other than 1 or B are answered by the checks in
    front of the launch (no device needed: the pointers are host buffers a launch would never survive)."""
    from ideas_amd import _lib
    lib = _lib.load()
    E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
    buf = ctypes.create_string_buffer(256)
    a = ctypes.addressof(buf)

    def fwd(out=a, x=a, noise=a, nw=a, bias=a, B=2, C=8, H=4, W=4, nb=2, dtype=_lib.F32):
        return lib.ideas_noise_bias_act(out, x, noise, nw, bias, B, C, H, W, nb, 0.2, 1.0, dtype, None)

    def bwd(gx=a, gb=a, gnw=a, gn=a, ws=a, gy=a, out=a, noise=a, nw=a, B=2, C=8, H=4, W=4, nb=2, dtype=_lib.F32):
        return lib.ideas_noise_bias_act_bwd(gx, gb, gnw, gn, ws, gy, out, noise, nw, B, C, H, W, nb, 0.2, 1.0, dtype, None)
    for f in (fwd, bwd):
        assert f(B=0) == E_SHAPE and f(C=0) == E_SHAPE and f(H=-1) == E_SHAPE and f(W=0) == E_SHAPE
        assert f(nb=3) == E_SHAPE and f(nb=0) == E_SHAPE and f(B=4, nb=2) == E_SHAPE
        assert f(dtype=_lib.F16) == E_UNSUPPORTED and f(dtype=_lib.F64) == E_UNSUPPORTED and f(dtype=17) == E_UNSUPPORTED
        assert f(noise=None) == E_NULL and f(nw=None) == E_NULL and f(out=None) == E_NULL
    assert fwd(x=None) == E_NULL and fwd(bias=None) == E_NULL
    assert bwd(gx=None) == E_NULL and bwd(gnw=None) == E_NULL and bwd(ws=None) == E_NULL and bwd(gy=None) == E_NULL


def test_cpu_tensors_fail_loudly():
    import ideas_amd.op as op
    from ideas_amd.model import Downsample, Generator, NoiseInjection, StyledConv, ToRGB, Upsample
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.noise_bias_act(torch.zeros(2, 8, 4, 4), torch.zeros(2, 1, 4, 4), torch.zeros(1), torch.zeros(8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        StyledConv(8, 8, 3, 16)(torch.zeros(2, 8, 4, 4), torch.zeros(2, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ToRGB(8, 16)(torch.zeros(2, 8, 4, 4), torch.zeros(2, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Upsample([1, 3, 3, 1])(torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Downsample([1, 3, 3, 1])(torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Generator(8, 32, 2)([torch.zeros(2, 32)])
    out = NoiseInjection()(torch.ones(2, 3, 4, 4), noise=torch.ones(2, 1, 4, 4))         # plain torch: weight = 0 -> identity
    assert torch.equal(out, torch.ones(2, 3, 4, 4))


def test_op_refuses_malformed_arguments():
    """Shape errors are raised before the device check, so they show on any host."""
    import ideas_amd.op as op
    x, nz, nw, b = torch.zeros(2, 8, 4, 4), torch.zeros(2, 1, 4, 4), torch.zeros(1), torch.zeros(8)
    for args in ((x[0], nz, nw, b), (x, torch.zeros(3, 1, 4, 4), nw, b), (x, torch.zeros(2, 1, 4, 5), nw, b), (x, torch.zeros(2, 2, 4, 4), nw, b),
                 (x, nz, torch.zeros(2), b), (x, nz, nw, torch.zeros(7))):
        with pytest.raises(RuntimeError):
            op.noise_bias_act(*args)
