"""GPU parity of perceptual path length: ``op.path_endpoints`` (lerp bitwise against its composition, slerp against the reference's
f64 values), ``op.pair_prepare`` (bitwise in the identity case, against ``F.interpolate`` + the scaling otherwise), the C ABI's
refusals, ``ppl.path_distances`` against what the reference computed in f64 (tests/golden/ppl.npz) and against the unfused path on
the same device, and the two command lines.

Tolerances.  Exact where the arithmetic is the same (``torch.equal``).  Against the reference: the rule of tests/test_lpips_gpu.py,
``max(1e-5, 4 x the reference's own f32-from-f64 deviation)``.  The deviations tests/golden/make_golden_ppl.py printed (stored as
``*/f32_dev``): slerp rows 9.2e-8 .. 1.5e-7; distances ``w_e4`` 3.4e-4, ``w_e2`` 9.9e-6, ``wcrop_e4`` 7.1e-4, ``z_e4`` 3.3e-3,
``z_e2`` 3.4e-5 (at eps = 1e-4 the f32 rounding of t + eps alone moves the step by up to 6e-4 of its length).  The resize: 1e-5 (f32)
and 6e-3 (bf16) of the largest element, what tests/test_ops_gpu.py::test_patchify_random_vs_oracle allows ``ideas_patch_resize`` for the
same arithmetic.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, Golden, rel_err
import lpips_ref as LR

pytestmark = pytest.mark.gpu
CL = torch.channels_last
BF = torch.bfloat16
TOL = 1e-5                                   # tests/test_lpips_gpu.py::TOL
RESIZE_TOL = {torch.float32: 1e-5, BF: 6e-3}
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
_ids = lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c).replace("torch.", "")


@pytest.fixture(scope="module")
def gold():
    return Golden("ppl.npz")


@pytest.fixture(scope="module")
def op():
    import ideas_amd.op as op
    return op


def _consts():
    sh = torch.tensor(SHIFT, device="cuda").view(1, 3, 1, 1)
    sc = torch.tensor(SCALE, device="cuda").view(1, 3, 1, 1)
    return sh, sc


# ------------------------------------------------------------------------------------------------- op.path_endpoints
@pytest.mark.parametrize("D", (1, 32, 100, 512))
@pytest.mark.parametrize("B", (1, 3, 64))
def test_path_endpoints_lerp_is_bitwise_the_composition(op, B, D):
    """D = 1: one lane; 32: 16-byte vectors in 8 lanes; 100: vectors in 25 lanes, no multiple of a wave; 512: two vectors a lane.
    B = 3: a block with an idle wave; 64: sixteen blocks.  (The element path: the misaligned view below.)"""
    from ideas_amd.op.ppl import path_endpoints_composition
    g = torch.Generator().manual_seed(100 * B + D)
    lat = torch.randn(2 * B, D, generator=g).cuda()
    t = torch.rand(B, generator=g).cuda()
    for eps in (1e-4, 1e-2):
        got = op.path_endpoints(lat, t, eps, "lerp")
        want = path_endpoints_composition(lat, t, eps, "lerp")
        assert got.dtype == torch.float32 and got.shape == lat.shape
        assert torch.equal(got, want)
        a, b = lat[::2], lat[1::2]                               # the rows, spelled out: 2i at t, 2i + 1 at t + eps (an f32 sum)
        assert torch.equal(got[::2], a + (b - a) * t[:, None])
        assert torch.equal(got[1::2], a + (b - a) * (t[:, None] + eps))
        assert D == 1 or not torch.equal(got[::2], got[1::2])
    assert torch.equal(op.path_endpoints(lat, t, 1e-4, 0), op.path_endpoints(lat, t, 1e-4, "lerp"))


def test_path_endpoints_takes_the_element_path_on_a_misaligned_view(op):
    """D = 32 behind an offset of one float: the rows are not 16-byte aligned.  lerp gives the same bits; slerp adds its row sums in
    another order (one element a lane, not four)."""
    g = torch.Generator().manual_seed(9)
    base = torch.randn(6 * 32 + 1, generator=g).cuda()
    lat = base[1:].view(6, 32)
    t = torch.rand(3, generator=g).cuda()
    assert lat.data_ptr() % 16 != 0
    assert torch.equal(op.path_endpoints(lat, t, 1e-4, "lerp"), op.path_endpoints(lat.clone(), t, 1e-4, "lerp"))
    assert rel_err(op.path_endpoints(lat, t, 1e-4, "slerp"), op.path_endpoints(lat.clone(), t, 1e-4, "slerp")) < TOL


@pytest.mark.parametrize("D", (67, 130, 4095, 4096))
def test_path_endpoints_element_path_and_the_cap(op, D):
    """D % 4 != 0: one element a lane and chunk (67: two chunks, the second in 3 lanes; 4095: all 64).  4096: the cap, 16 vectors a
    lane.  lerp bitwise; slerp against the composition in f64 on the same rows."""
    from ideas_amd.op.ppl import path_endpoints_composition
    g = torch.Generator().manual_seed(D)
    lat = torch.randn(10, D, generator=g).cuda()
    t = torch.rand(5, generator=g).cuda()
    assert torch.equal(op.path_endpoints(lat, t, 1e-4, "lerp"), path_endpoints_composition(lat, t, 1e-4, "lerp"))
    got = op.path_endpoints(lat, t, 1e-2, "slerp")
    e = rel_err(got, path_endpoints_composition(lat.double(), t.double(), 1e-2, "slerp"))
    print(D, "slerp", e)
    assert e < TOL, e
    with pytest.raises(RuntimeError, match="at most 4096"):
        op.path_endpoints(torch.zeros(2, 4097, device="cuda"), t[:1], 1e-4, "lerp")


def test_path_endpoints_slerp_against_the_reference(gold, op):
    meta = gold.json("meta")["interp"]
    for d, b in meta["cases"]:
        tag = f"interp/{d}_{b}"
        bound = max(TOL, 4 * float(gold.z[f"{tag}/f32_dev"][0]))
        lat, t = gold.t(f"{tag}/lat").cuda(), gold.t(f"{tag}/t").cuda()
        got = op.path_endpoints(lat, t, meta["eps"], "slerp")
        e = rel_err(got, gold.t(f"{tag}/slerp"))
        norm = float((got.double().pow(2).sum(-1).sqrt() - 1).abs().max())
        print(tag, "slerp", e, "unit norm", norm, "bound", bound)
        assert e < bound, (tag, e)
        assert norm < bound, (tag, norm)
        assert torch.equal(got, op.path_endpoints(lat, t, meta["eps"], 1))
        # the step between the two rows of a path, which is what PPL measures, against the reference's
        ref = gold.t(f"{tag}/slerp").double()
        step, ref_step = got.double().cpu()[1::2] - got.double().cpu()[::2], ref[1::2] - ref[::2]
        print(tag, "step", rel_err(step, ref_step))


def test_path_endpoints_slerp_of_identical_ends_is_nan_as_in_the_reference(op):
    from ideas_amd.op.ppl import path_endpoints_composition
    g = torch.Generator().manual_seed(4)
    lat = torch.randn(4, 64, generator=g)
    lat[0] = 0                                                   # four equal entries: norm 3, direction 0.5, the dot product 1 exactly
    lat[0, 7:11] = 1.5
    lat[1] = lat[0]
    lat, t = lat.cuda(), torch.tensor([0.25, 0.5]).cuda()
    got, want = op.path_endpoints(lat, t, 1e-4, "slerp"), path_endpoints_composition(lat, t, 1e-4, "slerp")
    assert bool(torch.isnan(want[:2]).all()) and bool(torch.isnan(got[:2]).all())
    assert bool(torch.isfinite(got[2:]).all()) and rel_err(got[2:], want[2:].double()) < TOL


def test_f64_takes_the_compositions(op):
    from ideas_amd.op.ppl import pair_prepare_composition, path_endpoints_composition
    lat = torch.randn(6, 20, dtype=torch.float64, device="cuda")
    t = torch.rand(3, dtype=torch.float64, device="cuda")
    assert torch.equal(op.path_endpoints(lat, t, 1e-4, "slerp"), path_endpoints_composition(lat, t, 1e-4, "slerp"))
    x = torch.randn(4, 3, 8, 8, dtype=torch.float64, device="cuda")
    assert torch.equal(op.pair_prepare(x, (1, 2, 4, 4), (6, 6), SHIFT, SCALE), pair_prepare_composition(x, (1, 2, 4, 4), (6, 6), SHIFT, SCALE))


def test_ops_are_forward_only(op):
    lat = torch.randn(4, 8, device="cuda", requires_grad=True)
    with pytest.raises(RuntimeError, match="forward only"):
        op.path_endpoints(lat, torch.rand(2, device="cuda"), 1e-4, "lerp")
    x = torch.randn(2, 3, 8, 8, device="cuda", requires_grad=True)
    with pytest.raises(RuntimeError, match="forward only"):
        op.pair_prepare(x, (0, 0, 8, 8), (8, 8), SHIFT, SCALE)
    with torch.no_grad():
        assert not op.pair_prepare(x, (0, 0, 8, 8), (8, 8), SHIFT, SCALE).requires_grad


# ------------------------------------------------------------------------------------------------- op.pair_prepare
def _layout(x, layout):
    return x.contiguous(memory_format=CL) if layout == "nhwc" else x.contiguous()


def _split(x):
    return torch.cat([x[::2], x[1::2]], 0)


@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
@pytest.mark.parametrize("dtype", (torch.float32, BF), ids=_ids)
@pytest.mark.parametrize("case", (((6, 3, 20, 12), None), ((4, 3, 16, 16), 2)), ids=("whole", "pplcrop"))
def test_pair_prepare_identity_is_bitwise_the_scaling_layer(op, case, dtype, layout):
    """A box of the output's size: taps (1, 0), so the result is ``(x - shift) / scale`` (f32 arithmetic, rounded once for bf16) of the
    cropped pixels, even samples first."""
    from ideas_amd.op.ppl import pair_prepare_composition
    shape, c = case
    g = torch.Generator().manual_seed(sum(shape))
    x = _layout(torch.randn(*shape, generator=g).to(dtype).cuda(), layout)
    h, w = shape[2], shape[3]
    box = (0, 0, h, w) if c is None else (3 * c, 2 * c, 4 * c, 4 * c)
    got = op.pair_prepare(x, box, (box[2], box[3]), SHIFT, SCALE)
    sh, sc = _consts()
    crop = x[:, :, box[0]:box[0] + box[2], box[1]:box[1] + box[3]]
    want = _split(((crop.float() - sh) / sc).to(dtype))
    assert got.dtype == dtype and tuple(got.shape) == (shape[0], 3, box[2], box[3]) and got.is_contiguous(memory_format=CL)
    assert torch.equal(got, want)
    assert torch.equal(got, pair_prepare_composition(x, box, (box[2], box[3]), SHIFT, SCALE))
    if dtype == torch.float32:                                   # the module itself
        from ideas_amd.lpips import ScalingLayer
        assert torch.equal(got, _split(ScalingLayer().cuda()(crop)))


@pytest.mark.parametrize("dtype", (torch.float32, BF), ids=_ids)
@pytest.mark.parametrize("crop", (False, True), ids=("whole", "crop"))
@pytest.mark.parametrize("sizes", ((32, 16), (32, 8), (24, 16)), ids=_ids)
def test_pair_prepare_resize_against_interpolate(op, sizes, crop, dtype):
    src, dst = sizes
    n = src * 2 if crop else src                                 # the PPL crop of an image twice the size is src x src
    g = torch.Generator().manual_seed(src + dst)
    x = torch.randn(6, 3, n, n, generator=g).to(dtype).cuda().contiguous(memory_format=CL)
    c = n // 8
    box = (3 * c, 2 * c, 4 * c, 4 * c) if crop else (0, 0, n, n)
    assert box[2] == src
    got = op.pair_prepare(x, box, (dst, dst), SHIFT, SCALE)
    sh, sc = _consts()
    view = x[:, :, box[0]:box[0] + box[2], box[1]:box[1] + box[3]].float()
    want = _split((F.interpolate(view, size=(dst, dst), mode="bilinear", align_corners=False) - sh) / sc)
    e = rel_err(got, want)
    print(sizes, crop, dtype, e)
    assert tuple(got.shape) == (6, 3, dst, dst) and got.dtype == dtype
    assert e < RESIZE_TOL[dtype], e


# ------------------------------------------------------------------------------------------------- C ABI
def test_c_abi_refusals_come_before_any_launch():
    """Every pointer is a host buffer that a launch would not survive."""
    from ideas_amd import _lib
    lib = _lib.load()
    E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
    buf = ctypes.create_string_buffer(256)
    a = ctypes.addressof(buf)
    f3 = (ctypes.c_float * 3)(1.0, 1.0, 1.0)

    def ends(out=a, lat=a, t=a, B=2, D=8, mode=0):
        return lib.ideas_path_endpoints(out, lat, t, 1e-4, B, D, mode, None)

    def prep(y=a, x=a, box=(0, 0, 4, 4), shift=f3, scale=f3, B=1, C=3, H=8, W=8, oh=4, ow=4, dtype=_lib.F32):
        bx = None if box is None else (ctypes.c_int * 4)(*box)
        return lib.ideas_pair_prepare(y, x, bx, shift, scale, B, C, H, W, oh, ow, dtype, None)
    assert all(ends(**{k: None}) == E_NULL for k in ("out", "lat", "t"))
    assert ends(B=0) == E_SHAPE and ends(B=-1) == E_SHAPE and ends(D=0) == E_SHAPE
    assert ends(D=_lib.PATH_MAX_DIM + 1) == E_UNSUPPORTED and ends(D=1 << 20) == E_UNSUPPORTED
    assert ends(mode=2) == E_UNSUPPORTED and ends(mode=-1) == E_UNSUPPORTED
    assert all(prep(**{k: None}) == E_NULL for k in ("y", "x", "box", "shift", "scale"))
    assert prep(C=1) == E_UNSUPPORTED and prep(C=4) == E_UNSUPPORTED
    assert prep(dtype=_lib.F16) == E_UNSUPPORTED and prep(dtype=_lib.F64) == E_UNSUPPORTED
    assert prep(B=0) == E_SHAPE and prep(H=0) == E_SHAPE and prep(oh=0) == E_SHAPE and prep(ow=-1) == E_SHAPE
    for box in ((5, 0, 4, 4), (0, 5, 4, 4), (-1, 0, 4, 4), (0, 0, 9, 4), (0, 0, 4, 0), (0, 0, -2, 4)):
        assert prep(box=box) == E_SHAPE, box


# ------------------------------------------------------------------------------------------------- ppl.path_distances
@pytest.fixture(scope="module")
def percept(gold):
    from ideas_amd.lpips import PerceptualLoss
    lin = {f"lin{k}.model.1.weight": gold.t(f"lin/{k}").reshape(1, -1, 1, 1) for k in range(5)}
    return PerceptualLoss(model="net-lin", net="vgg", backbone=LR.backbone_state(), lin_weights=lin).cuda()


@pytest.fixture(scope="module")
def gens(gold):
    from ideas_amd.model import Generator
    nets = {}
    for size in (32, 64):
        meta = gold.json("meta")[f"gen{size}"]
        torch.manual_seed(meta["seed"])
        net = Generator(meta["size"], meta["style_dim"], meta["n_mlp"])
        sums = LR.checksums(net.state_dict())
        for k, (s, a) in meta["checksums"].items():
            assert sums[k][0] == pytest.approx(s, rel=1e-5, abs=1e-5) and sums[k][1] == pytest.approx(a, rel=1e-5), k
        pre = f"gen{size}/fill/"
        named = dict(net.named_parameters())
        fill = {k[len(pre):]: gold.t(k) for k in gold.keys() if k.startswith(pre)}
        assert set(fill) == {n for n in named if n.endswith("bias") or n.endswith("noise.weight")}
        with torch.no_grad():
            for n, v in fill.items():
                named[n].copy_(v)
        nets[size] = net.eval().cuda()
    return nets


def _case(gold, tag):
    meta = {c["tag"]: c for c in gold.json("meta")["cases"]}[tag]
    noise = [gold.t(f"{tag}/noise{i}").cuda() for i in range(meta["n_noises"])]
    return meta, gold.t(f"{tag}/z").cuda(), gold.t(f"{tag}/t").cuda(), noise


def _unfused(g, percept, z, t, noise, space, eps, crop, resize_to):
    """The reference's per-batch steps on this package's modules, launch by launch: slices, interpolation, stack, G, crop,
    ``F.interpolate``, ``image[::2]`` / ``image[1::2]``, ``percept(a, b)``."""
    from ideas_amd.ppl import lerp, slerp
    with torch.no_grad():
        if space == "w":
            latent = g.get_latent(z)
            a, b = latent[::2], latent[1::2]
            latent_e = torch.stack([lerp(a, b, t[:, None]), lerp(a, b, t[:, None] + eps)], 1).view(*latent.shape)
        else:
            a, b = z[::2], z[1::2]
            latent_e = g.get_latent(torch.stack([slerp(a, b, t[:, None]), slerp(a, b, t[:, None] + eps)], 1).view(*z.shape))
        image, _ = g([latent_e], input_is_latent=True, noise=noise)
        if crop:
            c = image.shape[2] // 8
            image = image[:, :, c * 3:c * 7, c * 2:c * 6]
        if image.shape[2] // resize_to > 1:
            image = F.interpolate(image, size=(resize_to, resize_to), mode="bilinear", align_corners=False)
        return percept(image[::2], image[1::2]).view(image.shape[0] // 2) / (eps ** 2)


CASE_TAGS = ("w_e4", "w_e2", "wcrop_e4", "z_e4", "z_e2")


@pytest.mark.parametrize("tag", CASE_TAGS)
def test_path_distances_against_the_reference(gold, percept, gens, tag):
    from ideas_amd.ppl import path_distances
    meta, z, t, noise = _case(gold, tag)
    bound = max(TOL, 4 * float(gold.z[f"{tag}/f32_dev"]))
    got = path_distances(gens[meta["size"]], percept, z, t, noise, space=meta["space"], eps=meta["eps"], crop=meta["crop"])
    assert got.dtype == torch.float32 and tuple(got.shape) == (4,) and not got.requires_grad
    e = rel_err(got, gold.t(f"{tag}/dist"))
    print(tag, "distances", got.tolist(), "rel err", e, "bound", bound)
    assert e < bound, (tag, e, bound)


@pytest.mark.parametrize("tag", CASE_TAGS + ("wcrop_e4_resize16",))
def test_path_distances_against_the_unfused_path(gold, percept, gens, tag):
    """The same bound as against the reference: the two differ in the VGG's batch size, hence possibly in summation order, and in
    z-space in the rounding of slerp.  ``wcrop_e4_resize16``: the inputs of ``wcrop_e4`` on the size-64 generator with ``resize_to=16``,
    with the crop a 32 // 16 = 2-fold and without it a 4-fold resize -- the resize branch without a 512-pixel network.  Its bound is
    that of ``wcrop_e4``: the same generator, inputs and eps, and the resize adds one rounding a pixel to those already there."""
    from ideas_amd.ppl import path_distances
    if tag == "wcrop_e4_resize16":
        meta, z, t, noise = _case(gold, "wcrop_e4")
        runs = [dict(space="w", eps=meta["eps"], crop=True, resize_to=16), dict(space="w", eps=meta["eps"], crop=False, resize_to=16)]
        bound = max(TOL, 4 * float(gold.z["wcrop_e4/f32_dev"]))
    else:
        meta, z, t, noise = _case(gold, tag)
        runs = [dict(space=meta["space"], eps=meta["eps"], crop=meta["crop"], resize_to=256)]
        bound = max(TOL, 4 * float(gold.z[f"{tag}/f32_dev"]))
    g = gens[meta["size"]]
    for kw in runs:
        got = path_distances(g, percept, z, t, noise, **kw)
        want = _unfused(g, percept, z, t, noise, **kw)
        e = rel_err(got, want)
        print(tag, kw, "rel err", e, "bound", bound)
        assert bool(torch.isfinite(got).all()) and e < bound, (tag, kw, e, bound)


def test_path_distances_with_the_generator_in_slices(gold, percept, gens, monkeypatch):
    """``generate_images`` under a byte budget that cuts the 8 images of ``w_e2`` into 3 + 3 + 2 (a pair across two slices): the
    samples are independent, so the distances are those of the single pass, to that case's bound."""
    from ideas_amd import ppl as P
    meta, z, t, noise = _case(gold, "w_e2")
    g = gens[32]
    whole = P.path_distances(g, percept, z, t, noise, space="w", eps=meta["eps"])
    calls = []
    forward = g.forward
    monkeypatch.setattr(g, "forward", lambda styles, **kw: calls.append(styles[0].shape[0]) or forward(styles, **kw))
    monkeypatch.setattr(P, "LAUNCH_BYTES", 6 << 20)              # 2 MiB an image (512 channels at 32 x 32): 16 MiB in 3 slices
    sliced = P.path_distances(g, percept, z, t, noise, space="w", eps=meta["eps"])
    per_sample = [n.expand(8, -1, -1, -1).contiguous() for n in noise]
    sliced2 = P.path_distances(g, percept, z, t, per_sample, space="w", eps=meta["eps"])
    assert calls == [3, 3, 2] * 2
    bound = max(TOL, 4 * float(gold.z["w_e2/f32_dev"]))
    e, e2 = rel_err(sliced, whole), rel_err(sliced2, whole)
    print("sliced generator", e, e2, "bound", bound)
    assert e < bound and e2 < bound, (e, e2)


# ------------------------------------------------------------------------------------------------- command lines
def test_ppl_cli_prints_compute_ppl(gold, percept, tmp_path):
    from ideas_amd.model import Generator
    from ideas_amd.ppl import compute_ppl
    torch.manual_seed(7)
    g = Generator(32, 32, 2)
    torch.save({"g_ema": g.state_dict()}, tmp_path / "g.pt")
    torch.save(LR.backbone_state(), tmp_path / "vgg16.pth")
    torch.save({f"lin{k}.model.1.weight": gold.t(f"lin/{k}").reshape(1, -1, 1, 1) for k in range(5)}, tmp_path / "lin.pth")
    cmd = [sys.executable, os.path.join(ROOT, "ppl.py"), "--space", "w", "--size", "32", "--latent", "32", "--n_mlp", "2", "--n_sample", "6",
           "--batch", "4", "--seed", "1", "--vgg", str(tmp_path / "vgg16.pth"), "--lpips_lin", str(tmp_path / "lin.pth"), str(tmp_path / "g.pt")]
    r = subprocess.run(cmd, cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("ppl: ")]
    assert len(lines) == 1, r.stdout[-2000:]
    want = compute_ppl(g.eval().cuda(), percept, 6, 4, "w", 1e-4, False, seed=1)
    print("ppl.py:", lines[0], "compute_ppl:", want)
    assert float(lines[0][len("ppl: "):]) == want


def test_generate_cli_writes_the_sheets(tmp_path):
    from PIL import Image
    from ideas_amd.model import Generator
    torch.manual_seed(7)
    torch.save({"g_ema": Generator(32, 32, 2).state_dict()}, tmp_path / "g.pt")
    cmd = [sys.executable, os.path.join(ROOT, "generate.py"), "--ckpt", str(tmp_path / "g.pt"), "--size", "32", "--latent", "32", "--n_mlp", "2",
           "--sample", "2", "--pics", "2", "--truncation", "0.7", "--truncation_mean", "16", "--seed", "1", "--out", str(tmp_path / "sample")]
    r = subprocess.run(cmd, cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(tmp_path / "sample")) == ["000000.png", "000001.png"]
    sheets = [Image.open(tmp_path / "sample" / f"00000{i}.png") for i in range(2)]
    for png in sheets:
        assert png.mode == "RGB" and png.size == (32 + 2 * 2, 2 * 32 + 3 * 2)         # (width, height)
    assert np.asarray(sheets[0]).std() > 0 and not np.array_equal(np.asarray(sheets[0]), np.asarray(sheets[1]))
