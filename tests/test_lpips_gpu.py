"""GPU parity of LPIPS and the projector: ``op.max_pool2x2`` against ``F.max_pool2d`` on the CPU (exact), ``op.lpips_layer`` against an
f64 restatement on the same rounded operands, ``VGG16Features`` / ``PerceptualLoss`` / ``projector.project`` against what the reference
computed in f64 (tests/golden/lpips.npz), and the command line.

Tolerances.  Ops: 1e-5 forward, 1e-4 gradients, of the largest element (DESIGN.md "Tolerances"); bf16 tensors ``close_bf16``.  Networks:
the rule of tests/test_non_leaking_gpu.py, ``max(1e-5, 4 x the reference's own f32-from-f64 deviation)`` for outputs and ``max(1e-4, 4 x
...)`` for gradients.  The deviations tests/golden/make_golden_lpips.py printed (and stored as ``*/f32_dev``): pair ``near`` taps 5.5e-7,
layers 6.7e-7, val 4.1e-7, d val / d pred 1.07e-5; ``far`` 5.5e-7, 6.1e-8, 8.7e-8, 2.2e-6; ``near01`` 5.8e-7, 3.0e-7, 2.9e-7, 7.9e-6; the
projector replay: losses 7.6e-6 (W) / 6.3e-6 (W+), step-0 latent gradient 8.7e-5 / 6.8e-5, noise gradients 2.0e-6; the update
``latent_in - latent_mean`` of the reference's f32 run against its f64 run 1.3e-4 (W) / 3.2e-4 (W+) in relative L2, no sign flips.
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
from test_bf16_gpu import close_bf16
import lpips_ref as LR

pytestmark = pytest.mark.gpu
CL = torch.channels_last
BF = torch.bfloat16
TOL, GTOL = 1e-5, 1e-4
DTYPES = (torch.float32, BF)
_ids = lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c).replace("torch.", "")


@pytest.fixture(scope="module")
def gold():
    return Golden("lpips.npz")


@pytest.fixture(scope="module")
def op():
    import ideas_amd.op as op
    return op


def fmt(t, layout):
    return t.contiguous(memory_format=CL) if layout == "nhwc" else t.contiguous()


# ------------------------------------------------------------------------------------------------- op.max_pool2x2
# odd extents and the scalar channel path (5, 3), one window, 64 vectors a pixel and more
POOL_CASES = [(2, 8, 6, 6), (1, 5, 7, 5), (2, 64, 9, 4), (1, 3, 2, 2), (2, 512, 3, 3)]


def _pool_check(op, x64, dtype, layout):
    """Forward and backward against F.max_pool2d on the CPU in f64 on the same rounded values: both are exact (a copy)."""
    x = x64.to(dtype)
    ref_in = x.double().requires_grad_(True)
    ref = F.max_pool2d(ref_in, 2, 2)
    g = torch.Generator().manual_seed(5)
    gy = torch.randn(ref.shape, generator=g).to(dtype)
    (ref_gx,) = torch.autograd.grad(ref, ref_in, gy.double())
    xd = fmt(x.cuda(), layout).requires_grad_(True)
    y = op.max_pool2x2(xd)
    (gx,) = torch.autograd.grad(y, xd, fmt(gy.cuda(), layout))
    assert y.dtype == dtype and tuple(y.shape) == tuple(ref.shape) and gx.dtype == dtype and gx.shape == xd.shape
    assert torch.equal(y.double().cpu(), ref.detach())
    assert torch.equal(gx.double().cpu(), ref_gx)


@pytest.mark.parametrize("layout", ("nchw", "nhwc"))
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", POOL_CASES, ids=_ids)
def test_max_pool2x2(op, case, dtype, layout):
    g = torch.Generator().manual_seed(3 + sum(case))
    _pool_check(op, torch.randn(*case, generator=g), dtype, layout)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_max_pool2x2_ties_go_to_the_first_element(op, dtype):
    """Inputs from {0, 1} after a ReLU: most windows tie; forward equal and backward torch.equal to F.max_pool2d's on the CPU."""
    g = torch.Generator().manual_seed(17)
    x = torch.relu(torch.randint(-1, 2, (2, 8, 7, 6), generator=g).float())
    assert set(x.unique().tolist()) == {0.0, 1.0}
    _pool_check(op, x, dtype, "nhwc")
    _pool_check(op, torch.zeros(1, 5, 4, 4), dtype, "nchw")


def test_max_pool2x2_nan_is_the_maximum(op):
    x = torch.tensor([[1.0, float("nan")], [3.0, 2.0]]).view(1, 1, 2, 2).repeat(1, 4, 1, 1)
    xd = x.cuda().requires_grad_(True)
    y = op.max_pool2x2(xd)
    (gx,) = torch.autograd.grad(y, xd, torch.ones_like(y))
    assert bool(torch.isnan(y).all())
    assert torch.equal(gx.cpu(), torch.tensor([[0.0, 1.0], [0.0, 0.0]]).view(1, 1, 2, 2).repeat(1, 4, 1, 1))


def test_f64_takes_the_composition(op):
    x = torch.randn(1, 4, 6, 6, dtype=torch.float64, device="cuda")
    assert torch.equal(op.max_pool2x2(x), F.max_pool2d(x, 2, 2))
    f0 = torch.randn(2, 8, 3, 3, dtype=torch.float64, device="cuda")
    f1, w = torch.randn_like(f0), torch.rand(8, dtype=torch.float64, device="cuda")
    d, _ = LR.lpips_layer_f64(f0.cpu(), f1.cpu(), w.cpu())
    assert rel_err(op.lpips_layer(f0, f1, w), d) < 1e-12


def test_second_order_takes_the_composition(op):
    """Inside ``op.modulated_conv.second_order()`` both ops are torch compositions, so a ``create_graph`` pass can be differentiated
    again (against the same composition in f64 on the CPU); outside it the kernels' backward builds no graph, so a second differentiation raises."""
    from ideas_amd.op.lpips import lpips_layer_composition
    from ideas_amd.op.modulated_conv import second_order
    g = torch.Generator().manual_seed(41)
    x0, x1, wt = torch.randn(2, 8, 6, 6, generator=g), torch.randn(2, 8, 6, 6, generator=g), torch.rand(8, generator=g)

    def twice(x0, x1, wt, pool, head):
        a = x0.clone().requires_grad_(True)
        d = head(pool(a), pool(x1), wt)
        (ga,) = torch.autograd.grad(d.sum(), a, create_graph=True)
        (gga,) = torch.autograd.grad((ga ** 2).sum(), a)
        return d.detach(), ga.detach(), gga
    ref = twice(x0.double(), x1.double(), wt.double(), lambda t: F.max_pool2d(t, 2, 2), lpips_layer_composition)
    with second_order():
        got = twice(x0.cuda(), x1.cuda(), wt.cuda(), op.max_pool2x2, op.lpips_layer)
    for name, a, b, tol in (("d", got[0], ref[0], TOL), ("g", got[1], ref[1], GTOL), ("gg", got[2], ref[2], GTOL)):
        e = rel_err(a, b)
        print("second order", name, e)
        assert e < tol, (name, e)
    with pytest.raises(RuntimeError, match="once_differentiable|does not require grad"):
        twice(x0.cuda(), x1.cuda(), wt.cuda(), op.max_pool2x2, op.lpips_layer)


# ------------------------------------------------------------------------------------------------- op.lpips_layer
# vector and scalar (5, 70) paths, 64 lanes a pixel with several vectors each (512), uneven lanes (70), and (3, 128, 33, 33): 1089
# pixels a sample against blocks of 8 (f32) / 16 (bf16) pixels -- several partials a sample (all 64 in f32), each block ONE trip
# through its pixel loop (4 pixels are in flight a group).  More than one trip: MULTI_TRIP_CASES.
LAYER_CASES = [(2, 8, 3, 3), (1, 5, 4, 4), (2, 64, 5, 7), (2, 512, 2, 2), (2, 70, 3, 3), (3, 128, 33, 33)]
# Sized against the split csrc/lpips.hip documents (_trips) so that a block goes through its pixel loop more than once:
# (1, 256, 47, 47): forward 3 (f32) / 2 (bf16) trips on the vector paths; (3, 33, 150, 150): the scalar path, forward 22 trips, and
# 67500 pixels against the backward's grid cap of 4096 blocks of 4 pixels, 2 in flight: 3 trips; (5, 256, 82, 82), f32 only: the
# vector path past the backward's cap (33620 pixels > 4096 * 4 * 2: 2 trips).
MULTI_TRIP_CASES = [((1, 256, 47, 47), torch.float32), ((1, 256, 47, 47), BF), ((3, 33, 150, 150), torch.float32), ((3, 33, 150, 150), BF),
                    ((5, 256, 82, 82), torch.float32)]
_layer_cache = {}


def _trips(case, dtype):
    """(forward, backward) passes of a block through its pixel loop, from the split csrc/lpips.hip documents: L vectors of 4 f32 / 8
    bf16 elements (elements when C is no multiple), G = the power of two >= min(L, 64) lanes a pixel, KV = ceil(L / G) vectors a
    lane, 256 / G pixels a block; 4 (forward) / 2 (backward) pixels in flight a group when a lane holds at most 8 elements of a
    tensor, else 1; forward: at most IDEAS_LPIPS_MAX_PARTIALS blocks a sample; backward: at most 4096 blocks over all samples."""
    from ideas_amd import _lib
    b, c, h, w = case
    vw = 8 if dtype == BF else 4
    vw = vw if c % vw == 0 else 1
    vectors = c // vw
    g = 1
    while g < vectors and g < 64:
        g *= 2
    small = -(-vectors // g) * vw <= 8
    per_block = 256 // g
    trips = lambda npix, cap, u: -(-npix // (min(-(-npix // per_block), cap) * per_block * u))
    return trips(h * w, _lib.LPIPS_MAX_PARTIALS, 4 if small else 1), trips(b * h * w, 4096, 2 if small else 1)


def _layer_case(case, dtype, zeros_in_w=False):
    """Operands as the kernel sees them (rounded to ``dtype``) and the f64 reference, computed once."""
    key = (case, dtype, zeros_in_w)
    if key not in _layer_cache:
        b, c, h, w = case
        g = torch.Generator().manual_seed(29 + sum(case))
        f0 = torch.relu(torch.randn(b, c, h, w, generator=g) + 0.5).to(dtype)
        f1 = torch.relu(torch.randn(b, c, h, w, generator=g) + 0.5).to(dtype)
        wt = torch.rand(c, generator=g)
        if zeros_in_w:
            wt[::3] = 0.0
        gd = torch.randn(b, generator=g)
        d, grads = LR.lpips_layer_f64(f0, f1, wt)
        _layer_cache[key] = (f0, f1, wt, gd, d, grads(gd))
    return _layer_cache[key]


def _layer_run(op, f0, f1, wt, gd, need=(True, True), layout="nhwc"):
    a = fmt(f0.cuda(), layout).requires_grad_(need[0])
    b = fmt(f1.cuda(), layout).requires_grad_(need[1])
    d = op.lpips_layer(a, b, wt.cuda())
    leaves = [t for t, n in zip((a, b), need) if n]
    grads = list(torch.autograd.grad(d, leaves, gd.cuda()))
    return d.detach(), (grads.pop(0) if need[0] else None), (grads.pop(0) if need[1] else None)


def _layer_compare(case, dtype, got, ref):
    d, g0, g1 = got
    rd, (r0, r1) = ref
    assert d.dtype == torch.float32 and tuple(d.shape) == (case[0],)
    e = rel_err(d, rd)
    print(case, dtype, "d", e)
    assert e < TOL, (case, e)
    for name, g, r in (("gf0", g0, r0), ("gf1", g1, r1)):
        if g is None:
            continue
        assert g.dtype == dtype and tuple(g.shape) == case
        if dtype == BF:
            close_bf16(g, r, name)
        else:
            e = rel_err(g, r)
            print(case, name, e)
            assert e < GTOL, (case, name, e)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", LAYER_CASES, ids=_ids)
def test_lpips_layer(op, case, dtype):
    f0, f1, wt, gd, d, grads = _layer_case(case, dtype)
    _layer_compare(case, dtype, _layer_run(op, f0, f1, wt, gd), (d, grads))


@pytest.mark.parametrize("case,dtype", MULTI_TRIP_CASES, ids=lambda v: _ids(v))
def test_lpips_layer_blocks_take_their_pixel_loop_more_than_once(op, case, dtype):
    fwd, bwd = _trips(case, dtype)
    assert fwd > 1 and (bwd > 1 or case[0] == 1), (fwd, bwd)
    f0, f1, wt, gd, d, grads = _layer_case(case, dtype)
    got = _layer_run(op, f0, f1, wt, gd)
    _layer_compare(case, dtype, got, (d, grads))
    _layer_cache.pop((case, dtype, False))                 # (the large operands are used once)


def test_trip_counts_of_the_documented_split():
    assert _trips((3, 128, 33, 33), torch.float32) == (1, 1) and _trips((3, 128, 33, 33), BF) == (1, 1)
    assert _trips((1, 256, 47, 47), torch.float32) == (3, 1) and _trips((1, 256, 47, 47), BF) == (2, 1)
    assert _trips((3, 33, 150, 150), torch.float32) == (22, 3) and _trips((3, 33, 150, 150), BF) == (22, 3)
    assert _trips((5, 256, 82, 82), torch.float32) == (7, 2)
    assert _trips((4, 64, 256, 256), torch.float32) == (16, 2)         # the benchmark's first tap


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_lpips_layer_weights_with_zeros_nchw_input_and_single_gradients(op, dtype):
    case = (2, 64, 5, 7)
    f0, f1, wt, gd, d, grads = _layer_case(case, dtype, zeros_in_w=True)
    assert int((wt == 0).sum()) > 0
    both = _layer_run(op, f0, f1, wt, gd, layout="nchw")
    _layer_compare(case, dtype, both, (d, grads))
    only0 = _layer_run(op, f0, f1, wt, gd, need=(True, False))
    only1 = _layer_run(op, f0, f1, wt, gd, need=(False, True))
    assert only0[2] is None and only1[1] is None
    # the same kernel arithmetic whichever outputs are asked for
    assert torch.equal(only0[1], both[1]) and torch.equal(only1[2], both[2]) and torch.equal(only0[0], both[0])
    # an odd channel count (the scalar path): gf0 only / gf1 only against the reference
    case = (2, 70, 3, 3)
    f0, f1, wt, gd, d, grads = _layer_case(case, dtype)
    _layer_compare(case, dtype, _layer_run(op, f0, f1, wt, gd, need=(True, False)), (d, grads))
    _layer_compare(case, dtype, _layer_run(op, f0, f1, wt, gd, need=(False, True)), (d, grads))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_lpips_layer_all_zero_pixel(op, dtype):
    """The deliberate difference: n = 0 gives u = 0 in the distance and a zero gradient, where the reference's backward gives NaN."""
    case = (2, 64, 5, 7)
    f0, f1, wt, gd, _, _ = _layer_case(case, dtype)
    f0 = f0.clone()
    f0[0, :, 1, 2] = 0
    f0[1, :, 4, 6] = 0
    d, grads = LR.lpips_layer_f64(f0, f1, wt)
    got = _layer_run(op, f0, f1, wt, gd)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    _layer_compare(case, dtype, got, (d, grads(gd)))
    assert float(got[1][0, :, 1, 2].abs().max()) == 0.0 and float(got[1][1, :, 4, 6].abs().max()) == 0.0
    assert float(got[2][0, :, 1, 2].abs().max()) > 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_lpips_layer_identical_pair_is_zero(op, dtype):
    f0, _, wt, gd, _, _ = _layer_case((3, 128, 33, 33), dtype)
    d, g0, g1 = _layer_run(op, f0, f0.clone(), wt, gd)
    assert float(d.abs().max()) == 0.0 and float(g0.abs().max()) == 0.0 and float(g1.abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_lpips_layer_is_bitwise_reproducible(op, dtype):
    f0, f1, wt, gd, _, _ = _layer_case((3, 128, 33, 33), dtype)
    a, b = _layer_run(op, f0, f1, wt, gd), _layer_run(op, f0, f1, wt, gd)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_c_abi_argument_checks_run_before_any_launch():
    """NULL pointers, non-positive sizes and dtypes without a kernel are answered by the checks in front of the launch (the
    pointers are host buffers a launch would never survive)."""
    from ideas_amd import _lib
    lib = _lib.load()
    E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
    buf = ctypes.create_string_buffer(256)
    a = ctypes.addressof(buf)

    def pool_fwd(y=a, x=a, B=2, C=8, H=4, W=4, dtype=_lib.F32):
        return lib.ideas_maxpool2x2_fwd(y, x, B, C, H, W, dtype, None)

    def pool_bwd(gx=a, gy=a, x=a, B=2, C=8, H=4, W=4, dtype=_lib.F32):
        return lib.ideas_maxpool2x2_bwd(gx, gy, x, B, C, H, W, dtype, None)

    def head_fwd(d=a, ws=a, f0=a, f1=a, w=a, B=2, C=8, H=4, W=4, dtype=_lib.F32):
        return lib.ideas_lpips_layer_fwd(d, ws, f0, f1, w, B, C, H, W, dtype, None)

    def head_bwd(gf0=a, gf1=a, gd=a, f0=a, f1=a, w=a, B=2, C=8, H=4, W=4, dtype=_lib.F32):
        return lib.ideas_lpips_layer_bwd(gf0, gf1, gd, f0, f1, w, B, C, H, W, dtype, None)
    for f in (pool_fwd, pool_bwd, head_fwd, head_bwd):
        assert f(B=0) == E_SHAPE and f(C=0) == E_SHAPE and f(H=-1) == E_SHAPE and f(W=0) == E_SHAPE
        assert f(dtype=_lib.F16) == E_UNSUPPORTED and f(dtype=_lib.F64) == E_UNSUPPORTED and f(dtype=17) == E_UNSUPPORTED
    assert pool_fwd(H=1) == E_SHAPE and pool_bwd(W=1) == E_SHAPE                   # no window fits
    assert pool_fwd(y=None) == E_NULL and pool_fwd(x=None) == E_NULL
    assert pool_bwd(gx=None) == E_NULL and pool_bwd(gy=None) == E_NULL and pool_bwd(x=None) == E_NULL
    assert all(head_fwd(**{k: None}) == E_NULL for k in ("d", "ws", "f0", "f1", "w"))
    assert all(head_bwd(**{k: None}) == E_NULL for k in ("gd", "f0", "f1", "w"))
    assert head_bwd(gf0=None, gf1=None) == E_NULL                                  # (one of the two may be left out)
    assert head_fwd(C=4096) == E_UNSUPPORTED and head_bwd(C=4096) == E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------- VGG16Features / PerceptualLoss
@pytest.fixture(scope="module")
def percept(gold):
    from ideas_amd.lpips import PerceptualLoss
    lin = {f"lin{k}.model.1.weight": gold.t(f"lin/{k}").reshape(1, -1, 1, 1) for k in range(5)}
    return PerceptualLoss(model="net-lin", net="vgg", backbone=LR.backbone_state(), lin_weights=lin).cuda()


def _bounds(gold, tag):
    taps, layers, val, gpred = gold.z[f"{tag}/f32_dev"].tolist()
    return max(TOL, 4 * taps), max(TOL, 4 * layers), max(TOL, 4 * val), max(GTOL, 4 * gpred)


@pytest.mark.parametrize("tag", ("near", "far", "same", "near01"))
def test_perceptual_loss_against_the_reference(gold, percept, tag):
    """Taps, per-layer distances, val and d val.sum() / d pred in f32 against the reference's f64 values; ``near01``: normalize=True."""
    b_taps, b_layers, b_val, b_g = _bounds(gold, tag)
    normalize = tag == "near01"
    pred = gold.t(f"{tag}/pred").cuda().requires_grad_(True)
    target = gold.t(f"{tag}/target").cuda()
    val, res = percept(pred, target, normalize=normalize, ret_per_layer=True)
    assert tuple(val.shape) == (2, 1, 1, 1) and val.dtype == torch.float32
    (g,) = torch.autograd.grad(val.sum(), pred)
    with torch.no_grad():
        taps = percept.features(2 * pred - 1 if normalize else pred.detach())
    sums = gold.z[f"{tag}/tap_sums"]
    for k, h in enumerate(taps):
        assert h.shape[1] == (64, 128, 256, 512, 512)[k] and not h.requires_grad
        if tag == "near":
            e = rel_err(h[0], gold.t(f"near/tap{k}"))
            print(tag, "tap", k, e, "bound", b_taps)
            assert e < b_taps, (k, e)
        if tag == "far" and k >= 2:                          # a second pair elementwise: the three deep taps of sample 1
            e = rel_err(h[1], gold.t(f"far/tap{k}"))
            print(tag, "tap", k, e, "bound", b_taps)
            assert e < b_taps, (k, e)
        for n in range(2):
            # every element is within b_taps * max|tap| of the reference's, so a sum is within numel times that
            slack = b_taps * float(h.abs().max()) * h[n].numel()
            assert abs(float(h[n].double().sum()) - sums[k, n, 0]) <= slack and abs(float(h[n].double().abs().sum()) - sums[k, n, 1]) <= slack
    layers = torch.stack([r.reshape(-1) for r in res])
    e_l, e_v, e_g = rel_err(layers, gold.t(f"{tag}/layers")), rel_err(val.reshape(-1), gold.t(f"{tag}/val")), rel_err(g, gold.t(f"{tag}/gpred"))
    print(tag, "layers", e_l, "bound", b_layers, "val", e_v, "bound", b_val, "gpred", e_g, "bound", b_g)
    assert e_l < b_layers and e_v < b_val and e_g < b_g, (e_l, e_v, e_g)
    if tag == "same":
        assert float(val.detach().abs().max()) == 0.0 and float(g.abs().max()) == 0.0
    plain = percept(pred.detach(), target, normalize=normalize)
    assert not plain.requires_grad and torch.equal(plain, val.detach())


# ------------------------------------------------------------------------------------------------- projector.project
@pytest.fixture(scope="module")
def g_ema(gold):
    from ideas_amd.model import Generator
    meta = gold.json("meta")["gen"]
    torch.manual_seed(meta["seed"])
    net = Generator(meta["size"], meta["style_dim"], meta["n_mlp"])
    sums = LR.checksums(net.state_dict())
    for k, (s, a) in meta["checksums"].items():
        assert sums[k][0] == pytest.approx(s, rel=1e-5, abs=1e-5) and sums[k][1] == pytest.approx(a, rel=1e-5), k
    pre = "proj/fill/"
    named = dict(net.named_parameters())
    fill = {k[len(pre):]: gold.t(k) for k in gold.keys() if k.startswith(pre)}
    assert set(fill) == {n for n in named if n.endswith("bias") or n.endswith("noise.weight")}
    with torch.no_grad():
        for n, v in fill.items():
            named[n].copy_(v)
    return net.eval().cuda()


@pytest.mark.parametrize("tag", ("w", "wplus"))
def test_project_replays_the_reference(gold, percept, g_ema, tag):
    """Three steps of the reference's loop (--noise 0, noise_regularize 1e5, mse 0.1) from the stored latent_mean, latent_std and
    noises: step-0 gradients elementwise, the three losses of each step, the update by relative L2 (4 x the reference's own f32 /
    f64 figure: 1.3e-4 (W), 3.2e-4 (W+)) and at most 2 % sign flips."""
    from ideas_amd import projector as P
    meta = gold.json("meta")["proj"]
    devs = gold.z[f"proj/{tag}/f32_dev"].tolist()
    noises = [gold.t(f"proj/noise{i}").cuda() for i in range(meta["n_noises"])]
    latent_mean = gold.t("proj/latent_mean").cuda()
    kept = {}

    def after_backward(i, latent_in, nz):
        if i == 0:
            kept["g_latent"] = latent_in.grad.detach().clone()
            kept["g_noise"] = [n.grad.detach().clone() for n in nz]
    results, path, losses = P.project(g_ema, gold.t("proj/imgs").cuda(), percept, step=meta["step"], lr=meta["lr"], noise=meta["noise"],
                                      noise_ramp=meta["noise_ramp"], noise_regularize=meta["noise_regularize"], mse=meta["mse"],
                                      w_plus=tag == "wplus", latent_mean=latent_mean, latent_std=float(gold.t("proj/latent_std")),
                                      noises=noises, after_backward=after_backward)
    assert len(results) == 2 and set(results[0]) == {"img", "latent", "noise"} and len(path) == 1 and tuple(losses.shape) == (3, 3)
    assert tuple(results[0]["img"].shape) == (3, 32, 32) and len(results[0]["noise"]) == meta["n_noises"]
    b_loss, b_gl, b_gn = max(TOL, 4 * devs[0]), max(GTOL, 4 * devs[1]), max(GTOL, 4 * devs[2])
    e = rel_err(kept["g_latent"], gold.t(f"proj/{tag}/g_latent"))
    print(tag, "g_latent", e, "bound", b_gl)
    assert e < b_gl, e
    for i, g in enumerate(kept["g_noise"]):
        e = rel_err(g, gold.t(f"proj/{tag}/g_noise{i}"))
        print(tag, "g_noise", i, e, "bound", b_gn)
        assert e < b_gn, (i, e)
    ref_losses = gold.t(f"proj/{tag}/losses")
    for j, name in enumerate(("p_loss", "n_loss", "mse_loss")):
        e = rel_err(losses[:, j], ref_losses[:, j])
        print(tag, name, e, "bound", b_loss)
        assert e < b_loss, (name, e)
    final = torch.stack([r["latent"] for r in results]).detach().double().cpu()
    assert torch.equal(final, path[-1].double().cpu())
    ref_update = gold.t(f"proj/{tag}/update").double()
    update = final - latent_mean.double().cpu().reshape((1,) * (final.dim() - 1) + (-1,))
    l2 = float((update - ref_update).norm() / ref_update.norm())
    flips = float((torch.sign(update) != torch.sign(ref_update)).double().mean())
    bound = 4 * float(gold.z[f"proj/{tag}/update_dev"])
    print(tag, "update relative L2", l2, "bound", bound, "sign flips", flips)
    assert l2 < bound, (l2, bound)
    assert flips <= 0.02, flips


# ------------------------------------------------------------------------------------------------- command line
def test_projector_cli_writes_the_references_outputs(gold, tmp_path):
    from PIL import Image
    from ideas_amd.model import Generator
    torch.manual_seed(7)
    torch.save({"g_ema": Generator(32, 32, 2).state_dict()}, tmp_path / "g.pt")
    torch.save(LR.backbone_state(), tmp_path / "vgg16.pth")
    torch.save({f"lin{k}.model.1.weight": gold.t(f"lin/{k}").reshape(1, -1, 1, 1) for k in range(5)}, tmp_path / "lin.pth")
    rng = np.random.RandomState(0)
    Image.fromarray(rng.randint(0, 256, (40, 48, 3), dtype=np.uint8)).save(tmp_path / "toy.png")
    cmd = [sys.executable, os.path.join(ROOT, "projector.py"), "--ckpt", str(tmp_path / "g.pt"), "--size", "32", "--latent", "32", "--n_mlp", "2",
           "--step", "2", "--vgg", str(tmp_path / "vgg16.pth"), "--lpips_lin", str(tmp_path / "lin.pth"), str(tmp_path / "toy.png")]
    r = subprocess.run(cmd, cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = torch.load(tmp_path / "toy.pt", map_location="cpu")
    assert list(out) == [str(tmp_path / "toy.png")]
    rec = out[str(tmp_path / "toy.png")]
    assert set(rec) == {"img", "latent", "noise"}
    assert tuple(rec["img"].shape) == (3, 32, 32) and tuple(rec["latent"].shape) == (32,) and len(rec["noise"]) == 7
    assert [tuple(n.shape) for n in rec["noise"]] == [(1, 1, s, s) for s in (4, 8, 8, 16, 16, 32, 32)]
    assert bool(torch.isfinite(rec["img"]).all())
    png = Image.open(tmp_path / "toy-project.png")
    assert png.size == (32, 32) and png.mode == "RGB"
