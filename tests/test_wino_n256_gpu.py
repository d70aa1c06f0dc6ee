"""The 64-pair x 256-channel tile of conv_b3_wino2d_kernel (csrc/conv_b3_wino.hip) against its 128-channel tile.

Every accumulator of the 256-channel tile receives the products of the 128-channel tile in the same order, so the two
must agree BITWISE.  IDEAS_B3_WINO_N256 is read per call: "0" keeps the 128-channel tile, a positive number is the fewest
64 x 256 tiles for which the wide tile is taken ("1" = wherever Cout % 256 == 0), unset = the library's threshold.  The
small shapes below have only a handful of tiles, far below that threshold, so they are compared between "0" and "1";
the default dispatch is checked on a launch with more tiles than persistent blocks."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
CL = torch.channels_last
ENV = "IDEAS_B3_WINO_N256"


def _tiles(B, H, W, cin, cout):
    """64 x 256 tiles the forward dispatch takes under the present environment (0: the 128-channel tile)."""
    import ctypes as C
    from ideas_amd import _lib
    fn = _lib.load().ideas_b3_wino_n256_tiles
    fn.restype, fn.argtypes = C.c_int64, [C.c_int] * 5
    return int(fn(B, H, W, cin, cout))


def _inputs(B, cin, cout, H, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    u = lambda *s: torch.rand(*s, device="cuda", generator=g) + 0.5
    return dict(x=r(B, cin, H, W).contiguous(memory_format=CL), w=r(cout, cin, 3, 3), lin=u(B, cin), lout=u(B, cout),
                bias=r(cout), resid=r(B, cout, H, W).contiguous(memory_format=CL),
                gy=r(B, cin, H, W).contiguous(memory_format=CL), wt=r(cin, cout, 3, 3))


def _configs(t, H, W):
    """name -> thunk: the five fast epilogues, two that land on the generic one, mirror padding, the input gradient."""
    import ideas_amd.op.conv as CV
    from ideas_amd.op.conv_plan import ConvGeom
    cin = t["x"].shape[1]
    gain = 1.0 / math.sqrt(cin * 9)
    g, gr = ConvGeom(3, 3, 1, 1, False), ConvGeom(3, 3, 1, 1, True)
    x, w = t["x"], t["w"]
    return {
        "plain": lambda: CV.conv_fwd_raw(x, w, g, gain),
        "lin_lout": lambda: CV.conv_fwd_raw(x, w, g, gain, lin=t["lin"], lout=t["lout"]),
        "bias_act": lambda: CV.conv_fwd_raw(x, w, g, gain, bias=t["bias"], act=True, act_gain=math.sqrt(2)),
        "lout_bias_act": lambda: CV.conv_fwd_raw(x, w, g, gain, lin=t["lin"], lout=t["lout"], bias=t["bias"], act=True,
                                                 act_gain=math.sqrt(2)),
        "lout_bias_act_resid": lambda: CV.conv_fwd_raw(x, w, g, gain, lin=t["lin"], lout=t["lout"], bias=t["bias"], act=True,
                                                       act_gain=math.sqrt(2), resid=t["resid"], resid_gain=1 / math.sqrt(2)),
        # no fast epilogue for these two: bias without activation; residual without an output scale
        "generic_bias": lambda: CV.conv_fwd_raw(x, w, g, gain, bias=t["bias"]),
        "generic_resid": lambda: CV.conv_fwd_raw(x, w, g, gain, bias=t["bias"], act=True, resid=t["resid"], resid_gain=0.5),
        "reflect": lambda: CV.conv_fwd_raw(x, w, gr, gain, lin=t["lin"], lout=t["lout"]),
        "reflect_plain": lambda: CV.conv_fwd_raw(x, w, gr, gain),
        # input gradient of a layer with cout -> cin channels: gy has cin channels here, the result cout (% 256 == 0)
        "dgrad": lambda: CV.conv_dgrad_raw(t["gy"], t["wt"], g, (H, W), gain),
        "dgrad_mod": lambda: CV.conv_dgrad_raw(t["gy"], t["wt"], g, (H, W), gain, lin=t["lin"], lout=t["lout"]),
    }


def _run_all(cfgs, monkeypatch, value):
    if value is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, value)
    out = {k: f().clone() for k, f in cfgs.items()}
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("hw", [(2, 64), (4, 32), (8, 16), (6, 64)])
@pytest.mark.parametrize("cout", [256, 512])
@pytest.mark.parametrize("cin", [32, 64])
@pytest.mark.parametrize("B", [1, 2])
def test_n256_tile_is_bitwise_the_128_channel_tile(B, cin, cout, hw, monkeypatch):
    """TP = 32 / 16 / 8 patches, one and several patches per image, 2 and 4 chunks, 1 and 2 N tiles; every epilogue."""
    H, W = hw
    t = _inputs(B, cin, cout, H, W, seed=B * 1000 + cin + cout + H * W)
    cfgs = _configs(t, H, W)
    monkeypatch.setenv(ENV, "0")
    assert _tiles(B, H, W, cin, cout) == 0
    old = _run_all(cfgs, monkeypatch, "0")
    monkeypatch.setenv(ENV, "1")
    assert _tiles(B, H, W, cin, cout) == B * H * (W // 2) // 64 * (cout // 256) > 0      # the wide tile is what runs
    new = _run_all(cfgs, monkeypatch, "1")
    for k in cfgs:
        assert torch.isfinite(new[k]).all(), k
        assert torch.equal(old[k], new[k]), (k, float((old[k] - new[k]).abs().max()))


def test_n256_default_dispatch_on_more_tiles_than_blocks(monkeypatch):
    """B = 3, 64 x 64, Cout = 512: 192 wide tiles, one per block (the 128-channel tile has 384 there, more than its 256 persistent
    blocks).  The default dispatch takes the wide tile, and agrees bitwise with the 128-channel tile."""
    B, cin, cout, H, W = 3, 32, 512, 64, 64
    t = _inputs(B, cin, cout, H, W, seed=7)
    cfgs = {k: f for k, f in _configs(t, H, W).items() if k in ("plain", "lout_bias_act_resid", "reflect", "dgrad_mod")}
    monkeypatch.delenv(ENV, raising=False)
    assert _tiles(B, H, W, cin, cout) == 192, "the default threshold no longer admits this launch"
    new = _run_all(cfgs, monkeypatch, None)
    old = _run_all(cfgs, monkeypatch, "0")
    for k in cfgs:
        assert torch.equal(old[k], new[k]), (k, float((old[k] - new[k]).abs().max()))


@pytest.mark.parametrize("case", [(7, 32, 512, 64, 64, None), (10, 96, 512, 64, 32, "1"), (20, 64, 512, 64, 16, "1")])
def test_n256_persistent_blocks_walk_several_tiles(case, monkeypatch):
    """More wide tiles than the 256 persistent blocks, so a block runs two tiles (and, at 448 = 256 + 192 and at 320, some blocks
    two and some one): the next tile's first window and weight quarter are fetched under the epilogue of the current one, and the
    chunk / step counters start again.  2 x 32 patches under the default rule (448 tiles: last round three quarters full), 4 x 16
    and 8 x 8 patches forced (320 tiles, which the default rule leaves to the 128-channel tile)."""
    B, cin, cout, H, W, env = case
    t = _inputs(B, cin, cout, H, W, seed=sum(case[:5]))
    cfgs = {k: f for k, f in _configs(t, H, W).items() if k in ("plain", "lout_bias_act_resid", "generic_bias", "reflect", "dgrad_mod")}
    if env is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, env)
    nt = _tiles(B, H, W, cin, cout)
    assert nt == B * H * (W // 2) // 64 * (cout // 256) > 256, nt
    new = _run_all(cfgs, monkeypatch, env)
    old = _run_all(cfgs, monkeypatch, "0")
    for k in cfgs:
        assert torch.isfinite(new[k]).all(), k
        assert torch.equal(old[k], new[k]), (k, float((old[k] - new[k]).abs().max()))


@pytest.mark.parametrize("shape", [(2, 32, 384, 8, 64), (2, 32, 128, 8, 64), (2, 64, 256, 8, 64), (1, 32, 256, 5, 64),
                                   (1, 32, 256, 8, 12)])
def test_n256_fallback_shapes_keep_the_old_tile(shape, monkeypatch):
    """Cout = 384 and 128, a launch below the tile-count threshold, and shapes the patch does not divide: the 128-channel tile (or
    the kernel before it) with the switch unset, off and forced alike, and identical output."""
    B, cin, cout, H, W = shape
    t = _inputs(B, cin, cout, H, W, seed=sum(shape))
    cfgs = {k: f for k, f in _configs(t, H, W).items() if k in ("plain", "lout_bias_act", "dgrad")}
    outs = []
    below_threshold = shape == (2, 64, 256, 8, 64)
    for v in (None, "0") if below_threshold else (None, "0", "1"):
        if v is None:
            monkeypatch.delenv(ENV, raising=False)
        else:
            monkeypatch.setenv(ENV, v)
        assert _tiles(B, H, W, cin, cout) == 0, v
        outs.append(_run_all(cfgs, monkeypatch, v))
    for o in outs[1:]:
        for k in cfgs:
            assert torch.equal(outs[0][k], o[k]), k


def test_n256_tile_has_the_f32_kernels_error(monkeypatch):
    """Cin = 64, Cout = 256, 8 x 64 against float64 conv2d on the CPU, bounded as tests/test_ops_gpu.py::
    test_b3_kernels_have_the_f32_kernels_error bounds the 128-channel tile: rms error (in units of sum |x * w|) at most 1.5 x
    that of the exact-f32 kernel, which is measured here on the same inputs."""
    import ideas_amd.op.conv as CV
    from ideas_amd import _lib
    from ideas_amd.op.conv_plan import ConvGeom
    B, cin, cout, H, W = 2, 64, 256, 8, 64
    torch.manual_seed(64 + 256 + 8)
    x = torch.randn(B, cin, H, W, dtype=torch.float64) * (torch.rand(B, cin, 1, 1, dtype=torch.float64) * 3 + 0.1)
    w = torch.randn(cout, cin, 3, 3, dtype=torch.float64)
    gain = 1.0 / math.sqrt(cin * 9)
    ref = F.conv2d(x, w * gain, padding=1)
    scale = F.conv2d(x.abs(), w.abs() * gain, padding=1)
    xd, wd = x.float().cuda().contiguous(memory_format=CL), w.float().cuda()
    g = ConvGeom(3, 3, 1, 1, False)
    monkeypatch.setenv(ENV, "1")
    assert _tiles(B, H, W, cin, cout) > 0
    rms = {}
    math0 = CV.MATH
    for name, mode in (("f32", _lib.F32), ("n256", _lib.F32_B3)):
        CV.MATH = mode
        try:
            y = CV.conv_fwd_raw(xd, wd, g, gain)
        finally:
            CV.MATH = math0
        e = (y.double().cpu() - ref).abs() / scale
        rms[name] = float(e.pow(2).mean().sqrt())
        assert float(e.max()) < 1e-6, (name, float(e.max()))
    print("rms error / sum|x*w|:", rms)
    assert rms["n256"] <= 1.5 * rms["f32"] + 1e-9, rms
