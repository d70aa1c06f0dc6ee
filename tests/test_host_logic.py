"""CPU: host-side logic of the product (no kernels): state-dict/init parity with the reference, the message
codec, patchify, the C ABI surface, and the product's train_iteration() driven with oracle-backed networks
against the step vectors captured from the reference's own train()."""
import argparse
import ctypes
import json
import os
import re

import pytest
import torch

from conftest import GOLDEN, ROOT, Golden, rel_err
import oracle.torch_ref as O


def test_init_matches_reference_seeded_init():
    from ideas_amd.models import init_model
    from ideas_amd.train_step import NET_CLASSES
    gold = json.load(open(os.path.join(GOLDEN, "init_checksums.json")))
    a = argparse.Namespace(channel=32, structure_channel=8, texture_channel=2048, N=1, image_size=256,
                           channel_multiplier=1, blur_kernel=(1, 3, 3, 1))
    for tag, cls in NET_CLASSES.items():
        torch.manual_seed(1234)
        net = init_model(cls, a)
        sd = net.state_dict()
        g = gold[tag]
        assert [[k, list(v.shape)] for k, v in sd.items()] == g["keys"], tag       # key names, order, shapes
        assert [k for k, _ in net.named_parameters()] == g["param_keys"], tag
        assert sum(p.numel() for p in net.parameters()) == g["n_params"], tag
        for k, v in g["sums"].items():
            assert abs(float(sd[k].double().sum()) - v) < 1e-9, (tag, k)
        assert abs(float(sum(v.double().abs().sum() for v in sd.values())) - g["total_abs"]) < 1e-6 * g["total_abs"]


def test_codec_and_patchify_product(ops_golden):
    from ideas_amd.utils import message_to_tensor, patchify_image, tensor_to_message
    g = ops_golden
    for c in g.json("meta")["codec"]:
        k = c["key"]
        Z = message_to_tensor(g.t(k + ".M"), c["sigma"], c["delta"], jitter=g.t(k + ".jitter"))
        assert torch.equal(Z, g.t(k + ".Z"))
        assert torch.equal(tensor_to_message(Z, c["sigma"]), g.t(k + ".M"))
    boxes = [tuple(int(v) for v in b) for b in g.t("patch.boxes").tolist()]
    assert torch.equal(patchify_image(g.t("patch.img"), 3, boxes=boxes), g.t("patch.out"))
    # edge cases: all-zero / all-one messages, values outside [-1, 1] are clamped
    for sigma in (1, 2, 3):
        for bit in (0.0, 1.0):
            M = torch.full((2, 6 * sigma), bit)
            assert torch.equal(tensor_to_message(message_to_tensor(M, sigma, 0.5), sigma), M)
    assert torch.equal(tensor_to_message(torch.tensor([[-3.0, 3.0, 0.0, -0.0]]), 1), torch.tensor([[0.0, 1.0, 1.0, 1.0]]))


def test_draw_boxes_matches_reference_rng_order(ops_golden):
    import random
    from ideas_amd.utils import draw_boxes
    g = ops_golden
    torch.manual_seed(11)
    random.seed(11)
    torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(1))  # independent generator: no effect
    boxes = draw_boxes(64, 64, 3)
    assert boxes == [tuple(int(v) for v in b) for b in g.t("patch.boxes").tolist()]


def test_c_abi_exports_every_declared_symbol():
    """The shared library loads (no GPU needed) and exports exactly what include/ideas_hip.h declares."""
    from ideas_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ideas_hip.h")).read()
    declared = set(re.findall(r"\b(ideas_[a-z0-9_]+)\s*\(", hdr)) - {"ideas_conv_params"}
    assert declared, "no declarations parsed"
    assert os.path.exists(_lib.LIB_PATH), "build libideas_hip.so first (__graft_entry__.build())"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in ideas_hip.h but not exported"
    assert set(_lib.EXPORTS) == declared
    assert _lib.load().ideas_abi_version() == _lib.ABI_VERSION == 4
    assert _lib.load().ideas_strerror(-2) == b"bad or inconsistent dimension"
    assert ctypes.sizeof(_lib.ConvParams) == _lib.load().ideas_sizeof_conv_params() == 28 * 4


def splitk_plan_rows(lib, cases, site, scaled, slots=None):
    """ideas_conv_splitk_plan (the diagnostic beside the ABI, csrc/conv_igemm.hip) over rows of (B, OH, OW, Cin, Cout, taps, slots):
    what the split-K launcher `site` would pass to its kernel.  `slots` overrides the column (0 = the launcher's own count)."""
    import numpy as np
    from ideas_amd import _lib
    fn = lib.ideas_conv_splitk_plan
    fn.argtypes = [ctypes.c_int, ctypes.POINTER(_lib.ConvParams), ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    fn.restype = ctypes.c_int
    rows = np.zeros((len(cases), 4), dtype=np.int64)
    out = (ctypes.c_int64 * 4)()
    for i, (B, OH, OW, Cin, Cout, K, s) in enumerate(cases):
        p = _lib.ConvParams(B=B, IH=OH, IW=OW, Cin=Cin, YH=OH, YW=OW, Cout=Cout, OH=OH, OW=OW, TY=K, TX=K, sy=1, sx=1, dy=1, dx=1,
                            offy=-(K // 2), offx=-(K // 2), osy=1, osx=1)
        assert fn(site, ctypes.byref(p), scaled, s if slots is None else slots, out) == 0
        rows[i] = out[:]
    return rows


def test_splitk_plans_match_pinned():
    """Every split-K launcher sizes its grid as the commit before the launch rules were consolidated did: the library's plan query over
    the sweep of tests/golden/make_golden_splitk_plans.py (a transcription of that commit's arithmetic) against its digests."""
    import hashlib
    import numpy as np
    from ideas_amd import _lib
    g = np.load(os.path.join(GOLDEN, "splitk_plans.npz"))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    cases = g["cases"].astype(np.int64)
    names = sorted(k[:-5] for k in g.files if k.endswith("/site"))
    assert len(names) == 8
    for name in names:
        site, scaled = (int(v) for v in g[name + "/site"])
        sel = cases[g[name + "/idx"]].tolist()
        assert len(sel) == int(g[name + "/n"]) > 1000, name
        rows = splitk_plan_rows(lib, sel, site, scaled)
        assert (rows[:16] == g[name + "/head"]).all(), (name, rows[:16], g[name + "/head"])
        assert hashlib.sha256(rows.tobytes()).digest() == bytes(g[name + "/sha256"]), name


def _wgrad3_params(B, ci, co, OH, OW, pad=1, stride=1):
    """ideas_conv_params of the weight-gradient launch of a 3x3 conv whose output is OH x OW (op/conv_plan.py::plan_wgrad)."""
    import ideas_amd.op.conv as CV
    from ideas_amd.op.conv_plan import ConvGeom, plan_wgrad
    ih, iw = (OH - 1) * stride + 3 - 2 * pad, (OW - 1) * stride + 3 - 2 * pad
    return CV._params(plan_wgrad((B, ci, ih, iw), (B, co, OH, OW), ConvGeom(3, 3, stride, pad, False)), 1.0)


def test_bf16_wgrad3_query_and_work_floor(monkeypatch):
    """ideas_bf16_wgrad3_supported (csrc/conv_bf16.hip: the function ideas_bf16_wgrad itself asks before it launches
    conv_bf16_wgrad3_kernel) and the floor IDEAS_BF16_WGRAD3_MIN_WORK under it.  Unset, the dispatch is what it always was: 6e9
    products, so the small 3x3 / stride-1 shapes of test_bf16_gpu.py::CONV_CASES are the generic kernel's and 512 -> 512 at
    104 x 128, B = 2 the tap-fused one's.  At 0 every row of WGRAD3_CASES is admitted (what test_bf16_tap_fused_weight_gradient_vs_f64 rests
    on), IDEAS_BF16_WGRAD3=0 refuses everything, each geometric condition refuses alone, and the plan query gives every row the
    parts, rows per part and strips it names."""
    from ideas_amd import _lib
    from test_bf16_gpu import WGRAD3_CASES, WGRAD3_OP_CASES, wgrad3_launch
    lib = _lib.load()
    q = lambda p: lib.ideas_bf16_wgrad3_supported(ctypes.byref(p))
    # (B, Cin, Cout, OH, OW).  The third small one is the shape of test_bf16_image_and_tap_fused_kernels_full_size, G.layers.7.conv2 at
    # B = 4: 2^32 = 4.3e9 products, under the floor -- that test moves the floor to reach the kernel; the layer at the bench's B = 32
    # and the 104 x 128 test's shape are over it
    small = [(3, 64, 64, 40, 96), (2, 128, 128, 16, 32), (4, 128, 128, 256, 256)]
    big = [(2, 512, 512, 104, 128), (32, 128, 128, 256, 256)]
    for var in ("IDEAS_BF16_WGRAD3_MIN_WORK", "IDEAS_BF16_WGRAD3"):
        monkeypatch.delenv(var, raising=False)
    assert [q(_wgrad3_params(*s)) for s in small] == [0, 0, 0] and [q(_wgrad3_params(*s)) for s in big] == [1, 1]
    assert [s[0] * s[3] * s[4] * s[1] * s[2] >= 6000000000 for s in small + big] == [False, False, False, True, True]
    monkeypatch.setenv("IDEAS_BF16_WGRAD3_MIN_WORK", "6000000000")      # the default, spelled out
    assert [q(_wgrad3_params(*s)) for s in small + big] == [0, 0, 0, 1, 1]
    monkeypatch.setenv("IDEAS_BF16_WGRAD3_MIN_WORK", str(2 * 512 * 512 * 104 * 128 + 1))      # the floor is the number given
    assert [q(_wgrad3_params(*s)) for s in big] == [0, 1]
    monkeypatch.setenv("IDEAS_BF16_WGRAD3_MIN_WORK", str(2 * 512 * 512 * 104 * 128))
    assert [q(_wgrad3_params(*s)) for s in big] == [1, 1]
    assert lib.ideas_bf16_wgrad3_supported(None) == 0

    monkeypatch.setenv("IDEAS_BF16_WGRAD3_MIN_WORK", "0")
    rows = [wgrad3_launch(case)[3] for case, _ in WGRAD3_CASES]
    rows += [_wgrad3_params(B, ci, co, H, W) for B, ci, co, k, s, pad, refl, H, W in WGRAD3_OP_CASES] + [_wgrad3_params(*s) for s in small + big]
    assert all(q(p) == 1 for p in rows)
    assert {(p.offy, p.offx) for p in rows} == {(-1, -1), (0, 0), (-2, -2)} and {p.reflect for p in rows} == {0, 1}
    # each geometric condition, broken alone on an admitted shape
    ok = (2, 64, 64, 8, 32)
    assert q(_wgrad3_params(*ok)) == 1
    for what, p in (("OW % 32", _wgrad3_params(2, 64, 64, 8, 48)), ("OW % 32", _wgrad3_params(2, 64, 64, 8, 16)),
                    ("Cin % 64", _wgrad3_params(2, 32, 64, 8, 32)), ("Cin % 64", _wgrad3_params(2, 96, 64, 8, 32)),
                    ("Cout % 64", _wgrad3_params(2, 64, 32, 8, 32)), ("Cout % 64", _wgrad3_params(2, 64, 96, 8, 32)),
                    ("OH < 8", _wgrad3_params(2, 64, 64, 7, 32)), ("stride 2", _wgrad3_params(2, 64, 64, 8, 32, pad=0, stride=2)),
                    ("offx = 1", None), ("offy = 1", None), ("offx = -3", _wgrad3_params(2, 64, 64, 8, 32, pad=3)), ("5 taps", None),
                    ("dilation", None)):
        if p is None:
            p = _wgrad3_params(*ok)
            if what.startswith("off"):
                setattr(p, what[:4], 1)
            elif what == "5 taps":
                p.TX = 5
            else:
                p.dx = 2
        assert q(p) == 0, what
    monkeypatch.setenv("IDEAS_BF16_WGRAD3", "0")
    assert not any(q(p) for p in rows)
    monkeypatch.delenv("IDEAS_BF16_WGRAD3")
    # the part structure the rows name: {strips x B x parts, rows per part, parts} from the launcher's own plan (site 6)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for (B, ci, co, OH, OW, *_), (parts, per, strips) in WGRAD3_CASES:
        assert OW == 32 * strips
        got = splitk_plan_rows(raw, [(B, OH, OW, ci, co, 3, 0)], 6, 0)[0].tolist()
        assert got == [strips * B * parts, per, parts, 512], ((B, ci, co, OH, OW), got)
        assert (parts - 1) * per < OH <= parts * per               # every part has rows; the last one OH - (parts - 1) * per
    last = {c[3]: c[3] - (pl[0] - 1) * pl[1] for c, pl in WGRAD3_CASES}
    assert last[97] == 31 and last[65] == 32
    assert sorted({(c[3] + 2) % 6 for c, _ in WGRAD3_CASES}) == [0, 1, 2, 3, 4, 5]      # every exit of the unrolled step loop


def test_bf16_forward_tile_query():
    """ideas_bf16_fwd_choice (the diagnostic beside the ABI, driven by bf16_fwd_tile itself): the 8-wave 256 x 128 tile exactly for
    Cout >= 256 with >= 256 rows, rows counted per image for per-sample packs; the 4-wave ladder below it by Cout; and the LDS-image
    kernel's claim on 3x3 / stride-1 launches reported beside the tile."""
    import ideas_amd.op.conv as CV
    from ideas_amd.op.conv_plan import ConvGeom, plan_fwd
    from test_bf16_gpu import TILE_8WAVE, fwd_choice

    def params(B, ci, co, H, W, k=3, stride=2, pad=0):
        return CV._params(plan_fwd((B, ci, H, W), torch.empty(co, ci, k, k), ConvGeom(k, k, stride, pad, False)), 1.0)
    p = params(1, 32, 256, 33, 33)                                  # 16 x 16 = 256 rows
    assert (p.OH, p.OW) == (16, 16)
    assert fwd_choice(p, 0) == (TILE_8WAVE, 0) and fwd_choice(p, 1) == (TILE_8WAVE, 0)
    assert fwd_choice(params(1, 32, 252, 33, 33), 0)[0] == (128, 128, 4)           # 255 would break Cout % 4; the rule is Cout >= 256
    p.Cout = 255
    assert fwd_choice(p, 0)[0] == (128, 128, 4)
    p = params(1, 32, 256, 33, 35)                                  # 16 x 17 = 272 rows
    p.OH, p.OW = 15, 17                                             # 255 rows
    assert fwd_choice(p, 0)[0] == (128, 128, 4)
    p.OH, p.OW = 16, 16
    assert fwd_choice(p, 0)[0] == TILE_8WAVE
    p = params(2, 32, 256, 33, 31)                                  # 16 x 15 = 240 rows an image, 480 in all
    assert fwd_choice(p, 0)[0] == TILE_8WAVE and fwd_choice(p, 1)[0] == (128, 128, 4)
    p = params(3, 32, 512, 21, 21)                                  # 100 rows an image, 300 in all
    assert fwd_choice(p, 0)[0] == TILE_8WAVE and fwd_choice(p, 1)[0] == (128, 128, 4)
    for co, tile in ((1024, TILE_8WAVE), (256, TILE_8WAVE), (252, (128, 128, 4)), (68, (128, 128, 4)), (64, (128, 64, 4)),
                     (36, (128, 64, 4)), (32, (128, 32, 4)), (4, (128, 32, 4))):
        assert fwd_choice(params(2, 32, co, 33, 33), 0)[0] == tile, co
    # the LDS-image kernel takes 3x3 / stride 1 / pad 1 at W % 16 == 0 and whole patches first: 16 x 16 in 16-wide patches, 8 x 64 in 64-wide
    assert fwd_choice(params(1, 256, 384, 16, 16, 3, 1, 1), 0) == (TILE_8WAVE, 16)
    assert fwd_choice(params(2, 64, 128, 8, 64, 3, 1, 1), 0) == ((128, 128, 4), 64)
    assert fwd_choice(params(1, 32, 256, 17, 18, 3, 1, 1), 0) == (TILE_8WAVE, 0)       # 18 columns: the generic tile
    assert fwd_choice(params(1, 256, 256, 16, 17, 1, 1, 0), 0) == (TILE_8WAVE, 0)


def prep_plan_reference(op, a, s, w_addr):
    """What the commit before csrc/weight_prep.hip computed for a derived-weight job, transcribed from its three places: the entry
    points' validation (ideas_b3_split_weights_strided, ideas_b3_wino_split_weights, ideas_bf16_pack_weights_strided), op/conv.py's
    ``_prep`` (the `unit` flag and the work-item count the batched kernels trusted) and the grid rule, written as ideas_prep_blocks in C
    and again in op/conv_plan.py.  Returns (code, unit, nblocks, dst_elems); a = dims, s = strides in floats, w_addr = source address."""
    from ideas_amd import _lib
    wino = op == _lib.PREP_B3_WINO
    vec, planes, taps = {_lib.PREP_B3_SPLIT: (4, 3, 1), _lib.PREP_B3_WINO: (4, 12, 3), _lib.PREP_BF16_PACK: (8, 1, 1)}[op]
    dims = a[:2] if wino else a[:4]
    if any(d <= 0 for d in dims):
        return (-2, None, None, None)                        # IDEAS_E_SHAPE
    if dims[-1] % (4 * vec):
        return (-4, None, None, None)                        # IDEAS_E_ALIGN: Cin % 16 (b3), Cin % 32 (bf16), C % 16 (wino)
    n = taps
    for d in dims:
        n *= d
    unit = (not wino) and s[3] == 1 and w_addr % 16 == 0 and s[0] % 4 == 0 and s[1] % 4 == 0 and s[2] % 4 == 0
    work = n // vec
    return (0, int(unit), min(work // 256 + 1, 2048), planes * n)


def test_weight_prep_plan_is_the_rule_it_replaced():
    """ideas_weight_prep_plan (csrc/weight_prep.hip: the one statement of the channel granularities, the element counts, the 16-byte
    `unit` rule and the grid rule of the derived-weight kernels) against prep_plan_reference over dims around every granularity and
    block-count boundary, strides with each of sc / sn / sty / stx on and off the rule, and sources at 0 / 4 / 8 / 12 mod 16."""
    import itertools
    from ideas_amd import _lib
    lib = _lib.load()
    strides = [(1152, 384, 128, 1), (1152, 384, 128, 2), (1153, 384, 128, 1), (1154, 384, 128, 1), (1152, 385, 128, 1),
               (1152, 386, 128, 1), (1152, 384, 129, 1), (1152, 384, 130, 1), (1, -384, -128, 1152), (0, 0, 0, 1), (-4, 8, -12, 1),
               (1156, 388, 132, 9)]
    couts = (-1, 0, 1, 3, 5, 15, 16, 17, 255, 256, 257, 8191, 8192, 32736, 32752, 32768)
    cins = (-16, 0, 1, 15, 16, 17, 31, 32, 33, 48, 64, 96, 128)
    taps = ((1, 1), (1, 3), (3, 3), (0, 3), (3, -1))
    n, numel, seen = 0, ctypes.c_int64(), set()
    for op in (_lib.PREP_B3_SPLIT, _lib.PREP_B3_WINO, _lib.PREP_BF16_PACK):
        for (co, ci, (ty, tx)), st, addr in itertools.product(itertools.product(couts, cins, taps), strides, (0, 4, 8, 12)):
            # the Winograd form has a = (N, C) and five strides (the last one the base offset); it reads no other field
            a = (co, ci, 7 * ty, 0) if op == _lib.PREP_B3_WINO else (co, ty, tx, ci)
            if op == _lib.PREP_B3_WINO and tx != 3:
                continue
            d = _lib.PrepDesc(dst=0, w=(1 << 20) + addr, s=st + (addr,), a=a, unit=7, block0=5, nblocks=-3)
            numel.value = -1
            rc = lib.ideas_weight_prep_plan(ctypes.byref(d), op, ctypes.byref(numel))
            want = prep_plan_reference(op, a, st, (1 << 20) + addr)
            got = (rc, d.unit, d.nblocks, numel.value) if rc == 0 else (rc, None, None, None)
            assert got == want, (op, a, st, addr, got, want)
            assert d.block0 == 5 and d.dst is None and list(d.a) == list(a)         # the plan fills unit and nblocks, nothing else
            seen.add(want[:3])
            n += 1
    assert n > 5000
    assert {(-2, None, None), (-4, None, None), (0, 0, 1), (0, 1, 1), (0, 1, 2048), (0, 0, 2048), (0, 1, 2047)} <= seen
    assert lib.ideas_weight_prep_plan(ctypes.byref(d), 3, ctypes.byref(numel)) == -3                 # unknown form
    assert lib.ideas_weight_prep_plan(None, 0, ctypes.byref(numel)) == -1 and lib.ideas_weight_prep_plan(ctypes.byref(d), 0, None) == -1


def test_ops_fail_loudly_on_cpu_tensors():
    import ideas_amd.op as op
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.fused_leaky_relu(torch.zeros(1, 4), torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.modulated_conv2d(torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 3, 3), torch.zeros(1, 4))


# ---------------------------------------------------------------------------------------------------
class OracleBacked(torch.nn.Module):
    """Product module's parameters + the oracle's functional forward: lets the product step run on CPU."""

    def __init__(self, module, fn, cfg):
        super().__init__()
        self.m, self.fn, self.cfg = module, fn, cfg

    def forward(self, *a, **k):
        P = dict(self.m.named_parameters())
        P.update(dict(self.m.named_buffers()))
        return self.fn(P, self.cfg, *a, **k)


def _oracle_trainer(trainer, args):
    cfg = O.Cfg(channel=args.channel, structure_channel=args.structure_channel, texture_channel=args.texture_channel,
                N=args.N, image_size=args.image_size, channel_multiplier=args.channel_multiplier)
    out = dict(trainer)
    for name, fn in O.NETS.items():
        if name == "Dco" and not hasattr(trainer[name], "encoder"):
            continue   # ZeroDco stand-in
        out[name] = OracleBacked(trainer[name], fn, cfg)
        if name + "_ema" in trainer:
            out[name + "_ema"] = OracleBacked(trainer[name + "_ema"], fn, cfg)
    return out


@pytest.mark.parametrize("which", ["r64", "r256", "r64_N2", "r256_N2", "r256_full"])
def test_product_step_logic_against_reference_train(which):
    """ideas_amd.train_step.train_iteration (host logic) with oracle-backed nets == reference train() vectors."""
    from test_nets_gpu import check_replay, replay_step
    torch.set_num_threads(8)
    g, meta, trainer, out, log = replay_step(which, "cpu", build_nets=_oracle_trainer)
    check_replay(g, meta, trainer, out, log)


def test_literal_second_backward_gives_same_ex_gradient(monkeypatch):
    """elide_second_backward=True takes Ex's gradient over the Ex sub-graph only; the reference's literal
    second traversal (train.py:214-215) must give the same Ex update.  (The G phase's paired generator pass of round 6 is taken
    with the elided backward only; it is switched off here so that both runs evaluate the same forward, bit for bit.)"""
    from ideas_amd import train_step as TS
    monkeypatch.setattr(TS, "_G_PAIR", "x")
    from ideas_amd.models import init_model
    from test_nets_gpu import ZeroDco
    res = []
    for elide in (True, False):
        args = TS.default_args(channel=4, texture_channel=64, channel_multiplier=0.125, image_size=64, batch_size=1,
                               d_reg_every=4, num_iters=10, elide_second_backward=elide)
        torch.manual_seed(5)
        tr = _oracle_trainer(TS.build_trainer(args, "cpu", init_model, dco_factory=ZeroDco), args)
        torch.manual_seed(6)
        import random
        random.seed(6)
        X = torch.rand(1, 3, 64, 64) * 2 - 1
        TS.train_iteration(tr, args, X, 1)
        res.append(torch.cat([p.detach().flatten() for p in tr["Ex"].parameters()]))
    assert torch.allclose(res[0], res[1], rtol=0, atol=1e-7)


def test_flop_table_matches_reference_hooks():
    """recompute the per-net forward GFLOPs from the product's own layer table; must match the
    numbers hooks measured on the reference (Appendix A) to 1 %."""
    from ideas_amd.flops import forward_flops
    from ideas_amd.models import init_model
    from ideas_amd.train_step import NET_CLASSES
    a = argparse.Namespace(channel=32, structure_channel=8, texture_channel=2048, N=1, image_size=256,
                           channel_multiplier=1, blur_kernel=(1, 3, 3, 1))
    ref = {"E": 16.516215808, "G": 95.992446976, "Gstru": 0.207896576, "Ex": 0.1937408, "Dreal": 53.2562688,
           "Dco": 0.998638592, "Ddist": 0.00223648}
    for tag, cls in NET_CLASSES.items():
        gf = forward_flops(init_model(cls, a), 256) / 1e9
        assert abs(gf - ref[tag]) <= 0.01 * ref[tag], (tag, gf, ref[tag])


def test_checkpoint_roundtrip_in_reference_format(tmp_path):
    """ideas_amd.checkpoint writes/reads the reference's .pt layout (train.py:308-322, 435-442): all 11 nets + 3
    optimisers, iter_idx, N, args; a state-dict produced by the reference's key set loads strictly."""
    from ideas_amd import checkpoint as CK, train_step as TS
    from ideas_amd.models import init_model
    args = TS.default_args(channel=4, texture_channel=64, channel_multiplier=0.125, image_size=64)
    torch.manual_seed(1)
    tr = TS.build_trainer(args, "cpu", init_model)
    # give the optimisers some state
    for name in ("g_optim", "ex_optim", "d_optim"):
        for grp in tr[name].param_groups:
            for p in grp["params"]:
                p.grad = torch.randn_like(p) * 1e-3
        tr[name].step()
    path = str(tmp_path / "7.pt")
    CK.save(path, tr, args, 7)
    raw = torch.load(path, map_location="cpu", weights_only=False)
    assert set(raw) == {"iter_idx", "N", "trainer", "args"} and raw["iter_idx"] == 7 and raw["N"] == args.N
    assert set(raw["trainer"]) == set(CK.TRAINER_KEYS)
    gold = json.load(open(os.path.join(GOLDEN, "init_checksums.json")))
    assert list(raw["trainer"]["G"].keys()) == [k for k, _ in gold["G"]["keys"]]      # the reference's key names/order
    torch.manual_seed(2)
    tr2 = TS.build_trainer(args, "cpu", init_model)
    assert CK.load(path, tr2) == 7
    for name in ("E", "G", "Gstru", "Ex", "Dreal", "Dco", "Ddist", "G_ema"):
        for (k1, v1), (k2, v2) in zip(tr[name].state_dict().items(), tr2[name].state_dict().items()):
            assert k1 == k2 and torch.equal(v1, v2)
        assert all(p.is_contiguous(memory_format=torch.channels_last) for p in tr2[name].parameters() if p.dim() == 4)
    s1, s2 = tr["d_optim"].state_dict(), tr2["d_optim"].state_dict()
    assert s1["param_groups"] == s2["param_groups"]
    assert all(torch.equal(s1["state"][i]["exp_avg_sq"], s2["state"][i]["exp_avg_sq"]) for i in s1["state"])


def _ckpt_trainer(seed):
    from ideas_amd import train_step as TS
    from ideas_amd.models import init_model
    args = TS.default_args(channel=4, texture_channel=64, channel_multiplier=0.125, image_size=256, batch_size=1, d_reg_every=2, num_iters=2)
    torch.manual_seed(seed)
    return TS.build_trainer(args, "cpu", init_model), args


def _assert_loaded(trainer, raw, skip=()):
    """Every tensor of the reference-format checkpoint `raw` is what `trainer` now holds (values; layout-agnostic)."""
    for name, sd in raw["trainer"].items():
        if name.endswith("_optim"):
            got = trainer[name].state_dict()
            assert [g_["params"] for g_ in got["param_groups"]] == [g_["params"] for g_ in sd["param_groups"]]
            for k in ("lr", "betas", "eps", "weight_decay", "amsgrad"):
                assert got["param_groups"][0][k] == sd["param_groups"][0][k], (name, k)
            assert set(got["state"]) == set(sd["state"])
            for i, st in sd["state"].items():
                for k, v in st.items():
                    if f"ck.{name}.state.{i}.{k}" in skip:
                        continue
                    assert torch.equal(torch.as_tensor(got["state"][i][k]).float().cpu(), torch.as_tensor(v).float()), (name, i, k)
        else:
            mine = trainer[name].state_dict()
            assert list(mine.keys()) == list(sd.keys()), name              # the reference's key names AND order
            for k, v in sd.items():
                if f"ck.{name}/{k}" in skip:
                    continue
                assert mine[k].shape == v.shape and torch.equal(mine[k].cpu(), v), (name, k)


def test_checkpoint_written_by_the_reference_loads_strictly(tmp_path):
    """VERDICT r5 item 5b.  tests/golden/ckpt_r256.npz holds the tensors of the file the reference's unmodified train() saved after
    its first iteration (train.py:308-322; tiny width, 256x256, real Dco): rebuilt into the reference's dict, written with torch.save
    and read by ideas_amd.checkpoint.load with strict load_state_dict on all 11 networks and the 3 optimisers (train.py:435-442).
    (The 13 largest tensors of the reference's un-narrowable Dreal + their Adam state are not in the fixture: zeros here; the GPU test
    fills them from its own first iteration.)"""
    from conftest import Golden
    from ckpt_fixture import build_reference_checkpoint, omitted_entries
    from ideas_amd import checkpoint as CK
    g = Golden("ckpt_r256.npz")
    raw = build_reference_checkpoint(g, lambda key, shape: torch.zeros(shape))
    assert list(raw["trainer"].keys()) == list(CK.TRAINER_KEYS) and raw["iter_idx"] == 1 and raw["N"] == 1
    path = str(tmp_path / "1.pt")
    torch.save(raw, path)
    tr, _ = _ckpt_trainer(5)
    assert CK.load(path, tr) == 1
    _assert_loaded(tr, raw)
    # what the fixture kept of the tensors it does not store is consistent with the parameters' shapes
    shapes = {f"ck.Dreal/{k}": tuple(v.shape) for k, v in tr["Dreal"].state_dict().items()}
    for key, shape, *_ in omitted_entries(g):
        if key.startswith("ck.Dreal/"):
            assert shapes[key] == tuple(shape)
    for p in tr["G"].parameters():
        if p.dim() == 4:
            assert p.is_contiguous(memory_format=torch.channels_last)


def test_sample_sheet_layout_and_quantisation(tmp_path):
    """ideas_amd.utils.save_image_grid = torchvision.utils.save_image(sample, path, nrow, normalize=True, range=(-1, 1)) of
    train.py:295-301 (torchvision is absent here: its published make_grid / save_image arithmetic restated in numpy)."""
    import numpy as np
    from PIL import Image
    from ideas_amd.utils import save_image_grid
    g = torch.Generator().manual_seed(2)
    x = torch.randn(7, 3, 5, 6, generator=g) * 0.8              # values outside [-1, 1] are clamped
    path = str(tmp_path / "s.png")
    save_image_grid(x, path, nrow=3)
    got = np.asarray(Image.open(path))
    n = ((x.clamp(-1, 1) + 1) / 2).numpy()
    want = np.zeros((3 * 7 + 2, 3 * 8 + 2, 3), np.float32)          # ceil(7 / 3) = 3 rows, 3 columns, 2-pixel black padding
    for k in range(7):
        y0, x0 = (k // 3) * 7 + 2, (k % 3) * 8 + 2
        want[y0:y0 + 5, x0:x0 + 6] = n[k].transpose(1, 2, 0)
    want = np.clip(want * 255 + 0.5, 0, 255).astype(np.uint8)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert got[0, 0].tolist() == [0, 0, 0] and got[-1, -1].tolist() == [0, 0, 0]       # the empty ninth cell stays black too


def test_derived_weight_cache_scope():
    """op/conv_plan.py cache: off by default (plain op calls never see stale derived weights), memoises only (views of)
    Parameters while on, and is emptied by cache_clear() -- which train_step._step calls after every optimiser step with that
    optimiser's parameters, so the other networks' derived weights survive."""
    import torch
    from ideas_amd.op import conv_plan as P
    w = torch.nn.Parameter(torch.randn(4, 3, 3, 3))
    calls = []

    def make():
        calls.append(1)
        return w.detach() * 2
    assert P._CACHE is None
    P.cached(w, ("k",), make); P.cached(w, ("k",), make)
    assert len(calls) == 2                                   # cache off: recomputed every time
    P.cache_begin()
    try:
        a = P.cached(w, ("k",), make); b = P.cached(w, ("k",), make)
        assert a is b and len(calls) == 3                    # memoised
        assert P.cached(w[:2], ("k",), make) is not a        # another view: another entry
        t = torch.randn(4, 3, 3, 3)                          # not a Parameter: never cached
        P.cached(t, ("k",), make); P.cached(t, ("k",), make)
        n = len(calls)
        P.cache_clear()                                      # a full clear
        assert P.cached(w, ("k",), make) is not a and len(calls) == n + 1
        # what an optimiser step triggers: only what derives from the parameters it stepped (views of a flat buffer included)
        flat = torch.nn.Parameter(torch.randn(100))
        other = torch.nn.Parameter(torch.randn(2, 3, 3, 3))
        va, vb = flat[:54].view(2, 3, 3, 3), flat[54:]
        ea, eb, eo, ew = (P.cached(va, ("k",), make), P.cached(vb, ("k",), make), P.cached(other, ("k",), make),
                          P.cached(w, ("k",), make))
        P.cache_clear([flat])
        assert P.cached(other, ("k",), make) is eo and P.cached(w, ("k",), make) is ew       # untouched parameters keep their entries
        assert P.cached(va, ("k",), make) is not ea and P.cached(vb, ("k",), make) is not eb
    finally:
        P.cache_end()
    assert P._CACHE is None


def test_bench_flop_model_matches_survey_and_layer_table():
    """bench.flop_per_image is the roofline denominator: its three schedules must reproduce SURVEY.md §8(d)'s totals
    (2713 literal, 2454.6 with the redundant second backward elided, 2342.1 with the shared forward on top), and its per-net
    constants must be the ones the product's own layer table (ideas_amd/flops.py) yields."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert abs(bench.flop_per_image(elided=False, shared=False) - 2713.0) < 0.01 * 2713.0
    assert abs(bench.flop_per_image(elided=True, shared=False) - 2454.6) < 0.002 * 2454.6
    assert abs(bench.flop_per_image(elided=True, shared=True) - 2342.1) < 0.002 * 2342.1
    # R1 amortisation: every d_reg_every-th iteration pays 6 (Dreal + 40 Dco) forward-equivalents
    full, lazy = bench.flop_per_image(True, 1), bench.flop_per_image(True, 16)
    assert abs((full - lazy) - 6 * (bench.F_DR + 40 * bench.F_DC) * (1 - 1 / 16)) < 1e-6
    from ideas_amd.flops import forward_flops
    from ideas_amd.models import init_model
    from ideas_amd.train_step import NET_CLASSES
    a = argparse.Namespace(channel=32, structure_channel=8, texture_channel=2048, N=1, image_size=256,
                           channel_multiplier=1, blur_kernel=(1, 3, 3, 1))
    for tag, const in (("E", bench.F_E), ("G", bench.F_G), ("Gstru", bench.F_GS), ("Ex", bench.F_EX), ("Dreal", bench.F_DR),
                       ("Dco", bench.F_DC)):
        # bench.py quotes SURVEY's two-decimal figures: 1 % for the heavy nets, the rounding of 0.21 / 0.19 for Gstru / Ex
        assert abs(forward_flops(init_model(NET_CLASSES[tag], a), 256) / 1e9 - const) <= max(0.01 * const, 0.005), tag


def test_lmdb_dataset_fails_loudly_without_lmdb():
    import importlib.util
    import pytest
    from ideas_amd import data as D
    if importlib.util.find_spec("lmdb") is None:
        with pytest.raises(ImportError):
            D.set_dataset("lmdb", "/nonexistent", 64)


def test_deferred_d_step_guards_discriminators_and_is_always_waited():
    """between the start of the D group's gradient exchange and the deferred optimiser step no discriminator may run
    (it would read pre-step weights), and an exception in between must still complete the exchange.  A reducer with an asynchronous
    ``start`` and a G network that raises: the handle is waited, the guard flag is cleared, a discriminator call in the window raises."""
    from ideas_amd import train_step as TS
    from ideas_amd.models import init_model
    from test_nets_gpu import ZeroDco
    args = TS.default_args(channel=4, texture_channel=64, channel_multiplier=0.125, image_size=64, batch_size=1, d_reg_every=4,
                           num_iters=10)
    torch.manual_seed(5)
    tr = _oracle_trainer(TS.build_trainer(args, "cpu", init_model, dco_factory=ZeroDco), args)
    waited = []

    class Handle:
        def __init__(self, tag):
            self.tag = tag

        def wait(self):
            waited.append(self.tag)

    class Reducer:
        def __call__(self, tag, params):
            pass

        def start(self, tag, params):
            return Handle(tag)

    calls = {"n": 0}
    real_g = tr["G"]

    class Boom(torch.nn.Module):
        def forward(self, *a, **k):
            calls["n"] += 1
            if calls["n"] == 4:          # the first G call of the G phase: inside the window of the deferred D step
                assert tr["_d_pending"]
                with pytest.raises(TS.DeferredStepError):
                    tr["Ddist"](torch.zeros(1, 64))
                raise ValueError("boom")
            return real_g(*a, **k)

        def parameters(self, recurse=True):
            return real_g.parameters(recurse)
    tr["G"] = Boom()
    X = torch.rand(1, 3, 64, 64) * 2 - 1
    with pytest.raises(ValueError, match="boom"):
        TS.train_iteration(tr, args, X, 1, reducer=Reducer())
    assert waited == ["d"] and not tr["_d_pending"]
    tr["G"] = real_g
    waited.clear()
    TS.train_iteration(tr, args, X, 1, reducer=Reducer())          # the normal path still completes every exchange exactly once
    assert sorted(waited) == ["d", "ex"] and not tr["_d_pending"]
    # the flag is per trainer, and a DIRECT _train_iteration call that raises cleans up after itself -- a second trainer's
    # (or an evaluation's) discriminators keep working in the same process
    tr["G"] = Boom()
    calls["n"] = 0
    waited.clear()
    with pytest.raises(ValueError, match="boom"):
        TS._train_iteration(tr, args, X, 1, reducer=Reducer())
    assert waited == ["d"] and not tr["_d_pending"]
    tr["G"] = real_g
    torch.manual_seed(6)
    other = _oracle_trainer(TS.build_trainer(args, "cpu", init_model, dco_factory=ZeroDco), args)
    TS._guard_discriminators(other)
    tr["_d_pending"] = True
    try:
        other["Ddist"](torch.zeros(1, 64))                          # not this trainer's deferred step: runs
        with pytest.raises(TS.DeferredStepError):
            tr["Ddist"](torch.zeros(1, 64))
    finally:
        tr["_d_pending"] = False


def test_bench_evidence_readers_drop_stale_files(tmp_path, monkeypatch):
    """bench.py quotes two kinds of committed measurements that it cannot take itself -- PMC traffic of the roofline kernels and the
    stock-eager comparator -- and must drop either when it no longer describes the tree (evidence hygiene): the PMC rows
    carry a hash of the kernel sources, the eager files a torch version / comparator source hash / batch sidecar.  Also: the entry's
    own launch is picked when a pass holds several shapes or instantiations of the kernel."""
    import csv
    import hashlib
    import bench
    prof = tmp_path / "profiles"
    prof.mkdir()
    (tmp_path / "ideas_amd" / "csrc").mkdir(parents=True)
    (tmp_path / "ideas_amd" / "csrc" / "k.hip").write_text("kernel v1")
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    sha = bench._src_sha(["k.hip"])
    (prof / "rX_pmc_k_source.json").write_text(json.dumps({"files": ["k.hip"], "sha": sha}))
    hdr = ["Grid_Size", "Kernel_Name", "Counter_Name", "Counter_Value"]
    rows = [(1000, "void k<4, 4, 1, false>(float*)", 100.0), (1000, "void k<4, 4, 1, true>(float*)", 400.0), (3000, "void k<4, 4, 1, false>(float*)", 900.0)]
    for cname, fn, mul in (("FETCH_SIZE", "rX_pmc_k_fetch_size.csv", 1.0), ("WRITE_SIZE", "rX_pmc_k_write_size.csv", 0.5)):
        with open(prof / fn, "w", newline="") as fp:
            w = csv.writer(fp)
            w.writerow(hdr)
            for g_, n_, v_ in rows:
                w.writerow([g_, n_, cname, v_ * mul])
    kb = lambda fetch, write: int((2 * fetch + write) * 1024)
    assert bench._pmc_traffic_of("k<4, 4, 1, false>", "rX_pmc_k")[0] == kb(500.0, 250.0)                    # both grids of that instantiation
    assert bench._pmc_traffic_of("k<4, 4, 1, false>", "rX_pmc_k", smallest_grid=True)[0] == kb(100.0, 50.0) # the entry's own launch
    assert bench._pmc_traffic_of("k<4, 4, 1, true>", "rX_pmc_k")[0] == kb(400.0, 200.0)
    # the newest round whose passes are current wins (round 6: PMC_ROUNDS); a round without files is skipped
    monkeypatch.setattr(bench, "PMC_ROUNDS", ("rY", "rX"))
    assert bench._pmc_traffic("k<4, 4, 1, false>", "pmc_k")[0] == kb(500.0, 250.0)
    (tmp_path / "ideas_amd" / "csrc" / "k.hip").write_text("kernel v2")                                     # the kernel changed: stale
    val, note = bench._pmc_traffic_of("k<4, 4, 1, false>", "rX_pmc_k")
    assert val is None and "stale" in note
    assert bench._pmc_traffic("k<4, 4, 1, false>", "pmc_k")[0] is None

    # eager comparator files: full (default find mode) preferred over fast; any sidecar mismatch drops the file
    for f in ("oracle/torch_ref.py", "tests/eager_baseline.py"):
        os.makedirs(os.path.dirname(tmp_path / f), exist_ok=True)
        (tmp_path / f).write_text("source of " + f)
    src = b"".join(open(tmp_path / f, "rb").read() for f in ("oracle/torch_ref.py", "tests/eager_baseline.py"))
    side = dict(torch_version=torch.__version__, source_sha16=hashlib.sha256(src).hexdigest()[:16], batch=32, convs="MIOpen", steps=3,
                ms_per_step=1000.0)
    a = argparse.Namespace(batch=32)
    assert bench.eager_complete(a) is None
    (prof / "r04_eager_fast.json").write_text(json.dumps(dict(side, eager_gpu_images_per_sec=16.0)))
    assert bench.eager_complete(a)["eager_gpu_images_per_sec"] == 16.0
    (prof / "r04_eager_full.json").write_text(json.dumps(dict(side, eager_gpu_images_per_sec=18.0)))
    assert bench.eager_complete(a)["file"] == "profiles/r04_eager_full.json"
    assert bench.eager_complete(argparse.Namespace(batch=16)) is None                                        # another batch
    (prof / "r04_eager_full.json").write_text(json.dumps(dict(side, eager_gpu_images_per_sec=18.0, torch_version="0.0")))
    assert bench.eager_complete(a)["file"] == "profiles/r04_eager_fast.json"                                 # stale full -> the fast one
    (prof / "r06_eager_full.json").write_text(json.dumps(dict(side, eager_gpu_images_per_sec=18.1)))         # the newest measurement first
    assert bench.eager_complete(a)["file"] == "profiles/r06_eager_full.json"
    (tmp_path / "oracle" / "torch_ref.py").write_text("the comparator's step changed")
    assert bench.eager_complete(a) is None


def test_bench_plain_run_and_output_dump():
    """A plain bench run measures its window only (every side measurement is behind --full, explicit switches still win), and
    --dump-outputs writes the losses and a fixed, seeded, float32 parameter sample per network: the same on every call."""
    import bench
    import numpy as np
    a = bench.parse([])
    assert not a.full and (a.cpu_baseline, a.roofline, a.also_bf16, a.dump_outputs) == ("skip", "off", "off", None)
    a = bench.parse(["--full"])
    assert (a.cpu_baseline, a.roofline, a.also_bf16) == ("auto", "on", "on")
    assert bench.parse(["--roofline", "only"]).roofline == "only" and bench.parse(["--full", "--cpu-baseline", "skip"]).cpu_baseline == "skip"
    torch.manual_seed(0)
    nets = {"big": torch.nn.Sequential(torch.nn.Conv2d(96, 96, 3), torch.nn.Linear(96, 16)), "small": torch.nn.Linear(3, 2), "opt": object()}
    nets["big"][0].weight.data = nets["big"][0].weight.data.contiguous(memory_format=torch.channels_last)
    losses = {"L": torch.tensor(1.5), "hat_Z": torch.randn(2, 1, 4, 4)}
    out = bench.capture_outputs(nets, losses)
    assert set(out) == {"loss_L", "loss_hat_Z", "params_big", "params_small"}
    assert out["params_big"].shape == (bench.DUMP_SAMPLE,) and out["params_big"].dtype == np.float32
    assert np.array_equal(out["params_small"], torch.cat([p.detach().reshape(-1) for p in nets["small"].parameters()]).numpy())
    flat = torch.cat([p.detach().reshape(-1) for p in nets["big"].parameters()]).numpy()
    assert np.isin(out["params_big"], flat).all()                   # values of the parameters, in logical order
    again = bench.capture_outputs(nets, losses)
    assert all(np.array_equal(out[k], again[k]) for k in out)
    assert np.array_equal(out["loss_hat_Z"], losses["hat_Z"].numpy())


def test_bench_restores_the_starting_state_before_every_iteration():
    """bench.py runs every iteration from the same starting state, so that what its timed path computes is the same in every run:
    the restorer puts back every parameter (EMA copies included) and empties the Adam state (the --torch-adam form; the fused
    optimisers' flat buffers need a GPU and are exercised by every bench run)."""
    import bench
    torch.manual_seed(1)
    net, ema = torch.nn.Linear(5, 4), torch.nn.Linear(5, 4)
    tr = {"G": net, "G_ema": ema, "g_optim": torch.optim.Adam(net.parameters(), lr=0.1)}
    before = [p.detach().clone() for p in list(net.parameters()) + list(ema.parameters())]
    restore = bench.state_restorer(tr)
    for _ in range(2):
        net(torch.randn(3, 5)).square().sum().backward()
        tr["g_optim"].step()
        with torch.no_grad():
            for e, p in zip(ema.parameters(), net.parameters()):
                e.lerp_(p, 0.5)
        assert tr["g_optim"].state and not torch.equal(net.weight, before[0])
        restore()
        assert not tr["g_optim"].state
        assert all(torch.equal(p, b) for p, b in zip(list(net.parameters()) + list(ema.parameters()), before))
    with pytest.raises(RuntimeError):
        net(torch.randn(3, 5)).sum().backward()
        tr["g_optim"].step()
        bench.state_restorer(tr)


def test_conv_bias_call_sites_are_the_rgb_head_only():
    """op.conv._AddBias adds the f32 bias parameter to the conv output under torch's type promotion, so in bf16 mode a conv
    with a conv bias and no activation returns f32.  That is intended for G's RGB head (the image leaves G in f32 with one rounding)
    and is only acceptable if no other layer of the seven networks takes that path: a ConvLayer gets a conv bias only with
    ``bias and not activate`` (models.py:54-56 of the reference), which in IDEAS is G.to_rgb alone (models.py:294)."""
    from ideas_amd import train_step as TS
    from ideas_amd.model import EqualConv2d
    from ideas_amd.models import EqualConvTranspose2d, init_model
    args = TS.default_args(channel=4, texture_channel=64, channel_multiplier=0.125, image_size=256)
    sites = []
    for tag, cls in TS.NET_CLASSES.items():
        net = init_model(cls, args)
        for name, m in net.named_modules():
            if isinstance(m, (EqualConv2d, EqualConvTranspose2d)) and m.bias is not None:
                sites.append(f"{tag}.{name}")
    assert sites == ["G.to_rgb.0"], sites


def test_wino_weight_gradient_scratch_is_dropped_when_a_launch_fails(monkeypatch):
    """op.conv._GU keeps ONE zeroed dU scratch per (stream, size), re-zeroed only by the fold that follows the Winograd
    weight-gradient launch.  If that launch or the fold fails, nothing has cleared what was accumulated: the entry must leave _GU,
    so that the next weight gradient of that size starts from a fresh zeroed buffer instead of adding to the leftovers."""
    from ideas_amd import _lib
    from ideas_amd.op import conv as CV
    from ideas_amd.op.conv_plan import ConvGeom

    class Lib:
        fail = None
        seen = []

        def ideas_conv3x3_wino_wgrad(self, gu, *rest):
            (buf,) = [b for b in CV._GU.values() if b.data_ptr() == gu]
            self.seen.append(buf.clone())
            buf.fill_(1.0)                                   # the kernel accumulates dU into the scratch
            return 1 if self.fail == "wgrad" else 0

        def ideas_wino_wgrad_fold(self, tgt, gu, *rest):
            if self.fail == "fold":
                return 1
            (buf,) = [b for b in CV._GU.values() if b.data_ptr() == gu]
            buf.zero_()                                      # clear = 1: re-zeroed behind the read
            return 0

        def ideas_strerror(self, rc):
            return b"injected failure"

    lib = Lib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0)
    monkeypatch.setattr(CV, "_GU", {})
    monkeypatch.setattr(CV, "MATH", _lib.F32)
    monkeypatch.setattr(CV, "WINOGRAD", True)
    g = ConvGeom(3, 3, 1, 1, False)
    x, gy = torch.randn(1, 8, 4, 4), torch.randn(1, 4, 4, 4)

    def run():
        return CV.conv_wgrad_raw(gy, x, g, (4, 8, 3, 3), 1.0)
    for stage in ("wgrad", "fold"):
        lib.fail = stage
        with pytest.raises(RuntimeError, match="injected failure"):
            run()
        assert CV._GU == {}, f"dirty scratch kept after a failing {stage}"
        lib.fail = None
        run()
        assert not lib.seen[-1].any(), f"the launch after a failing {stage} was handed a dirty scratch"
        (buf,) = CV._GU.values()
        assert not buf.any()
        run()                                                # and a good call keeps (and reuses) its scratch
        assert list(CV._GU.values())[0] is buf and not lib.seen[-1].any()
        CV._GU.clear()


def test_cache_cycle_leaves_no_dependency_records(monkeypatch):
    """conv_plan._DEPS (cache key -> further parameters an entry derives from) is keyed like _CACHE and must not outlive
    it: a cache_begin / cache_end cycle leaves it empty, and a new cycle does not start with the last one's records."""
    from ideas_amd.op import conv_plan as P
    monkeypatch.setattr(P, "PREFILL", False)
    w, dep = torch.nn.Parameter(torch.randn(4, 4)), torch.nn.Parameter(torch.randn(4))
    t = torch.randn(2, 4)
    assert P._CACHE is None and not P._DEPS
    P.cache_begin()
    try:
        P.cached_on(w, ("k",), t, lambda: w.detach() * 2, deps=(dep,))
        assert list(P._DEPS.values()) == [(dep.data_ptr(),)]
    finally:
        P.cache_end()
    assert not P._DEPS
    P._DEPS[("left over",)] = (dep.data_ptr(),)              # (whatever put it there)
    P.cache_begin()
    try:
        assert not P._DEPS
    finally:
        P.cache_end()
    assert not P._DEPS
