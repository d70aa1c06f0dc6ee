#!/usr/bin/env python3
"""Writes tests/golden/splitk_plans.npz: the split-K plans of the convolution weight-gradient launchers as commit c810799 computed
them, for tests/test_host_logic.py::test_splitk_plans_match_pinned.

Each ``plan_*`` below is a literal transcription into Python of the launcher's host arithmetic at that commit (file and lines cited;
every quantity is positive, so ``//`` is C's integer division).  Where the launcher used a fixed number of resident blocks, that
constant is the ``slots`` argument here, as it is in the library's diagnostic query (ideas_conv_splitk_plan).  A row of results is
what the launcher passed to its kernel: (splits | ranges, units per split, splits per image | parts | 0, slots).

The npz holds the sweep (``cases``: B, OH, OW, Cin, Cout, taps per side, slots) and per site the indices of the cases it admits,
the SHA-256 of the int64 result array and its first 16 rows.  No GPU and no library are needed to run this:
    python tests/golden/make_golden_splitk_plans.py [out.npz]
"""
import hashlib
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
GOLDEN = os.path.join(HERE, "splitk_plans.npz")
SLOTS = (256, 512, 768, 1024)


def cdiv(a, b):
    return (a + b - 1) // b


_JUST_ABOVE = [False]


def _waves_rebalance(P, per, splits, tiles, slots, step):
    # conv_igemm.hip:508-518 (and, line for line, conv_b3_wgrad.hip:243-253, conv_wino.hip:468-474)
    blocks = tiles * splits
    waves = blocks // slots
    _JUST_ABOVE[0] = waves >= 1 and 0 < blocks % slots <= slots // 16      # (for sweep() below; not part of the transcription)
    if waves >= 1 and blocks % slots:
        want = (waves * slots) // tiles
        if want >= 1:
            per = cdiv(cdiv(P, want), step) * step
            splits = cdiv(P, per)
    return per, splits


def _igemm_tile(Cout):
    # conv_igemm.hip:613-615: <2,2,2,2> 128 x 128, <2,2,1,2> 64 x 128, <1,4,1,1> 32 x 128 (BM = WM*MT*32, BN = WN*NT*32)
    return (128, 128) if Cout > 64 else (64, 128) if Cout > 32 else (32, 128)


def plan_igemm(B, OH, OW, Cin, Cout, K, slots):
    # conv_igemm.hip:477-518 (launch_wgrad_cfg), BK = 16 (line 31)
    BM, BN = _igemm_tile(Cout)
    BK = 16
    P = B * OH * OW
    Ktot = K * K * Cin
    tiles = cdiv(Cout, BM) * cdiv(Ktot, BN)
    max_splits = cdiv(P, 16 * BK)
    splits = (2 * slots) // tiles
    if splits < 1:
        splits = 1
    if splits > max_splits:
        splits = max_splits
    if splits > 65535:
        splits = 65535
    per = cdiv(cdiv(P, splits), BK) * BK
    splits = cdiv(P, per)
    per, splits = _waves_rebalance(P, per, splits, tiles, slots, BK)
    return splits, per, 0, slots


def plan_wino(B, OH, OW, Cin, Cout, K, slots):
    # conv_wino.hip:449-474 (ideas_conv3x3_wino_wgrad), GBM = 64, GBN = 128, GBK = 8 (line 227); IH = OH, IW = OW
    GBM, GBN, GBK = 64, 128, 8
    P2 = B * OH * (OW // 2)
    Ktot = 3 * Cin
    tiles = cdiv(Cout, GBM) * cdiv(Ktot, GBN)
    max_splits = cdiv(P2, 16 * GBK)
    splits = (2 * slots) // tiles
    if splits < 1:
        splits = 1
    if splits > max_splits:
        splits = max_splits
    if splits > 65535:
        splits = 65535
    per = cdiv(cdiv(P2, splits), GBK) * GBK
    splits = cdiv(P2, per)
    per, splits = _waves_rebalance(P2, per, splits, tiles, slots, GBK)
    return splits, per, 0, slots


def plan_b3_wgrad(B, OH, OW, Cin, Cout, K, slots):
    # conv_b3_wgrad.hip:215-253 (launch_b3_wgrad_cfg); tiles of lines 287-288: <2,2,1,3> 64 x 192 for Cout <= 64, else 128 x 128
    BM, BN = (64, 192) if Cout <= 64 else (128, 128)
    P = B * OH * OW
    Ktot = K * K * Cin
    tiles = cdiv(Cout, BM) * cdiv(Ktot, BN)
    max_splits = cdiv(P, 16 * 16)
    splits = (4 * slots) // tiles
    if splits < 1 or P // splits < 4096:
        splits = (2 * slots) // tiles
    if splits < 1:
        splits = 1
    if splits > max_splits:
        splits = max_splits
    if splits > 65535:
        splits = 65535
    per = cdiv(cdiv(P, splits), 16) * 16
    splits = cdiv(P, per)
    per, splits = _waves_rebalance(P, per, splits, tiles, slots, 16)
    return splits, per, 0, slots


def plan_b3_wgrad3(B, OH, OW, Cin, Cout, K, slots):
    # conv_b3_wgrad3.hip:294-306 (launch_wgrad3); `slots` was the constant 512 (line 298)
    tiles_ci = Cin // 64
    tiles = (Cout // 64) * tiles_ci
    strips = OW // 16
    rows_total = B * OH
    spl = (4 * slots) // (tiles * strips)
    if spl < 1 or rows_total // spl < 128:
        spl = (2 * slots) // (tiles * strips)
    if spl < 1:
        spl = 1
    max_spl = rows_total // 16 if rows_total // 16 > 0 else 1
    if spl > max_spl:
        spl = max_spl
    per = cdiv(rows_total, spl)
    spl = cdiv(rows_total, per)
    splits = spl * strips
    return splits, per, 0, slots


def plan_b3_pw(B, OH, OW, Cin, Cout, K, slots):
    # conv_b3_pw.hip:569-576 (ideas_b3_pw_wgrad); `slots` was the constant 2048 (line 572)
    M = B * OH * OW
    tiles_ci = Cin // 64
    tiles = (Cout // 64) * tiles_ci
    ranges = slots // tiles
    if ranges < 1:
        ranges = 1
    if M // ranges < 256:
        ranges = M // 256 if M // 256 > 0 else 1
    per = cdiv(cdiv(M, ranges), 32) * 32
    ranges = cdiv(M, per)
    return ranges, per, 0, slots


def _plan_bf16(sc, B, OH, OW, Cin, Cout, K, slots):
    # conv_bf16.hip:865-894 (launch_bf16_wgrad_cfg); tiles of lines 1262-1264 = those of conv_igemm.hip; `slots` was
    # (WM * WN == 8 ? 1 : 2) * 256 = 512 for all three tiles (line 874)
    BM, BN = _igemm_tile(Cout)
    P = B * OH * OW
    Ktot = K * K * Cin
    tiles = cdiv(Cout, BM) * cdiv(Ktot, BN)
    img = OH * OW
    splits = (4 * slots) // tiles
    if splits < 1 or P // splits < 4096:
        splits = (2 * slots) // tiles
    if splits < 1:
        splits = 1
    spi = 1
    if sc:
        spi = splits // B
        max_spi = cdiv(img, 32 * 4)
        if spi > max_spi:
            spi = max_spi
        if spi < 1:
            spi = 1
        per = cdiv(cdiv(img, spi), 32) * 32
        spi = cdiv(img, per)
        splits = spi * B
    else:
        max_splits = cdiv(P, 32 * 8)
        if splits > max_splits:
            splits = max_splits
        per = cdiv(cdiv(P, splits), 32) * 32
        splits = cdiv(P, per)
    return splits, per, spi, slots


def plan_bf16(*a):
    return _plan_bf16(False, *a)


def plan_bf16_scaled(*a):
    return _plan_bf16(True, *a)


def plan_bf16_wgrad3(B, OH, OW, Cin, Cout, K, slots):
    # conv_bf16.hip:1231-1241 (launch_bf16_wgrad3); `slots` was the constant 512 (line 1235: 4 * 512)
    tiles_ci = Cin // 64
    tiles = (Cout // 64) * tiles_ci
    strips = OW // 32
    base = tiles * strips * B
    parts = (4 * slots) // base
    if parts < 1:
        parts = 1
    while parts > 1 and OH // parts < 32:
        parts -= 1
    if parts > OH // 8:
        parts = OH // 8 if OH // 8 > 0 else 1
    rows = cdiv(OH, parts)
    parts = cdiv(OH, rows)
    splits = strips * B * parts
    return splits, rows, parts, slots


def _c64(Cin, Cout):
    return Cin % 64 == 0 and Cout % 64 == 0


# name -> (site number of ideas_conv_splitk_plan, its scaled flag, the transcription, the cases whose arithmetic the launcher's
# *_supported rule allows: no division by zero tiles / strips)
SITES = {
    "igemm": (0, 0, plan_igemm, lambda B, OH, OW, Cin, Cout, K, s: True),
    "wino": (1, 0, plan_wino, lambda B, OH, OW, Cin, Cout, K, s: K == 3 and OW % 2 == 0),
    "b3_wgrad": (2, 0, plan_b3_wgrad, lambda B, OH, OW, Cin, Cout, K, s: True),
    "b3_wgrad3": (3, 0, plan_b3_wgrad3, lambda B, OH, OW, Cin, Cout, K, s: K == 3 and OW % 16 == 0 and _c64(Cin, Cout)),
    "b3_pw": (4, 0, plan_b3_pw, lambda B, OH, OW, Cin, Cout, K, s: K == 1 and _c64(Cin, Cout)),
    "bf16": (5, 0, plan_bf16, lambda B, OH, OW, Cin, Cout, K, s: True),
    "bf16_scaled": (5, 1, plan_bf16_scaled, lambda B, OH, OW, Cin, Cout, K, s: True),
    "bf16_wgrad3": (6, 0, plan_bf16_wgrad3, lambda B, OH, OW, Cin, Cout, K, s: K == 3 and OW % 32 == 0 and _c64(Cin, Cout) and OH >= 8),
}


def network_layers(image_size=256):
    """(Cin, Cout, taps, OH, OW, samples per image) of every convolution weight gradient of the six networks at the benchmark's
    configuration, by the shape walk of ideas_amd/flops.py (no tensors, no device).  A transposed conv's weight gradient is the
    conv weight gradient with the roles of x and gy exchanged: reduction over the INPUT grid, Cin = its output channels."""
    from torch import nn
    from ideas_amd import models as M
    from ideas_amd.model import Blur, EqualConv2d, StyledConv_without_noise
    from ideas_amd.train_step import NET_CLASSES
    args = SimpleNamespace(channel=32, channel_multiplier=1, structure_channel=8, texture_channel=2048, N=1, image_size=image_size,
                           blur_kernel=(1, 3, 3, 1))
    out = []

    def conv_layer(seq, c, h, w, mult):
        for m in seq:
            if isinstance(m, Blur):
                kh, kw = m.kernel.shape
                h, w = h + m.pad[0] + m.pad[1] - kh + 1, w + m.pad[0] + m.pad[1] - kw + 1
            elif isinstance(m, nn.ReflectionPad2d):
                h, w = h + 2 * m.padding[0], w + 2 * m.padding[0]
            elif isinstance(m, EqualConv2d):
                o, i, k, _ = m.weight.shape
                h, w = (h + 2 * m.padding - k) // m.stride + 1, (w + 2 * m.padding - k) // m.stride + 1
                out.append((i, o, k, h, w, mult))
                c = o
            elif isinstance(m, M.EqualConvTranspose2d):
                i, o, k, _ = m.weight.shape
                out.append((o, i, k, h, w, mult))
                c, h, w = o, (h - 1) * m.stride + k, (w - 1) * m.stride + k
        return c, h, w

    def styled(sc, c, h, w):
        m = sc.conv
        _, o, i, k, _ = m.weight.shape
        out.append((o, i, k, h, w, 1) if m.upsample else (i, o, k, h, w, 1))
        if m.upsample:
            h, w = 2 * h + 1, 2 * w + 1
            kh, kw = m.blur.kernel.shape
            h, w = h + m.blur.pad[0] + m.blur.pad[1] - kh + 1, w + m.blur.pad[0] + m.blur.pad[1] - kw + 1
        return o, h, w

    def seq(mods, c, h, w, mult=1):
        for m in mods:
            if isinstance(m, M.ConvLayer):
                c, h, w = conv_layer(m, c, h, w, mult)
            elif isinstance(m, M.ResBlock):
                if m.skip is not None:
                    conv_layer(m.skip, c, h, w, mult)
                c, h, w = conv_layer(m.conv2, *conv_layer(m.conv1, c, h, w, mult), mult)
            elif isinstance(m, nn.AdaptiveAvgPool2d):
                h, w = 1, 1
        return c, h, w

    r = image_size
    for name in sorted(set(NET_CLASSES.values())):
        net = M.init_model(name, args)
        if isinstance(net, M.DisentanglementEncoder):
            c, h, w = seq(net.stem, 3, r, r)
            seq(net.structure, c, h, w)
            seq(net.texture, c, h, w)
        elif isinstance(net, M.Generator):
            c, h, w = net.layers[0].conv1.conv.in_channel, r // 16, r // 16
            for layer in net.layers:
                if layer.skip is not None:
                    conv_layer(layer.skip, c, h, w, 1)
                c, h, w = styled(layer.conv2, *styled(layer.conv1, c, h, w))
            conv_layer(net.to_rgb, c, h, w, 1)
        elif isinstance(net, M.StructureGenerator):
            seq(net.structure, net.structure[0][0].weight.shape[1], r // 16, r // 16)
        elif isinstance(net, M.TensorExtractor):
            seq(net.extract, net.extract[0][0].weight.shape[1], r // 16, r // 16)
        elif isinstance(net, M.ImageLevelDiscriminator):
            c, h, w = seq(net.convs, 3, r, r)
            conv_layer(net.final_conv, c, h, w, 1)
        elif isinstance(net, M.CooccurenceDiscriminator):
            seq(net.encoder, 3, r // 4, r // 4, mult=8)      # 8 patches per image
    return sorted(set(out))


def sweep():
    cases = set()
    # the six networks: the benchmark's configuration (B = 32) and B = 1, 2, 3
    for (ci, co, k, oh, ow, mult) in network_layers():
        if k in (1, 3):
            for B in (32, 1, 2, 3):
                for s in SLOTS:
                    cases.add((B * mult, oh, ow, ci, co, k, s))
    # the grid
    for B in (1, 2, 3, 32):
        for hw in (4, 8, 16, 32, 64, 256):
            for ci in (32, 64, 128, 512):
                for co in (32, 64, 128, 512):
                    for k in (1, 3):
                        for s in SLOTS:
                            cases.add((B, hw, hw, ci, co, k, s))
    # block counts just above a whole number of waves (conv_igemm.hip:483-484: 1026 blocks on 1024 slots): every shape of a scan at
    # which one of the three launchers with the re-balance finds at most slots / 16 blocks in the last wave
    for B in range(1, 9):
        for hw in range(16, 129, 4):
            for (ci, co) in ((64, 64), (128, 128), (64, 256), (512, 512), (32, 96)):
                for s in SLOTS:
                    c = (B, hw, hw, ci, co, 3, s)
                    for f in (plan_igemm, plan_wino, plan_b3_wgrad):
                        f(*c)
                        if _JUST_ABOVE[0]:
                            cases.add(c)
    # scaled bf16: images smaller than one split (32 pixels), and a little larger
    for B in (1, 5, 64, 200):
        for (oh, ow) in ((4, 4), (2, 8), (4, 8), (8, 8), (6, 6), (12, 12)):
            for (ci, co) in ((64, 64), (512, 512)):
                cases.add((B, oh, ow, ci, co, 3, 512))
    # the tap-fused launchers: OH not a multiple of the part size
    for B in (1, 2, 3, 32):
        for oh in (8, 9, 31, 33, 40, 72, 100, 136, 250):
            for ow in (32, 64, 96):
                for (ci, co) in ((64, 64), (128, 256), (512, 512)):
                    for s in (512, 768):
                        cases.add((B, oh, ow, ci, co, 3, s))
    # irregular shapes (seeded): batch and image sizes that are no powers of two land ON the thresholds of the rules (a share of
    # exactly 4096 pixels, 128 rows, 256 pixels ...), which the regular grid above mostly steps over; 2048 = the flat kernel's count
    rng = np.random.RandomState(20261019)
    for _ in range(6000):
        B = int(rng.choice((1, 2, 3, 5, 6, 7, 12, 24, 32, 40, 96)))
        ow = int(rng.choice((8, 16, 32, 48, 64, 96, 128, 160, 256)))
        oh = int(rng.choice((4, 8, 12, 16, 24, 31, 32, 33, 40, 64, 65, 100, 128, 136, 256, 257)))
        ci, co = (int(rng.choice((32, 64, 128, 192, 256, 512))) for _ in range(2))
        cases.add((B, oh, ow, ci, co, int(rng.choice((1, 3))), int(rng.choice(SLOTS + (2048,)))))
    # thresholds the shapes above do not land on: the flat kernel's 256 pixels per range (M = 256 * (ranges + 1): 19 x 27 x 256 on
    # 512 ranges) and a share of exactly 4096 pixels on four waves of 512 slots
    cases.add((19, 27, 256, 128, 128, 1, 2048))
    cases.add((32, 512, 512, 128, 128, 1, 512))
    return np.array(sorted(cases), dtype=np.int64)


def digest(rows):
    a = np.ascontiguousarray(rows, dtype=np.int64)
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    cases = sweep()
    d = {"cases": cases.astype(np.int32)}
    for name, (site, scaled, plan, admits) in SITES.items():
        idx = np.array([i for i, c in enumerate(cases.tolist()) if admits(*c)], dtype=np.int32)
        rows = np.array([plan(*cases[i].tolist()) for i in idx], dtype=np.int64)
        d[name + "/site"] = np.array([site, scaled], dtype=np.int64)
        d[name + "/idx"] = idx
        d[name + "/n"] = np.int64(len(idx))
        d[name + "/sha256"] = digest(rows)
        d[name + "/head"] = rows[:16]
        print(name, len(idx), bytes(d[name + "/sha256"]).hex()[:16])
    np.savez_compressed(out, **d)
    print("wrote", out, os.path.getsize(out), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
