#!/usr/bin/env python3
"""Forward of the downsampling modulated conv: the fused launch (ideas_b3_blur_conv_s2_mod, csrc/conv_b3_s2fir.hip with per-sample
scales) against the two-kernel chain it replaces -- upfirdn2d(x, fir, pad) then conv_fwd_raw(ConvGeom(3, 3, 2, 0), lin=s, lout=d) --
in one process, the two alternating sample by sample.  A sample = `--inner` back-to-back launches between two events; reported: the
median over `--samples` samples per launch, after a warm-up of both.  `blocks` = workgroups of the fused launch (the quantity
op.conv.BLUR_CONV_MOD_MIN_BLOCKS thresholds).  The outputs are compared as well (y: rel. max error; side output: bitwise).
    python tools/bench_modconv_down.py [--samples 30] [--inner 10] > profiles/modconv_down_fwd.txt"""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ideas_amd.model import make_kernel  # noqa: E402
from ideas_amd.op import conv as convmod  # noqa: E402
from ideas_amd.op import conv_plan  # noqa: E402
from ideas_amd.op.conv_plan import ConvGeom  # noqa: E402
from ideas_amd.op.upfirdn2d import upfirdn2d_raw  # noqa: E402

CL = torch.channels_last
# B, Cin, Cout, raw H: the dispatched shapes of tests/test_modconv_down_gpu.py first, then a sweep over the workgroup count
SHAPES = [(4, 64, 128, 64), (2, 128, 256, 64), (2, 512, 512, 32),
          (16, 64, 128, 64), (64, 64, 128, 64), (8, 64, 64, 128), (32, 64, 64, 128), (8, 128, 128, 128), (32, 128, 128, 128),
          (8, 128, 256, 64), (32, 256, 256, 64), (16, 256, 512, 32), (8, 512, 512, 32), (32, 512, 512, 32), (64, 512, 512, 16)]


def sample(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_modconv_down.py measures on the GPU; none found")
    fir = make_kernel((1, 3, 3, 1)).cuda()
    g = ConvGeom(3, 3, 2, 0, False)
    conv_plan.cache_begin()
    print(f"# {torch.cuda.get_device_name(0)}; median of {a.samples} samples x {a.inner} launches, ms per launch; chain = blur + scaled conv")
    print("#  B  Cin Cout    H blocks |  chain   fused  ratio | fused+xb  ratio | y vs chain  xb bitwise")
    for B, ci, co, H in SHAPES:
        torch.manual_seed(B + ci + co + H)
        x = torch.randn(B, ci, H, H, device="cuda").contiguous(memory_format=CL)
        w = torch.nn.Parameter(torch.randn(co, ci, 3, 3, device="cuda").contiguous(memory_format=CL))
        s = torch.rand(B, ci, device="cuda") + 0.5
        d = torch.rand(B, co, device="cuda") + 0.5
        gain = 1 / math.sqrt(9 * ci)
        hb = H + 1
        if not convmod.blur_conv_s2_ok(x, w, fir, (2, 2), want_xb=True):
            print(f"{B:4d} {ci:4d} {co:4d} {H:4d}: not covered by the fused kernel")
            continue
        blocks = convmod._blur_conv_blocks(convmod._blur_conv_plan(tuple(x.shape), w, fir, (2, 2))[0])

        def chain():
            xb = upfirdn2d_raw(x, fir, (1, 1), (1, 1), (2, 2, 2, 2), (hb, hb), flip=True)
            return convmod.conv_fwd_raw(xb, w, g, gain, lin=s, lout=d), xb

        def fused():
            return convmod.blur_conv_s2_raw(x, w, fir, (2, 2), gain, lin=s, lout=d)

        def fused_xb():
            return convmod.blur_conv_s2_raw(x, w, fir, (2, 2), gain, lin=s, lout=d, want_xb=True)
        fns = (chain, fused, fused_xb)
        for fn in fns:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ts = [[], [], []]
        for _ in range(a.samples):
            for i, fn in enumerate(fns):
                ts[i].append(sample(fn, a.inner))
        tc, tf, tx = (statistics.median(t) for t in ts)
        y0, xb0 = chain()
        y1, xb1 = fused_xb()
        err = float((y1 - y0).abs().max() / y0.abs().max())
        print(f"{B:4d} {ci:4d} {co:4d} {H:4d} {blocks:6d} | {tc:6.3f} {tf:6.3f} {tf / tc:6.3f} | {tx:8.3f} {tx / tc:6.3f} | {err:10.1e}  "
              f"{bool(torch.equal(xb1, xb0))}", flush=True)
        del x, y0, y1, xb0, xb1
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
