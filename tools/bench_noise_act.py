#!/usr/bin/env python3
"""Time ``op.noise_bias_act`` (one pass forward, one pass backward) against the two-op composition it replaces,
``fused_leaky_relu(x + noise_weight * noise, bias)``, at the ``StyledConv`` output shapes of ``Generator(256)``, batch 32, in f32 and bf16.

Device events around each call, warm-up, many repetitions, median; the two variants alternate inside one process.  Bytes are the
ones the fused kernels need (x + out forward; gy + out + gx backward), so "GB/s" of the composition is the same useful traffic over
its longer time.  Needs a GPU.

    python tools/bench_noise_act.py [--out profiles/noise_act.txt] [--batch 32] [--reps 30]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (channels, resolution) of the StyledConv outputs of Generator(256, channel_multiplier=2): conv1, then two per resolution
SHAPES = [(512, 4), (512, 8), (512, 16), (512, 32), (512, 64), (256, 128), (128, 256)]


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_act.txt"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_noise_act needs a GPU")
    import ideas_amd.op as op
    lines = ["noise_bias_act vs fused_leaky_relu(x + w * noise, bias): median of %d, ms (useful GB/s); batch %d" % (args.reps, args.batch),
             "%-6s %-18s %22s %22s %22s %22s" % ("dtype", "C x H x W", "fused fwd", "composed fwd", "fused bwd", "composed bwd")]
    for dtype, name, esz in ((torch.float32, "f32", 4), (torch.bfloat16, "bf16", 2)):
        for c, r in SHAPES:
            g = torch.Generator(device="cuda").manual_seed(c + r)
            x = torch.randn(args.batch, c, r, r, device="cuda", generator=g).to(dtype).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            gy = torch.randn(args.batch, c, r, r, device="cuda", generator=g).to(dtype).contiguous(memory_format=torch.channels_last)
            noise = torch.randn(args.batch, 1, r, r, device="cuda", generator=g)
            nw = torch.full((1,), 0.3, device="cuda", requires_grad=True)
            bias = torch.randn(c, device="cuda", generator=g).requires_grad_(True)
            fused = lambda: op.noise_bias_act(x, noise, nw, bias)
            composed = lambda: op.fused_leaky_relu(x + (nw * noise).to(dtype), bias)
            res = []
            for fwd in (fused, composed):
                t_f = timed(lambda: fwd(), args.warmup, args.reps)
                out = fwd()
                t_b = timed(lambda: torch.autograd.grad(out, (x, nw, bias), gy, retain_graph=True), args.warmup, args.reps)
                res.append((t_f, t_b))
                del out
            n = x.numel()
            cell = lambda ms, passes: "%8.3f (%7.0f)" % (ms, passes * n * esz / ms / 1e6)
            lines.append("%-6s %-18s %22s %22s %22s %22s" % (name, "%d x %d x %d" % (c, r, r), cell(res[0][0], 2), cell(res[1][0], 2),
                                                             cell(res[0][1], 3), cell(res[1][1], 3)))
            print(lines[-1], flush=True)
            del x, gy, noise
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
