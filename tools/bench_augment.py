#!/usr/bin/env python3
"""Time ``non_leaking.augment`` forward + backward at (32, 3, 256, 256), p = 0.6, fixed matrices, f32, next to the same pipeline
with the two fused ops replaced by the compositions f16 / f64 tensors take (``op.upfirdn2d`` + the grid built from theta + stock
``F.grid_sample`` + the permute / matmul colour step), and the two 12x12 FIR passes on their own.

Device events around forward + backward, warm-up, the variants alternating inside one process, median and spread.  The two variants'
outputs and input gradients are compared at the timed size.  Needs a GPU.

    python tools/bench_augment.py [--out profiles/augment.txt] [--batch 32] [--size 256] [--reps 30]
"""
import argparse
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment.txt"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--p", type=float, default=0.6)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment needs a GPU")
    import ideas_amd.op as op
    import ideas_amd.non_leaking as NL
    from ideas_amd.op.augment import affine_warp_composition, color_affine_composition

    b, r = args.batch, args.size
    torch.manual_seed(0)
    while True:                                   # fixed matrices that admit a reflect pad
        G = NL.sample_affine(args.p, b, r, r)
        pads = NL.get_padding(torch.inverse(G), r, r)
        if max(pads) + 6 < r:
            break
    C = NL.sample_color(args.p, b)
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(b, 3, r, r, device="cuda", generator=gen).requires_grad_(True)
    cot = torch.randn(b, 3, r, r, device="cuda", generator=gen)
    composed_ops = types.SimpleNamespace(upfirdn2d=op.upfirdn2d, affine_warp=affine_warp_composition, color_affine=color_affine_composition)

    def step(ops):
        NL.op = ops
        try:
            y, _ = NL.augment(x, args.p, (G, C))
            (gx,) = torch.autograd.grad(y, x, cot)
        finally:
            NL.op = op
        return y.detach(), gx

    k1 = torch.tensor(NL.SYM6)
    k = torch.ger(k1, k1).cuda()
    kf = torch.flip(k, (0, 1))
    h2, w2 = NL.warp_hw((r, r), pads, 12)
    x_pad = torch.randn(b, 3, (h2 + 11) // 2, (w2 + 11) // 2, device="cuda", generator=gen).requires_grad_(True)
    x_2x = torch.randn(b, 3, h2, w2, device="cuda", generator=gen).requires_grad_(True)

    def fir_only():
        u = op.upfirdn2d(x_pad, kf, up=2)
        d = op.upfirdn2d(x_2x, k, down=2)
        torch.autograd.grad((u, d), (x_pad, x_2x), (torch.ones_like(u), torch.ones_like(d)))

    variants = (("fused", lambda: step(op)), ("composed", lambda: step(composed_ops)), ("fir_only", fir_only))
    for _ in range(args.warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in variants}
    for _ in range(args.reps):
        for name, fn in variants:
            ts[name].append(event_ms(fn))
    (y_a, g_a), (y_b, g_b) = step(op), step(composed_ops)
    dy = float((y_a - y_b).abs().max() / y_b.abs().max())
    dg = float((g_a - g_b).abs().max() / g_b.abs().max())
    lines = ["augment forward + backward, (%d, 3, %d, %d), p = %.1f, f32, pads %s, 2x image %d x %d; median of %d alternating runs, ms [min .. max]"
             % (b, r, r, args.p, pads, h2, w2, args.reps)]
    for name, _ in variants:
        v = ts[name]
        lines.append("%-9s %8.3f  [%8.3f .. %8.3f]" % (name, statistics.median(v), min(v), max(v)))
    lines.append("fused vs composed: output %.2e, input gradient %.2e (max abs over max abs)" % (dy, dg))
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
