#!/usr/bin/env python3
"""Time ``PerceptualLoss`` forward + backward with respect to ``pred`` at (4, 3, 256, 256) f32 (seeded random weights: the time does
not depend on their values), and the head ``op.lpips_layer`` alone, forward + backward with respect to the prediction side, on the
five tap shapes of that input -- each next to the torch composition of the same formulas on the same device (for the network:
a second ``PerceptualLoss`` whose head and pool are ``lpips_layer_composition`` / ``F.max_pool2d``; the convolutions are the same).

Device events around forward + backward, warm-up, the variants alternating inside one process, median and spread.  Needs a GPU.

    python tools/bench_lpips.py [--out profiles/lpips.txt] [--batch 4] [--size 256] [--reps 30]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHANNELS = (64, 128, 256, 512, 512)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def seeded_weights(seed=0):
    from ideas_amd.lpips import VGG16_CFG
    gen = torch.Generator().manual_seed(seed)
    sd, cin, idx = {}, 3, 0
    for c in VGG16_CFG:
        if c == "M":
            idx += 1
            continue
        sd[f"features.{idx}.weight"] = torch.randn(c, cin, 3, 3, generator=gen) * (2.0 / (cin * 9)) ** 0.5
        sd[f"features.{idx}.bias"] = torch.randn(c, generator=gen) * 0.1
        cin, idx = c, idx + 2
    lin = {f"lin{k}.model.1.weight": torch.rand(1, c, 1, 1, generator=gen) for k, c in enumerate(CHANNELS)}
    return sd, lin


def alternate(variants, warmup, reps):
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in variants}
    for _ in range(reps):
        for name, fn in variants:
            ts[name].append(event_ms(fn))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips.txt"))
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips needs a GPU")
    import torch.nn.functional as F
    import ideas_amd.lpips as L
    import ideas_amd.op as op
    from ideas_amd.op.lpips import lpips_layer_composition

    b, r = args.batch, args.size
    sd, lin = seeded_weights()
    percept = L.PerceptualLoss(backbone=sd, lin_weights=lin).cuda()
    composed = L.PerceptualLoss(backbone=sd, lin_weights=lin).cuda()        # the same convolutions; pool and head as torch compositions
    composed.net.pool = lambda x: F.max_pool2d(x, 2, 2)
    composed.head = lpips_layer_composition
    gen = torch.Generator(device="cuda").manual_seed(1)
    pred = (torch.rand(b, 3, r, r, device="cuda", generator=gen) * 2 - 1).requires_grad_(True)
    target = torch.rand(b, 3, r, r, device="cuda", generator=gen) * 2 - 1

    def step(module):
        val = module(pred, target)
        (g,) = torch.autograd.grad(val.sum(), pred)
        return val.detach(), g

    lines = []
    ts = alternate((("kernels", lambda: step(percept)), ("composed", lambda: step(composed))), args.warmup, args.reps)
    (v_a, g_a), (v_b, g_b) = step(percept), step(composed)
    lines.append("PerceptualLoss forward + backward w.r.t. pred, (%d, 3, %d, %d) f32; median of %d alternating runs, ms [min .. max]" % (b, r, r, args.reps))
    for name in ("kernels", "composed"):
        v = ts[name]
        lines.append("%-9s %8.3f  [%8.3f .. %8.3f]" % (name, statistics.median(v), min(v), max(v)))
    lines.append("kernels vs composed: val %.2e, input gradient %.2e (max abs over max abs)"
                 % (float((v_a - v_b).abs().max() / v_b.abs().max()), float((g_a - g_b).abs().max() / g_b.abs().max())))

    lines.append("op.lpips_layer forward + backward w.r.t. the prediction side alone, per tap shape:")
    for k, c in enumerate(CHANNELS):
        hw = r >> k
        f0 = torch.relu(torch.randn(b, c, hw, hw, device="cuda", generator=gen)).contiguous(memory_format=torch.channels_last)
        f1 = torch.relu(torch.randn(b, c, hw, hw, device="cuda", generator=gen)).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        w = percept.lin(k)

        def head(fn, f0=f0, f1=f1, w=w):
            d = fn(f0, f1, w)
            (g,) = torch.autograd.grad(d.sum(), f1)
            return d.detach(), g
        ts = alternate((("kernel", lambda: head(op.lpips_layer)), ("composed", lambda: head(lpips_layer_composition))), args.warmup, args.reps)
        (d_a, g_a), (d_b, g_b) = head(op.lpips_layer), head(lpips_layer_composition)
        lines.append("(%d, %3d, %3d, %3d)  kernel %8.3f [%8.3f .. %8.3f]   composed %8.3f [%8.3f .. %8.3f]   d %.1e  grad %.1e"
                     % (b, c, hw, hw, statistics.median(ts["kernel"]), min(ts["kernel"]), max(ts["kernel"]), statistics.median(ts["composed"]),
                        min(ts["composed"]), max(ts["composed"]), float((d_a - d_b).abs().max() / d_b.abs().max()),
                        float((g_a - g_b).abs().max() / g_b.abs().max())))
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
