#!/usr/bin/env python3
"""Time the FID path at batch 64 (seeded random weights: the time does not depend on their values):

* ``InceptionV3([3])`` forward on (64, 3, 299, 299) f32, next to a second instance whose fourteen 3x3 pools and global average are
  the torch compositions (``F.max_pool2d`` / ``F.avg_pool2d`` / ``F.adaptive_avg_pool2d`` on the same device; the convolutions are the
  same kernels);
* ``op.pool3x3`` / ``op.global_avg_pool`` alone on the shapes the network gives them, against the same compositions;
* ``FeatureStats.update`` on (64, 2048) features against ``features.double().T @ features.double()`` (+ the column sum) added into
  f64 accumulators.

Device events, warm-up, the variants alternating inside one process, median and spread.  Needs a GPU.  The weights are the seeded
stand-in of tests/fid_ref.py.

    python tools/bench_fid.py [--out profiles/fid.txt] [--batch 64] [--reps 20]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


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


def row(ts, name):
    v = ts[name]
    return "%s %9.3f [%9.3f .. %9.3f]" % (name, statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fid.txt"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fid needs a GPU")
    import fid_ref as FR
    from ideas_amd.fid import FeatureStats
    from ideas_amd.inception import InceptionV3
    from ideas_amd.op import pool as P

    b = args.batch
    sd = FR.backbone_state()
    net = InceptionV3([3], normalize_input=False, weights=sd).cuda()
    composed = InceptionV3([3], normalize_input=False, weights=sd).cuda()     # the same convolutions; the pools as torch compositions
    for m in composed.modules():
        if hasattr(m, "pool3x3"):
            m.pool3x3 = P.pool3x3_composition
    composed.global_avg_pool = P.global_avg_pool_composition
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(b, 3, 299, 299, device="cuda", generator=gen) * 2 - 1
    lines = []
    ts = alternate((("kernels ", lambda: net(x)), ("composed", lambda: composed(x))), args.warmup, args.reps)
    fa, fb = net(x)[0], composed(x)[0]
    lines.append("InceptionV3([3]) forward, (%d, 3, 299, 299) f32; median of %d alternating runs, ms [min .. max]" % (b, args.reps))
    lines += [row(ts, "kernels "), row(ts, "composed")]
    lines.append("kernels vs composed: features %.2e (max abs over max abs); %.1f images/s on the kernels"
                 % (float((fa - fb).abs().max() / fb.abs().max()), 1e3 * b / statistics.median(ts["kernels "])))

    lines.append("the pools alone, channels_last f32, on the shapes of the network:")
    shapes = [((64, 147, 147), P.MAX_S2, "MAX_S2"), ((192, 71, 71), P.MAX_S2, "MAX_S2"), ((288, 35, 35), P.AVG_S1P1_VALID, "AVG_S1P1_VALID"),
              ((288, 35, 35), P.MAX_S2, "MAX_S2"), ((768, 17, 17), P.AVG_S1P1_VALID, "AVG_S1P1_VALID"), ((768, 17, 17), P.MAX_S2, "MAX_S2"),
              ((1280, 8, 8), P.AVG_S1P1_VALID, "AVG_S1P1_VALID"), ((2048, 8, 8), P.MAX_S1P1, "MAX_S1P1")]
    for (c, h, w), mode, name in shapes:
        t = torch.randn(b, c, h, w, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
        ts = alternate((("kernel", lambda: P.pool3x3(t, mode)), ("composed", lambda: P.pool3x3_composition(t, mode))), args.warmup, args.reps)
        d = float((P.pool3x3(t, mode) - P.pool3x3_composition(t, mode)).abs().max())
        gb = (t.numel() + P.pool3x3(t, mode).numel()) * 4 / 1e9
        lines.append("(%d, %4d, %3d, %3d) %-14s %s   %s   diff %.1e   kernel %.0f GB/s"
                     % (b, c, h, w, name, row(ts, "kernel"), row(ts, "composed"), d, gb / (statistics.median(ts["kernel"]) * 1e-3)))
    t = torch.randn(b, 2048, 8, 8, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    ts = alternate((("kernel", lambda: P.global_avg_pool(t)), ("composed", lambda: P.global_avg_pool_composition(t))), args.warmup, args.reps)
    lines.append("(%d, 2048,   8,   8) %-14s %s   %s" % (b, "global average", row(ts, "kernel"), row(ts, "composed")))

    feats = torch.relu(torch.randn(b, 2048, device="cuda", generator=gen))
    st = FeatureStats(2048).update(feats)
    gram = torch.zeros(2048, 2048, device="cuda", dtype=torch.float64)
    ssum = torch.zeros(2048, device="cuda", dtype=torch.float64)

    def torch_update():
        f = feats.double()
        gram.add_(f.T @ f)
        ssum.add_(f.sum(0))
    ts = alternate((("kernel", lambda: st.update(feats)), ("torch", torch_update)), args.warmup, args.reps)
    lines.append("FeatureStats.update, (%d, 2048) features into f64 moments:" % b)
    lines.append("%s   %s   (features.double().T @ features.double() + sum, added in place)" % (row(ts, "kernel"), row(ts, "torch")))
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
