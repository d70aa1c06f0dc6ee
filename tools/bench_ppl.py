#!/usr/bin/env python3
"""Time one batch of ``ideas_amd.ppl.path_distances`` (w-space, size 256, batch 64: 128 images; seeded random weights, the time does
not depend on their values) next to the unfused path on the same device and modules -- slices, lerps, stack, generator,
``image[::2]`` / ``image[1::2]``, ``percept(a, b)`` -- and the two kernels alone next to their torch compositions.

Device events, warm-up, the variants alternating inside one process, median and spread.  Needs a GPU.

    python tools/bench_ppl.py [--out profiles/ppl_bench.txt] [--batch 64] [--size 256] [--reps 10]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_lpips import alternate, seeded_weights          # noqa: E402


def unfused(g, percept, z, t, noise, eps):
    from ideas_amd.ppl import generate_images, lerp
    with torch.no_grad():
        latent = g.get_latent(z)
        a, b = latent[::2], latent[1::2]
        latent_e = torch.stack([lerp(a, b, t[:, None]), lerp(a, b, t[:, None] + eps)], 1).view(*latent.shape)
        image = generate_images(g, latent_e, noise)          # (two slices of 64 at the defaults: ideas_amd/ppl.py::LAUNCH_BYTES)
        return percept(image[::2], image[1::2]).view(image.shape[0] // 2) / (eps ** 2)


def row(name, v):
    return "%-12s %9.3f  [%9.3f .. %9.3f]" % (name, statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppl_bench.txt"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ppl needs a GPU")
    import ideas_amd.op as op
    from ideas_amd.lpips import PerceptualLoss
    from ideas_amd.op.ppl import pair_prepare_composition, path_endpoints_composition
    from ideas_amd.ppl import _scaling_constants, path_distances
    from ideas_amd.stylegan2_gen import Generator

    b, eps = args.batch, 1e-4
    torch.manual_seed(0)
    g = Generator(args.size, 512, 8).eval().cuda()
    sd, lin = seeded_weights()
    percept = PerceptualLoss(backbone=sd, lin_weights=lin).cuda()
    noise = g.make_noise()
    z = torch.randn(2 * b, 512, device="cuda")
    t = torch.rand(b, device="cuda")
    shift, scale = _scaling_constants(percept)

    fused = lambda: path_distances(g, percept, z, t, noise, space="w", eps=eps)
    plain = lambda: unfused(g, percept, z, t, noise, eps)
    ts = alternate((("fused", fused), ("unfused", plain)), args.warmup, args.reps)
    d_a, d_b = fused(), plain()
    lines = ["path_distances, w-space, Generator(%d, 512, 8), batch %d (%d images) f32; median of %d alternating runs, ms [min .. max]"
             % (args.size, b, 2 * b, args.reps), row("fused", ts["fused"]), row("unfused", ts["unfused"]),
             "fused vs unfused distances: %.2e (max abs over max abs)" % float((d_a - d_b).abs().max() / d_b.abs().max())]

    with torch.no_grad():
        lat = g.get_latent(z)
        img = torch.randn(2 * b, 3, args.size, args.size, device="cuda").contiguous(memory_format=torch.channels_last)
        box = (0, 0, args.size, args.size)
        ts = alternate((("kernel", lambda: op.path_endpoints(lat, t, eps, "lerp")),
                        ("composition", lambda: path_endpoints_composition(lat, t, eps, "lerp"))), 5, 50)
        lines += ["op.path_endpoints, lerp, [%d, 512]:" % (2 * b), row("kernel", ts["kernel"]), row("composition", ts["composition"])]
        ts = alternate((("kernel", lambda: op.pair_prepare(img, box, box[2:], shift, scale)),
                        ("composition", lambda: pair_prepare_composition(img, box, box[2:], shift, scale))), 5, 50)
        lines += ["op.pair_prepare, whole image, [%d, 3, %d, %d] channels_last:" % (2 * b, args.size, args.size), row("kernel", ts["kernel"]),
                  row("composition", ts["composition"])]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
