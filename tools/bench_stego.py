#!/usr/bin/env python3
"""Time the container's trip through 8 bits at (32, 3, 256, 256) f32 channels_last: ``ideas_image_f32_to_u8`` with the dequantised
image (one launch: the entry point on preallocated outputs, and through ``op.quantize_image``) next to the torch-op spelling of the same
two results.

Device events around windows of ``--launches`` calls, warm-up, the variants alternating inside one process, median and spread of
the per-call time.  The calls of a window rotate over ``--sets`` input tensors (more bytes than the 256 MiB Infinity Cache holds), so
reads come from HBM.  The kernel's time is also given as the bytes it must move, B*C*H*W*(4 + 1 + 4), over the measured HBM copy rate
and the spec peak.  The results are compared at the timed size.  Needs a GPU.

    python tools/bench_stego.py [--out profiles/stego_quantize.txt] [--batch 32] [--size 256] [--reps 20]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12        # bytes / s: float4 copy, datasheet


def torch_spelling(x):
    u8 = ((x.clamp(-1, 1) + 1) / 2 * 255 + 0.5).clamp(0, 255).to(torch.uint8)
    y = (u8.to(torch.float32) / 255 - 0.5) / 0.5
    return u8.permute(0, 2, 3, 1), y


def window_ms(fn, xs, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(launches):
        fn(xs[i % len(xs)])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stego_quantize.txt"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--sets", type=int, default=12)
    ap.add_argument("--launches", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stego needs a GPU")
    from ideas_amd import _lib
    from ideas_amd.op import quantize_image

    b, r = args.batch, args.size
    gen = torch.Generator(device="cuda").manual_seed(0)
    xs = [(torch.rand(b, 3, r, r, device="cuda", generator=gen) * 2.2 - 1.1).contiguous(memory_format=torch.channels_last)
          for _ in range(args.sets)]
    n = b * 3 * r * r
    u8_out = torch.empty(b, r, r, 3, device="cuda", dtype=torch.uint8)
    y_out = torch.empty(b, r, r, 3, device="cuda", dtype=torch.float32)
    entry, stream = _lib.load().ideas_image_f32_to_u8, _lib.stream_ptr()

    def kernel_raw(x):                                # the entry point alone: outputs allocated once, no wrapper
        entry(u8_out.data_ptr(), y_out.data_ptr(), x.data_ptr(), b, 3, r, r, _lib.NHWC, _lib.F32, stream)

    variants = (("kernel", kernel_raw), ("op", quantize_image), ("torch_ops", torch_spelling))
    for _ in range(args.warmup):
        for _, fn in variants:
            window_ms(fn, xs, args.launches)
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in variants}
    for _ in range(args.reps):
        for name, fn in variants:
            ts[name].append(window_ms(fn, xs, args.launches))
    (u_a, y_a), (u_b, y_b) = quantize_image(xs[0]), torch_spelling(xs[0])
    kernel_raw(xs[0])
    raw_same = bool(torch.equal(u8_out, u_a)) and bool(torch.equal(y_out, y_a.permute(0, 2, 3, 1)))
    dy = float((y_a - y_b).abs().max())
    moved = n * (4 + 1 + 4)
    lines = ["container -> 8 bits -> received image, (%d, 3, %d, %d) f32 channels_last; per-call ms over windows of %d calls rotating over "
             "%d inputs (%.0f MiB), median of %d alternating windows [min .. max]"
             % (b, r, r, args.launches, args.sets, args.sets * n * 4 / 2 ** 20, args.reps)]
    for name, _ in variants:
        v = ts[name]
        lines.append("%-9s %9.5f  [%9.5f .. %9.5f]" % (name, statistics.median(v), min(v), max(v)))
    t = statistics.median(ts["kernel"]) * 1e-3
    lines.append("kernel: %d bytes moved (B*C*H*W*(4+1+4)) -> %.2f TB/s = %.0f %% of the measured HBM copy rate (6.29 TB/s), %.0f %% of the "
                 "8.0 TB/s spec peak (the window includes the launch gaps)"
                 % (moved, moved / t / 1e12, 100 * moved / t / HBM_MEASURED, 100 * moved / t / HBM_SPEC))
    lines.append("torch_ops / kernel: %.1fx; kernel == op: %s; torch_ops vs op: bytes identical %s, received image max abs difference %.1e "
                 "(torch divides by 255 on the device as a multiplication by the reciprocal; the kernel divides, as the host transforms do)"
                 % (statistics.median(ts["torch_ops"]) / statistics.median(ts["kernel"]), raw_same, bool(torch.equal(u_a, u_b)), dy))
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
