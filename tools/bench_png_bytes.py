#!/usr/bin/env python3
"""Time the PNG file written on the device against what ``hide.py`` does by default, at (32, 256, 256, 3), in one process:

    device   ``op.png_file_encode`` (filters, code tables, packing, checksums) and ``png_files_to_host``: finished files as ``bytes``
             on the host
    coder    ``op.png_file_encode`` alone: the files stay on the device
    pillow   ``u8.cpu()`` and one ``Image.save(f, "PNG")`` into memory per image (zlib at level 6, as ``hide.py`` writes them)

The method is tools/bench_attack.py's: device events around windows of ``--launches`` calls that rotate over ``--sets`` inputs, warm-up,
the variants alternating, median and spread of the per-call time.  Every variant ends on the host or is followed by the window's closing
event, so the events see the host's share too; the wall clock of the same windows is printed beside them.  The two paths write
different bytes for the same pixels (the device's stream has no matches): every device file is opened with Pillow and compared with its
input, and the sizes of the two paths are printed.  Needs a GPU and Pillow.

``--trace N`` runs the device path N times and nothing else: the run to put under ``rocprofv3 --kernel-trace --stats``;
``--kernel_csv`` appends the rows of that run's per-kernel table (kernel_stats.csv) to the output.

    python tools/bench_png_bytes.py [--out profiles/png_bytes.txt] [--batch 32] [--size 256] [--reps 20] [--kernel_csv stats.csv]
"""
import argparse
import csv
import io
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("filter_kernel", "tables_kernel", "pack_kernel", "finish_kernel", "fillBuffer", "Memset", "memset")


def window(fn, xs, launches):
    """(ms per call by device events, ms per call by the wall clock) of one window"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for i in range(launches):
        fn(xs[i % len(xs)])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches, (time.perf_counter() - t0) * 1e3 / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_bytes.txt"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", type=int, default=0, metavar="N", help="run the device path N times and exit (for a kernel trace)")
    ap.add_argument("--kernel_csv", default=None, help="the kernel_stats.csv of a --trace 20 run under rocprofv3, to append")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_png_bytes needs a GPU")
    from PIL import Image
    import numpy as np
    from ideas_amd.op import png_file_encode, png_files_to_host

    b, r = args.batch, args.size
    gen = torch.Generator(device="cuda").manual_seed(0)
    xs = []                                               # smooth plus grain, as a generated image is (tools/bench_attack.py)
    for _ in range(args.sets):
        low = torch.rand(b, 3, r // 8, r // 8, device="cuda", generator=gen)
        img = torch.nn.functional.interpolate(low, size=(r, r), mode="bilinear", align_corners=False) * 255
        img = img + (torch.rand(b, 3, r, r, device="cuda", generator=gen) - 0.5) * 16
        xs.append(img.clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous())

    def device(x):
        return png_files_to_host(*png_file_encode(x))

    def coder(x):
        return png_file_encode(x)

    def pillow(x):
        files = []
        for img in x.cpu().numpy():
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, "PNG")
            files.append(buf.getvalue())
        return files

    if args.trace:
        for i in range(2 + args.trace):                   # two calls of warm-up
            device(xs[i % len(xs)])
        torch.cuda.synchronize()
        return

    variants = (("device", device), ("coder", coder), ("pillow", pillow))
    for _ in range(args.warmup):
        for _, fn in variants:
            window(fn, xs, args.launches)
    ts = {name: [] for name, _ in variants}
    for _ in range(args.reps):
        for name, fn in variants:
            ts[name].append(window(fn, xs, args.launches))
    ours, theirs = device(xs[0]), pillow(xs[0])
    same = 0
    for data, img in zip(ours, xs[0].cpu().numpy()):
        with Image.open(io.BytesIO(data)) as im:
            same += int(np.array_equal(np.asarray(im, dtype=np.uint8), img))
    lines = ["container -> PNG files, (%d, %d, %d, 3) uint8; per-call ms over windows of %d calls rotating over %d inputs, median of %d "
             "alternating windows [min .. max] by device events, then by the wall clock" % (b, r, r, args.launches, args.sets, args.reps)]
    for name, _ in variants:
        ev, wall = [t[0] for t in ts[name]], [t[1] for t in ts[name]]
        lines.append("%-7s %9.4f  [%9.4f .. %9.4f]   wall %9.4f  [%9.4f .. %9.4f]"
                     % (name, statistics.median(ev), min(ev), max(ev), statistics.median(wall), min(wall), max(wall)))
    med = {name: statistics.median(t[0] for t in ts[name]) for name, _ in variants}
    lines.append("pillow / device: %.1fx; Pillow opens %d of %d device files to their input; %d bytes of device files a batch against %d of "
                 "Pillow's (%.3f); %d bytes copied to the host a batch (the rows up to their bound)"
                 % (med["pillow"] / med["device"], same, len(ours), sum(len(f) for f in ours), sum(len(f) for f in theirs),
                    sum(len(f) for f in ours) / sum(len(f) for f in theirs), b * (4 + coder(xs[0])[0].shape[1])))
    if args.kernel_csv:
        lines += ["", "per kernel, from a kernel trace (rocprofv3 --kernel-trace --stats) of %d calls of the device path after warm-up "
                  "in a run of its own: the four kernels and the clearing of the histograms and the bit buffer" % 20]
        with open(args.kernel_csv, newline="") as f:
            for row in csv.DictReader(f):
                name = next(iter(row.values()))
                if any(k in name for k in KERNELS):
                    rest = ", ".join("%s %s" % (k, v) for k, v in list(row.items())[1:])
                    lines.append("%-46s %s" % (name.replace("(anonymous namespace)::", "").replace("void ", "")[:46], rest))
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
