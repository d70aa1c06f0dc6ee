#!/usr/bin/env python3
"""Time the JPEG file read on the device against what ``extract.py`` does by default, at (32, 256, 256, 3), quality 75, 4:2:0, in one
process.  Both paths start from the files as ``bytes`` on the host and end with uint8 [B, H, W, 3] on the device:

    device   ``op.jpeg_file_decode``: the headers parsed and the scans packed on the host, ONE copy, the kernels
    pillow   per file ``Image.open`` + ``convert("RGB")`` + ``np.asarray``, then ``torch.stack`` and ``.to(device)`` (extract.py's loop;
             the files come from memory here, not from disk)

The method is tools/bench_jpeg_bytes.py's: device events around windows of ``--launches`` calls that rotate over ``--sets`` inputs,
warm-up, the variants alternating, median and spread of the per-call time, the wall clock of the same windows beside them.  The pixels
of the two paths are compared at the timed size, and the rounds the synchronise kernel takes on the inputs are counted by running its
schedule in Python (tests/jpegdecode_ref.py::sync_rounds).  The files are written by ``op.jpeg_file_encode``.  Needs a GPU and Pillow.

``--trace N`` runs the device path N times and nothing else: the run to put under ``rocprofv3 --kernel-trace --stats``;
``--kernel_csv`` appends the rows of that run's per-kernel table (kernel_stats.csv) to the output.  ``--label`` names the build (the
library of ``IDEAS_HIP_LIB``, e.g. one compiled with another ``-DIDEAS_JPEG_SUBSEQ_BITS``), ``--append`` adds to ``--out``.

    python tools/bench_jpeg_decode.py [--out profiles/jpeg_decode.txt] [--batch 32] [--size 256] [--quality 75] [--reps 20]
        [--kernel_csv stats.csv] [--label TEXT] [--subseq_bits L] [--append]
"""
import argparse
import csv
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = ("unstuff_kernel", "sync_kernel", "emit_kernel", "dc_kernel", "decode_chroma420_kernel", "decode_pixels_kernel", "fillBuffer",
           "Memset", "memset", "Copy", "copy")


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode.txt"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", type=int, default=0, metavar="N", help="run the device path N times and exit (for a kernel trace)")
    ap.add_argument("--kernel_csv", default=None, help="the kernel_stats.csv of a --trace 20 run under rocprofv3, to append")
    ap.add_argument("--label", default="", help="a name for the build that is measured")
    ap.add_argument("--subseq_bits", type=int, default=0, help="IDEAS_JPEG_SUBSEQ_BITS of the measured build, if not the binding's")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_decode needs a GPU")
    from PIL import Image
    from ideas_amd import _lib
    from ideas_amd.op import jpeg_file_decode, jpeg_file_encode, jpeg_files_to_host

    b, r, q = args.batch, args.size, args.quality
    gen = torch.Generator(device="cuda").manual_seed(0)
    xs = []                                               # smooth plus grain, as a generated image is (tools/bench_attack.py)
    for _ in range(args.sets):
        low = torch.rand(b, 3, r // 8, r // 8, device="cuda", generator=gen)
        img = torch.nn.functional.interpolate(low, size=(r, r), mode="bilinear", align_corners=False) * 255
        img = img + (torch.rand(b, 3, r, r, device="cuda", generator=gen) - 0.5) * 16
        x = img.clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        xs.append(jpeg_files_to_host(*jpeg_file_encode(x, q, "4:2:0")))

    def device(files):
        return jpeg_file_decode(files)[0]

    def pillow(files):
        batch = []
        for data in files:
            with Image.open(io.BytesIO(data)) as img:
                batch.append(torch.from_numpy(np.asarray(img.convert("RGB"), dtype=np.uint8).copy()))
        return torch.stack(batch).to("cuda")

    if args.trace:
        for i in range(2 + args.trace):                   # two calls of warm-up
            device(xs[i % len(xs)])
        torch.cuda.synchronize()
        return

    variants = (("device", device), ("pillow", pillow))
    for _ in range(args.warmup):
        for _, fn in variants:
            window(fn, xs, args.launches)
    ts = {name: [] for name, _ in variants}
    for _ in range(args.reps):
        for name, fn in variants:
            ts[name].append(window(fn, xs, args.launches))
    same = int((device(xs[0]) == pillow(xs[0])).flatten(1).all(1).sum())
    import jpegdecode_ref
    L = args.subseq_bits or _lib.JPEG_SUBSEQ_BITS
    rounds = [jpegdecode_ref.sync_rounds(f, L) for f in xs[0][:8]]
    lines = ["%sJPEG files -> container, quality %d, 4:2:0, (%d, %d, %d, 3) uint8; per-call ms over windows of %d calls rotating over %d "
             "inputs, median of %d alternating windows [min .. max] by device events, then by the wall clock"
             % (args.label + ": " if args.label else "", q, b, r, r, args.launches, args.sets, args.reps)]
    for name, _ in variants:
        ev, wall = [t[0] for t in ts[name]], [t[1] for t in ts[name]]
        lines.append("%-7s %9.4f  [%9.4f .. %9.4f]   wall %9.4f  [%9.4f .. %9.4f]"
                     % (name, statistics.median(ev), min(ev), max(ev), statistics.median(wall), min(wall), max(wall)))
    med = {name: statistics.median(t[0] for t in ts[name]) for name, _ in variants}
    lines.append("pillow / device: %.1fx; %d of %d images of the two paths are the same pixels; %d bytes of files a batch"
                 % (med["pillow"] / med["device"], same, b, sum(len(f) for f in xs[0])))
    lines.append("synchronise kernel at L = %d, first 8 files of input 0: (rounds, subsequences) = %s"
                 % (L, ", ".join(str(v) for v in rounds)))
    if args.kernel_csv:
        lines += ["", "per kernel, from a kernel trace (rocprofv3 --kernel-trace --stats) of %d calls of the device path after warm-up "
                  "in a run of its own" % 20]
        with open(args.kernel_csv, newline="") as f:
            for row in csv.DictReader(f):
                name = next(iter(row.values()))
                if any(k in name for k in KERNELS):
                    rest = ", ".join("%s %s" % (k, v) for k, v in list(row.items())[1:])
                    lines.append("%-46s %s" % (name.replace("(anonymous namespace)::", "").replace("void ", "")[:46], rest))
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n" + ("\n" if args.append else ""))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
