#!/usr/bin/env python3
"""Time the JPEG round trip of the 8-bit container at (32, 256, 256, 3), quality 75: ``ideas_jpeg_roundtrip`` with the received image
(one launch: the entry point on preallocated outputs, and through ``op.jpeg_roundtrip``) next to the obvious torch spelling of the same
model -- blocks by reshape, two 8x8 matmuls, divide, round, and back -- which is what a user would otherwise write on the device.

Device events around windows of ``--launches`` calls, warm-up, the variants alternating inside one process, median and spread of the
per-call time.  The calls of a window rotate over ``--sets`` input tensors.  The kernel's time is also given as the bytes it must move,
B*H*W*C*(1 + 1 + 4), over the measured HBM copy rate.  The results are compared at the timed size.  Needs a GPU.

The spatial attacks (``op.resize_u8`` to half size and back -- the two launches of ``scale:0.5`` --, ``op.gaussian_blur_u8`` and
``op.median_u8``) are timed the same way at the same size, through their ops, and written to ``--spatial_out``; so are the JPEG file
channel (``op.jpeg_file_roundtrip``, 4:2:0 and 4:4:4) and ``op.pixel_attack`` with noise and with salt and pepper (draws made once,
outside the timed window), written to ``--file_out``.

    python tools/bench_attack.py [--out profiles/attack_jpeg.txt] [--spatial_out profiles/attack_spatial.txt]
        [--file_out profiles/attack_file_pixel.txt] [--batch 32] [--size 256] [--quality 75] [--reps 20]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_MEASURED = 6.29e12        # bytes / s: float4 copy


def torch_spelling(quality, device):
    """The model in torch ops for H, W multiples of 8 and C = 3: float colour and float coefficients throughout (no integer ties)."""
    import attacks_ref as R                            # the tables and the DCT matrix of the numpy restatement
    T = torch.from_numpy(R.quant_tables(quality)[[0, 1, 1]]).float().view(1, 3, 1, 1, 8, 8).to(device)
    D = torch.from_numpy(R.dct_matrix()).float().to(device)
    fwd = torch.tensor([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]], device=device)
    inv = torch.tensor([[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]], device=device)
    off = torch.tensor([0.0, 128.0, 128.0], device=device)

    def run(u8):
        b, h, w, _ = u8.shape
        ycc = (u8.float() @ fwd.T + off).round().clamp(0, 255)
        blk = (ycc - 128).permute(0, 3, 1, 2).reshape(b, 3, h // 8, 8, w // 8, 8).permute(0, 1, 2, 4, 3, 5)
        F = D @ blk @ D.T
        q = torch.sign(F) * torch.floor(F.abs() / T + 0.5)
        rec = (D.T @ (q * T) @ D + 128 + 0.5).floor().clamp(0, 255)
        ycc = rec.permute(0, 1, 2, 4, 3, 5).reshape(b, 3, h, w).permute(0, 2, 3, 1)
        out = ((ycc - off) @ inv.T + 0.5).floor().clamp(0, 255).to(torch.uint8)
        return out, ((out.float() / 255 - 0.5) / 0.5).permute(0, 3, 1, 2)
    return run


def window_ms(fn, xs, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(launches):
        fn(xs[i % len(xs)])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def timed_ops(title, variants, xs, args):
    """Per-call times of ``variants`` (name, fn, launches, bytes moved) through their ops, and the bytes over the measured HBM copy rate."""
    b, r = args.batch, args.size
    for _ in range(args.warmup):
        for _, fn, _, _ in variants:
            window_ms(fn, xs, args.launches)
    torch.cuda.synchronize()
    ts = {name: [] for name, _, _, _ in variants}
    for _ in range(args.reps):
        for name, fn, _, _ in variants:
            ts[name].append(window_ms(fn, xs, args.launches))
    lines = ["%s on the container, (%d, %d, %d, %d) uint8 with the received image, through the ops (output allocation included); "
             "per-call ms over windows of %d calls rotating over %d inputs, median of %d alternating windows [min .. max]; bytes = input, "
             "output and received image of every launch" % (title, b, r, r, xs[0].shape[3], args.launches, args.sets, args.reps)]
    for name, _, launches, moved in variants:
        v = ts[name]
        t = statistics.median(v)
        lines.append("%-13s %9.5f  [%9.5f .. %9.5f]  %d launch(es), %.1f MB -> %.2f TB/s = %.0f %% of the measured HBM copy rate"
                     % (name, t, min(v), max(v), launches, moved / 1e6, moved / (t * 1e-3) / 1e12, 100 * moved / (t * 1e-3) / HBM_MEASURED))
    return lines


def spatial(xs, args):
    from ideas_amd.op import gaussian_blur_u8, median_u8, resize_u8
    b, r = args.batch, args.size
    n = b * 3 * r * r
    half = (max(1, r // 2), max(1, r // 2))
    variants = (("scale:0.5", lambda x: resize_u8(resize_u8(x, half)[0], (r, r)), 2, n * (1 + 0.25 * 5) + n * (0.25 + 5)),
                ("gblur:1", lambda x: gaussian_blur_u8(x, 1.0), 1, n * 6), ("gblur:4", lambda x: gaussian_blur_u8(x, 4.0), 1, n * 6),
                ("median:3", lambda x: median_u8(x, 3), 1, n * 6), ("median:5", lambda x: median_u8(x, 5), 1, n * 6))
    return timed_ops("spatial attacks", variants, xs, args)


def behind(x):
    """a copy of ``x`` that starts one byte behind an aligned address: every kernel takes its byte path"""
    buf = torch.empty(x.numel() + 1, device=x.device, dtype=x.dtype)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    return v


def file_and_pixel(xs, args):
    """The JPEG file channel (4:2:0: two launches and the half-resolution chroma workspace, written and read) and the pixel attack
    (noise: 4 more bytes a byte read; salt and pepper: 4 a pixel); then the instantiations that the vector path at C = 3 does not
    reach: the byte path (inputs one byte behind an aligned address), C = 1, and both."""
    from ideas_amd.op import jpeg_file_roundtrip, jpeg_roundtrip, pixel_attack
    b, r, q = args.batch, args.size, args.quality
    gen = torch.Generator(device="cuda").manual_seed(1)
    noise = torch.randn(b, r, r, 3, device="cuda", generator=gen)
    u = torch.rand(b, r, r, device="cuda", generator=gen)

    def variants(c, first):
        n = b * c * r * r
        nz = noise[..., :c].contiguous()
        v = (("jpegfile:444", lambda x: jpeg_file_roundtrip(x, q, "4:4:4"), 1, n * 6),
             ("pixel:noise", lambda x: pixel_attack(x, sigma=8.0, noise=nz), 1, n * 10),
             ("pixel:sp", lambda x: pixel_attack(x, sp=0.05, u=u), 1, n * 6 + 4 * (n // c)))
        if c == 3:
            v = (("jpegfile:420", lambda x: jpeg_file_roundtrip(x, q, "4:2:0"), 2, n * 6 + n + 2 * (n // 6)),) + v
        return v if first else (("jpeg", lambda x: jpeg_roundtrip(x, q), 1, n * 6),) + v

    title = "JPEG file channel (quality %d) and pixel attacks" % q
    lines = timed_ops(title, variants(3, True), xs, args)
    x1 = [x[..., :1].contiguous() for x in xs]
    for what, c, inputs in (("byte path", 3, [behind(x) for x in xs]), ("C = 1", 1, x1), ("C = 1, byte path", 1, [behind(x) for x in x1])):
        lines += [""] + timed_ops("JPEG round trip, %s, %s" % (title, what), variants(c, False), inputs, args)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attack_jpeg.txt"))
    ap.add_argument("--spatial_out", default=os.path.join(ROOT, "profiles", "attack_spatial.txt"))
    ap.add_argument("--file_out", default=os.path.join(ROOT, "profiles", "attack_file_pixel.txt"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--sets", type=int, default=48)
    ap.add_argument("--launches", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attack needs a GPU")
    from ideas_amd import _lib
    from ideas_amd.op import jpeg_roundtrip

    b, r, q = args.batch, args.size, args.quality
    gen = torch.Generator(device="cuda").manual_seed(0)
    # smooth plus grain, as a generated image is: a random field at 1/8 resolution, upsampled, with +-8 levels of noise
    xs = []
    for _ in range(args.sets):
        low = torch.rand(b, 3, r // 8, r // 8, device="cuda", generator=gen)
        img = torch.nn.functional.interpolate(low, size=(r, r), mode="bilinear", align_corners=False) * 255
        img = img + (torch.rand(b, 3, r, r, device="cuda", generator=gen) - 0.5) * 16
        xs.append(img.clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous())
    n = b * 3 * r * r
    out = torch.empty(b, r, r, 3, device="cuda", dtype=torch.uint8)
    y = torch.empty(b, r, r, 3, device="cuda", dtype=torch.float32)
    entry, stream = _lib.load().ideas_jpeg_roundtrip, _lib.stream_ptr()

    def kernel_raw(x):                                # the entry point alone: outputs allocated once, no wrapper
        entry(out.data_ptr(), y.data_ptr(), None, x.data_ptr(), b, 3, r, r, q, stream)

    def op(x):
        return jpeg_roundtrip(x, q)

    spelled = torch_spelling(q, "cuda")
    variants = (("kernel", kernel_raw), ("op", op), ("torch_ops", spelled))
    for _ in range(args.warmup):
        for _, fn in variants:
            window_ms(fn, xs, args.launches)
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in variants}
    for _ in range(args.reps):
        for name, fn in variants:
            ts[name].append(window_ms(fn, xs, args.launches))
    (u_a, y_a), (u_b, _) = op(xs[0]), spelled(xs[0])
    kernel_raw(xs[0])
    raw_same = bool(torch.equal(out, u_a)) and bool(torch.equal(y, y_a.permute(0, 2, 3, 1)))
    d = (u_a.int() - u_b.int()).abs()
    moved = n * (1 + 1 + 4)
    lines = ["container -> JPEG quality %d (4:4:4) -> received image, (%d, %d, %d, 3) uint8; per-call ms over windows of %d calls rotating over "
             "%d inputs (%.0f MiB), median of %d alternating windows [min .. max]"
             % (q, b, r, r, args.launches, args.sets, args.sets * n / 2 ** 20, args.reps)]
    for name, _ in variants:
        v = ts[name]
        lines.append("%-9s %9.5f  [%9.5f .. %9.5f]" % (name, statistics.median(v), min(v), max(v)))
    t = statistics.median(ts["kernel"]) * 1e-3
    lines.append("kernel: %d bytes moved (B*H*W*C*(1+1+4): bytes in, bytes out, the received image) -> %.2f TB/s = %.0f %% of the measured "
                 "HBM copy rate (6.29 TB/s; the window includes the launch gaps); the bytes alone, %d each way, are %.0f %% of that time"
                 % (moved, moved / t / 1e12, 100 * moved / t / HBM_MEASURED, n, 100 * (2 * n / HBM_MEASURED) / t))
    lines.append("torch_ops / kernel: %.1fx; kernel == op: %s; torch_ops (float colour, f32 matmuls) vs op: %.3f %% of the bytes differ, "
                 "largest difference %d levels"
                 % (statistics.median(ts["torch_ops"]) / statistics.median(ts["kernel"]), raw_same, 100 * float((d > 0).float().mean()),
                    int(d.max())))
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)
    lines = spatial(xs, args)
    print("\n".join(lines), flush=True)
    with open(args.spatial_out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.spatial_out)
    lines = file_and_pixel(xs, args)
    print("\n".join(lines), flush=True)
    with open(args.file_out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.file_out)


if __name__ == "__main__":
    main()
