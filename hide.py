#!/usr/bin/env python3
"""Hide a file in synthesised images (the sender of IDEAS: payload bits -> secret tensor -> Gstru -> G -> 8-bit PNGs).

    python hide.py --ckpt CHECKPOINT --payload FILE --out DIR [--sigma 1] [--delta 0.5] [--seed 0] [--batch 32] [--ecc RATE]
                   [--format png|jpeg] [--png_encoder pillow|device] [--jpeg_quality 90] [--jpeg_subsampling 420|444]
                   [--jpeg_encoder pillow|device]

The payload is framed (4-byte length, CRC32, payload, random padding: ``ideas_amd.stego.frame``) into whole images of
``N * (image_size / 16)^2 * sigma`` bits each and written as ``DIR/000000.png``, ``DIR/000001.png``, ...  ``extract.py`` with the same
checkpoint and ``--sigma`` reads them back.  The same ``--seed`` gives the same files.

``--ecc RATE`` (1/2, 2/3 or 3/4) protects the frame with forward error correction (``ideas_amd.ecc``): every image then carries one
codeword of a punctured convolutional code, fewer payload bytes, and ``extract.py --ecc RATE`` corrects the receiver's wrong bits.

``--format jpeg`` writes ``DIR/000000.jpg``, ... through Pillow with ``quality=--jpeg_quality`` and ``subsampling=2`` (4:2:0, the
default) or ``0`` (``--jpeg_subsampling 444``), nothing else.  A JPEG file is a lossy channel: what ``extract.py`` reads out of it is
``op.jpeg_file_roundtrip`` of the container's bytes, and ``evaluate.py --attack jpegfile:Q`` (``jpegfile:Q:444``) gives the accuracy
to expect behind it; use ``--ecc``.  ``--jpeg_encoder device`` writes the files of ``op.jpeg_file_encode`` instead: the entropy coder runs on
the GPU, one copy a batch brings the finished files over, and Pillow is not in the loop.  They are the files Pillow writes, byte for
byte (a one-channel container at ``420`` differs in one header byte, the sampling factors, which Pillow sets to 2x2 and the device
leaves at 1x1; both decode alike).

``--png_encoder device`` (with the default ``--format png``) writes the files of ``op.png_file_encode`` instead of Pillow's: row filters,
Huffman coding and checksums run on the GPU and one copy a batch brings the finished files over.  They hold the same pixels, so
``extract.py`` reads the same payload, but not the same bytes: the device's deflate stream has no matches (include/ideas_hip.h, "The PNG
file, written"), which costs photograph-like images next to nothing and a flat image one bit a byte.
"""
import argparse
import os

import torch


def main(argv=None):
    parser = argparse.ArgumentParser(description="hide a payload file in images synthesised by a trained IDEAS checkpoint")
    parser.add_argument("--ckpt", type=str, required=True, help="checkpoint in the reference's format ({iter}.pt)")
    parser.add_argument("--payload", type=str, required=True, help="the file to hide")
    parser.add_argument("--out", type=str, required=True, help="directory for the containers")
    parser.add_argument("--sigma", type=int, default=1, help="bits per element of the secret tensor (1..8)")
    parser.add_argument("--delta", type=float, default=0.5, help="jitter half-width as a fraction of a bin")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--batch", type=int, default=32)
    parser.add_argument("--ecc", type=str, default=None, metavar="RATE", help="forward error correction of rate 1/2, 2/3 or 3/4")
    parser.add_argument("--format", choices=("png", "jpeg"), default="png", help="container files: lossless PNG or JPEG (a lossy channel)")
    parser.add_argument("--jpeg_quality", type=int, default=90, metavar="Q", help="with --format jpeg: the quality, 1..100")
    parser.add_argument("--jpeg_subsampling", choices=("420", "444"), default="420", help="with --format jpeg: the chroma subsampling")
    parser.add_argument("--jpeg_encoder", choices=("pillow", "device"), default="pillow",
                        help="with --format jpeg: who writes the files, Pillow on the host or the entropy coder on the GPU (the same bytes)")
    parser.add_argument("--png_encoder", choices=("pillow", "device"), default="pillow",
                        help="with --format png: who writes the files, Pillow on the host or the filters and the Huffman coder on the "
                             "GPU (the same pixels, other bytes)")
    opt = parser.parse_args(argv)
    if not 1 <= opt.jpeg_quality <= 100:
        parser.error(f"--jpeg_quality: {opt.jpeg_quality} is outside 1..100")
    from ideas_amd import ecc
    if opt.ecc is not None and opt.ecc not in ecc.RATES:
        parser.error(f"--ecc: unknown rate {opt.ecc!r} (known: {', '.join(ecc.RATES)})")

    if not torch.cuda.is_available():
        raise SystemExit("hide.py needs a GPU (ideas_amd has no CPU path)")
    from ideas_amd import stego
    from ideas_amd.op import jpeg_file_encode, jpeg_files_to_host, png_file_encode, png_files_to_host, quantize_image

    device = torch.device("cuda")
    models, args = stego.load_models(opt.ckpt, device)
    cap = stego.capacity_bits(args, opt.sigma)
    if cap % 8:
        raise SystemExit(f"hide.py: the capacity of an image ({cap} bits) is not a whole number of bytes (needs image_size >= 64)")
    with open(opt.payload, "rb") as f:
        payload = f.read()
    if opt.ecc is None:
        rows = stego.frame(payload, cap // 8, torch.Generator().manual_seed(opt.seed))
        room = f"{cap} bits ({cap // 8} bytes)"
    else:
        try:
            code = ecc.Code(cap, opt.ecc)
        except ValueError as e:
            raise SystemExit(f"hide.py: {e}")
        rows = stego.frame_coded(payload, code, torch.Generator().manual_seed(opt.seed), device)
        room = f"{cap} bits, ECC {opt.ecc}: {code.k_bytes} info bytes"
    gen = torch.Generator(device=device).manual_seed(opt.seed)
    os.makedirs(opt.out, exist_ok=True)
    print(f"capacity per image: {room}; payload {len(payload)} bytes -> {rows.shape[0]} image(s)")
    on_device, written = (opt.jpeg_encoder if opt.format == "jpeg" else opt.png_encoder) == "device", 0
    ext = "jpg" if opt.format == "jpeg" else "png"
    if not on_device:
        from PIL import Image
    for i0 in range(0, rows.shape[0], opt.batch):
        bits = rows[i0:i0 + opt.batch].to(device)
        images, _ = stego.hide(models, args, bits, opt.sigma, opt.delta, generator=gen)
        u8, _ = quantize_image(images, dequantize=False)
        if on_device:
            if opt.format == "jpeg":
                files = jpeg_files_to_host(*jpeg_file_encode(u8, opt.jpeg_quality, 2 if opt.jpeg_subsampling == "420" else 0))
            else:
                files = png_files_to_host(*png_file_encode(u8))
            for k, data in enumerate(files):
                with open(os.path.join(opt.out, f"{i0 + k:06d}.{ext}"), "wb") as f:
                    f.write(data)
                written += len(data)
            continue
        for k, img in enumerate(u8.cpu().numpy()):
            im = Image.fromarray(img[..., 0] if img.shape[2] == 1 else img)
            if opt.format == "jpeg":
                im.save(os.path.join(opt.out, f"{i0 + k:06d}.jpg"), "JPEG", quality=opt.jpeg_quality,
                        subsampling=2 if opt.jpeg_subsampling == "420" else 0)
            else:
                im.save(os.path.join(opt.out, f"{i0 + k:06d}.png"))
    print(f"wrote {rows.shape[0]} image(s) to {opt.out}" + (f", {written} bytes" if on_device else ""))


if __name__ == "__main__":
    main()
