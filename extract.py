#!/usr/bin/env python3
"""Get a hidden file back from container images (the receiver of IDEAS: 8-bit images -> E -> Ex -> bits -> payload).

    python extract.py --ckpt CHECKPOINT [--sigma 1] --out FILE [--dump_bits F.npy] [--batch 32] [--ecc RATE]
                      [--jpeg_decoder pillow|device] IMAGES...

``IMAGES`` are the files ``hide.py`` wrote, in order.  Exit status 0 and the payload in ``FILE`` when the length and the CRC32 of the
frame hold; status 1 with a one-line message and no payload file when they do not.  ``--dump_bits`` saves the extracted packed bits
(uint8 [n_images, capacity / 8]) whatever the check says.

``--ecc RATE`` as given to ``hide.py``: the rows are decoded from soft values of the extractor's output (``ideas_amd.ecc``) before the
frame is checked, and ``--dump_bits`` saves the decoded information rows (uint8 [n_images, info bytes per image]).

``--jpeg_decoder device`` reads JPEG files on the GPU (``ideas_amd.op.jpeg_file_decode_grouped``: Pillow's pixels, without the host
decoding them), a batch at a time.  A JPEG file of a kind the device decoder does not read (progressive, 4:2:2, restart markers, ...)
falls back to Pillow with one line on stderr; a corrupt one ends the run.  Other formats are read by Pillow either way.
"""
import argparse
import sys

import numpy as np
import torch


def main(argv=None):
    parser = argparse.ArgumentParser(description="extract a hidden payload from IDEAS container images")
    parser.add_argument("--ckpt", type=str, required=True, help="the checkpoint hide.py used")
    parser.add_argument("--sigma", type=int, default=1, help="bits per element of the secret tensor (1..8), as given to hide.py")
    parser.add_argument("--out", type=str, required=True, help="where the payload is written")
    parser.add_argument("--dump_bits", type=str, default=None, metavar="F.npy", help="also save the extracted packed bits")
    parser.add_argument("--batch", type=int, default=32)
    parser.add_argument("--ecc", type=str, default=None, metavar="RATE", help="the forward error correction given to hide.py")
    parser.add_argument("--jpeg_decoder", choices=("pillow", "device"), default="pillow",
                        help="who decodes .jpg containers: Pillow on the host (default: pillow) or the HIP decoder on the device")
    parser.add_argument("images", metavar="IMAGES", nargs="+")
    opt = parser.parse_args(argv)
    from ideas_amd import ecc
    if opt.ecc is not None and opt.ecc not in ecc.RATES:
        parser.error(f"--ecc: unknown rate {opt.ecc!r} (known: {', '.join(ecc.RATES)})")

    if not torch.cuda.is_available():
        raise SystemExit("extract.py needs a GPU (ideas_amd has no CPU path)")
    from PIL import Image
    from ideas_amd import stego

    device = torch.device("cuda")
    models, args = stego.load_models(opt.ckpt, device)
    cap = stego.capacity_bits(args, opt.sigma)
    if cap % 8:
        raise SystemExit(f"extract.py: the capacity of an image ({cap} bits) is not a whole number of bytes (needs image_size >= 64)")
    code = None
    if opt.ecc is not None:
        try:
            code = ecc.Code(cap, opt.ecc)
        except ValueError as e:
            raise SystemExit(f"extract.py: {e}")
    size = int(args.image_size)

    def open_image(path):
        with Image.open(path) as img:
            arr = np.asarray(img.convert("RGB"), dtype=np.uint8)
        if arr.shape != (size, size, 3):
            raise SystemExit(f"extract.py: {path} is {arr.shape[1]}x{arr.shape[0]}, the checkpoint's images are {size}x{size}")
        return torch.from_numpy(arr.copy())

    def load_on_device(paths):
        """uint8 [n, size, size, 3] on the device: JPEG files through the device decoder, everything else through Pillow."""
        from ideas_amd.op import CorruptJpeg, UnsupportedJpeg, jpeg_file_decode_grouped, parse_jpeg
        host, files, where = {}, {1: [], 3: []}, {1: [], 3: []}
        for k, path in enumerate(paths):
            with open(path, "rb") as f:
                data = f.read()
            info = None
            if data[:2] == b"\xff\xd8":
                try:
                    info = parse_jpeg(data)
                except (UnsupportedJpeg, ValueError) as e:
                    print(f"extract.py: {path}: {e}; falls back to Pillow", file=sys.stderr)
            if info is None:
                host[k] = open_image(path)
                continue
            if (info.h, info.w) != (size, size):
                raise SystemExit(f"extract.py: {path} is {info.w}x{info.h}, the checkpoint's images are {size}x{size}")
            files[info.c].append(data)
            where[info.c].append(k)
        out = torch.empty((len(paths), size, size, 3), dtype=torch.uint8, device=device)
        for c in (1, 3):
            if files[c]:
                try:
                    got = jpeg_file_decode_grouped(files[c], device)
                except CorruptJpeg as e:
                    raise SystemExit("extract.py: corrupt JPEG data in " + ", ".join(paths[where[c][i]] for i in e.indices))
                out[torch.tensor(where[c], device=device)] = got.expand(-1, -1, -1, 3)
        if host:
            out[torch.tensor(sorted(host), device=device)] = torch.stack([host[k] for k in sorted(host)]).to(device)
        return out

    rows = []
    for i0 in range(0, len(opt.images), opt.batch):
        paths = opt.images[i0:i0 + opt.batch]
        x = load_on_device(paths) if opt.jpeg_decoder == "device" else torch.stack([open_image(p) for p in paths]).to(device)
        if code is None:
            bits, _ = stego.extract(models, args, x, opt.sigma)
        else:
            bits, _, _ = stego.extract_coded(models, args, x, opt.sigma, code)
        rows.append(bits.cpu())
    rows = torch.cat(rows, 0)
    if opt.dump_bits:
        np.save(opt.dump_bits, rows.numpy())
    try:
        payload = stego.unframe(rows)
    except stego.PayloadError as e:
        print(f"extract.py: no payload recovered, the length / CRC check of the frame failed: {e}", file=sys.stderr)
        return 1
    with open(opt.out, "wb") as f:
        f.write(payload)
    print(f"recovered {len(payload)} bytes from {rows.shape[0]} image(s) -> {opt.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
