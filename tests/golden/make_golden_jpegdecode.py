#!/usr/bin/env python3
"""Writes tests/golden/jpegdecode.npz: JPEG files Pillow writes with options that leave the standard stream of
tests/golden/jpegfile_bytes.npz -- Huffman tables of their own, tables no quality gives, a one-channel file marked 4:2:0 -- with the
pixels Pillow's ``Image.open`` reads out of them, and three files the device decoder has to refuse.

    python tests/golden/make_golden_jpegdecode.py

pillow_version, libjpeg_version   as in jpegfile_bytes.npz
file/<tag>                     uint8 [n]: the bytes of Image.save(f, "JPEG", **options) of make_image(kind, H, W, C)
pixels/<tag>                   uint8 [H, W, C]: np.asarray(Image.open(file))
refused/<reason>               uint8 [n]: a progressive file, a 4:2:2 file and a file with restart markers (where this Pillow writes them)
sha256/<key of jpegfile_bytes.npz>
                               uint8 [32]: the SHA-256 of the pixels Image.open reads out of that file (the 60 files are not stored
                               twice, and their pixels would not fit: the file has to stay under 100 KB)
"""
import hashlib
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from jpegbytes_ref import make_image  # noqa: E402
from make_golden_jpegfile_bytes import libjpeg_version  # noqa: E402

CASES = (
    ("opt95/17x33x3/noise", dict(quality=95, optimize=True)),
    ("opt95/9x129x1/binary", dict(quality=95, optimize=True)),
    ("opt100/24x40x3/noise", dict(quality=100, optimize=True, subsampling=0)),
    ("opt100/23x7x1/noise", dict(quality=100, optimize=True)),
    ("qtables/17x33x3/smooth", dict(qtables=[list(range(1, 65)), [3] * 64])),
    ("qtables/24x40x1/noise", dict(qtables=[list(range(1, 65)), [3] * 64])),
    ("l420/9x129x1/noise", dict(quality=75, subsampling=2)),
    ("q1/23x7x3/noise", dict(quality=1)),
    ("q1/24x40x1/binary", dict(quality=1)),
)
REFUSED = (
    ("progressive", "17x33x3/noise", dict(quality=75, progressive=True)),
    ("422", "17x33x3/noise", dict(quality=75, subsampling=1)),
    ("restart", "24x40x3/noise", dict(quality=75, restart_marker_blocks=2)),
)


def image_of(tag):
    shape, kind = tag.split("/")[-2:]
    h, w, c = (int(v) for v in shape.split("x"))
    return make_image(kind, h, w, c)


def pillow_file(img, **options):
    buf = io.BytesIO()
    Image.fromarray(img[..., 0] if img.shape[2] == 1 else img).save(buf, "JPEG", **options)
    return buf.getvalue()


def pillow_pixels(data, shape):
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im, dtype=np.uint8).reshape(shape)


def main():
    out = {"pillow_version": np.array(PIL.__version__), "libjpeg_version": np.array(libjpeg_version())}
    for tag, options in CASES:
        img = image_of(tag)
        data = pillow_file(img, **options)
        out["file/" + tag] = np.frombuffer(data, np.uint8)
        out["pixels/" + tag] = pillow_pixels(data, img.shape)
    for reason, tag, options in REFUSED:
        plain = pillow_file(image_of(tag), quality=75)
        data = pillow_file(image_of(tag), **options)
        if data != plain:                                    # (a Pillow that ignores the option writes the plain file)
            out["refused/" + reason] = np.frombuffer(data, np.uint8)
    old = np.load(os.path.join(HERE, "jpegfile_bytes.npz"), allow_pickle=False)
    for key in old.files:
        if key.startswith("file/"):
            h, w, c = (int(v) for v in key.split("/")[1].split("x"))
            pix = pillow_pixels(old[key].tobytes(), (h, w, c))
            out["sha256/" + key] = np.frombuffer(hashlib.sha256(pix.tobytes()).digest(), np.uint8)
    path = os.path.join(HERE, "jpegdecode.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out) - 2, "entries")


if __name__ == "__main__":
    main()
