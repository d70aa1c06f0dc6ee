#!/usr/bin/env python3
"""Writes tests/golden/jpegfile_bytes.npz: the JPEG FILES Pillow writes for a fixed set of small images, which tests/jpegbytes_ref.py
makes by integer arithmetic (``make_image``), so that they are not stored.

    python tests/golden/make_golden_jpegfile_bytes.py

pillow_version                 the version that wrote the file
libjpeg_version                the JPEG library inside it, e.g. "libjpeg-turbo 3.1.0" (PIL.features)
file/<H>x<W>x<C>/<kind>/q<Q>/s<S>
                               uint8 [n]: the bytes of Image.save(f, "JPEG", quality=Q, subsampling=S) of make_image(kind, H, W, C);
                               S = 0 (4:4:4) and 2 (4:2:0) for C = 3, S = 0 alone for C = 1 (mode "L")

CASES is the set: noise and 0/255 images at quality 100 and a flat one at quality 1, which between them take every branch of the coder
(tests/test_jpeg_bytes.py asserts it), and noise at quality 75, on shapes with odd block grids.  The file has to stay under 100 KB.
"""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from jpegbytes_ref import make_image  # noqa: E402

SHAPES = ((1, 1), (9, 129), (17, 33), (24, 40), (23, 7))
CASES = (("noise", 100), ("binary", 100), ("flat", 1), ("noise", 75))


def pillow_file(img, quality, subsampling):
    buf = io.BytesIO()
    Image.fromarray(img[..., 0] if img.shape[2] == 1 else img).save(buf, "JPEG", quality=quality, subsampling=subsampling)
    return buf.getvalue()


def libjpeg_version():
    if features.check_feature("libjpeg_turbo"):
        return "libjpeg-turbo " + str(features.version_feature("libjpeg_turbo"))
    return "libjpeg " + str(features.version_codec("jpg"))


def main():
    out = {"pillow_version": np.array(PIL.__version__), "libjpeg_version": np.array(libjpeg_version())}
    for h, w in SHAPES:
        for c in (1, 3):
            for kind, q in CASES:
                for s in ((0, 2) if c == 3 else (0,)):
                    out[f"file/{h}x{w}x{c}/{kind}/q{q}/s{s}"] = np.frombuffer(pillow_file(make_image(kind, h, w, c), q, s), np.uint8)
    path = os.path.join(HERE, "jpegfile_bytes.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out) - 2, "files")


if __name__ == "__main__":
    main()
