#!/usr/bin/env python3
"""Writes tests/golden/jpegfile.npz: what Pillow decodes from the JPEG files it encoded, for the four img/* images of attacks.npz (read
from there, not duplicated).

    python tests/golden/make_golden_jpegfile.py

pillow_version            the version that wrote the file
libjpeg_version           the JPEG library inside it, e.g. "libjpeg-turbo 3.1.0" (PIL.features)
rt/q<Q>/s<S>/<name>       uint8 [H, W, C]: Image.open of Image.save(f, "JPEG", quality=Q, subsampling=S), Q in QUALITIES, S = 0 (4:4:4)
                          and 2 (4:2:0); a one-channel image is saved in mode "L", where S has no effect

Every image is stored as its differences from the row above, modulo 256 (the first row as it is), like spatial.npz: decoded grain does
not deflate, its differences do better, and the file has to stay under 100 KB.  ``np.cumsum(a, axis=0, dtype=np.uint8)`` restores the
image.
"""
import io
import os

import numpy as np
import PIL
from PIL import Image, features

QUALITIES = (10, 75, 95)
SUBSAMPLINGS = (0, 2)
NAMES = ("smooth", "odd", "gray", "noise")
HERE = os.path.dirname(os.path.abspath(__file__))


def pillow_roundtrip(img, quality, subsampling):
    """uint8 [H, W, C] -> what Pillow reads back from the JPEG file it wrote: quality and subsampling, nothing else."""
    buf = io.BytesIO()
    Image.fromarray(img[..., 0] if img.shape[2] == 1 else img).save(buf, "JPEG", quality=quality, subsampling=subsampling)
    a = np.asarray(Image.open(io.BytesIO(buf.getvalue())), dtype=np.uint8)
    return a[..., None] if a.ndim == 2 else a


def libjpeg_version():
    if features.check_feature("libjpeg_turbo"):
        return "libjpeg-turbo " + str(features.version_feature("libjpeg_turbo"))
    return "libjpeg " + str(features.version_codec("jpg"))


def main():
    src = np.load(os.path.join(HERE, "attacks.npz"), allow_pickle=False)
    out = {"pillow_version": np.array(PIL.__version__), "libjpeg_version": np.array(libjpeg_version())}
    for name in NAMES:
        img = src[f"img/{name}"]
        for q in QUALITIES:
            for s in SUBSAMPLINGS:
                a = pillow_roundtrip(img, q, s)
                assert a.shape == img.shape
                d = a.copy()
                d[1:] -= a[:-1]                              # uint8: modulo 256
                assert np.array_equal(np.cumsum(d, axis=0, dtype=np.uint8), a)
                out[f"rt/q{q}/s{s}/{name}"] = d
    path = os.path.join(HERE, "jpegfile.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
