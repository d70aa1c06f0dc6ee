#!/usr/bin/env python3
"""Writes tests/golden/spatial.npz: what Pillow makes of the four img/* images of attacks.npz (read from there, not duplicated) under
the spatial channel attacks.

    python tests/golden/make_golden_spatial.py

pillow_version            the version that wrote the file
resize/f<F>/<name>        uint8 [H2, W2, C]: Image.resize((W2, H2), Image.BILINEAR), (H2, W2) = max(1, floor(size * F + 0.5)), for
                          F in FACTORS
back/f<F>/<name>          uint8 [H, W, C]: that image resized back to the original size
resize/aniso/odd          uint8 [20, 8, 3]: the 13 x 21 image resized to 20 rows x 8 columns (one axis grows, the other shrinks)
median/k<K>/<name>        uint8 [H, W, C]: ImageFilter.MedianFilter(K), K = 3 and 5

Every image is stored as its differences from the row above, modulo 256 (the first row as it is): interpolated grain does not deflate,
its differences do, and the file has to stay under 100 KB.  ``np.cumsum(a, axis=0, dtype=np.uint8)`` restores the image.
"""
import math
import os

import numpy as np
import PIL
from PIL import Image, ImageFilter

FACTORS = (0.25, 0.3, 0.5, 0.75, 1.5, 2.0, 3.7)
NAMES = ("smooth", "odd", "gray", "noise")
HERE = os.path.dirname(os.path.abspath(__file__))


def to_pil(img):
    return Image.fromarray(img[..., 0] if img.shape[2] == 1 else img)


def from_pil(im):
    a = np.asarray(im, dtype=np.uint8)
    return a[..., None] if a.ndim == 2 else a


def resize(img, h2, w2):
    return from_pil(to_pil(img).resize((w2, h2), Image.BILINEAR))


def main():
    src = np.load(os.path.join(HERE, "attacks.npz"), allow_pickle=False)
    out = {"pillow_version": np.array(PIL.__version__)}
    for name in NAMES:
        img = src[f"img/{name}"]
        h, w = img.shape[:2]
        for f in FACTORS:
            h2, w2 = max(1, math.floor(h * f + 0.5)), max(1, math.floor(w * f + 0.5))
            small = resize(img, h2, w2)
            assert small.shape == (h2, w2, img.shape[2])
            out[f"resize/f{f:g}/{name}"] = small
            out[f"back/f{f:g}/{name}"] = resize(small, h, w)
        for k in (3, 5):
            out[f"median/k{k}/{name}"] = from_pil(to_pil(img).filter(ImageFilter.MedianFilter(k)))
    out["resize/aniso/odd"] = resize(src["img/odd"], 20, 8)
    for key, a in out.items():
        if a.ndim == 3:
            d = a.copy()
            d[1:] -= a[:-1]                                  # uint8: modulo 256
            assert np.array_equal(np.cumsum(d, axis=0, dtype=np.uint8), a)
            out[key] = d
    path = os.path.join(HERE, "spatial.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
