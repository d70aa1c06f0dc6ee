#!/usr/bin/env python3
"""Writes tests/golden/attacks.npz: the fixture images of the channel-attack tests and what PIL (libjpeg-turbo) makes of them.

    python tests/golden/make_golden_attacks.py

img/<name>            uint8 [H, W, C]: smooth (40x24x3, smooth plus grain), odd (13x21x3), gray (16x8x1), noise (8x8x3)
tie/<name>            uint8 [8, 8 n, 1], one case per 8x8 block, and the quality it is built for in tie/<name>/quality:
    dc_q50            flat blocks 128 + d, d odd: F(0,0) / T = 8 d / 16 lies exactly on k + 0.5, both signs
    sample_q62        flat blocks 128 +- 1, 128 +- 2: the DC quantises to +-1, T = 12, the sample is 128 +- 1.5
    sample_q1         flat blocks near black and white: the DC quantises to -+4, T = 255, the samples are 0.5 and 255.5
    basis             128 + d + a s(j) + c s(i) + b s(i) s(j), s = (+ - - + + - - +): only (0,0), (0,4), (4,0), (4,4) are non-zero
pil/q<q>/tables       int32 [2, 64]: Image.quantization of a file saved with quality=q, subsampling=0 (natural order, 8 u + v)
pil/q<q>/<name>       uint8 [H, W, C]: PIL's decode of that file, for every img/ image
"""
import io
import os

import numpy as np
from PIL import Image

QUALITIES = (1, 10, 50, 75, 90, 100)
HERE = os.path.dirname(os.path.abspath(__file__))


def images():
    # the seeds: the first for which, at every quality, under 0.5 % of the non-rational coefficients and of the samples lie in the
    # tie window of tests/attacks_ref.py (blocks in which only the rational coefficients survive put whole blocks on exact eighths)
    rng = np.random.default_rng(3)
    yy, xx = np.meshgrid(np.arange(40), np.arange(24), indexing="ij")
    smooth = np.stack([128 + 90 * np.sin(yy / 9.0 + 0.3 * c) * np.cos(xx / 7.0 - 0.3 * c) + 12 * (yy - xx) / 40.0 for c in range(3)], -1)
    smooth = np.clip(smooth + rng.normal(0, 4, smooth.shape), 0, 255).astype(np.uint8)
    rng = np.random.default_rng(1)
    yy, xx = np.meshgrid(np.arange(13), np.arange(21), indexing="ij")
    odd = np.stack([110 + 70 * np.cos(xx / 3.0 + 0.7 * c) + 40 * np.sin(yy / 2.0) for c in range(3)], -1)
    odd = np.clip(odd + rng.normal(0, 10, odd.shape), 0, 255).astype(np.uint8)
    # (gray: also the first whose PIL decode at quality 100 is nearer to the model's bytes than to the input; with one channel and
    # T = 1 both differ from PIL only by roundings of the transform, a near-tie that other seeds lose)
    rng = np.random.default_rng(106)
    yy, xx = np.meshgrid(np.arange(16), np.arange(8), indexing="ij")
    gray = np.clip(40 + 11 * yy + 6 * xx + rng.normal(0, 6, (16, 8)), 0, 255).astype(np.uint8)[..., None]
    noise = np.random.default_rng(212).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    return {"smooth": smooth, "odd": odd, "gray": gray, "noise": noise}


def flat_row(values):
    return np.concatenate([np.full((8, 8), v) for v in values], 1).astype(np.uint8)[..., None]


def tie_images():
    s = np.array([1, -1, -1, 1, 1, -1, -1, 1])
    basis = []
    for d, a, c, b in ((0, 12, 0, 0), (0, 0, 0, 9), (0, 12, 0, 9), (5, 12, 7, 9), (-40, -30, 20, 25), (60, 3, -3, 1), (0, 0, 18, 0),
                       (-1, 6, 6, 6)):
        blk = 128 + d + a * s[None, :] + c * s[:, None] + b * s[:, None] * s[None, :]
        assert blk.min() >= 0 and blk.max() <= 255
        basis.append(blk)
    return {"dc_q50": (flat_row(128 + np.array([1, -1, 3, -3, 5, -5, 127, -127])), 50),
            "sample_q62": (flat_row(128 + np.array([1, -1, 2, -2])), 62),
            "sample_q1": (flat_row([0, 8, 16, 240, 248, 255]), 1),
            "basis": (np.concatenate(basis, 1).astype(np.uint8)[..., None], 50)}


def pil_round_trip(img, quality):
    f = io.BytesIO()
    Image.fromarray(img[..., 0] if img.shape[2] == 1 else img).save(f, format="JPEG", quality=quality, subsampling=0)
    with Image.open(io.BytesIO(f.getvalue())) as im:
        tables = {k: np.array(v, np.int32) for k, v in im.quantization.items()}
        dec = np.asarray(im, dtype=np.uint8)
    return tables, (dec[..., None] if dec.ndim == 2 else dec)


def main():
    out = {}
    every = images()
    for name, img in every.items():
        out[f"img/{name}"] = img
    for name, (img, q) in tie_images().items():
        out[f"tie/{name}"] = img
        out[f"tie/{name}/quality"] = np.int32(q)
    for q in QUALITIES:
        for name, img in every.items():
            tables, dec = pil_round_trip(img, q)
            assert dec.shape == img.shape
            out[f"pil/q{q}/{name}"] = dec
            if img.shape[2] == 3:
                out[f"pil/q{q}/tables"] = np.stack((tables[0], tables[1]))
    path = os.path.join(HERE, "attacks.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
