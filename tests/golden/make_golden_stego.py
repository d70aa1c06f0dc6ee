#!/usr/bin/env python3
"""Generate tests/golden/stego.npz: the REFERENCE's own message codec (utils.py:74-97, ``message_to_tensor`` / ``tensor_to_message``)
on the CPU, as the vectors the packed-bit kernels of csrc/stego.hip are compared with bit for bit.

Runs only where the reference is available (``make_golden.import_reference``); nothing of the reference is copied: the script imports
its utils.py, feeds seeded inputs and stores arrays.

* ``enc/{tag}/M`` uint8 [B, L * sigma] (0 / 1), ``enc/{tag}/jitter`` f32 [B, L], ``enc/{tag}/Z`` f32 [B, L] = ``message_to_tensor(M, sigma,
  delta)`` for sigma in {1, 2, 3, 5, 8} x delta in {0, .25, .5}; ``meta["enc"]`` lists tag, sigma, delta, B, L.  The function draws its
  jitter with ``torch.rand_like``: the stored jitter is the same draw, recovered by re-seeding (as the codec vectors of ops.npz).
  Shapes: (1, 4) and (2, 256) at sigma 1; (3, 5) at sigma 2, 3, 5 (elements straddling bytes, pad bits); (2, 16) at sigma 8.
* ``dec/z`` f32 [1, n]: every bin edge of sigma = 8 (they contain the edges of every smaller sigma) with its two f32 neighbours,
  +-1e-9, +-0.0, +-1.5, +-inf, NaN, the smallest denormals, 500 uniform values in [-1.25, 1.25] and 500 normal ones (std 0.6).
  ``dec/s{sigma}`` uint8 [1, n * sigma] = ``tensor_to_message(z, sigma)``.

The archive is written with fixed member timestamps, so a re-run reproduces the file byte for byte.

    python tests/golden/make_golden_stego.py
"""
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                      # noqa: E402

SIGMAS = (1, 2, 3, 5, 8)
DELTAS = (0.0, 0.25, 0.5)
ENC_SHAPES = {1: ((1, 4), (2, 256)), 2: ((3, 5),), 3: ((3, 5),), 5: ((3, 5),), 8: ((2, 16),)}
DEC_SEED = 7100


def gen_encode(RU, out, meta):
    meta["enc"] = []
    for sigma in SIGMAS:
        for (b, l) in ENC_SHAPES[sigma]:
            for delta in DELTAS:
                seed = 7000 + sigma * 100 + int(delta * 100) + l
                g = torch.Generator().manual_seed(seed)
                M = torch.randint(0, 2, (b, l * sigma), generator=g, dtype=torch.float)
                torch.manual_seed(seed + 1)
                jitter = torch.rand(b, l)
                torch.manual_seed(seed + 1)
                Z = RU.message_to_tensor(M, sigma, delta)
                assert Z.dtype == torch.float32 and tuple(Z.shape) == (b, l)
                tag = f"s{sigma}_d{int(delta * 100)}_b{b}_l{l}"
                out[f"enc/{tag}/M"] = MG.npy(M).astype(np.uint8)
                out[f"enc/{tag}/jitter"] = MG.npy(jitter)
                out[f"enc/{tag}/Z"] = MG.npy(Z)
                meta["enc"].append(dict(tag=tag, sigma=sigma, delta=delta, B=b, L=l))


def decode_vector():
    edges = (np.arange(257, dtype=np.float64) / 128.0 - 1.0).astype(np.float32)
    lo, hi = np.nextafter(edges, np.float32(-np.inf)), np.nextafter(edges, np.float32(np.inf))
    tiny = np.float32(1e-45)                                 # the smallest denormal
    special = np.array([1e-9, -1e-9, 0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, np.nan, tiny, -tiny, 2 * tiny, -2 * tiny,
                        np.float32(1.1754942e-38), np.float32(-1.1754942e-38)], dtype=np.float32)
    g = torch.Generator().manual_seed(DEC_SEED)
    uni = (torch.rand(500, generator=g) * 2.5 - 1.25).numpy()
    nrm = (torch.randn(500, generator=g) * 0.6).numpy()
    return np.concatenate([edges, lo, hi, special, uni, nrm]).astype(np.float32)[None, :]


def gen_decode(RU, out, meta):
    z = decode_vector()
    out["dec/z"] = z
    for sigma in SIGMAS:
        msg = RU.tensor_to_message(torch.from_numpy(z.copy()), sigma)
        assert tuple(msg.shape) == (1, z.shape[1] * sigma) and bool(((msg == 0) | (msg == 1)).all())
        out[f"dec/s{sigma}"] = MG.npy(msg).astype(np.uint8)
    meta["dec"] = dict(n=int(z.shape[1]), sigmas=list(SIGMAS))


def save_reproducible(path, arrays):
    """np.savez_compressed with a fixed timestamp on every member."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name, arr in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    RM, RU, RL, RO = MG.import_reference()
    out, meta = {}, {}
    gen_encode(RU, out, meta)
    gen_decode(RU, out, meta)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(MG.OUT, "stego.npz")
    save_reproducible(path, out)
    size = os.path.getsize(path)
    print("stego.npz", len(out), "arrays,", size, "bytes")
    assert size < 100_000, size


if __name__ == "__main__":
    main()
