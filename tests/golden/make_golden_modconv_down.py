#!/usr/bin/env python3
"""Generate tests/golden/modconv_down.npz: the REFERENCE's own ``ModulatedConv2d(downsample=True)`` (stylegan2/model.py:181-277) on
the CPU -- inputs, parameters, output and the five gradients of a few small layers, and one seeded initial state dict.

Runs only where the reference is available (``make_golden.import_reference``); nothing of the reference is copied, the script
imports it, feeds seeded inputs and stores tensors.

    python tests/golden/make_golden_modconv_down.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG          # noqa: E402

STYLE_DIM = 24
INIT_SEED = 460
# (B, Cin, Cout, kernel, H, demodulate): 3x3 at even and odd sizes (the size class of mod0..3 of ops.npz), a 1x1 kernel, no demodulation
CASES = ((2, 8, 12, 3, 10, True), (2, 32, 16, 3, 7, True), (2, 16, 24, 3, 8, True), (2, 16, 8, 1, 7, True), (2, 8, 12, 3, 8, False))


def main():
    RM, RU, RL, RO = MG.import_reference()
    npy = MG.npy
    out = {}
    g = torch.Generator().manual_seed(41)
    meta = []
    for ci, (b, cin, cout, k, hw, demod) in enumerate(CASES):
        torch.manual_seed(440 + ci)
        m = RL.ModulatedConv2d(cin, cout, k, STYLE_DIM, demodulate=demod, downsample=True, blur_kernel=[1, 3, 3, 1])
        x = torch.randn(b, cin, hw, hw, generator=g).requires_grad_(True)
        st = torch.randn(b, STYLE_DIM, generator=g).requires_grad_(True)
        y = m(x, st)
        gy = torch.randn(*y.shape, generator=g)
        gx, gs, gw, gmw, gmb = torch.autograd.grad(y, (x, st, m.weight, m.modulation.weight, m.modulation.bias), gy)
        t = f"down{ci}"
        out.update({f"{t}.x": npy(x), f"{t}.style": npy(st), f"{t}.w": npy(m.weight), f"{t}.mw": npy(m.modulation.weight),
                    f"{t}.mb": npy(m.modulation.bias), f"{t}.fir": npy(m.blur.kernel), f"{t}.y": npy(y), f"{t}.gy": npy(gy),
                    f"{t}.gx": npy(gx), f"{t}.gstyle": npy(gs), f"{t}.gw": npy(gw), f"{t}.gmw": npy(gmw), f"{t}.gmb": npy(gmb)})
        meta.append(dict(i=ci, b=b, cin=cin, cout=cout, k=k, hw=hw, demodulate=demod, pad=list(m.blur.pad), out_hw=list(y.shape[2:])))
    b, cin, cout, k = CASES[0][:4]
    torch.manual_seed(INIT_SEED)
    m = RL.ModulatedConv2d(cin, cout, k, STYLE_DIM, downsample=True)
    sd = m.state_dict()
    for key, v in sd.items():
        out[f"init.sd/{key}"] = npy(v)
    out["meta"] = np.array(json.dumps(dict(cases=meta, style_dim=STYLE_DIM, init=dict(
        seed=INIT_SEED, cin=cin, cout=cout, k=k, keys=[[key, list(v.shape)] for key, v in sd.items()], repr=repr(m)))))
    path = os.path.join(MG.OUT, "modconv_down.npz")
    np.savez_compressed(path, **out)
    print("modconv_down.npz", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
