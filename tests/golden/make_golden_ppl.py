#!/usr/bin/env python3
"""Generate tests/golden/ppl.npz: the REFERENCE's own perceptual path length (stylegan2/ppl.py) on its ``Generator`` and its LPIPS
(``net-lin`` / ``vgg`` / version 0.1 on the seeded stand-in backbone of tests/lpips_ref.py), on the CPU, every case in f64 and again
in f32.

Runs only where the reference is available; nothing of the reference is copied: the script imports it (``import_lpips`` /
``build_pnet`` of make_golden_lpips.py), compiles ``normalize`` / ``slerp`` / ``lerp`` out of ppl.py's syntax tree (``slerp`` finds
``normalize`` in its globals) and cuts the ``for batch in tqdm(batch_sizes):`` statement -- the per-batch body -- out of the same tree.
The loop runs unmodified: ``g.make_noise``, ``torch.randn`` and ``torch.rand`` are answered with the stored noise, z and t (in that
order, which is asserted), everything else is the reference's.

* ``lin/{k}``: the five lin vectors; ``meta["backbone"]``: seed and checksums of the stand-in (not stored, 59 MB).
* ``gen{size}/fill/*``: the biases and noise weights ``MGG.fill`` put into ``Generator(size, 32, 2)`` (seeded: ``meta["gen{size}"]``).
* ``{case}/z`` [8, 32], ``{case}/t`` [4], ``{case}/noise{i}``, ``{case}/dist`` [4]: the f64 run's distances (already divided by
  eps^2) as a float32 array; ``{case}/f32_dev``: the reference's own f32 run against its f64 run, max-abs over max-abs -- the input of
  the tests' tolerance.  Cases: ``w_e4`` / ``w_e2`` (size 32, w-space, eps 1e-4 / 1e-2), ``wcrop_e4`` (size 64, ``--crop``: a 32 x 32
  crop), ``z_e4`` / ``z_e2`` (size 32).  For ``--space z`` the reference's loop never assigns ``latent_e`` (a NameError); the script
  assigns it from the reference's ``slerp`` and ``g.style`` and lets the loop go on from there.
* ``interp/{D}_{B}/lat`` [2B, D], ``t`` [B] and, as FLOAT64 arrays (tests/test_ppl.py holds the torch forms of ideas_amd.ppl to them
  at 1e-12), ``normalize`` [2B, D], ``slerp`` / ``lerp`` [2B, D] in the row order of ``torch.stack([e0, e1], 1).view(2B, D)`` with
  eps = 1e-4; ``f32_dev`` = [slerp, lerp] of the f32 run.

    python tests/golden/make_golden_ppl.py
"""
import argparse
import ast
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG                      # noqa: E402
import make_golden_stylegan2_gen as MGG       # noqa: E402
import make_golden_lpips as MGL               # noqa: E402
import lpips_ref as LR                        # noqa: E402

STYLE_DIM, N_MLP, BATCH = 32, 2, 4
GENS = {32: dict(seed=640, fill_seed=641), 64: dict(seed=642, fill_seed=643)}
CASES = (("w_e4", 32, "w", 1e-4, False, 4400), ("w_e2", 32, "w", 1e-2, False, 4401), ("wcrop_e4", 64, "w", 1e-4, True, 4402),
         ("z_e4", 32, "z", 1e-4, False, 4403), ("z_e2", 32, "z", 1e-2, False, 4404))
INTERP_SEED, INTERP_EPS = 4500, 1e-4
dev, f32 = MGL.dev, MGL.f32


def reference_functions():
    fns = {n: MG.load_reference_function("stylegan2/ppl.py", n) for n in ("normalize", "slerp", "lerp")}
    fns["slerp"].__globals__["normalize"] = fns["normalize"]
    return fns


def reference_loop():
    """The ``for batch in tqdm(batch_sizes):`` statement of stylegan2/ppl.py, compiled on its own."""
    path = os.path.join(MG.REF, "stylegan2", "ppl.py")
    tree = ast.parse(open(path).read())
    hits = [n for n in ast.walk(tree) if isinstance(n, ast.For) and ast.unparse(n.iter) == "tqdm(batch_sizes)"]
    assert len(hits) == 1, [(n.lineno, n.end_lineno) for n in hits]
    return compile(ast.Module(body=hits, type_ignores=[]), path, "exec")


class Draws:
    """Stands for ``torch`` inside the loop: ``randn`` / ``rand`` return the stored z / t, every other name is torch's own."""
    def __init__(self, z, t, order):
        self._z, self._t, self._order = z, t, order

    def randn(self, shape, device=None):
        assert list(shape) == list(self._z.shape), shape
        self._order.append("randn")
        return self._z

    def rand(self, n, device=None):
        assert n == self._t.shape[0], n
        self._order.append("rand")
        return self._t

    def __getattr__(self, name):
        return getattr(torch, name)


class Gen:
    """The reference's generator with ``make_noise`` answered from the stored maps."""
    def __init__(self, g, noise, order):
        self._g, self._noise, self._order = g, noise, order

    def make_noise(self):
        self._order.append("make_noise")
        return self._noise

    def get_latent(self, x):
        return self._g.get_latent(x)

    def __call__(self, *a, **k):
        return self._g(*a, **k)


def stack_ends(f, lat, t, eps):
    a, b = lat[::2], lat[1::2]
    return torch.stack([f(a, b, t[:, None]), f(a, b, t[:, None] + eps)], 1).view(*lat.shape)


def run_case(loop, fns, g, net, z, t, noise, space, eps, crop, dtype):
    from torch.nn import functional as F
    g, net = copy.deepcopy(g).to(dtype), copy.deepcopy(net).to(dtype)
    z, t, noise = z.to(dtype), t.to(dtype), [n.to(dtype) for n in noise]
    order, distances = [], []
    scope = dict(fns, torch=Draws(z, t, order), F=F, np=np, tqdm=lambda it: it, batch_sizes=[t.shape[0]], g=Gen(g, noise, order),
                 device="cpu", latent_dim=z.shape[1], args=argparse.Namespace(space=space, eps=eps, crop=crop),
                 percept=lambda a, b: net.forward(b, a), distances=distances)
    with torch.no_grad():
        if space == "z":                                   # what the reference's loop leaves out: latent_e for --space z
            scope["latent_e"] = g.style(stack_ends(fns["slerp"], z, t, eps))
        exec(loop, scope)
    assert order == ["make_noise", "randn", "rand"], order
    assert len(distances) == 1 and distances[0].shape == (t.shape[0],)
    return torch.from_numpy(distances[0])


def gen_cases(out, meta, RL, net32, fns):
    loop = reference_loop()
    gens = {}
    for size, cfg in GENS.items():
        torch.manual_seed(cfg["seed"])
        g = RL.Generator(size, STYLE_DIM, N_MLP)
        meta[f"gen{size}"] = dict(cfg, size=size, style_dim=STYLE_DIM, n_mlp=N_MLP, checksums=LR.checksums(g.state_dict()))
        for name, v in MGG.fill(g, cfg["fill_seed"]).items():
            out[f"gen{size}/fill/{name}"] = f32(v)
        gens[size] = g.eval()
    meta["cases"] = []
    for tag, size, space, eps, crop, seed in CASES:
        gen = torch.Generator().manual_seed(seed)
        g = gens[size]
        noise = [torch.randn(n.shape, generator=gen) for n in g.make_noise()]
        z = torch.randn(2 * BATCH, STYLE_DIM, generator=gen)
        t = torch.rand(BATCH, generator=gen)
        d64 = run_case(loop, fns, g, net32, z, t, noise, space, eps, crop, torch.float64)
        d32 = run_case(loop, fns, g, net32, z, t, noise, space, eps, crop, torch.float32)
        assert d64.dtype == torch.float64 and d32.dtype == torch.float32 and bool(torch.isfinite(d64).all())
        out[f"{tag}/z"], out[f"{tag}/t"], out[f"{tag}/dist"] = f32(z), f32(t), f32(d64)
        for i, n in enumerate(noise):
            out[f"{tag}/noise{i}"] = f32(n)
        out[f"{tag}/f32_dev"] = np.array(dev(d32, d64), np.float64)
        meta["cases"].append(dict(tag=tag, size=size, space=space, eps=eps, crop=crop, n_noises=len(noise)))
        print(tag, "dist", d64.tolist(), "f32_dev", dev(d32, d64))


def gen_interp(out, meta, fns):
    gen = torch.Generator().manual_seed(INTERP_SEED)
    meta["interp"] = dict(eps=INTERP_EPS, cases=[])
    for d in (32, 100, 512):
        for b in (1, 3):
            lat = torch.randn(2 * b, d, generator=gen)
            t = torch.rand(b, generator=gen)
            tag = f"interp/{d}_{b}"
            out[f"{tag}/lat"], out[f"{tag}/t"] = f32(lat), f32(t)
            r = {}
            for dtype in (torch.float64, torch.float32):
                r[dtype] = {n: stack_ends(fns[n], lat.to(dtype), t.to(dtype), INTERP_EPS) for n in ("slerp", "lerp")}
            out[f"{tag}/normalize"] = MG.npy(fns["normalize"](lat.double()))
            devs = []
            for n in ("slerp", "lerp"):
                out[f"{tag}/{n}"] = MG.npy(r[torch.float64][n])
                devs.append(dev(r[torch.float32][n], r[torch.float64][n]))
            out[f"{tag}/f32_dev"] = np.array(devs, np.float64)
            meta["interp"]["cases"].append([d, b])
            print(tag, "f32_dev (slerp, lerp)", devs)


def main():
    (RM, RU, RL, RO), RP = MGL.import_lpips()
    net32 = MGL.build_pnet(RP)
    out, meta = {}, {}
    sd = LR.backbone_state()
    meta["backbone"] = dict(seed=LR.BACKBONE_SEED, checksums=LR.checksums(sd))
    for k in range(5):
        out[f"lin/{k}"] = f32(getattr(net32, f"lin{k}").model[1].weight.reshape(-1))
    fns = reference_functions()
    gen_cases(out, meta, RL, net32, fns)
    gen_interp(out, meta, fns)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(MG.OUT, "ppl.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("ppl.npz", len(out), "arrays,", size, "bytes")
    assert size < 1_000_000, size


if __name__ == "__main__":
    main()
