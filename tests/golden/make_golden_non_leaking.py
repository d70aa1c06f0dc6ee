#!/usr/bin/env python3
"""Generate tests/golden/non_leaking.npz: the REFERENCE's own adaptive discriminator augmentation (stylegan2/non_leaking.py) on the
CPU, and the adaptation of its probability (stylegan2/train.py:194-213).

Runs only where the reference is available (``make_golden.import_reference``); nothing of the reference is copied, the script
imports it, feeds seeded inputs and stores arrays.  The reference module does ``from op import upfirdn2d``: after
``import_reference()`` the imported ``stylegan2.op`` is aliased as ``op`` and the reference's ``stylegan2`` directory is put on
``sys.path``; on the CPU the op takes its ``upfirdn2d_native`` branch.

* ``mats/seed{0..3}/p{0.3,1.0}/{G,C,pad}``: ``sample_affine(p, 4, 32, 32)`` then ``sample_color(p, 4)`` after ``torch.manual_seed(seed)``,
  and ``get_padding(inverse(G), 32, 32)``.
* Affine cases ``aff16`` / ``aff24x20`` / ``aff32`` / ``aff32_c5`` (``AFFINE_CASES``): after ``torch.manual_seed(seed)`` a float64 ``randn``
  input (its first three channels), ``G = sample_affine(1.0, B, H, W)``, then the input's further channels; run through ``random_apply_affine`` in float64:
  ``x`` (f64), ``G``, ``pads`` (asserted against the table: if the RNG stream ever changes the script stops instead of storing a case
  whose reflect pad does not exist), ``grid_dq`` -- the reference's final sampling grid ([B, h, w, 2]) in pixel coordinates of ``img_2x``,
  ``((g + 1) * size - 1) / 2``, as int32 fixed point in units of ``GRID_QUANTUM`` = 2^-20 pixel, differenced along ``ox`` (the grid is
  ``np.cumsum(grid_dq, axis=2) * GRID_QUANTUM``; the four float64 grids are 1.6 MB and do not compress, the steps of a near-affine grid
  do; the quantisation, 4.8e-7 pixel, is 200 times below what the test resolves) --, ``y``, ``cot``, ``gx`` = d(sum(y * cot))/dx
  (f32), and ``f32_dev`` = [output, gradient]: the reference's own f32 run against its f64 run, max-abs over max-abs.
* ``col``: ``C = sample_color(1.0, 3)`` at seed 0, ``x`` (3, 3, 9, 7), ``random_apply_color``: ``y``, ``cot``, ``gx``, ``f32_dev``.
* ``aug32``: ``augment(x, 1.0, (G, C))`` on the ``aff32`` inputs with ``C = sample_color(1.0, 2)`` at seed 0: ``C``, ``y``, ``cot``, ``gx``,
  ``f32_dev``.
* ``ada``: the ``if args.augment and args.augment_p == 0:`` block of stylegan2/train.py:194-213 -- cut out of the script's syntax tree and
  executed as it stands, stylegan2/train.py cannot be imported -- replayed over 40 seeded ``real_pred`` batches of 16 (mean +2 for the
  first 20, -2 after), ``ada_target = 0.6``, ``ada_length = 4000``, from ``p = 0`` (:152): ``ada/p`` with ``reduce_sum`` the identity (p
  rises, then falls back to the bound), ``ada/p_reduce8`` with ``reduce_sum = 8 * t`` (eight ranks holding the same tensor: p rises,
  clamps at 1, falls, clamps at 0).

    python tests/golden/make_golden_non_leaking.py
"""
import argparse
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG          # noqa: E402

GRID_QUANTUM = 2.0 ** -20
# tag, shape, seed, pads (x_low, x_high, y_low, y_high) the seeded G must give
AFFINE_CASES = (("aff16", (2, 3, 16, 16), 2, (5, 6, 8, 3)), ("aff24x20", (3, 3, 24, 20), 1, (12, 10, 4, 13)),
                ("aff32", (2, 3, 32, 32), 3, (20, 23, 17, 12)), ("aff32_c5", (2, 5, 32, 32), 2, (6, 6, 10, 4)))
ADA_TARGET, ADA_LENGTH, ADA_BATCHES, ADA_BATCH = 0.6, 4000, 40, 16


def import_non_leaking():
    mods = MG.import_reference()
    sys.modules["op"] = mods[3]
    sys.path.insert(0, os.path.join(MG.REF, "stylegan2"))
    import non_leaking as RN
    return RN


def dev(a32, a64):
    return float((a32.double() - a64).abs().max() / a64.abs().max())


def run_pair(fn, x64, gen):
    """fn(x) -> y in f64 and in f32 on the same input: y, a cotangent, d(sum(y * cot))/dx, and the f32 run's deviations."""
    x = x64.clone().requires_grad_(True)
    y = fn(x)
    cot = torch.randn(*y.shape, generator=gen, dtype=torch.float64)
    (gx,) = torch.autograd.grad((y * cot).sum(), x)
    x32 = x64.float().requires_grad_(True)
    y32 = fn(x32)
    assert y32.dtype == torch.float32
    (gx32,) = torch.autograd.grad((y32 * cot.float()).sum(), x32)
    return y.detach(), cot, gx, np.array([dev(y32.detach(), y.detach()), dev(gx32, gx)], np.float64)


def store(out, tag, y, cot, gx, f32_dev):
    npy = MG.npy
    out[f"{tag}/y"], out[f"{tag}/cot"], out[f"{tag}/gx"] = npy(y.float()), npy(cot.float()), npy(gx.float())
    out[f"{tag}/f32_dev"] = f32_dev
    print(tag, tuple(y.shape), "f32_dev (y, gx)", f32_dev)


class GridSpy:
    """Records the (input, grid) of the F.grid_sample calls made while it is active."""
    def __init__(self, F):
        self.F, self.calls = F, []

    def __enter__(self):
        self.orig = self.F.grid_sample
        spy = self

        def grid_sample(input, grid, *a, **k):
            assert k.get("align_corners") is False and k.get("padding_mode") == "zeros" and k.get("mode") == "bilinear"
            spy.calls.append((tuple(input.shape), grid.detach().clone()))
            return spy.orig(input, grid, *a, **k)
        self.F.grid_sample = grid_sample
        return self

    def __exit__(self, *exc):
        self.F.grid_sample = self.orig


def reference_ada_block():
    """The `if args.augment and args.augment_p == 0:` statement of the training loop of stylegan2/train.py, compiled on its own."""
    path = os.path.join(MG.REF, "stylegan2", "train.py")
    tree = ast.parse(open(path).read())
    hits = [n for n in ast.walk(tree) if isinstance(n, ast.If) and ast.unparse(n.test) == "args.augment and args.augment_p == 0"]
    assert len(hits) == 1 and (hits[0].lineno, hits[0].end_lineno) == (194, 213), [(n.lineno, n.end_lineno) for n in hits]
    return compile(ast.Module(body=hits, type_ignores=[]), path, "exec")


def replay_ada(block, preds, reduce_sum):
    scope = dict(torch=torch, device="cpu", args=argparse.Namespace(augment=True, augment_p=0, ada_target=ADA_TARGET, ada_length=ADA_LENGTH),
                 reduce_sum=reduce_sum)
    # stylegan2/train.py:151-154
    scope.update(ada_augment=torch.tensor([0.0, 0.0]), ada_aug_p=0.0, ada_aug_step=ADA_TARGET / ADA_LENGTH, r_t_stat=0)
    ps = []
    for real_pred in preds:
        scope["real_pred"] = real_pred
        exec(block, scope)
        ps.append(float(scope["ada_aug_p"]))
    return np.array(ps, np.float64)


def main():
    RN = import_non_leaking()
    npy = MG.npy
    out = {}

    for seed in range(4):
        for p in (0.3, 1.0):
            torch.manual_seed(seed)
            G = RN.sample_affine(p, 4, 32, 32)
            C = RN.sample_color(p, 4)
            tag = f"mats/seed{seed}/p{p}"
            out[f"{tag}/G"], out[f"{tag}/C"] = npy(G), npy(C)
            out[f"{tag}/pad"] = np.array(RN.get_padding(torch.inverse(G), 32, 32), np.int64)

    kept = {}
    for tag, shape, seed, want_pads in AFFINE_CASES:
        # draw order after the seed: the first three channels of x, then G, then x's further channels (C = 5)
        torch.manual_seed(seed)
        x = torch.randn(shape[0], 3, shape[2], shape[3], dtype=torch.float64)
        G = RN.sample_affine(1.0, shape[0], shape[2], shape[3])
        if shape[1] > 3:
            x = torch.cat((x, torch.randn(shape[0], shape[1] - 3, shape[2], shape[3], dtype=torch.float64)), 1)
        pads = RN.get_padding(torch.inverse(G), shape[2], shape[3])
        assert tuple(pads) == want_pads, (tag, pads, want_pads)     # a case without a reflect pad would spin in the reference
        gen = torch.Generator().manual_seed(1000 + seed)
        with GridSpy(RN.F) as spy:
            y, cot, gx, f32_dev = run_pair(lambda t: RN.random_apply_affine(t, 1.0, G)[0], x, gen)
        in_shape, grid = spy.calls[0]                               # the f64 run
        assert grid.dtype == torch.float64
        size = torch.tensor([in_shape[3], in_shape[2]], dtype=torch.float64)
        pix = ((grid + 1) * size - 1) / 2
        assert float(pix.abs().max()) * 2 ** 20 < 2 ** 31
        out[f"{tag}/x"], out[f"{tag}/G"], out[f"{tag}/pads"] = npy(x), npy(G), np.array(pads, np.int64)
        out[f"{tag}/grid_dq"] = np.diff(np.round(npy(pix) / GRID_QUANTUM).astype(np.int32), axis=2, prepend=np.int32(0))
        out[f"{tag}/img_2x_hw"] = np.array(in_shape[2:], np.int64)
        store(out, tag, y, cot, gx, f32_dev)
        kept[tag] = (x, G)

    torch.manual_seed(0)
    C = RN.sample_color(1.0, 3)
    gen = torch.Generator().manual_seed(2000)
    x = torch.randn(3, 3, 9, 7, generator=gen, dtype=torch.float64)
    out["col/x"], out["col/C"] = npy(x), npy(C)
    store(out, "col", *run_pair(lambda t: RN.random_apply_color(t, 1.0, C)[0], x, gen))

    x, G = kept["aff32"]
    torch.manual_seed(0)
    C = RN.sample_color(1.0, 2)
    gen = torch.Generator().manual_seed(3000)
    out["aug32/C"] = npy(C)
    store(out, "aug32", *run_pair(lambda t: RN.augment(t, 1.0, (G, C))[0], x, gen))

    gen = torch.Generator().manual_seed(4000)
    preds = [torch.randn(ADA_BATCH, 1, generator=gen) + (2.0 if i < ADA_BATCHES // 2 else -2.0) for i in range(ADA_BATCHES)]
    block = reference_ada_block()
    out["ada/real_pred"] = np.stack([npy(t) for t in preds])
    out["ada/p"] = replay_ada(block, preds, lambda t: t)
    out["ada/p_reduce8"] = replay_ada(block, preds, lambda t: t * 8)
    out["ada/settings"] = np.array([ADA_TARGET, ADA_LENGTH], np.float64)
    print("ada p", out["ada/p"][[0, 15, 16, 31, 39]], "reduce8", out["ada/p_reduce8"])

    path = os.path.join(MG.OUT, "non_leaking.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("non_leaking.npz", len(out), "arrays,", size, "bytes")
    assert size < 1_000_000, size


if __name__ == "__main__":
    main()
