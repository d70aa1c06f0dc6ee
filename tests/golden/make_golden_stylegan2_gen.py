#!/usr/bin/env python3
"""Generate tests/golden/stylegan2_gen.npz: the REFERENCE's own ``Generator``, ``StyledConv``, ``ToRGB``, ``Upsample``, ``Downsample``
and ``PixelNorm`` (stylegan2/model.py:14-72, 280-581) on the CPU.

Runs only where the reference is available (``make_golden.import_reference``); nothing of the reference is copied, the script
imports it, feeds seeded inputs and stores tensors.

* The weights are NOT stored: the tests rebuild them from the seed; ``meta["init"]`` carries keys / shapes, ``named_parameters`` order,
  per-key (sum, abs-sum) checksums and ``repr`` of the seeded construction for sizes 8 and 16.  After construction every ``*.bias``
  (``to_rgb*.bias`` and the modulation biases included) and every ``noise.weight`` is filled with seeded normal values -- at their
  initial zeros a wrong noise or bias path is invisible; those are stored (``gen8/fill/*``, ``gen16/fill/*``).
* ``gen8`` / ``gen16``: ``Generator(8, 32, 2)`` / ``Generator(16, 32, 2)``, batch 2, explicit per-layer noise [B, 1, H, W]: z, noises,
  image, latent, cotangent, d(sum(image * cot))/dz, per-parameter gradient norms.  ``gen8_bufs`` (``randomize_noise=False``),
  ``gen8_mix`` (two styles, ``inject_index=2``), ``gen8_trunc`` (``truncation=0.7`` with a stored ``truncation_latent``), ``gen8_wlat``
  (``input_is_latent=True``): the same record, on the registered noise buffers.
* ``gen8_path``: ``g_path_regularize`` of stylegan2/train.py on a [2, n_latent, 32] leaf latent (``input_is_latent=True``), stored image
  noise, ``mean_path_length = 0``: penalty, mean, lengths, per-parameter gradient norms of the penalty.
* Layer cases at small width (state dict, input, style, noise, output, cotangent, all gradients -- noise and style included):
  ``sc_same`` / ``sc_up`` / ``sc_c5`` (StyledConv), ``rgb_skip`` / ``rgb_plain`` (ToRGB), ``up`` / ``down`` (Upsample / Downsample), ``pn``.

    python tests/golden/make_golden_stylegan2_gen.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG          # noqa: E402

GEN_SEED, FILL_SEED, STYLE_DIM, N_MLP = 620, 621, 32, 2
SC_CASES = (dict(tag="sc_same", cin=8, cout=12, upsample=False), dict(tag="sc_up", cin=8, cout=12, upsample=True),
            dict(tag="sc_c5", cin=8, cout=5, upsample=False))


def is_filled(name):
    return name.endswith("bias") or name.endswith("noise.weight")


def fill(net, seed):
    gen = torch.Generator().manual_seed(seed)
    res = {}
    for name, p in net.named_parameters():
        if is_filled(name):
            p.data.copy_(torch.randn(p.shape, generator=gen))
            res[name] = p.detach().clone()
    return res


def checksums(sd):
    return {k: [float(v.double().sum()), float(v.double().abs().sum())] for k, v in sd.items()}


def record(out, tag, inputs, outputs, params, gen, names=None):
    """inputs: {name: leaf tensor}; outputs: {name: tensor}; the cotangent is drawn for outputs["y"]."""
    npy = MG.npy
    y = outputs["y"]
    cot = torch.randn(*y.shape, generator=gen)
    leaves = list(inputs.values())
    grads = torch.autograd.grad((y * cot).sum(), leaves + params, allow_unused=True)
    for k, v in inputs.items():
        out[f"{tag}/{k}"] = npy(v)
    for k, v in outputs.items():
        out[f"{tag}/{k}"] = npy(v)
    out[f"{tag}/cot"] = npy(cot)
    for k, g in zip(inputs, grads):
        out[f"{tag}/g_{k}"] = npy(g)
    pg = grads[len(leaves):]
    if names is None:
        out[f"{tag}/gparam_norms"] = np.array([0.0 if g is None else float(g.double().norm()) for g in pg], dtype=np.float64)
    else:
        for n, g in zip(names, pg):
            out[f"{tag}/g/{n}"] = npy(g)


def main():
    RM, RU, RL, RO = MG.import_reference()
    path_fn = MG.load_reference_function("stylegan2/train.py", "g_path_regularize")
    npy = MG.npy
    out, meta = {}, {}
    gen = torch.Generator().manual_seed(71)
    rn = lambda *s: torch.randn(*s, generator=gen)

    # ---- seeded construction: keys, shapes, order, checksums, repr (before anything is filled)
    init = {}
    for size in (8, 16):
        torch.manual_seed(GEN_SEED)
        net = RL.Generator(size, STYLE_DIM, N_MLP)
        sd = net.state_dict()
        init[str(size)] = dict(keys=[[k, list(v.shape)] for k, v in sd.items()], param_keys=[k for k, _ in net.named_parameters()],
                               checksums=checksums(sd), repr=repr(net), n_latent=net.n_latent, num_layers=net.num_layers,
                               log_size=net.log_size, n_params=sum(p.numel() for p in net.parameters()))
    meta["init"] = dict(seed=GEN_SEED, fill_seed=FILL_SEED, style_dim=STYLE_DIM, n_mlp=N_MLP, sizes=init)

    # ---- Generator(8) / Generator(16), batch 2
    nets = {}
    for size in (8, 16):
        torch.manual_seed(GEN_SEED)
        net = RL.Generator(size, STYLE_DIM, N_MLP)
        for name, v in fill(net, FILL_SEED).items():
            out[f"gen{size}/fill/{name}"] = npy(v)
        nets[size] = net
        params = [p for _, p in net.named_parameters()]
        z = rn(2, STYLE_DIM).requires_grad_(True)
        noises = [rn(2, 1, n.shape[2], n.shape[3]) for n in net.make_noise()]
        for i, n in enumerate(noises):
            out[f"gen{size}/noise{i}"] = npy(n)
        image, latent = net([z], return_latents=True, noise=noises)
        record(out, f"gen{size}", dict(z0=z), dict(y=image, latent=latent), params, gen)
    net = nets[8]
    params = [p for _, p in net.named_parameters()]
    z = rn(2, STYLE_DIM).requires_grad_(True)
    image, latent = net([z], return_latents=True, randomize_noise=False)
    record(out, "gen8_bufs", dict(z0=z), dict(y=image, latent=latent), params, gen)
    z0, z1 = rn(2, STYLE_DIM).requires_grad_(True), rn(2, STYLE_DIM).requires_grad_(True)
    image, latent = net([z0, z1], return_latents=True, inject_index=2, randomize_noise=False)
    record(out, "gen8_mix", dict(z0=z0, z1=z1), dict(y=image, latent=latent), params, gen)
    z = rn(2, STYLE_DIM).requires_grad_(True)
    tl = rn(1, STYLE_DIM)
    out["gen8_trunc/truncation_latent"] = npy(tl)
    image, latent = net([z], return_latents=True, truncation=0.7, truncation_latent=tl, randomize_noise=False)
    record(out, "gen8_trunc", dict(z0=z), dict(y=image, latent=latent), params, gen)
    w = rn(2, STYLE_DIM).requires_grad_(True)
    image, latent = net([w], return_latents=True, input_is_latent=True, randomize_noise=False)
    record(out, "gen8_wlat", dict(z0=w), dict(y=image, latent=latent), params, gen)

    # ---- path length on a [2, n_latent, 32] leaf latent
    lat = rn(2, net.n_latent, STYLE_DIM).requires_grad_(True)
    noises = [torch.from_numpy(out[f"gen8/noise{i}"]) for i in range(net.num_layers)]
    image, _ = net([lat], input_is_latent=True, noise=noises)
    img_noise = rn(*image.shape)
    o_randn_like = torch.randn_like
    torch.randn_like = lambda t, **k: img_noise.clone()        # the function draws its noise itself
    try:
        pen, mean, lengths = path_fn(image, lat, torch.tensor(0.0))
    finally:
        torch.randn_like = o_randn_like
    grads = torch.autograd.grad(pen, params, allow_unused=True)
    out.update({"gen8_path/latent": npy(lat), "gen8_path/img_noise": npy(img_noise), "gen8_path/image": npy(image),
                "gen8_path/penalty": npy(pen).astype(np.float64), "gen8_path/mean": npy(mean).astype(np.float64),
                "gen8_path/lengths": npy(lengths),
                "gen8_path/gparam_norms": np.array([0.0 if g is None else float(g.double().norm()) for g in grads], dtype=np.float64)})

    # ---- layers at small width
    meta["sc"] = []
    for i, c in enumerate(SC_CASES):
        torch.manual_seed(640 + i)
        m = RL.StyledConv(c["cin"], c["cout"], 3, 16, upsample=c["upsample"])
        fill(m, 650 + i)
        tag = c["tag"]
        for k, v in m.state_dict().items():
            out[f"{tag}/sd/{k}"] = npy(v)
        x, style = rn(2, c["cin"], 9, 9).requires_grad_(True), rn(2, 16).requires_grad_(True)
        hw = 18 if c["upsample"] else 9
        noise = rn(2, 1, hw, hw).requires_grad_(True)
        names = [n for n, _ in m.named_parameters()]
        record(out, tag, dict(x=x, style=style, noise=noise), dict(y=m(x, style, noise=noise)), [p for _, p in m.named_parameters()], gen, names)
        meta["sc"].append(dict(c, params=names, out_hw=hw))
    meta["rgb"] = []
    for i, (tag, ups) in enumerate((("rgb_skip", True), ("rgb_plain", False))):
        torch.manual_seed(660 + i)
        m = RL.ToRGB(8, 16, upsample=ups)
        fill(m, 670 + i)
        for k, v in m.state_dict().items():
            out[f"{tag}/sd/{k}"] = npy(v)
        x, style = rn(2, 8, 18, 18).requires_grad_(True), rn(2, 16).requires_grad_(True)
        names = [n for n, _ in m.named_parameters()]
        if ups:
            skip = rn(2, 3, 9, 9).requires_grad_(True)
            record(out, tag, dict(x=x, style=style, skip=skip), dict(y=m(x, style, skip)), [p for _, p in m.named_parameters()], gen, names)
        else:
            record(out, tag, dict(x=x, style=style), dict(y=m(x, style)), [p for _, p in m.named_parameters()], gen, names)
        meta["rgb"].append(dict(tag=tag, upsample=ups, params=names))
    for tag, m in (("up", RL.Upsample([1, 3, 3, 1])), ("down", RL.Downsample([1, 3, 3, 1]))):
        x = rn(2, 5, 9, 9).requires_grad_(True)
        record(out, tag, dict(x=x), dict(y=m(x)), [], gen, [])
        meta[tag] = dict(pad=list(m.pad), kernel=npy(m.kernel).tolist(), out_hw=list(out[f"{tag}/y"].shape[2:]))
    x = rn(3, STYLE_DIM).requires_grad_(True)
    record(out, "pn", dict(x=x), dict(y=RL.PixelNorm()(x)), [], gen, [])

    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(MG.OUT, "stylegan2_gen.npz")
    np.savez_compressed(path, **out)
    print("stylegan2_gen.npz", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
