#!/usr/bin/env python3
"""Generate tests/golden/stylegan2_disc.npz: the REFERENCE's own ``ConvLayer``, ``ResBlock`` and ``Discriminator``
(stylegan2/model.py:584-712) on the CPU.

Runs only where the reference is available (``make_golden.import_reference``); nothing of the reference is copied, the script
imports it, feeds seeded inputs and stores tensors.

* ``disc8_b8`` / ``disc8_b4``: ``Discriminator(8)`` on [8, 3, 8, 8] (M = 2 statistics) and [4, 3, 8, 8]: input, logits, d(sum logits)/dx,
  per-parameter gradient norms, the R1 penalty of ``utils.d_r1_loss`` with the gradient norms of its backward, and the tensor
  LEAVING the minibatch-stddev block (a forward hook on ``final_conv``): the reference's own inline expression is the op's golden.
  The tensor entering the block is its first 512 channels (``torch.cat`` copies), checked here against a hook on ``convs``.
  ``mb_b3``: the same capture for a batch of 3 (G = 3).  ``*/mb_stat64``: the statistic channel of the same expression evaluated in
  f64 on the captured (f32) block input -- the same Discriminator instance cast to double with ``convs`` swapped for an identity, so
  that ``forward`` applies its inline expression to the tensor it is given.
* The 11.5 M weights are NOT stored: the tests rebuild them from the seed; ``meta`` carries per-key (sum, abs-sum) checksums of the
  seeded construction for sizes 8 and 16.  After construction every ``*.bias`` is filled with seeded normal values (at their
  initial zeros a bias bug is invisible); those are stored.
* ``res``: ``ResBlock(16, 32)`` on [2, 16, 32, 32]; ``conv0..2``: the three ``ConvLayer`` shapes of a block on [2, 8, 9, 9] (the odd
  size exercises the blur pads) -- state dict, input, output, cotangent and all gradients.

    python tests/golden/make_golden_stylegan2_disc.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG          # noqa: E402

DISC_SEED, BIAS_SEED = 520, 521
CONV_CASES = (dict(cin=8, cout=8, k=3, downsample=False, bias=True, activate=True),
              dict(cin=8, cout=12, k=3, downsample=True, bias=True, activate=True),
              dict(cin=8, cout=12, k=1, downsample=True, bias=False, activate=False))


def fill_biases(net, seed):
    gen = torch.Generator().manual_seed(seed)
    res = {}
    for name, p in net.named_parameters():
        if name.endswith("bias"):
            p.data.copy_(torch.randn(p.shape, generator=gen))
            res[name] = p.detach().clone()
    return res


def checksums(sd):
    return {k: [float(v.double().sum()), float(v.double().abs().sum())] for k, v in sd.items()}


def layer_case(out, tag, m, x, gen):
    npy = MG.npy
    for k, v in m.state_dict().items():
        out[f"{tag}/sd/{k}"] = npy(v)
    x = x.requires_grad_(True)
    y = m(x)
    gy = torch.randn(*y.shape, generator=gen)
    names = [n for n, _ in m.named_parameters()]
    grads = torch.autograd.grad(y, [x] + [p for _, p in m.named_parameters()], gy)
    out.update({f"{tag}/x": npy(x), f"{tag}/y": npy(y), f"{tag}/gy": npy(gy), f"{tag}/gx": npy(grads[0])})
    for n, g in zip(names, grads[1:]):
        out[f"{tag}/g/{n}"] = npy(g)
    return names


def main():
    RM, RU, RL, RO = MG.import_reference()
    npy = MG.npy
    out, meta = {}, {}
    gen = torch.Generator().manual_seed(61)

    # ---- seeded construction: keys, shapes, checksums (before the biases are filled)
    init = {}
    for size in (8, 16):
        torch.manual_seed(DISC_SEED)
        net = RL.Discriminator(size)
        sd = net.state_dict()
        init[str(size)] = dict(keys=[[k, list(v.shape)] for k, v in sd.items()], param_keys=[k for k, _ in net.named_parameters()],
                               checksums=checksums(sd), repr=repr(net),
                               padding={n: m.padding for n, m in net.named_modules() if isinstance(m, RL.ConvLayer)})
    meta["init"] = dict(seed=DISC_SEED, bias_seed=BIAS_SEED, sizes=init)

    # ---- Discriminator(8)
    torch.manual_seed(DISC_SEED)
    net = RL.Discriminator(8)
    for name, b in fill_biases(net, BIAS_SEED).items():
        out[f"disc8/bias/{name}"] = npy(b)
    params = [p for _, p in net.named_parameters()]
    cap = {}
    h1 = net.convs.register_forward_hook(lambda mod, inp, res: cap.__setitem__("in", res.detach().clone()))
    h2 = net.final_conv.register_forward_hook(lambda mod, inp, res: cap.__setitem__("out", inp[0].detach().clone()))
    for tag, b in (("disc8_b8", 8), ("disc8_b4", 4)):
        x = torch.randn(b, 3, 8, 8, generator=gen).requires_grad_(True)
        logits = net(x)
        assert torch.equal(cap["out"][:, :512], cap["in"])            # cat copies: the block input is the first 512 channels
        grads = torch.autograd.grad(logits.sum(), [x] + params)
        out.update({f"{tag}/x": npy(x), f"{tag}/logits": npy(logits), f"{tag}/gx": npy(grads[0]), f"{tag}/mb_out": npy(cap["out"]),
                    f"{tag}/gparam_norms": np.array([float(g.norm()) for g in grads[1:]], dtype=np.float64)})
        x2 = x.detach().clone().requires_grad_(True)
        r1 = RU.d_r1_loss(net(x2), x2)
        gr = torch.autograd.grad(r1, params, allow_unused=True)
        out[f"{tag}/r1"] = np.array(float(r1.detach()), dtype=np.float64)
        out[f"{tag}/r1_gparam_norms"] = np.array([0.0 if g is None else float(g.norm()) for g in gr], dtype=np.float64)
    with torch.no_grad():
        net(torch.randn(3, 3, 8, 8, generator=gen))
    assert torch.equal(cap["out"][:, :512], cap["in"])
    out["mb_b3/mb_out"] = npy(cap["out"])
    h1.remove()
    net64 = net.double()
    net64.convs = torch.nn.Identity()
    with torch.no_grad():
        for tag in ("disc8_b8", "disc8_b4", "mb_b3"):
            net64(torch.from_numpy(out[f"{tag}/mb_out"][:, :512]).double())
            assert cap["out"].dtype == torch.float64
            out[f"{tag}/mb_stat64"] = npy(cap["out"][:, 512:])
    h2.remove()

    # ---- ResBlock(16, 32) and the three ConvLayer shapes of a block
    torch.manual_seed(530)
    m = RL.ResBlock(16, 32)
    fill_biases(m, 531)
    meta["res"] = dict(in_channel=16, out_channel=32, params=layer_case(out, "res", m, torch.randn(2, 16, 32, 32, generator=gen), gen))
    meta["conv"] = []
    for i, c in enumerate(CONV_CASES):
        torch.manual_seed(540 + i)
        m = RL.ConvLayer(c["cin"], c["cout"], c["k"], downsample=c["downsample"], bias=c["bias"], activate=c["activate"])
        fill_biases(m, 550 + i)
        names = layer_case(out, f"conv{i}", m, torch.randn(2, c["cin"], 9, 9, generator=gen), gen)
        meta["conv"].append(dict(c, i=i, padding=m.padding, params=names, out_hw=list(out[f"conv{i}/y"].shape[2:])))
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(MG.OUT, "stylegan2_disc.npz")
    np.savez_compressed(path, **out)
    print("stylegan2_disc.npz", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
