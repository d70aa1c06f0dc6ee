#!/usr/bin/env python3
"""Generate tests/golden/lpips.npz: the REFERENCE's own LPIPS (stylegan2/lpips, ``net-lin`` / ``vgg`` / version 0.1) and the helpers and
optimisation loop of stylegan2/projector.py, on the CPU, every quantity in f32 and again in f64.

Runs only where the reference is available (``make_golden.import_reference``); nothing of the reference is copied: the script imports
it (stub modules stand for ``skimage``, ``IPython`` and ``torchvision``; ``torchvision.models.vgg16`` is tests/lpips_ref.py's seeded
stand-in), cuts the functions and the ``for i in pbar:`` loop of projector.py out of its syntax tree, feeds seeded inputs and stores
arrays.  The f64 results are stored (as float32 arrays: the rounding, 6e-8, is far below what the tests resolve); ``*/f32_dev`` is the
reference's own f32 run against its f64 run, max-abs over max-abs -- the input of the tests' tolerances.

* The backbone is NOT stored (59 MB): ``meta["backbone"]`` has the seed, keys / shapes and per-key (sum, abs-sum) checksums.
* ``lin/{k}``: the five lin vectors of ``weights/v0.1/vgg.pth``.
* Pairs ``near`` (pred = target + 0.05 randn), ``far`` (unrelated) and ``same`` (identical), images (2, 3, 40, 24) in [-1, 1]:
  ``{pair}/pred``, ``{pair}/target``, ``{pair}/layers`` [5, 2] (``retPerLayer``; its first entry aliases the total in the
  reference, so layer 0 is recomputed from the reference's functions), ``{pair}/val`` [2], ``{pair}/gpred`` = d val.sum() / d pred,
  ``{pair}/tap_sums`` [5, 2, 2] (per tap and sample: sum and abs-sum of the pred side's tap), ``{pair}/f32_dev`` = [taps, layers, val,
  gpred].  ``near/tap{k}``: the pred side's five taps of sample 0; ``far/tap{2,3,4}``: the pred side's three deep taps of sample 1.  ``near01/*``: the ``near`` pair mapped to [0, 1] with ``normalize=True``.
  Every stored gradient is asserted finite (no all-zero pixel at these seeds).
* ``helpers/*``: ``noise_regularize`` (value, gradients) on noises of sizes 4 .. 32, ``noise_normalize_``, ``get_lr`` on a grid of t,
  ``make_image`` on a seeded tensor.
* ``proj/{w,wplus}/*``: 3 steps of the reference's loop on ``Generator(32, 32, 2)`` (seeded, biases and noise weights filled),
  ``--noise 0 --noise_regularize 1e5 --mse 0.1``, 2 images: ``latent_mean``, ``latent_std``, the initial ``noise{i}``, ``imgs``, per step
  ``losses`` [3, 3] (p, n, mse), the step-0 gradients ``g_latent`` / ``g_noise{i}``, the final ``latent_in``; ``f32_dev`` = [losses,
  g_latent, g_noise (max over layers)], ``update_dev`` = relative L2 of the f32 run's update ``latent_in - latent_mean`` against the f64
  run's, ``sign_frac`` = the fraction of the update's elements whose sign differs between the two (asserted <= 2 %).

    python tests/golden/make_golden_lpips.py
"""
import argparse
import ast
import copy
import json
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG                      # noqa: E402
import make_golden_stylegan2_gen as MGG       # noqa: E402
import lpips_ref as LR                        # noqa: E402

IMG_SEED, HELPER_SEED = 4100, 4200
GEN_SEED, FILL_SEED, PROJ_SEED, STYLE_DIM, N_MLP, GEN_SIZE = 630, 631, 4300, 32, 2, 32
PROJ = dict(step=3, lr=0.1, noise=0.0, noise_ramp=0.75, noise_regularize=1e5, mse=0.1)
SIGN_LIMIT = 0.02


def import_lpips():
    mods = MG.import_reference()
    tv = sys.modules["torchvision"]
    tv.models = types.ModuleType("torchvision.models")
    tv.models.vgg16 = lambda pretrained=False, **k: types.SimpleNamespace(features=LR.vgg16_features())
    sk = types.ModuleType("skimage")
    sk.measure, sk.color, sk.transform = (types.ModuleType("skimage." + n) for n in ("measure", "color", "transform"))
    sk.measure.compare_ssim = None
    ip = types.ModuleType("IPython")
    ip.embed = None
    sys.modules.update({"torchvision.models": tv.models, "skimage": sk, "skimage.measure": sk.measure, "skimage.color": sk.color,
                        "skimage.transform": sk.transform, "IPython": ip})
    sys.path.insert(0, os.path.join(MG.REF, "stylegan2"))
    import lpips as RP
    return mods, RP


def build_pnet(RP):
    """The PNetLin that ``PerceptualLoss(model='net-lin', net='vgg', use_gpu=False)`` holds, in eval mode."""
    try:
        percept = RP.PerceptualLoss(model="net-lin", net="vgg", use_gpu=False)
        net = percept.model.net
    except Exception as e:                                  # DistModel will not initialise here: build what it builds
        print("DistModel.initialize failed (%s: %s); building PNetLin directly" % (type(e).__name__, e))
        from lpips import networks_basic
        net = networks_basic.PNetLin(pnet_type="vgg", pnet_rand=True, use_dropout=True, version="0.1")
        path = os.path.join(MG.REF, "stylegan2", "lpips", "weights", "v0.1", "vgg.pth")
        net.load_state_dict(torch.load(path, map_location="cpu"), strict=False)
    return net.eval()


def dev(a32, a64):
    den = float(a64.abs().max())
    return float((a32.double() - a64).abs().max()) / (den if den > 0 else 1.0)


def f32(t):
    return MG.npy(t.detach().float())


def run_pair(net, pred, target, normalize=False):
    """val [N], layers [5, N], taps (pred side), d val.sum() / d pred, as the reference computes them in the dtype of ``net``."""
    dtype = next(net.parameters()).dtype
    pred = pred.to(dtype).clone().requires_grad_(True)
    target = target.to(dtype)
    p, t = (2 * pred - 1, 2 * target - 1) if normalize else (pred, target)
    val, res = net.forward(t, p, retPerLayer=True)          # PerceptualLoss.forward -> DistModel.forward(target, pred)
    res = torch.stack([r.reshape(-1) for r in res]).detach().clone()
    out_val = val.reshape(-1).detach().clone()
    (g,) = torch.autograd.grad(val.sum(), pred)
    with torch.no_grad():
        taps = [h.clone() for h in net.net.forward(net.scaling_layer(p.detach()))]
        # ``val = res[0]; val += res[l]`` (networks_basic.py:85-87) adds in place: the first entry of retPerLayer IS the total.  The
        # first layer's own distance, from the reference's functions on the first taps:
        tap_t = net.net.forward(net.scaling_layer(t))[0]
        import lpips as RP
        from lpips import networks_basic as NB
        assert torch.equal(res[0], out_val)
        res[0] = NB.spatial_average(net.lin0.model((RP.normalize_tensor(tap_t) - RP.normalize_tensor(taps[0])) ** 2)).reshape(-1)
        assert float((res.sum(0) - out_val).abs().max()) <= 1e-5 * float(out_val.abs().max()) + 1e-30
    assert val.dtype == dtype and bool(torch.isfinite(g).all()), "a stored reference gradient is not finite: pick another seed"
    return dict(val=out_val, layers=res, taps=taps, gpred=g)


def gen_pairs(out, net32, net64):
    gen = torch.Generator().manual_seed(IMG_SEED)
    target = torch.rand(2, 3, 40, 24, generator=gen, dtype=torch.float64) * 2 - 1
    near = (target + 0.05 * torch.randn(target.shape, generator=gen, dtype=torch.float64)).clamp(-1, 1)
    far = torch.rand(2, 3, 40, 24, generator=gen, dtype=torch.float64) * 2 - 1
    devs = {}
    for tag, pred, normalize in (("near", near, False), ("far", far, False), ("same", target.clone(), False), ("near01", near, True)):
        # the images are stored in f32 and both runs start from those values
        p, t = pred.float(), target.float()
        if normalize:
            p, t = (p + 1) / 2, (t + 1) / 2
        r64, r32 = run_pair(net64, p, t, normalize), run_pair(net32, p, t, normalize)
        d = [max(dev(a, b) for a, b in zip(r32["taps"], r64["taps"])), dev(r32["layers"], r64["layers"]), dev(r32["val"], r64["val"]),
             dev(r32["gpred"], r64["gpred"])]
        out[f"{tag}/pred"], out[f"{tag}/target"] = f32(p), f32(t)
        out[f"{tag}/layers"], out[f"{tag}/val"], out[f"{tag}/gpred"] = f32(r64["layers"]), f32(r64["val"]), f32(r64["gpred"])
        out[f"{tag}/tap_sums"] = np.array([[[float(h[n].sum()), float(h[n].abs().sum())] for n in range(2)] for h in r64["taps"]])
        out[f"{tag}/f32_dev"] = np.array(d, np.float64)
        if tag == "near":
            for k, h in enumerate(r64["taps"]):
                out[f"near/tap{k}"] = f32(h[0])
        if tag == "far":                                    # (the two large taps of a second pair would not fit the size limit)
            for k in (2, 3, 4):
                out[f"far/tap{k}"] = f32(r64["taps"][k][1])
        devs[tag] = d
        print(tag, "val", r64["val"].tolist(), "f32_dev (taps, layers, val, gpred)", d)
    assert float(np.abs(out["same/val"]).max()) == 0.0 and float(np.abs(out["same/gpred"]).max()) == 0.0
    return devs


def gen_helpers(out):
    fns = {n: MG.load_reference_function("stylegan2/projector.py", n)
           for n in ("noise_regularize", "noise_normalize_", "get_lr", "latent_noise", "make_image")}
    gen = torch.Generator().manual_seed(HELPER_SEED)
    noises = [torch.randn(2, 1, s, s, generator=gen, dtype=torch.float64) for s in (4, 8, 8, 16, 16, 32, 32)]
    d = []
    for dtype in (torch.float64, torch.float32):
        leaves = [n.to(dtype).clone().requires_grad_(True) for n in noises]
        loss = fns["noise_regularize"](leaves)
        grads = torch.autograd.grad(loss, leaves)
        normed = [n.to(dtype).clone() for n in noises]
        fns["noise_normalize_"](normed)
        if dtype == torch.float64:
            keep = (loss.detach(), grads, normed)
        else:
            d = [dev(loss.detach(), keep[0]), max(dev(a, b) for a, b in zip(grads, keep[1])), max(dev(a, b) for a, b in zip(normed, keep[2]))]
    for i, n in enumerate(noises):
        out[f"helpers/noise{i}"], out[f"helpers/nreg_g{i}"], out[f"helpers/normed{i}"] = f32(n), f32(keep[1][i]), f32(keep[2][i])
    out["helpers/nreg"] = np.array(float(keep[0]), np.float64)
    out["helpers/f32_dev"] = np.array(d, np.float64)
    ts = np.linspace(0.0, 1.0, 41)
    out["helpers/lr_t"] = ts
    out["helpers/lr"] = np.array([fns["get_lr"](float(t), 0.1) for t in ts], np.float64)
    out["helpers/lr_ramps"] = np.array([fns["get_lr"](float(t), 0.05, 0.5, 0.1) for t in ts], np.float64)
    x = torch.randn(2, 3, 6, 5, generator=gen) * 0.8
    out["helpers/img_in"] = f32(x)
    out["helpers/img_out"] = fns["make_image"](x.clone())
    print("helpers: noise_regularize", float(keep[0]), "f32_dev (nreg, grad, normalize)", d)
    return fns


def reference_loop():
    """The ``for i in pbar:`` statement of stylegan2/projector.py (:151-190), compiled on its own."""
    path = os.path.join(MG.REF, "stylegan2", "projector.py")
    tree = ast.parse(open(path).read())
    hits = [n for n in ast.walk(tree) if isinstance(n, ast.For) and ast.unparse(n.iter) == "pbar"]
    assert len(hits) == 1 and (hits[0].lineno, hits[0].end_lineno) == (151, 190), [(n.lineno, n.end_lineno) for n in hits]
    return compile(ast.Module(body=hits, type_ignores=[]), path, "exec")


class Bar:
    """Stands for tqdm: iterates the steps; ``set_description`` is the loop's last statement, where the step's losses and (after
    ``optimizer.step()``, which leaves them in place) its gradients are read."""
    def __init__(self, steps, scope, rec):
        self.steps, self.scope, self.rec = steps, scope, rec

    def __iter__(self):
        return iter(range(self.steps))

    def set_description(self, _):
        s = self.scope
        self.rec["losses"].append([float(s["p_loss"]), float(s["n_loss"]), float(s["mse_loss"])])
        if len(self.rec["losses"]) == 1:
            self.rec["g_latent"] = s["latent_in"].grad.detach().clone()
            self.rec["g_noise"] = [n.grad.detach().clone() for n in s["noises"]]


def replay(loop, fns, g_ema, net, imgs, latent_mean, latent_std, noises0, w_plus, dtype):
    from torch import optim
    from torch.nn import functional as F
    g_ema, net = copy.deepcopy(g_ema).to(dtype), copy.deepcopy(net).to(dtype)
    imgs = imgs.to(dtype)
    noises = [n.to(dtype).clone() for n in noises0]
    latent_in = latent_mean.to(dtype).detach().clone().unsqueeze(0).repeat(imgs.shape[0], 1)      # stylegan2/projector.py:136-146
    if w_plus:
        latent_in = latent_in.unsqueeze(1).repeat(1, g_ema.n_latent, 1)
    latent_in.requires_grad = True
    for n in noises:
        n.requires_grad = True
    args = argparse.Namespace(**PROJ)
    optimizer = optim.Adam([latent_in] + noises, lr=args.lr)
    rec = dict(losses=[])
    scope = dict(fns, torch=torch, math=math, F=F, args=args, g_ema=g_ema, imgs=imgs, noises=noises, latent_in=latent_in,
                 optimizer=optimizer, latent_std=latent_std.to(dtype), latent_path=[], percept=lambda a, b: net.forward(b, a))
    scope["pbar"] = Bar(args.step, scope, rec)
    exec(loop, scope)
    rec["latent_in"] = latent_in.detach().clone()
    rec["losses"] = torch.tensor(rec["losses"], dtype=torch.float64)
    return rec


def gen_projector(out, meta, RL, net32, fns):
    loop = reference_loop()
    torch.manual_seed(GEN_SEED)
    g_ema = RL.Generator(GEN_SIZE, STYLE_DIM, N_MLP)
    meta["gen"] = dict(seed=GEN_SEED, fill_seed=FILL_SEED, size=GEN_SIZE, style_dim=STYLE_DIM, n_mlp=N_MLP,
                       checksums=LR.checksums(g_ema.state_dict()))
    for name, v in MGG.fill(g_ema, FILL_SEED).items():
        out[f"proj/fill/{name}"] = f32(v)
    g_ema.eval()
    gen = torch.Generator().manual_seed(PROJ_SEED)
    with torch.no_grad():                                                                          # stylegan2/projector.py:120-125
        latent_out = g_ema.style(torch.randn(10000, STYLE_DIM, generator=gen))
        latent_mean = latent_out.mean(0)
        latent_std = ((latent_out - latent_mean).pow(2).sum() / 10000) ** 0.5
    noises0 = [n.repeat(2, 1, 1, 1).copy_(torch.randn(2, 1, n.shape[2], n.shape[3], generator=gen)) for n in g_ema.make_noise()]
    imgs = torch.rand(2, 3, GEN_SIZE, GEN_SIZE, generator=gen) * 2 - 1
    out["proj/latent_mean"], out["proj/latent_std"], out["proj/imgs"] = f32(latent_mean), f32(latent_std), f32(imgs)
    for i, n in enumerate(noises0):
        out[f"proj/noise{i}"] = f32(n)
    meta["proj"] = dict(PROJ, n_noises=len(noises0), sign_limit=SIGN_LIMIT)
    for tag, w_plus in (("w", False), ("wplus", True)):
        r64 = replay(loop, fns, g_ema, net32, imgs, latent_mean, latent_std, noises0, w_plus, torch.float64)
        r32 = replay(loop, fns, g_ema, net32, imgs, latent_mean, latent_std, noises0, w_plus, torch.float32)
        assert all(bool(torch.isfinite(g).all()) for g in [r64["g_latent"]] + r64["g_noise"])
        base = latent_mean.double().reshape((1,) * (r64["latent_in"].dim() - 1) + (-1,))
        u64, u32 = r64["latent_in"] - base, r32["latent_in"].double() - base
        update_dev = float((u32 - u64).norm() / u64.norm())
        sign_frac = float((torch.sign(u32) != torch.sign(u64)).double().mean())
        assert sign_frac <= SIGN_LIMIT, (tag, sign_frac, "pick another PROJ_SEED")
        d = [dev(r32["losses"], r64["losses"]), dev(r32["g_latent"], r64["g_latent"]),
             max(dev(a, b) for a, b in zip(r32["g_noise"], r64["g_noise"]))]
        out[f"proj/{tag}/losses"] = MG.npy(r64["losses"])
        out[f"proj/{tag}/g_latent"], out[f"proj/{tag}/latent_in"] = f32(r64["g_latent"]), f32(r64["latent_in"])
        out[f"proj/{tag}/update"] = MG.npy(u64)
        for i, g in enumerate(r64["g_noise"]):
            out[f"proj/{tag}/g_noise{i}"] = f32(g)
        out[f"proj/{tag}/f32_dev"] = np.array(d, np.float64)
        out[f"proj/{tag}/update_dev"], out[f"proj/{tag}/sign_frac"] = np.array(update_dev), np.array(sign_frac)
        print("proj", tag, "losses", r64["losses"].tolist(), "f32_dev (losses, g_latent, g_noise)", d, "update_dev", update_dev,
              "sign_frac", sign_frac, "|update|", float(u64.norm()))


def main():
    (RM, RU, RL, RO), RP = import_lpips()
    net32 = build_pnet(RP)
    net64 = copy.deepcopy(net32).double()
    out, meta = {}, {}
    sd = LR.backbone_state()
    ref_sd = net32.net.state_dict()                         # slice{n}.{idx}.weight: the same tensors under the reference's names
    assert len(ref_sd) == len(sd) and all(torch.equal(v, sd["features." + k.split(".", 1)[1]]) for k, v in ref_sd.items())
    meta["backbone"] = dict(seed=LR.BACKBONE_SEED, keys=[[k, list(v.shape)] for k, v in sd.items()], checksums=LR.checksums(sd))
    for k in range(5):
        w = getattr(net32, f"lin{k}").model[1].weight
        out[f"lin/{k}"] = f32(w.reshape(-1))
        assert float(w.min()) >= 0
    gen_pairs(out, net32, net64)
    fns = gen_helpers(out)
    gen_projector(out, meta, RL, net32, fns)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(MG.OUT, "lpips.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("lpips.npz", len(out), "arrays,", size, "bytes")
    assert size < 1_000_000, size


if __name__ == "__main__":
    main()
