#!/usr/bin/env python3
"""Perceptual path length of a trained StyleGAN2 generator (the command line of stylegan2/ppl.py).

    python ppl.py --space w --size 256 --vgg vgg16.pth --lpips_lin vgg_lin.pth [--crop] CHECKPOINT

``--vgg`` is a torchvision VGG16 state dict and ``--lpips_lin`` the LPIPS ``weights/v0.1/vgg.pth`` file: neither is shipped.  Prints
``ppl: <value>``.  ``--latent`` / ``--n_mlp`` / ``--channel_multiplier`` describe the generator (the reference hard-codes 512 / 8 / 2,
which stay the defaults); ``--seed`` seeds the draws.  ``--space z`` runs the z-space path length on the reference's ``slerp``, which
the reference's own loop stops short of (ideas_amd/ppl.py).
"""
import argparse

import torch

from ideas_amd import ppl as P
from ideas_amd.lpips import PerceptualLoss
from ideas_amd.stylegan2_gen import Generator


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--space", choices=["z", "w"], required=True)
    parser.add_argument("--batch", type=int, default=64)
    parser.add_argument("--n_sample", type=int, default=5000)
    parser.add_argument("--size", type=int, default=256)
    parser.add_argument("--eps", type=float, default=1e-4)
    parser.add_argument("--crop", action="store_true")
    parser.add_argument("--vgg", type=str, required=True, help="torchvision VGG16 state dict (.pth)")
    parser.add_argument("--lpips_lin", type=str, required=True, help="LPIPS weights/v0.1/vgg.pth")
    parser.add_argument("--latent", type=int, default=512)
    parser.add_argument("--n_mlp", type=int, default=8)
    parser.add_argument("--channel_multiplier", type=int, default=2)
    parser.add_argument("--seed", type=int, default=None)
    parser.add_argument("ckpt", metavar="CHECKPOINT")
    args = parser.parse_args(argv)

    if not torch.cuda.is_available():
        raise SystemExit("ppl.py needs a GPU (ideas_amd has no CPU path)")
    device = "cuda"
    g = Generator(args.size, args.latent, args.n_mlp, channel_multiplier=args.channel_multiplier)
    g.load_state_dict(torch.load(args.ckpt, map_location="cpu")["g_ema"], strict=True)
    g.eval()
    g = g.to(device)
    percept = PerceptualLoss(model="net-lin", net="vgg", backbone=args.vgg, lin_weights=args.lpips_lin).to(device)
    print("ppl:", P.compute_ppl(g, percept, args.n_sample, args.batch, args.space, args.eps, args.crop, seed=args.seed))


if __name__ == "__main__":
    main()
