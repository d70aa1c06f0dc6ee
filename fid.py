#!/usr/bin/env python3
"""Frechet Inception distance of a trained StyleGAN2 generator against dataset statistics (the command line of stylegan2/fid.py).

    python fid.py --inception inception_<name>.pkl --inception_weights pt_inception-2015-12-05-6726825d.pth [--truncation 1]
        [--truncation_mean 4096] [--batch 64] [--n_sample 50000] [--size 256] CHECKPOINT

``--inception`` is the pickle calc_inception.py wrote; ``--inception_weights`` pytorch-fid's FID Inception state dict (not shipped).
``--latent`` / ``--n_mlp`` / ``--channel_multiplier`` describe the generator: the reference hard-codes 512 / 8 / 2, which stay the
defaults.  Prints ``fid: <value>``.
"""
import argparse
import pickle

import torch

from ideas_amd.fid import calc_fid, sample_statistics
from ideas_amd.inception import InceptionV3
from ideas_amd.stylegan2_gen import Generator


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--truncation", type=float, default=1)
    parser.add_argument("--truncation_mean", type=int, default=4096)
    parser.add_argument("--batch", type=int, default=64)
    parser.add_argument("--n_sample", type=int, default=50000)
    parser.add_argument("--size", type=int, default=256)
    parser.add_argument("--inception", type=str, default=None, required=True)
    parser.add_argument("--inception_weights", type=str, required=True, help="pt_inception-2015-12-05-6726825d.pth (pytorch-fid)")
    parser.add_argument("--latent", type=int, default=512)
    parser.add_argument("--n_mlp", type=int, default=8)
    parser.add_argument("--channel_multiplier", type=int, default=2)
    parser.add_argument("ckpt", metavar="CHECKPOINT")
    args = parser.parse_args(argv)

    if not torch.cuda.is_available():
        raise SystemExit("fid.py needs a GPU (ideas_amd has no CPU path)")
    device = "cuda"
    g = Generator(args.size, args.latent, args.n_mlp, channel_multiplier=args.channel_multiplier)
    g.load_state_dict(torch.load(args.ckpt, map_location="cpu")["g_ema"])
    g = g.to(device).eval()
    mean_latent = None
    if args.truncation < 1:
        with torch.no_grad():
            mean_latent = g.mean_latent(args.truncation_mean)
    inception = InceptionV3([3], normalize_input=False, weights=args.inception_weights).to(device)

    stats = sample_statistics(g, inception, args.truncation, mean_latent, args.batch, args.n_sample, device)
    print(f"extracted {stats.n} features")
    with open(args.inception, "rb") as f:
        embeds = pickle.load(f)
    fid = calc_fid(stats.mean(), stats.cov(), embeds["mean"], embeds["cov"])
    print("fid:", fid)


if __name__ == "__main__":
    main()
