#!/usr/bin/env python3
"""Project images into the latent space of a trained StyleGAN2 generator (the command line of stylegan2/projector.py).

    python projector.py --ckpt g.pt --size 256 --vgg vgg16.pth --lpips_lin vgg_lin.pth [--w_plus] FILES...

``--vgg`` is a torchvision VGG16 state dict and ``--lpips_lin`` the LPIPS ``weights/v0.1/vgg.pth`` file: neither is shipped.  Writes
``<first file>.pt`` (per input file: ``img``, ``latent``, ``noise``) and ``<file>-project.png`` per input into the working directory.
``--latent`` / ``--n_mlp`` / ``--channel_multiplier`` describe the generator: the reference hard-codes 512 / 8 / 2, which stay the
defaults; a checkpoint of any other generator (the narrow ones the tests train) could not be loaded without them.
"""
import argparse
import os

import numpy as np
import torch
from PIL import Image

from ideas_amd import projector as P
from ideas_amd.lpips import PerceptualLoss
from ideas_amd.stylegan2_gen import Generator


def load_image(path: str, resize: int) -> torch.Tensor:
    """Resize(resize) + CenterCrop(resize) + ToTensor + Normalize(0.5, 0.5) with PIL: the smaller edge to ``resize`` (bilinear), the
    centre square, [0, 255] -> [-1, 1]."""
    img = Image.open(path).convert("RGB")
    w, h = img.size
    if w <= h:
        nw, nh = resize, int(resize * h / w)
    else:
        nw, nh = int(resize * w / h), resize
    if (nw, nh) != (w, h):
        img = img.resize((nw, nh), Image.BILINEAR)
    left, top = int(round((nw - resize) / 2.0)), int(round((nh - resize) / 2.0))
    img = img.crop((left, top, left + resize, top + resize))
    arr = np.asarray(img, dtype=np.float32) / 255.0
    return (torch.from_numpy(arr).permute(2, 0, 1) - 0.5) / 0.5


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--ckpt", type=str, required=True)
    parser.add_argument("--size", type=int, default=256)
    # --lr_rampup / --lr_rampdown are parsed and NOT used, as in the reference: its loop calls get_lr(t, args.lr) with the defaults
    parser.add_argument("--lr_rampup", type=float, default=0.05)
    parser.add_argument("--lr_rampdown", type=float, default=0.25)
    parser.add_argument("--lr", type=float, default=0.1)
    parser.add_argument("--noise", type=float, default=0.05)
    parser.add_argument("--noise_ramp", type=float, default=0.75)
    parser.add_argument("--step", type=int, default=1000)
    parser.add_argument("--noise_regularize", type=float, default=1e5)
    parser.add_argument("--mse", type=float, default=0)
    parser.add_argument("--w_plus", action="store_true")
    parser.add_argument("--vgg", type=str, required=True, help="torchvision VGG16 state dict (.pth)")
    parser.add_argument("--lpips_lin", type=str, required=True, help="LPIPS weights/v0.1/vgg.pth")
    parser.add_argument("--latent", type=int, default=512)
    parser.add_argument("--n_mlp", type=int, default=8)
    parser.add_argument("--channel_multiplier", type=int, default=2)
    parser.add_argument("files", metavar="FILES", nargs="+")
    args = parser.parse_args(argv)

    if not torch.cuda.is_available():
        raise SystemExit("projector.py needs a GPU (ideas_amd has no CPU path)")
    device = "cuda"
    resize = min(args.size, 256)
    imgs = torch.stack([load_image(f, resize) for f in args.files], 0).to(device)

    g_ema = Generator(args.size, args.latent, args.n_mlp, channel_multiplier=args.channel_multiplier)
    g_ema.load_state_dict(torch.load(args.ckpt, map_location="cpu")["g_ema"], strict=False)
    g_ema.eval()
    g_ema = g_ema.to(device)
    percept = PerceptualLoss(model="net-lin", net="vgg", backbone=args.vgg, lin_weights=args.lpips_lin).to(device)

    results, _, losses = P.project(g_ema, imgs, percept, step=args.step, lr=args.lr, noise=args.noise, noise_ramp=args.noise_ramp,
                                   noise_regularize=args.noise_regularize, mse=args.mse, w_plus=args.w_plus)
    if len(losses):
        p_loss, n_loss, mse_loss = (float(v) for v in losses[-1])
        print(f"perceptual: {p_loss:.4f}; noise regularize: {n_loss:.4f}; mse: {mse_loss:.4f}")

    img_ar = P.make_image(torch.stack([r["img"] for r in results], 0))
    result_file = {}
    for i, input_name in enumerate(args.files):
        result_file[input_name] = results[i]
        img_name = os.path.splitext(os.path.basename(input_name))[0] + "-project.png"
        Image.fromarray(img_ar[i]).save(img_name)
    filename = os.path.splitext(os.path.basename(args.files[0]))[0] + ".pt"
    torch.save(result_file, filename)


if __name__ == "__main__":
    main()
