#!/usr/bin/env python3
"""Extraction accuracy (and FID) of a trained IDEAS checkpoint per jitter width: random bits -> containers -> 8-bit images -> bits.

    python evaluate.py [--sigma 1] [--delta 0 0.25 0.5] [--n_sample 50000] [--batch 32] [--container u8] [--seed 0]
        [--attack SPEC [SPEC ...]] [--ecc RATE] [--inception inception_<name>.pkl --inception_weights pt_inception-2015-12-05-6726825d.pth] CHECKPOINT

Prints one line per delta, ``sigma=1 delta=25% ACC: 0.9999 FID: 15.56``.  The FID is printed only when both inception arguments are
given: ``--inception`` is the pickle calc_inception.py wrote for the dataset, ``--inception_weights`` pytorch-fid's FID Inception state
dict (not shipped); it is computed as fid.py does, on the containers the receiver sees.  ``--container float`` skips the 8-bit file.

``--attack`` sends the 8-bit containers through a channel before the receiver sees them (``ideas_amd.attacks``): ``none``, ``jpeg:Q``
(quality 1..100; an f32 model at 4:4:4), ``jpegfile:Q`` (the JPEG file libjpeg / Pillow writes at quality Q, 4:2:0, exact to the byte;
``jpegfile:Q:444`` without chroma subsampling), ``noise:S`` (Gaussian, S in 8-bit levels), ``sp:P`` (salt and pepper, fraction P), ``gain:G``, ``offset:D``,
``scale:F`` (Pillow's bilinear resize to F times the size and back, 0.25..4), ``gblur:S`` (Gaussian filter, sigma S pixels, up to 4),
``median:K`` (K x K median, K = 3 or 5), or a chain such as ``noise:3+jpeg:75`` or ``scale:0.5+jpeg:75``.  One line per attack and
delta, ``sigma=1 delta=25% attack=jpeg:75 ACC: 0.9871``; the generator is re-seeded for every line, so every attack sees the same
messages and textures.

``--ecc RATE`` (1/2, 2/3 or 3/4) makes every container carry one codeword of ``ideas_amd.ecc``: ACC then counts the channel's errors
on the coded bits, and each line ends in `` ECC=1/2 INFO_ACC: 0.9999 FER: 0.0003``, the accuracy of the decoded information bits and
the fraction of images with any wrong one.
"""
import argparse
import pickle

import torch


def main(argv=None):
    parser = argparse.ArgumentParser(description="extraction accuracy / FID of a trained IDEAS checkpoint")
    parser.add_argument("--sigma", type=int, default=1, help="bits per element of the secret tensor (1..8)")
    parser.add_argument("--delta", type=float, nargs="+", default=[0.0, 0.25, 0.5], help="jitter half-widths as fractions of a bin")
    parser.add_argument("--n_sample", type=int, default=50000)
    parser.add_argument("--batch", type=int, default=32)
    parser.add_argument("--container", choices=("u8", "float"), default="u8")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--attack", type=str, nargs="+", default=None, metavar="SPEC",
                        help="channel attacks on the 8-bit container: none, jpeg:Q, jpegfile:Q[:444], noise:S, sp:P, gain:G, offset:D, scale:F, gblur:S, "
                             "median:K, chained with +")
    parser.add_argument("--ecc", type=str, default=None, metavar="RATE", help="forward error correction of rate 1/2, 2/3 or 3/4")
    parser.add_argument("--inception", type=str, default=None, help="dataset statistics written by calc_inception.py")
    parser.add_argument("--inception_weights", type=str, default=None, help="pt_inception-2015-12-05-6726825d.pth (pytorch-fid)")
    parser.add_argument("ckpt", metavar="CHECKPOINT", nargs="?")
    opt = parser.parse_args(argv)
    if opt.ckpt is None and opt.attack and len(opt.attack) > 1:
        opt.ckpt = opt.attack.pop()                           # "--attack none jpeg:75 CHECKPOINT": the list took the positional
    if opt.ckpt is None:
        parser.error("the following arguments are required: CHECKPOINT")
    if (opt.inception is None) != (opt.inception_weights is None):
        parser.error("--inception and --inception_weights go together")
    from ideas_amd import attacks as attacks_mod
    try:
        attacks = [None] if opt.attack is None else [attacks_mod.parse(a) for a in opt.attack]
    except ValueError as e:
        parser.error(str(e))
    if opt.attack is not None and opt.container != "u8":
        parser.error("--attack acts on the 8-bit container: it needs --container u8")
    from ideas_amd import ecc
    if opt.ecc is not None and opt.ecc not in ecc.RATES:
        parser.error(f"--ecc: unknown rate {opt.ecc!r} (known: {', '.join(ecc.RATES)})")

    if not torch.cuda.is_available():
        raise SystemExit("evaluate.py needs a GPU (ideas_amd has no CPU path)")
    from ideas_amd import stego
    from ideas_amd.fid import calc_fid

    device = torch.device("cuda")
    models, args = stego.load_models(opt.ckpt, device)
    cap = stego.capacity_bits(args, opt.sigma)
    if cap % 8:
        raise SystemExit(f"evaluate.py: the capacity of an image ({cap} bits) is not a whole number of bytes (needs image_size >= 64)")
    code = None
    if opt.ecc is not None:
        try:
            code = ecc.Code(cap, opt.ecc)
        except ValueError as e:
            raise SystemExit(f"evaluate.py: {e}")
    inception, embeds = None, None
    if opt.inception is not None:
        from ideas_amd.inception import InceptionV3
        inception = InceptionV3([3], normalize_input=False, weights=opt.inception_weights).to(device)
        with open(opt.inception, "rb") as f:
            embeds = pickle.load(f)
    for attack in attacks:
        for delta in opt.delta:
            gen = torch.Generator(device=device).manual_seed(opt.seed)
            res = stego.evaluate(models, args, opt.sigma, delta, opt.n_sample, opt.batch, gen, container=opt.container,
                                 inception=inception, attack=attack, code=code)
            line = f"sigma={opt.sigma} delta={delta * 100:g}%" + ("" if attack is None else f" attack={attack.name}")
            line += f" ACC: {res['acc']:.4f}"
            if inception is not None:
                stats = res["stats"]
                line += f" FID: {calc_fid(stats.mean(), stats.cov(), embeds['mean'], embeds['cov']):.2f}"
            if code is not None:
                line += f" ECC={code.rate} INFO_ACC: {res['info_acc']:.4f} FER: {res['n_row_err'] / opt.n_sample:.4f}"
            print(line)


if __name__ == "__main__":
    main()
