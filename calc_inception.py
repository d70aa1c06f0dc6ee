#!/usr/bin/env python3
"""Inception statistics of a dataset for the Frechet Inception distance (the command line of stylegan2/calc_inception.py).

    python calc_inception.py --size 256 --batch 64 --n_sample 50000 [--flip] --inception_weights pt_inception-2015-12-05-6726825d.pth \\
        [--dataset_type normal|lmdb|multires] PATH

``--inception_weights`` is pytorch-fid's FID Inception state dict: it is not shipped.  ``--dataset_type`` selects the dataset class as
train.py does (``normal``: a folder of image files; ``lmdb``: an LMDB of encoded images; ``multires``: the multi-resolution LMDB of
stylegan2/prepare_data.py, which the reference's calc_inception.py reads).  Writes ``inception_<name>.pkl`` into the
working directory with the reference's keys: ``mean`` [2048], ``cov`` [2048, 2048] (divisor n - 1), ``size`` and ``path``.  The
features of the first ``--n_sample`` images are reduced to their moments on the device, batch by batch, in f64.
"""
import argparse
import os
import pickle

import torch

from ideas_amd import data
from ideas_amd.fid import feature_statistics
from ideas_amd.inception import InceptionV3


def main(argv=None):
    parser = argparse.ArgumentParser(description="Calculate Inception v3 features for datasets")
    parser.add_argument("--size", type=int, default=256)
    parser.add_argument("--batch", default=64, type=int, help="batch size")
    parser.add_argument("--n_sample", type=int, default=50000)
    parser.add_argument("--flip", action="store_true")
    parser.add_argument("--inception_weights", type=str, required=True, help="pt_inception-2015-12-05-6726825d.pth (pytorch-fid)")
    parser.add_argument("--dataset_type", type=str, default="normal", choices=("normal", "lmdb", "multires"))
    parser.add_argument("--num_workers", type=int, default=4)
    parser.add_argument("path", metavar="PATH", help="path to the dataset (folder or lmdb)")
    args = parser.parse_args(argv)

    if not torch.cuda.is_available():
        raise SystemExit("calc_inception.py needs a GPU (ideas_amd has no CPU path)")
    device = "cuda"
    inception = InceptionV3([3], normalize_input=False, weights=args.inception_weights).to(device)
    dset = data.set_dataset(args.dataset_type, args.path, args.size)
    if len(dset) == 0:
        raise SystemExit(f"calc_inception.py: no images found in {args.path}")
    loader = data.DeviceLoader(dset, args.batch, device=device, num_workers=args.num_workers, flip=args.flip)
    stats = feature_statistics(loader, inception, n_sample=args.n_sample)
    print(f"extracted {stats.n} features")

    name = os.path.splitext(os.path.basename(os.path.normpath(args.path)))[0]
    with open(f"inception_{name}.pkl", "wb") as f:
        pickle.dump({"mean": stats.mean(), "cov": stats.cov(), "size": args.size, "path": args.path}, f)


if __name__ == "__main__":
    main()
