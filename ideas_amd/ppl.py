"""Perceptual path length (stylegan2/ppl.py) of a trained ``Generator`` on the HIP ops.

Per batch the reference draws 2B latents and B positions t, interpolates each pair at t and t + eps, generates the 2B images, crops /
resizes them, and takes LPIPS between the two images of every pair, divided by eps^2.  Around the two big pieces (the generator, the
VGG) it issues four strided slices, two lerps and a stack, two more slices of the image batch, an ``F.interpolate``, the scaling layer
twice, two layout conversions and two half-batch VGG passes.  Here those are ``op.path_endpoints`` and ``op.pair_prepare`` (one launch
each) and ONE VGG pass over the 2B images (``PerceptualLoss.pair_distance``).  DESIGN.md 3.16.

``normalize`` / ``slerp`` / ``lerp`` are the reference's torch forms.  ``slerp`` has no clamp: identical ends give NaN, there and here.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import op
from .op.ppl import lerp, normalize, slerp          # noqa: F401  (the reference's names, ppl.py:12-28)


# The conv kernels address a tensor with 32-bit byte offsets (4 GiB a launch), and the upsampling layers hold intermediates a little
# larger than their output: the generator gets at most this many bytes of its largest activation at a time.  The reference's
# defaults (size 256, batch 64: 128 images of 128 channels) are 4 GiB exactly.
LAUNCH_BYTES = 1 << 31


def generate_images(g, latent_e: torch.Tensor, noise) -> torch.Tensor:
    """``g([latent_e], input_is_latent=True, noise=noise)[0]``, over as few equal slices of the batch as keep the largest activation of
    the synthesis network within ``LAUNCH_BYTES`` (one slice for all but the largest batches); the samples are independent."""
    n = latent_e.shape[0]
    per_image = 4 * max(c * r * r for r, c in g.channels.items() if r <= g.size)
    slices = -(-n * per_image // LAUNCH_BYTES)
    if slices <= 1:
        return g([latent_e], input_is_latent=True, noise=noise)[0]
    step = -(-n // slices)
    images = []
    for i in range(0, n, step):
        nz = noise if noise is None else [m if m is None or m.shape[0] == 1 else m[i:i + step] for m in noise]
        images.append(g([latent_e[i:i + step]], input_is_latent=True, noise=nz)[0])
    return torch.cat(images, 0)


def _scaling_constants(percept):
    """The three shifts and scales of ``percept.scaling_layer`` as Python floats, read from the device once per module."""
    consts = getattr(percept, "_pair_constants", None)
    if consts is None:
        layer = percept.scaling_layer
        consts = (layer.shift.flatten().tolist(), layer.scale.flatten().tolist())
        percept._pair_constants = consts
    return consts


def path_distances(g, percept, inputs: torch.Tensor, lerp_t: torch.Tensor, noise: Optional[Sequence[torch.Tensor]], space: str = "w",
                   eps: float = 1e-4, crop: bool = False, resize_to: int = 256) -> torch.Tensor:
    """The body of the reference's loop (ppl.py:71-93) for one batch: ``inputs`` [2B, D] are z draws, ``lerp_t`` [B] the positions,
    ``noise`` the list ``g.make_noise()`` returns (``generate_images`` runs the generator).  -> [B] float32, the LPIPS distance of every pair divided by ``eps ** 2``.

    ``space="w"``: ``g.get_latent(inputs)``, then lerp between rows 2i and 2i + 1 at t_i and t_i + eps (the sum in f32).
    ``space="z"``: slerp on ``inputs``, then ``g.get_latent``.  The reference defines ``slerp`` but its loop never assigns ``latent_e``
    for ``--space z`` and stops with a NameError; this is the z-space path length of the StyleGAN paper built on the reference's own
    ``slerp``.
    ``crop``: rows 3c:7c, columns 2c:6c with c = H // 8.  The images are resized to ``resize_to`` when ``cropped height // resize_to >
    1`` (the reference computes the factor after the crop, so a 512-pixel crop of a 1024 image is resized and a 256 one is not)."""
    if space not in ("w", "z"):
        raise RuntimeError(f"path_distances: space is 'w' or 'z', got {space!r}")
    with torch.no_grad():
        if space == "w":
            latent_e = op.path_endpoints(g.get_latent(inputs), lerp_t, eps, "lerp")
        else:
            latent_e = g.get_latent(op.path_endpoints(inputs, lerp_t, eps, "slerp"))
        image = generate_images(g, latent_e, noise)
        h, w = image.shape[2], image.shape[3]
        box = (0, 0, h, w)
        if crop:
            c = h // 8
            box = (3 * c, 2 * c, 4 * c, 4 * c)
        out_hw = (resize_to, resize_to) if box[2] // resize_to > 1 else (box[2], box[3])
        shift, scale = _scaling_constants(percept)
        dist = percept.pair_distance(op.pair_prepare(image, box, out_hw, shift, scale))
        return dist / (eps ** 2)


def filtered_mean(distances) -> float:
    """The mean of the distances between their 1st percentile (``'lower'``) and their 99th (``'higher'``), both ends included
    (ppl.py:98-104)."""
    d = np.asarray(distances)
    try:
        lo, hi = np.percentile(d, 1, method="lower"), np.percentile(d, 99, method="higher")
    except TypeError:                                    # numpy before 1.22 spells it interpolation=
        lo, hi = np.percentile(d, 1, interpolation="lower"), np.percentile(d, 99, interpolation="higher")
    return float(np.extract(np.logical_and(lo <= d, d <= hi), d).mean())


def batch_sizes(n_sample: int, batch: int) -> List[int]:
    """``[batch] * n + [resid]`` as the reference splits (ppl.py:60-62): the last entry is 0 when ``batch`` divides ``n_sample``."""
    n_batch = n_sample // batch
    return [batch] * n_batch + [n_sample - n_batch * batch]


def compute_ppl(g, percept, n_sample: int, batch: int, space: str = "w", eps: float = 1e-4, crop: bool = False,
                seed: Optional[int] = None, resize_to: int = 256) -> float:
    """Perceptual path length over ``n_sample`` paths in batches of ``batch``.  Per batch the random draws come in the reference's
    order: ``g.make_noise()``, ``randn([2 * batch, D])``, ``rand(batch)``.  A zero-sized last batch (``batch`` divides ``n_sample``)
    is skipped: the reference runs the generator on an empty batch there, which adds no distance.  ``seed``: ``torch.manual_seed``
    before the first draw."""
    if seed is not None:
        torch.manual_seed(seed)
    device = g.input.input.device
    distances = []
    for b in batch_sizes(n_sample, batch):
        if b == 0:
            continue
        noise = g.make_noise()
        inputs = torch.randn([b * 2, g.style_dim], device=device)
        lerp_t = torch.rand(b, device=device)
        distances.append(path_distances(g, percept, inputs, lerp_t, noise, space=space, eps=eps, crop=crop, resize_to=resize_to)
                         .cpu().numpy())
    return filtered_mean(np.concatenate(distances, 0))
