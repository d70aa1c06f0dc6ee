"""Latent projection (stylegan2/projector.py): invert images into the W (or W+) space and the noise maps of a trained generator by
optimising the LPIPS distance, the noise regulariser and, optionally, a pixel MSE.

``project`` is the loop of stylegan2/projector.py:131-192 as a function; the helpers keep the reference's names.  The generator, the
perceptual network and the noise gradient (``op.noise_bias_act``'s ``gnoise``) run on the HIP ops; ``noise_regularize`` is a torch
composition over the (small) noise maps -- a fused pyramid kernel is a follow-up.
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional, Sequence

import torch
from torch import optim
from torch.nn import functional as F


def _shift_correlation(x: torch.Tensor, dim: int) -> torch.Tensor:
    """Squared mean of the product of ``x`` with itself rolled by one pixel (circularly) along ``dim``."""
    return (x * torch.roll(x, 1, dim)).mean() ** 2


def noise_regularize(noises: Sequence[torch.Tensor]):
    """The noise regulariser of the StyleGAN2 projection: over every noise map [N, 1, s, s] and its pyramid of 2x2 block means
    down to 8x8, the squared mean autocorrelation at one pixel of horizontal and of vertical shift.  White noise scores zero."""
    total = 0
    for level in noises:
        side = level.shape[2]
        total = total + _shift_correlation(level, 3) + _shift_correlation(level, 2)
        while side > 8:
            level = F.avg_pool2d(level, 2)
            side //= 2
            total = total + _shift_correlation(level, 3) + _shift_correlation(level, 2)
    return total


def noise_normalize_(noises: Sequence[torch.Tensor]) -> None:
    """In place, outside autograd: each noise tensor to zero mean and unit (unbiased) standard deviation over all its elements."""
    with torch.no_grad():
        for nz in noises:
            centre, spread = nz.mean(), nz.std()
            nz.sub_(centre).div_(spread)


def get_lr(t: float, initial_lr: float, rampdown: float = 0.25, rampup: float = 0.05) -> float:
    """Learning rate at the fraction ``t`` of the run: a linear warm-up over the first ``rampup`` times a cosine decay over the last
    ``rampdown``."""
    decay_phase = min(1, (1 - t) / rampdown)
    cosine = 0.5 - 0.5 * math.cos(decay_phase * math.pi)
    warmup = min(1, t / rampup)
    return initial_lr * (cosine * warmup)


def latent_noise(latent: torch.Tensor, strength: float) -> torch.Tensor:
    """``latent`` plus normal noise of standard deviation ``strength`` (a draw is made even at strength 0)."""
    return latent + strength * torch.randn_like(latent)


def make_image(tensor: torch.Tensor):
    """[B, 3, H, W] in [-1, 1] -> uint8 [B, H, W, 3] on the host.  The clamp is applied IN PLACE to ``tensor``'s storage, which is
    what the reference's command line relies on for the ``img`` it saves."""
    x = tensor.detach()
    x.clamp_(-1.0, 1.0)
    u8 = ((x + 1) / 2 * 255).to(torch.uint8)
    return u8.permute(0, 2, 3, 1).cpu().numpy()


def latent_statistics(g_ema, n_mean_latent: int = 10000):
    """Mean [D] and scalar standard deviation of ``g_ema.style`` over ``n_mean_latent`` normal draws (projector.py:120-125)."""
    device = g_ema.input.input.device
    with torch.no_grad():
        noise_sample = torch.randn(n_mean_latent, g_ema.style_dim, device=device)
        latent_out = g_ema.style(noise_sample)
        latent_mean = latent_out.mean(0)
        latent_std = ((latent_out - latent_mean).pow(2).sum() / n_mean_latent) ** 0.5
    return latent_mean, latent_std


_noise_regularize = noise_regularize     # (``project`` takes the reference's flag name ``noise_regularize`` for the weight)


def project(g_ema, imgs: torch.Tensor, percept, *, step: int = 1000, lr: float = 0.1, noise: float = 0.05, noise_ramp: float = 0.75,
            noise_regularize: float = 1e5, mse: float = 0.0, w_plus: bool = False, latent_mean: Optional[torch.Tensor] = None,
            latent_std=None, noises: Optional[Sequence[torch.Tensor]] = None, n_mean_latent: int = 10000,
            after_backward: Optional[Callable] = None):
    """Project ``imgs`` ([N, 3, H, W] in [-1, 1], on the generator's device) into ``g_ema``.

    ``latent_mean`` ([D]), ``latent_std`` (scalar) and ``noises`` (one [N, 1, h, w] tensor per layer) replace the random draws of
    stylegan2/projector.py:120-134 when given -- with ``noise=0`` the run is then deterministic.  ``after_backward(i, latent_in,
    noises)`` is called after each step's ``backward()``, before the optimiser moves anything.

    Returns ``(results, latent_path, losses)``: per image ``{"img", "latent", "noise"}`` as the reference stores them; the latents
    kept every 100 steps (and after the last step); a float64 [step, 3] tensor of (perceptual, noise regulariser, mse) per step."""
    n = imgs.shape[0]
    if latent_mean is None or latent_std is None:
        drawn_mean, drawn_std = latent_statistics(g_ema, n_mean_latent)
        latent_mean = drawn_mean if latent_mean is None else latent_mean
        latent_std = drawn_std if latent_std is None else latent_std
    latent_std = float(latent_std)
    if noises is None:
        noises = [nz.repeat(n, 1, 1, 1).normal_() for nz in g_ema.make_noise()]
    else:
        noises = [nz.detach().clone() for nz in noises]
    latent_in = latent_mean.detach().clone().unsqueeze(0).repeat(n, 1)
    if w_plus:
        latent_in = latent_in.unsqueeze(1).repeat(1, g_ema.n_latent, 1)
    latent_in.requires_grad = True
    for nz in noises:
        nz.requires_grad = True
    optimizer = optim.Adam([latent_in] + list(noises), lr=lr)
    latent_path: List[torch.Tensor] = []
    losses = []
    for i in range(step):
        t = i / step
        optimizer.param_groups[0]["lr"] = get_lr(t, lr)
        noise_strength = latent_std * noise * max(0, 1 - t / noise_ramp) ** 2
        latent_n = latent_noise(latent_in, noise_strength)
        img_gen, _ = g_ema([latent_n], input_is_latent=True, noise=noises)
        batch, channel, height, width = img_gen.shape
        if height > 256:
            factor = height // 256
            img_gen = img_gen.reshape(batch, channel, height // factor, factor, width // factor, factor).mean([3, 5])
        p_loss = percept(img_gen, imgs).sum()
        n_loss = _noise_regularize(noises)
        mse_loss = F.mse_loss(img_gen, imgs)
        loss = p_loss + noise_regularize * n_loss + mse * mse_loss
        optimizer.zero_grad()
        loss.backward()
        if after_backward is not None:
            after_backward(i, latent_in, noises)
        optimizer.step()
        noise_normalize_(noises)
        if (i + 1) % 100 == 0 or i + 1 == step:
            latent_path.append(latent_in.detach().clone())
        losses.append(torch.stack([p_loss.detach().double(), n_loss.detach().double(), mse_loss.detach().double()]))
    final = latent_path[-1] if latent_path else latent_in.detach()
    with torch.no_grad():
        img_gen, _ = g_ema([final], input_is_latent=True, noise=noises)
    results = [{"img": img_gen[k], "latent": latent_in[k], "noise": [nz[k:k + 1] for nz in noises]} for k in range(n)]
    loss_table = torch.stack(losses).cpu() if losses else torch.zeros(0, 3, dtype=torch.float64)
    return results, latent_path, loss_table
