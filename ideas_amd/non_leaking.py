"""Adaptive discriminator augmentation (ADA): host-side mirror of stylegan2/non_leaking.py on the kernels of ``ideas_amd.op``.

Same names, same signatures and the same order of random draws as the reference: after ``torch.manual_seed(s)`` a call of
``sample_affine`` / ``sample_color`` / ``augment`` draws the reference's matrices.  The matrices are sampled on the CPU in f32, as
there; the image work runs on the device:

* ``random_apply_affine`` keeps the reference's structure (non_leaking.py:316-371) -- reflect pad, ``op.upfirdn2d(up=2)`` with the
  flipped outer product of the 12-tap ``SYM6`` filter, warp, ``op.upfirdn2d(down=2)``, crop.  The reference's make-grid / matmul /
  rescale / ``F.grid_sample`` steps (three full-size ``[N, h, w, 2..3]`` tensors) are ``warp_theta`` -- six floats a sample, composed
  on the host in float64 -- and ONE ``op.affine_warp`` launch; the grid tensor is never built.
* ``apply_color`` is one ``op.color_affine`` launch in place of permute, batched matmul, add and permute.

Gradients flow through both to the image (the fake images are augmented on the way from G to D); the matrices carry none.

One deliberate difference: when ``G`` is passed in and no reflect padding exists for it (a pad >= the image size), the reference's
``while True`` never ends (non_leaking.py:293-311); ``try_sample_affine_and_pad`` raises ``RuntimeError`` instead.  With ``G=None`` it
re-draws, as the reference does.

``AdaptiveAugment`` restates the adaptation of ``p`` of stylegan2/train.py:151-153, 194-213.
"""
from __future__ import annotations

import math
from typing import Callable, Optional, Sequence, Tuple

import torch
from torch.nn import functional as F

from . import op

SYM6 = (
    0.015404109327027373,
    0.0034907120842174702,
    -0.11799011114819057,
    -0.048311742585633,
    0.4910559419267466,
    0.787641141030194,
    0.3379294217276218,
    -0.07263752278646252,
    -0.021060292512300564,
    0.04472490177066578,
    0.0017677118642428036,
    -0.007800708325034148,
)


# ---- matrix builders: [batch, 3, 3] (image plane) and [batch, 4, 4] (colour space), f32 on the CPU ------------------------------------
def _eyes(n: int, batch: int) -> torch.Tensor:
    return torch.eye(n).unsqueeze(0).repeat(batch, 1, 1)


def translate_mat(t_x, t_y):
    mat = _eyes(3, t_x.shape[0])
    mat[:, :2, 2] = torch.stack((t_x, t_y), 1)
    return mat


def rotate_mat(theta):
    mat = _eyes(3, theta.shape[0])
    s, c = torch.sin(theta), torch.cos(theta)
    mat[:, :2, :2] = torch.stack((c, -s, s, c), 1).view(-1, 2, 2)
    return mat


def scale_mat(s_x, s_y):
    mat = _eyes(3, s_x.shape[0])
    mat[:, 0, 0] = s_x
    mat[:, 1, 1] = s_y
    return mat


def translate3d_mat(t_x, t_y, t_z):
    mat = _eyes(4, t_x.shape[0])
    mat[:, :3, 3] = torch.stack((t_x, t_y, t_z), 1)
    return mat


def rotate3d_mat(axis, theta):
    """Rodrigues' rotation about the unit ``axis`` by ``theta`` ([batch]) in the upper-left 3x3 of a 4x4."""
    u_x, u_y, u_z = axis
    cross = torch.tensor([(0, -u_z, u_y), (u_z, 0, -u_x), (-u_y, u_x, 0)]).unsqueeze(0)
    u = torch.tensor(axis)
    outer = (u.unsqueeze(1) * u).unsqueeze(0)
    s, c = torch.sin(theta).view(-1, 1, 1), torch.cos(theta).view(-1, 1, 1)
    mat = _eyes(4, theta.shape[0])
    mat[:, :3, :3] = c * torch.eye(3).unsqueeze(0) + s * cross + (1 - c) * outer
    return mat


def scale3d_mat(s_x, s_y, s_z):
    mat = _eyes(4, s_x.shape[0])
    mat[:, 0, 0] = s_x
    mat[:, 1, 1] = s_y
    mat[:, 2, 2] = s_z
    return mat


def luma_flip_mat(axis, i):
    """Householder reflection along ``axis`` for the samples with ``i == 1``."""
    v = torch.tensor(axis + (0,))
    return _eyes(4, i.shape[0]) - 2 * torch.ger(v, v) * i.view(-1, 1, 1)


def saturation_mat(axis, i):
    """Scale by ``i`` in the plane orthogonal to ``axis``."""
    v = torch.tensor(axis + (0,))
    proj = torch.ger(v, v)
    return proj + (_eyes(4, i.shape[0]) - proj) * i.view(-1, 1, 1)


# ---- samplers (each is ONE call into torch's global CPU generator, the reference's) --------------------------------------------------
def lognormal_sample(size, mean=0, std=1):
    return torch.empty(size).log_normal_(mean=mean, std=std)


def category_sample(size, categories):
    values = torch.tensor(categories)
    return values[torch.randint(high=len(categories), size=(size,))]


def uniform_sample(size, low, high):
    return torch.empty(size).uniform_(low, high)


def normal_sample(size, mean=0, std=1):
    return torch.empty(size).normal_(mean, std)


def bernoulli_sample(size, p):
    return torch.empty(size).bernoulli_(p)


def random_mat_apply(p, transform, prev, eye):
    """``transform @ prev`` for the samples a Bernoulli(p) draw selects, ``prev`` for the others."""
    size = transform.shape[0]
    select = bernoulli_sample(size, p).view(size, 1, 1)
    return (select * transform + (1 - select) * eye) @ prev


def sample_affine(p, size, height, width):
    """[size, 3, 3] geometric transforms in normalised coordinates: x-flip, 90-degree rotation, integer translation, isotropic scale,
    rotation, anisotropic scale, rotation, fractional translation -- each applied with probability ``p`` (the two free rotations with
    ``1 - sqrt(1 - p)`` each).  Draw order per step: the parameter, then the Bernoulli selection."""
    eye = _eyes(3, size)
    G = eye
    p_rot = 1 - math.sqrt(1 - p)
    log2 = math.log(2)

    def flip():
        return scale_mat(1 - 2.0 * category_sample(size, (0, 1)), torch.ones(size))

    def rot90():
        return rotate_mat(-math.pi / 2 * category_sample(size, (0, 3)))

    def int_translate():
        t = uniform_sample(size, -0.125, 0.125)
        t_y = torch.round(t * height) / height
        t_x = torch.round(t * width) / width
        return translate_mat(t_x, t_y)

    def iso_scale():
        s = lognormal_sample(size, std=0.2 * log2)
        return scale_mat(s, s)

    def rotate():
        return rotate_mat(-uniform_sample(size, -math.pi, math.pi))

    def aniso_scale():
        s = lognormal_sample(size, std=0.2 * log2)
        return scale_mat(s, 1 / s)

    def frac_translate():
        t = normal_sample(size, std=0.125)
        return translate_mat(t, t)

    for prob, draw in ((p, flip), (p, rot90), (p, int_translate), (p, iso_scale), (p_rot, rotate), (p, aniso_scale), (p_rot, rotate),
                       (p, frac_translate)):
        G = random_mat_apply(prob, draw(), G, eye)
    return G


def sample_color(p, size):
    """[size, 4, 4] colour transforms: brightness, contrast, luma flip, hue rotation, saturation, each with probability ``p``."""
    eye = _eyes(4, size)
    C = eye
    axis = (1 / math.sqrt(3),) * 3
    log2 = math.log(2)

    def brightness():
        b = normal_sample(size, std=0.2)
        return translate3d_mat(b, b, b)

    def contrast():
        c = lognormal_sample(size, std=0.5 * log2)
        return scale3d_mat(c, c, c)

    def luma_flip():
        return luma_flip_mat(axis, category_sample(size, (0, 1)))

    def hue():
        return rotate3d_mat(axis, uniform_sample(size, -math.pi, math.pi))

    def saturation():
        return saturation_mat(axis, lognormal_sample(size, std=1 * log2))

    for draw in (brightness, contrast, luma_flip, hue, saturation):
        C = random_mat_apply(p, draw(), C, eye)
    return C


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def get_padding(G, height, width):
    """Pixels of padding ``(x_low, x_high, y_low, y_high)`` that the images of the corners of [-1, 1]^2 under ``G`` ([B, 3, 3], the
    INVERSE of the sampled transform) need, the maximum over the batch."""
    corners = torch.tensor([(-1.0, -1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, 1)]).t()
    extreme = G[:, :2, :] @ corners
    size = torch.tensor((width, height))
    low = ((extreme.min(-1).values + 1) * size).clamp(max=0).abs().ceil().max(0).values.to(torch.int64).tolist()
    high = (extreme.max(-1).values * size - size).clamp(min=0).ceil().max(0).values.to(torch.int64).tolist()
    return low[0], high[0], low[1], high[1]


def try_sample_affine_and_pad(img, p, pad_k, G=None):
    """Reflect-pad ``img`` for the transform ``G`` (drawn here with probability ``p`` when ``None``) plus ``pad_k`` pixels of filter
    margin -> ``(img_pad, G, (pad_x1, pad_x2, pad_y1, pad_y2))``.  A reflect pad exists only below the image size: a drawn ``G`` that
    needs more is drawn again (as in the reference); a GIVEN one raises ``RuntimeError`` (the reference would spin forever)."""
    batch, _, height, width = img.shape
    while True:
        G_try = sample_affine(p, batch, height, width) if G is None else G
        pads = get_padding(torch.inverse(G_try), height, width)
        full = tuple(q + pad_k for q in pads)
        if max(full[0], full[1]) < width and max(full[2], full[3]) < height:
            return F.pad(img, full, mode="reflect"), G_try, pads
        if G is not None:
            raise RuntimeError(f"non_leaking: the given G needs a reflect padding of {full} (x_low, x_high, y_low, y_high) pixels, which "
                               f"a {height}x{width} image does not have")


def warp_theta(G, in_hw: Tuple[int, int], pads: Sequence[int], len_k: int, dtype=torch.float32) -> torch.Tensor:
    """``[B, 6]`` on the CPU (f32: what the kernel takes; ``dtype=torch.float64`` keeps the unrounded composition): the source position in pixels of the 2x-upsampled padded image, affine in the output pixel index, that
    the reference reaches through ``make_grid`` / ``affine_grid`` / rescale / ``F.grid_sample`` (non_leaking.py:340-357).

    Composed in float64 and rounded once: the ``linspace`` end points of ``make_grid``, ``inverse(G)[:, :2, :]`` (inverted in ``G``'s own
    precision, the reference's call), the ``[w_o / w_p, h_o / h_p]`` scale and offset of :349-353 and ``grid_sample``'s
    un-normalisation ``((g + 1) * size - 1) / 2`` (``align_corners=False``).  Row ``b`` is ``(t0..t5)`` of ``op.affine_warp``; the
    output of the warp has the 2x image's own size, ``warp_hw(in_hw, pads, len_k)``."""
    h_o, w_o = in_hw
    p_x1, _, p_y1, _ = pads
    h2, w2 = warp_hw(in_hw, pads, len_k)
    w_p, h_p = w_o + pads[0] + pads[1] + 1, h_o + pads[2] + pads[3] + 1
    A = torch.inverse(G)[:, :2, :].double()
    # make_grid: g = lo + (hi - lo) * index / (n - 1) per axis
    lo = torch.tensor([-2 * p_x1 / w_o - 1, -2 * p_y1 / h_o - 1], dtype=torch.float64)
    hi = torch.tensor([2 * (w_p - p_x1) / w_o - 1, 2 * (h_p - p_y1) / h_o - 1], dtype=torch.float64)
    step = (hi - lo) / torch.tensor([max(w2 - 1, 1), max(h2 - 1, 1)], dtype=torch.float64)
    # u = A @ (g_x, g_y, 1), as a function of (ox, oy, 1)
    M = torch.cat((A[:, :, :2] * step, (A[:, :, :2] * lo).sum(-1, keepdim=True) + A[:, :, 2:]), -1)
    # rescale into the padded image's normalised frame, then into pixels of the 2x image
    scale = torch.tensor([w_o / w_p, h_o / h_p], dtype=torch.float64).view(1, 2, 1)
    offset = torch.tensor([(w_o + 2 * p_x1) / w_p - 1, (h_o + 2 * p_y1) / h_p - 1], dtype=torch.float64).view(1, 2, 1)
    size = torch.tensor([w2, h2], dtype=torch.float64).view(1, 2, 1)
    M = M * scale
    M[:, :, 2:] += offset
    M = M * (size / 2)
    M[:, :, 2:] += (size - 1) / 2
    return M.reshape(-1, 6).to(dtype)


def warp_hw(in_hw: Tuple[int, int], pads: Sequence[int], len_k: int) -> Tuple[int, int]:
    """Size of the 2x-upsampled padded image: ``upfirdn2d(up=2)`` of the image padded by ``pads`` + ``(len_k + 1) // 2`` a side."""
    pad_k = (len_k + 1) // 2
    return (2 * (in_hw[0] + pads[2] + pads[3] + 2 * pad_k) - len_k + 1, 2 * (in_hw[1] + pads[0] + pads[1] + 2 * pad_k) - len_k + 1)


def random_apply_affine(img, p, G=None, antialiasing_kernel=SYM6):
    """Apply the geometric transform ``G`` ([B, 3, 3]; drawn with probability ``p`` when ``None``) to ``img`` with 2x supersampling
    through ``antialiasing_kernel`` -> ``(img, G)``."""
    len_k = len(antialiasing_kernel)
    pad_k = (len_k + 1) // 2
    k1 = torch.as_tensor(antialiasing_kernel)
    kernel = torch.ger(k1, k1).to(img)
    kernel_flip = torch.flip(kernel, (0, 1))

    img_pad, G, pads = try_sample_affine_and_pad(img, p, pad_k, G)
    pad_x1, pad_x2, pad_y1, pad_y2 = pads
    in_hw = (img.shape[2], img.shape[3])

    img_2x = op.upfirdn2d(img_pad, kernel_flip, up=2)
    theta = warp_theta(G, in_hw, pads, len_k, torch.float64 if img.dtype == torch.float64 else torch.float32).to(img.device)
    img_affine = op.affine_warp(img_2x, theta, img_2x.shape[2:])
    img_down = op.upfirdn2d(img_affine, kernel, down=2)

    end_y = img_down.shape[2] - pad_y2 - 1
    end_x = img_down.shape[3] - pad_x2 - 1
    return img_down[:, :, pad_y1:end_y, pad_x1:end_x], G


def apply_color(img, mat):
    """``img[b]`` ([3, H, W]) through the upper three rows of the 4x4 ``mat[b]``: a 3x3 mix of the channels plus an offset."""
    return op.color_affine(img, mat[:, :3, :].to(img.device))


def random_apply_color(img, p, C=None):
    if C is None:
        C = sample_color(p, img.shape[0])
    return apply_color(img, C), C


def augment(img, p, transform_matrix=(None, None)):
    """The ADA pipeline on ``img`` ([B, 3, H, W] on the device): geometric, then colour transforms, each drawn with probability ``p``
    unless given in ``transform_matrix = (G, C)`` -> ``(img, (G, C))``."""
    img, G = random_apply_affine(img, p, transform_matrix[0])
    img, C = random_apply_color(img, p, transform_matrix[1])
    return img, (G, C)


class AdaptiveAugment:
    """The adaptation of the augmentation probability of stylegan2/train.py:151-153, 194-213.

    ``tune(real_pred)`` adds ``[sum of sign(real_pred), batch]`` to an accumulator (through ``reduce_sum`` -- the sum over the ranks of
    a data-parallel job -- when one is given); once more than 255 predictions are in, ``r_t = signs / count`` is compared with
    ``ada_target``, ``p`` moves by ``ada_target / ada_length * count`` towards it (up when ``r_t`` is above the target: D is
    overfitting), is clamped to [0, 1], and the accumulator starts again.  Returns the current ``p``.

    The reference adapts only when ``--augment_p`` is 0; with ``--augment_p > 0`` the probability is fixed and ``tune`` is never called
    -- the caller then keeps ``initial_p`` and does not call ``tune`` either."""

    def __init__(self, ada_target: float, ada_length: float, initial_p: float = 0.0,
                 reduce_sum: Optional[Callable[[torch.Tensor], torch.Tensor]] = None):
        self.ada_target = ada_target
        self.ada_aug_step = ada_target / ada_length
        self.ada_aug_p = initial_p
        self.r_t_stat = 0.0
        self.reduce_sum = reduce_sum
        self.ada_augment: Optional[torch.Tensor] = None

    @torch.no_grad()
    def tune(self, real_pred: torch.Tensor) -> float:
        if self.ada_augment is None:
            self.ada_augment = torch.tensor([0.0, 0.0], device=real_pred.device)
        self.ada_augment += torch.tensor((torch.sign(real_pred).sum().item(), real_pred.shape[0]), device=real_pred.device)
        if self.reduce_sum is not None:
            self.ada_augment = self.reduce_sum(self.ada_augment)
        if self.ada_augment[1] > 255:
            pred_signs, n_pred = self.ada_augment.tolist()
            self.r_t_stat = pred_signs / n_pred
            sign = 1 if self.r_t_stat > self.ada_target else -1
            self.ada_aug_p += sign * self.ada_aug_step * n_pred
            self.ada_aug_p = min(1, max(0, self.ada_aug_p))
            self.ada_augment.mul_(0)
        return self.ada_aug_p
