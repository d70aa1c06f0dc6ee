"""LPIPS perceptual distance, VGG16 variant (the reference's vendored ``lpips`` package: stylegan2/lpips/), on the HIP ops.

``PerceptualLoss(model='net-lin', net='vgg')`` is what stylegan2/projector.py builds: VGG16 features at five taps, unit-normalised
over channels, squared difference, non-negative learned 1x1 weights, spatial mean, summed over the taps
(networks_basic.py:64-92, ``version='0.1'``, ``spatial=False``).  The thirteen conv + bias + ReLU layers run on
``op.conv2d_bias_act`` (``negative_slope=0, scale=1``), the four pools on ``op.max_pool2x2`` and each tap's head on ``op.lpips_layer``.

No weights are shipped: the VGG16 backbone (a torchvision ``vgg16`` state dict, or its ``features.*`` part) and the lin weights (the
LPIPS ``weights/v0.1/vgg.pth`` format) come from the user.  The alex / squeeze backbones, ``spatial=True``, the ``net`` / ``L2`` /
``SSIM`` models and training the lin layers are not implemented.
"""
from __future__ import annotations

from typing import Dict, List, Union

import torch
from torch import nn

from . import op

# torchvision's vgg16().features: the indices of the convs ('M' = a pool after the preceding ReLU) and the channel plan
VGG16_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512)
VGG16_CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
# the slices of lpips/pretrained_networks.py:107-116 end after the ReLUs of these convs: relu1_2, 2_2, 3_3, 4_3, 5_3
VGG16_TAP_INDICES = (2, 7, 14, 21, 28)
LPIPS_CHANNELS = (64, 128, 256, 512, 512)


class _Conv3x3ReLU(nn.Module):
    """3x3 / stride 1 / pad 1 conv + bias + ReLU in one kernel; ``weight`` / ``bias`` as ``nn.Conv2d`` names and shapes them."""

    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(cout, cin, 3, 3), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)

    def forward(self, x):
        return op.conv2d_bias_act(x, self.weight, self.bias, stride=1, padding=1, negative_slope=0.0, scale=1.0)


class VGG16Features(nn.Module):
    """torchvision's ``vgg16().features`` up to relu5_3, returning the five LPIPS taps.  State-dict keys are torchvision's
    (``features.{0,2,5,...,28}.{weight,bias}``); the parameters are frozen."""

    def __init__(self):
        super().__init__()
        convs, cin, idx = {}, 3, 0
        self._plan: List[Union[str, int]] = []
        for c in VGG16_CFG:
            if c == "M":
                self._plan.append("M")
                idx += 1
            else:
                convs[str(idx)] = _Conv3x3ReLU(cin, c)
                self._plan.append(idx)
                cin = c
                idx += 2
        assert tuple(int(k) for k in convs) == VGG16_CONV_INDICES
        self.features = nn.ModuleDict(convs)
        self.pool = op.max_pool2x2          # (an attribute so that tools/bench_lpips.py can time the torch composition in its place)

    def load_backbone(self, state: Dict[str, torch.Tensor]) -> None:
        """Load a torchvision VGG16 state dict (``classifier.*`` entries are ignored) with ``strict=True`` on the features."""
        feats = {k: v for k, v in state.items() if k.startswith("features.")}
        self.load_state_dict(feats, strict=True)

    def forward(self, x):
        taps = []
        for step in self._plan:
            if step == "M":
                x = self.pool(x)
            else:
                x = self.features[str(step)](x)
                if step in VGG16_TAP_INDICES:
                    taps.append(x)
        return taps


class ScalingLayer(nn.Module):
    """networks_basic.py:94-101: ``(x - shift) / scale`` on three channels (plain torch: 3 of the 64 .. 512 channels that follow)."""

    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer("scale", torch.tensor([.458, .448, .450])[None, :, None, None])

    def forward(self, inp):
        return (inp - self.shift) / self.scale


def _load(obj, what):
    if isinstance(obj, dict):
        return obj
    state = torch.load(obj, map_location="cpu")
    if not isinstance(state, dict):
        raise RuntimeError(f"{what}: {obj} does not hold a state dict")
    return state


class PerceptualLoss(nn.Module):
    """``lpips.PerceptualLoss(model='net-lin', net='vgg')`` (lpips/__init__.py:13-40 -> dist_model.py -> networks_basic.PNetLin).

    ``backbone``: a path to, or a dict of, a torchvision VGG16 state dict.  ``lin_weights``: a path to, or a dict in, the LPIPS
    ``weights/v0.1/vgg.pth`` format (``lin{k}.model.1.weight`` of shape [1, C, 1, 1]).  Neither is shipped with the package."""

    def __init__(self, model: str = "net-lin", net: str = "vgg", backbone=None, lin_weights=None):
        super().__init__()
        if model != "net-lin" or net not in ("vgg", "vgg16"):
            raise NotImplementedError(f"PerceptualLoss(model={model!r}, net={net!r}) is not implemented: only model='net-lin' with "
                                      "net='vgg' (the configuration of stylegan2/projector.py) is supported")
        if backbone is None and lin_weights is None:
            raise RuntimeError("PerceptualLoss needs weights and ships none: pass backbone= (a torchvision VGG16 state dict or its "
                               "path) and lin_weights= (LPIPS weights/v0.1/vgg.pth or its path)")
        if backbone is None or lin_weights is None:
            raise RuntimeError("PerceptualLoss needs both backbone= (a torchvision VGG16 state dict or its path) and lin_weights= "
                               "(LPIPS weights/v0.1/vgg.pth or its path)")
        self.scaling_layer = ScalingLayer()
        self.net = VGG16Features()
        self.net.load_backbone(_load(backbone, "backbone"))
        lins = _load(lin_weights, "lin_weights")
        for k, c in enumerate(LPIPS_CHANNELS):
            key = f"lin{k}.model.1.weight"
            if key not in lins:
                raise RuntimeError(f"lin_weights has no {key!r} (expected the LPIPS weights/v0.1/vgg.pth format)")
            w = lins[key]
            if tuple(w.shape) != (1, c, 1, 1):
                raise RuntimeError(f"lin_weights[{key!r}] has shape {tuple(w.shape)}, expected {(1, c, 1, 1)}")
            self.register_buffer(f"lin{k}", w.detach().float().reshape(c).clone())
        self.head = op.lpips_layer          # (an attribute, as VGG16Features.pool)
        self.eval()

    def lin(self, k: int) -> torch.Tensor:
        return getattr(self, f"lin{k}")

    def features(self, x: torch.Tensor) -> List[torch.Tensor]:
        """The five taps of one side; a side that does not require grad runs under ``no_grad`` (its activations are not kept)."""
        if torch.is_grad_enabled() and x.requires_grad:
            return self.net(self.scaling_layer(x))
        with torch.no_grad():
            return self.net(self.scaling_layer(x))

    def pair_distance(self, prepared: torch.Tensor) -> torch.Tensor:
        """``prepared``: [2B, 3, h, w], the output of ``op.pair_prepare`` -- already through the scaling layer, the first sides of the
        B pairs in the first half-batch and the second sides in the other.  ONE backbone pass over all 2B samples, each tap's head on
        its two halves -> [B] float32.  No gradient."""
        if prepared.dim() != 4 or prepared.shape[0] % 2 or prepared.shape[0] == 0:
            raise RuntimeError(f"pair_distance expects the [2B, 3, h, w] output of op.pair_prepare, got {tuple(prepared.shape)}")
        b = prepared.shape[0] // 2
        with torch.no_grad():
            taps = self.net(prepared)
            val = None
            for k, tap in enumerate(taps):
                r = self.head(tap[:b], tap[b:], self.lin(k))
                val = r if val is None else val + r
        return val.float()

    def forward(self, pred: torch.Tensor, target: torch.Tensor, normalize: bool = False, ret_per_layer: bool = False):
        """``pred``, ``target``: [N, 3, H, W] in [-1, 1] ([0, 1] with ``normalize=True``) -> [N, 1, 1, 1] float32."""
        if normalize:
            target = 2 * target - 1
            pred = 2 * pred - 1
        f0, f1 = self.features(target), self.features(pred)           # (the reference calls its model with (target, pred))
        res = [self.head(a, b, self.lin(k)) for k, (a, b) in enumerate(zip(f0, f1))]
        val = res[0]
        for r in res[1:]:
            val = val + r
        val = val.float().view(-1, 1, 1, 1)
        if ret_per_layer:
            return val, [r.float().view(-1, 1, 1, 1) for r in res]
        return val
