"""Shared by tests/golden/make_golden_lpips.py and the LPIPS tests: the seeded stand-in for torchvision's VGG16 backbone (there is no
torchvision, and no trained weights, here) and f64 restatements of the two ops of csrc/lpips.hip."""
import torch
from torch import nn

VGG16_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")
BACKBONE_SEED = 1312


def vgg16_features(seed=BACKBONE_SEED):
    """torchvision's ``vgg16().features`` layout (Conv2d 3x3 pad 1 / ReLU / MaxPool2d(2, 2), 31 modules) with seeded weights:
    normal with std sqrt(2 / fan_in), so that activations keep their scale through the thirteen layers, and normal(0, 0.1) biases."""
    gen = torch.Generator().manual_seed(seed)
    layers, cin = [], 3
    for c in VGG16_CFG:
        if c == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            conv = nn.Conv2d(cin, c, kernel_size=3, padding=1)
            with torch.no_grad():
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * (2.0 / (cin * 9)) ** 0.5)
                conv.bias.copy_(torch.randn(conv.bias.shape, generator=gen) * 0.1)
            layers += [conv, nn.ReLU(inplace=True)]
            cin = c
    return nn.Sequential(*layers)


def backbone_state(seed=BACKBONE_SEED):
    """The stand-in's weights under torchvision's state-dict names (``features.N.weight`` / ``features.N.bias``)."""
    return {f"features.{k}": v.detach().clone() for k, v in vgg16_features(seed).state_dict().items()}


def checksums(sd):
    return {k: [float(v.double().sum()), float(v.double().abs().sum())] for k, v in sd.items()}


def lpips_layer_f64(f0, f1, w):
    """d [B] and, for a cotangent gd, the gradients: the formulas of csrc/lpips.hip in f64 (u = 0 and a zero gradient where n = 0)."""
    f0, f1, w = f0.double(), f1.double(), w.double().reshape(1, -1, 1, 1)
    n0, n1 = f0.pow(2).sum(1, keepdim=True).sqrt(), f1.pow(2).sum(1, keepdim=True).sqrt()
    u0, u1 = f0 / (n0 + 1e-10), f1 / (n1 + 1e-10)
    d = (w * (u0 - u1) ** 2).sum(1).mean((1, 2))

    def grads(gd):
        hw = f0.shape[2] * f0.shape[3]
        g = 2 * w * (u0 - u1) * gd.double().reshape(-1, 1, 1, 1) / hw

        def one(f, n):
            a = n + 1e-10
            safe = torch.where(n > 0, n, torch.ones_like(n))
            r = g / a - f * (g * f).sum(1, keepdim=True) / (safe * a * a)
            return torch.where(n > 0, r, torch.zeros_like(r))
        return one(f0, n0), -one(f1, n1)
    return d, grads
