"""Shared by tests/golden/make_golden_fid.py and the FID tests: a plain-torch, seeded stand-in for ``torchvision.models.inception``
(there is no torchvision, and no trained weights, here).  ``BasicConv2d``, ``InceptionA`` .. ``InceptionE`` and ``inception_v3`` carry
the submodule names and constructor signatures that the reference's stylegan2/inception.py subclasses (``FIDInceptionA(in_channels,
pool_features)``, ``FIDInceptionC(in_channels, channels_7x7)``, ``FIDInceptionE_*(in_channels)``); their ``forward``s are
torchvision's (zero-padded averages), which the reference overrides for the blocks it patches.  Written from the architecture
table of the Inception-v3 paper as torchvision lays it out."""
import sys
import types

import torch
import torch.nn.functional as F
from torch import nn

BACKBONE_SEED = 2015
N_ENTRIES, N_PARAMS = 566, 23_850_960


class BasicConv2d(nn.Module):
    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, bias=False, **kwargs)
        self.bn = nn.BatchNorm2d(out_channels, eps=0.001)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)), inplace=True)


class InceptionA(nn.Module):
    def __init__(self, in_channels, pool_features):
        super().__init__()
        self.branch1x1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(in_channels, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(in_channels, pool_features, kernel_size=1)

    def forward(self, x):
        pool = self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
        return torch.cat([self.branch1x1(x), self.branch5x5_2(self.branch5x5_1(x)),
                          self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))), pool], 1)


class InceptionB(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch3x3 = BasicConv2d(in_channels, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)

    def forward(self, x):
        return torch.cat([self.branch3x3(x), self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))),
                          F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionC(nn.Module):
    def __init__(self, in_channels, channels_7x7):
        super().__init__()
        c7 = channels_7x7
        self.branch1x1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(in_channels, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(in_channels, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(in_channels, 192, kernel_size=1)

    def forward(self, x):
        b7 = self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)))
        bd = self.branch7x7dbl_1(x)
        for m in (self.branch7x7dbl_2, self.branch7x7dbl_3, self.branch7x7dbl_4, self.branch7x7dbl_5):
            bd = m(bd)
        pool = self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
        return torch.cat([self.branch1x1(x), b7, bd, pool], 1)


class InceptionD(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(in_channels, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)

    def forward(self, x):
        b7 = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        return torch.cat([self.branch3x3_2(self.branch3x3_1(x)), b7, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class InceptionE(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.branch1x1 = BasicConv2d(in_channels, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(in_channels, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(in_channels, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(in_channels, 192, kernel_size=1)

    def forward(self, x):
        a = self.branch3x3_1(x)
        d = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        pool = self.branch_pool(F.avg_pool2d(x, kernel_size=3, stride=1, padding=1))
        return torch.cat([self.branch1x1(x), self.branch3x3_2a(a), self.branch3x3_2b(a), self.branch3x3dbl_3a(d),
                          self.branch3x3dbl_3b(d), pool], 1)


class Inception3(nn.Module):
    def __init__(self, num_classes=1000, aux_logits=True):
        super().__init__()
        assert not aux_logits, "the stand-in has no auxiliary classifier (the FID network is built with aux_logits=False)"
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.Mixed_5b = InceptionA(192, pool_features=32)
        self.Mixed_5c = InceptionA(256, pool_features=64)
        self.Mixed_5d = InceptionA(288, pool_features=64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, channels_7x7=128)
        self.Mixed_6c = InceptionC(768, channels_7x7=160)
        self.Mixed_6d = InceptionC(768, channels_7x7=160)
        self.Mixed_6e = InceptionC(768, channels_7x7=192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280)
        self.Mixed_7c = InceptionE(2048)
        self.fc = nn.Linear(2048, num_classes)


def inception_v3(num_classes=1000, aux_logits=True, pretrained=False, **kwargs):
    assert not pretrained, "the stand-in has no trained weights"
    return Inception3(num_classes=num_classes, aux_logits=aux_logits)


def seed_(net, seed=BACKBONE_SEED):
    """Conv weights ~ N(0, 2 / fan_in); BN weight ~ U(0.75, 1.25), bias ~ N(0, 0.1), running_mean ~ N(0, 0.1), running_var ~
    U(0.5, 1.5); the fc layer ~ N(0, 0.01): all from one seeded generator, in module order, so that the BatchNorm folding has
    something to fold and activations keep their scale through the 94 layers."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                fan_in = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen) * (2.0 / fan_in) ** 0.5)
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(0.75 + 0.5 * torch.rand(m.weight.shape, generator=gen))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=gen))
                m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(m.bias.shape, generator=gen))
            elif isinstance(m, nn.Linear):
                m.weight.copy_(0.01 * torch.randn(m.weight.shape, generator=gen))
                m.bias.copy_(0.01 * torch.randn(m.bias.shape, generator=gen))
    return net


_STATE = {}


def backbone_state(seed=BACKBONE_SEED):
    """The seeded state dict under torchvision's names: what ``pt_inception-2015-12-05-6726825d.pth`` holds, in shape (made once)."""
    if seed not in _STATE:
        _STATE[seed] = {k: v.detach().clone() for k, v in seed_(inception_v3(num_classes=1008, aux_logits=False), seed).state_dict().items()}
    return _STATE[seed]


def checksums(sd):
    return {k: [float(v.double().sum()), float(v.double().abs().sum())] for k, v in sd.items()}


def as_torchvision_models():
    """A module object standing for ``torchvision.models``: ``inception_v3`` and the ``inception`` submodule with the classes."""
    models = types.ModuleType("torchvision.models")
    inception = types.ModuleType("torchvision.models.inception")
    this = sys.modules[__name__]
    for name in ("BasicConv2d", "InceptionA", "InceptionB", "InceptionC", "InceptionD", "InceptionE", "Inception3", "inception_v3"):
        setattr(inception, name, getattr(this, name))
    models.inception = inception
    models.inception_v3 = inception_v3
    return models


# ---- the seeded inputs of tests/golden/fid.npz (too large to store: remade on both sides, guarded by stored checksums) -------------
CASES = {"up": (64, 48, False), "same": (299, 299, False), "down": (320, 320, False), "norm01": (64, 48, True)}
INPUT_SEED, STATS_SEED = 5000, 5300


def case_input(tag):
    """[2, 3, H, W] f32: sample 0 a smooth image (a few low-frequency waves per channel), sample 1 uniform noise; in [-1, 1], or
    mapped to [0, 1] for the ``normalize_input`` case."""
    h, w, normalize = CASES[tag]
    gen = torch.Generator().manual_seed(INPUT_SEED + list(CASES).index(tag))
    yy = torch.arange(h, dtype=torch.float64).view(1, h, 1) / h
    xx = torch.arange(w, dtype=torch.float64).view(1, 1, w) / w
    fy = torch.tensor([1.0, 2.0, 0.5], dtype=torch.float64).view(3, 1, 1)
    fx = torch.tensor([1.5, 0.5, 2.5], dtype=torch.float64).view(3, 1, 1)
    ph = torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64).view(3, 1, 1)
    smooth = 0.8 * torch.sin(2 * torch.pi * (fy * yy + fx * xx) + ph)
    noise = torch.rand(3, h, w, generator=gen, dtype=torch.float64) * 2 - 1
    x = torch.stack([smooth, noise]).float()
    return (x + 1) / 2 if normalize else x


def block_slice(t):
    """The stored part of a block output [B, C, H, W]: the first and the last 16 channels at the 3x3 top-left pixels."""
    return torch.cat([t[:, :16, :3, :3], t[:, -16:, :3, :3]], 1)


def stats_features():
    """[37, 2048] f32, feature-like (non-negative, a third of them zero, spread comparable with the mean): relu(N(0.3, 1))."""
    gen = torch.Generator().manual_seed(STATS_SEED)
    return torch.relu(0.3 + torch.randn(37, 2048, generator=gen, dtype=torch.float64)).float()
