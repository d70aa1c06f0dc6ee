"""The discriminator side of the layer library: ``ConvLayer``, ``ResBlock`` and ``Discriminator`` of stylegan2/model.py:584-712.

Same constructor signatures, attribute names, ``nn.Sequential`` indices and parameter creation order as the reference, so
state-dict keys and shapes match a reference discriminator checkpoint and ``torch.manual_seed(s)`` yields the reference's initial
weights.  Importable from ``ideas_amd.model`` (the layer library re-exports the three names lazily: ``models.py`` imports
``model.py``, and these classes build on ``models.ConvLayer`` / ``models.ResBlock``).

The forwards are those of the IDEAS blocks (models.py): the 1x1 stem, blur + stride-2 residual blocks on ``down_pair`` /
``fork_down2`` / the ``post_blur`` pairing with the residual add in a conv epilogue, fused conv + bias + leaky-ReLU, and
``EqualLinear``; the one op the IDEAS networks do not have is the minibatch standard deviation (``op.minibatch_stddev``).
"""
from __future__ import annotations

import math

from torch import nn

from . import models as _M
from .model import EqualConv2d, EqualLinear
from .op import minibatch_stddev
from .precision import to_f32


class ConvLayer(_M.ConvLayer):
    """[Blur] -> EqualConv2d -> [FusedLeakyReLU | ScaledLeakyReLU] (stylegan2/model.py:584-630): the zero-padded, non-upsampling
    subset of ``models.ConvLayer``, whose forward (and fused routes) it inherits."""

    def __init__(self, in_channel, out_channel, kernel_size, downsample=False, blur_kernel=[1, 3, 3, 1], bias=True, activate=True):
        super().__init__(in_channel, out_channel, kernel_size, downsample=downsample, blur_kernel=blur_kernel, bias=bias,
                         activate=activate)
        if not downsample:
            # the reference pads kernel_size // 2 (model.py:610); models.ConvLayer (kernel_size - 1) // 2 -- the same for odd kernels
            self.padding = kernel_size // 2
            next(m for m in self if isinstance(m, EqualConv2d)).padding = self.padding


class ResBlock(_M.ResBlock):
    """conv1 in->in, conv2 in->out behind blur + stride 2, 1x1 downsampling skip, merged as (body + skip) / sqrt(2)
    (stylegan2/model.py:633-651).  Only the constructor differs from ``models.ResBlock`` (whose conv1 already widens to
    ``out_channel``); the forward is inherited."""

    def __init__(self, in_channel, out_channel, blur_kernel=[1, 3, 3, 1]):
        nn.Module.__init__(self)
        # (the reference does not hand ``blur_kernel`` on to its layers, model.py:637-642: they keep the default taps)
        self.conv1 = ConvLayer(in_channel, in_channel, 3)
        self.conv2 = ConvLayer(in_channel, out_channel, 3, downsample=True)
        self.skip = ConvLayer(in_channel, out_channel, 1, downsample=True, activate=False, bias=False)


class Discriminator(nn.Module):
    """image -> logit (stylegan2/model.py:654-712); logits are f32 in every activation mode."""

    def __init__(self, size, channel_multiplier=2, blur_kernel=[1, 3, 3, 1]):
        super().__init__()
        cm = channel_multiplier
        channels = {4: 512, 8: 512, 16: 512, 32: 512, 64: 256 * cm, 128: 128 * cm, 256: 64 * cm, 512: 32 * cm, 1024: 16 * cm}
        convs = [ConvLayer(3, channels[size], 1)]
        in_channel = channels[size]
        for i in range(int(math.log(size, 2)), 2, -1):
            out_channel = channels[2 ** (i - 1)]
            convs.append(ResBlock(in_channel, out_channel, blur_kernel))
            in_channel = out_channel
        self.convs = nn.Sequential(*convs)
        self.stddev_group = 4
        self.stddev_feat = 1
        self.final_conv = ConvLayer(in_channel + 1, channels[4], 3)
        self.final_linear = nn.Sequential(
            EqualLinear(channels[4] * 4 * 4, channels[4], activation="fused_lrelu"),
            EqualLinear(channels[4], 1),
        )

    def forward(self, input):
        out = self.convs(input)
        out = minibatch_stddev(out, self.stddev_group, self.stddev_feat)
        out = self.final_conv(out)
        # the reference flattens its NCHW tensor (model.py:709): final_linear.0.weight is indexed c * 16 + h * 4 + w.  reshape()
        # follows the logical [B, C, H, W] order whatever the memory format
        return self.final_linear(to_f32(out).reshape(out.shape[0], -1))
