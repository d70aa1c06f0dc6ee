"""The seven IDEAS networks on the ideas_amd layer library.

Host-side mirror of the reference's models.py (EqualConvTranspose2d :11-46, ConvLayer :49-134,
StyledResBlock :137-178, ResBlock :181-227, DisentanglementEncoder :230-268, Generator :271-306,
StructureGenerator :309-329, ImageLevelDiscriminator :332-376, CooccurenceDiscriminator :379-426,
DistributionDiscriminator :429-441, TensorExtractor :444-465, init_model :468-513).

What is kept identical: class names, constructor arguments, attribute names, the positional indices inside
every ``nn.Sequential`` and the order in which parameters are created — so state-dict keys/shapes match the
reference checkpoint format and ``torch.manual_seed(s)`` yields the reference's initial weights.
What differs: forwards run on the gfx950 kernels (NHWC), ``ReflectionPad2d`` is folded into the conv's gather
instead of materialising a padded tensor, and residual merges use one fused multiply-add.
"""
from __future__ import annotations

import math
import os

import torch
from torch import nn

from .model import (CL, Blur, EqualConv2d, EqualLinear, ScaledLeakyReLU,
                    StyledConv_without_noise as StyledConv, styles_for)
from .op import FusedLeakyReLU, conv2d, conv_transpose2d, upfirdn2d
from .op.conv import down_pair, down_pair_ok, fork_conv2d
from .op.upfirdn2d import blur_pads, fork_down2, upfirdn2d_up2_add
from .precision import to_act, to_f32

_INV_SQRT2 = 1.0 / math.sqrt(2)
FUSE_RESIDUAL_ADDS = True     # big residual blocks: block input forked by one autograd node (gradient sum / merge add ride in kernels)
FUSE_BLUR_CONV = os.environ.get("IDEAS_BLUR_CONV", "1") != "0"   # downsampling ResBlock body with conv2's Blur inside its conv kernel
DCO_MERGE = os.environ.get("IDEAS_DCO_MERGE", "2")               # CooccurDiscriminator.forward_pair: encoder passes merged (A/B)
FUSE_BLUR_BACKWARD = True     # ResBlock: conv1 + conv2's Blur as one Function whose backward is one kernel (A/B switch for tools / tests)


class EqualConvTranspose2d(nn.Module):
    """Stride-2 transposed conv with equalised-lr weights [Cin, Cout, k, k] (only k=1 is used, in skips)."""

    def __init__(self, in_channel, out_channel, kernel_size, stride=1, padding=0, bias=True):
        super().__init__()
        if padding != 0:
            raise NotImplementedError("IDEAS only uses padding=0 transposed convs (models.py:80-88)")
        w = torch.randn(in_channel, out_channel, kernel_size, kernel_size)
        self.weight = nn.Parameter(w.contiguous(memory_format=CL))
        self.scale = 1 / math.sqrt(in_channel * kernel_size ** 2)
        self.stride = stride
        self.padding = padding
        self.bias = nn.Parameter(torch.zeros(out_channel)) if bias else None

    def forward(self, input, post_gain: float = 1.0):
        return conv_transpose2d(input, self.weight, self.bias, stride=self.stride, gain=self.scale * post_gain)

    def __repr__(self):
        i, o, k, _ = self.weight.shape
        return f"{self.__class__.__name__}({i}, {o}, {k}, stride={self.stride}, padding={self.padding})"


class ConvLayer(nn.Sequential):
    """[Blur] -> (ConvT -> Blur | [ReflectionPad] -> Conv) -> [FusedLeakyReLU | Tanh | ScaledLeakyReLU]."""

    def __init__(self, in_channel, out_channel, kernel_size, upsample=False, downsample=False,
                 blur_kernel=(1, 3, 3, 1), bias=True, activate=True, padding="zero", tanh=False):
        mods = []
        conv_bias = bias and not activate
        conv_pad, stride = 0, 1
        if downsample:
            mods.append(Blur(blur_kernel, pad=blur_pads(len(blur_kernel), kernel_size, up=False)))
            stride = 2
        if upsample:
            mods.append(EqualConvTranspose2d(in_channel, out_channel, kernel_size, padding=0, stride=2, bias=conv_bias))
            mods.append(Blur(blur_kernel, pad=blur_pads(len(blur_kernel), kernel_size, up=True)))
        else:
            if not downsample:
                half = (kernel_size - 1) // 2
                if padding == "zero":
                    conv_pad = half
                elif padding == "reflect":
                    if half > 0:
                        mods.append(nn.ReflectionPad2d(half))
                elif padding != "valid":
                    raise ValueError('Padding should be "zero", "reflect", or "valid"')
            mods.append(EqualConv2d(in_channel, out_channel, kernel_size, padding=conv_pad, stride=stride,
                                    bias=conv_bias))
        if activate:
            if tanh:
                mods.append(nn.Tanh())
            elif bias:
                mods.append(FusedLeakyReLU(out_channel))
            else:
                mods.append(ScaledLeakyReLU(0.2))
        super().__init__(*mods)
        self.padding = conv_pad

    def forward(self, input, post_gain: float = 1.0, resid=None, post_blur=None, skip_blur: bool = False):
        """``post_gain`` scales the layer output (folded into the conv / activation gain — every op after the conv is
        linear or the scaled leaky-ReLU, so the fold is exact up to rounding); ``resid`` is added in the last conv's
        epilogue (no-grad passes only).  ``post_blur`` (a Blur module): apply the NEXT layer's blur behind this layer's conv +
        activation (that layer is then called with ``skip_blur``) — same values, but the pair shares one backward kernel."""
        x = input
        mods = list(self)
        i = 1 if (skip_blur and isinstance(mods[0], Blur)) else 0
        while i < len(mods):
            m = mods[i]
            refl = 0
            if isinstance(m, nn.ReflectionPad2d) and i + 1 < len(mods) and isinstance(mods[i + 1], EqualConv2d):
                refl = m.padding[0]                            # mirror padding folded into the conv gather
                i += 1
                m = mods[i]
            nxt_m = mods[i + 1] if i + 1 < len(mods) else None
            if (isinstance(m, Blur) and isinstance(nxt_m, EqualConv2d) and nxt_m.stride == 2 and nxt_m.padding == 0
                    and tuple(nxt_m.weight.shape[2:]) == (1, 1)):
                # blur -> 1x1 stride-2 conv (downsampling skip, models.py:78-95): only every second blurred pixel is used, so
                # the FIR is evaluated at the output resolution (down = 2) and the conv runs unstrided on a quarter of the pixels
                x = upfirdn2d(x, m.kernel, down=2, pad=m.pad)
                act = mods[i + 2] if i + 2 < len(mods) and isinstance(mods[i + 2], FusedLeakyReLU) else None
                nxt = i + (3 if act is not None else 2)
                if nxt < len(mods) and post_gain != 1.0:
                    raise RuntimeError("post_gain needs the conv (+activation) to end the layer")
                x = nxt_m(x, act=act, post_gain=post_gain, resid=resid, stride=1)
                i = nxt
                continue
            if (isinstance(m, EqualConvTranspose2d) and isinstance(nxt_m, Blur) and m.stride == 2 and m.bias is None
                    and tuple(m.weight.shape[2:]) == (1, 1)):
                # 1x1 stride-2 transposed conv -> blur (upsampling skip): three of four pixels of the transposed conv's output are
                # structural zeros.  The 1x1 conv runs at the input resolution and the FIR does the zero-stuffing (up = 2); the
                # transposed conv's output is one pixel short of the zero-stuffed size, hence pad1 - 1.
                x = conv2d(x, m.weight.transpose(0, 1), None, gain=m.scale * post_gain)
                x = upfirdn2d(x, nxt_m.kernel, up=2, pad=(nxt_m.pad[0], nxt_m.pad[1] - 1))
                i += 2
                continue
            if isinstance(m, EqualConv2d):
                act = mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], FusedLeakyReLU) else None
                nxt = i + (2 if act is not None else 1)
                if nxt < len(mods) and post_gain != 1.0:
                    raise RuntimeError("post_gain needs the conv (+activation) to end the layer")
                pb = None
                if post_blur is not None:
                    if act is None or nxt < len(mods):
                        raise RuntimeError("post_blur needs a layer ending in conv + FusedLeakyReLU")
                    pb = (post_blur.kernel, post_blur.pad)
                x = m(x, reflect_pad=refl, act=act, post_gain=post_gain, resid=resid, post_blur=pb)
                i = nxt
                continue
            if isinstance(m, EqualConvTranspose2d):
                x = m(x, post_gain=post_gain)                  # the blur that follows is linear
                i += 1
                continue
            x = m(x)
            i += 1
        return x


def _res_merge(block, body, last, input):
    """(body(input) + skip(input)) / sqrt(2) with the 1/sqrt(2) folded into both branches' gains (no multiply pass),
    and — when no graph is being built — the add folded into the last conv's epilogue as well."""
    if block.skip is None:
        return (last(body(input)) + input) * _INV_SQRT2
    if not torch.is_grad_enabled():
        skip = block.skip(input, post_gain=_INV_SQRT2)
        return last(body(input), post_gain=_INV_SQRT2, resid=skip)
    if FUSE_RESIDUAL_ADDS and torch.is_grad_enabled() and input.is_cuda:
        y = _res_merge_forked(block, body, last, input)
        if y is not None:
            return y
    out = last(body(input), post_gain=_INV_SQRT2)
    if isinstance(block.skip[-1], EqualConv2d):
        # the skip branch ends in a bias-free linear conv (same-resolution and downsampling blocks): the merge add rides in
        # that conv's epilogue and differentiates trivially (d/d out = the incoming gradient)
        return block.skip(input, post_gain=_INV_SQRT2, resid=out)
    return out + block.skip(input, post_gain=_INV_SQRT2)      # upsampling skip ends in a blur


def _res_merge_forked(block, body, last, input):
    """The two big blocks' shapes with the block input forked by ONE autograd node, so that the sum of its two gradients rides in a
    kernel that runs anyway instead of autograd's accumulation pass, and (upsampling) the merge add rides in the skip's FIR:
      downsampling  skip = [Blur, 1x1 stride-2 conv]     -> (x, fir_down2(x)) = fork_down2;  backward: fir_up2(g_skip) + g_body
      upsampling    skip = [1x1 stride-2 convT, Blur]    -> (x, conv1x1(x)) = fork_conv2d;  backward: dgrad(g_skip) + g_body in the
                                                            epilogue; forward merge: fir_up2(conv1x1(x)) + body(x) in the FIR
    Returns None for any other block (same-resolution skips are 16x16 tensors)."""
    mods = list(block.skip)
    if (len(mods) == 2 and isinstance(mods[0], Blur) and isinstance(mods[1], EqualConv2d) and mods[1].stride == 2
            and mods[1].padding == 0 and tuple(mods[1].weight.shape[2:]) == (1, 1) and mods[1].bias is None
            and input.shape[1] % 4 == 0):
        xa, h = fork_down2(to_act(input), mods[0].kernel, mods[0].pad)
        out = last(body(xa), post_gain=_INV_SQRT2)
        return mods[1](h, post_gain=_INV_SQRT2, resid=out, stride=1)
    if (len(mods) == 2 and isinstance(mods[0], EqualConvTranspose2d) and isinstance(mods[1], Blur) and mods[0].stride == 2
            and mods[0].bias is None and tuple(mods[0].weight.shape[2:]) == (1, 1) and input.shape[1] % 4 == 0
            and mods[0].weight.shape[1] % 4 == 0):
        m, blur = mods
        xa, h = fork_conv2d(input, m.weight.transpose(0, 1), gain=m.scale * _INV_SQRT2)
        out = last(body(xa), post_gain=_INV_SQRT2)
        return upfirdn2d_up2_add(h, blur.kernel, (blur.pad[0], blur.pad[1] - 1), out)
    return None


class StyledResBlock(nn.Module):
    def __init__(self, in_channel, out_channel, style_dim, upsample, blur_kernel=(1, 3, 3, 1)):
        super().__init__()
        self.conv1 = StyledConv(in_channel, out_channel, 3, style_dim, upsample=upsample, blur_kernel=blur_kernel)
        self.conv2 = StyledConv(out_channel, out_channel, 3, style_dim)
        if upsample or in_channel != out_channel:
            self.skip = ConvLayer(in_channel, out_channel, 1, upsample=upsample, blur_kernel=blur_kernel, bias=False,
                                  activate=False)
        else:
            self.skip = None

    def forward(self, input, style, noise=None):
        return _res_merge(self, lambda x: self.conv1(x, style), lambda h, **kw: self.conv2(h, style, **kw), input)


class ResBlock(nn.Module):
    """conv1 in->out, conv2 out->out (optionally blur + stride 2), 1x1 skip; differs from stock StyleGAN2."""

    def __init__(self, in_channel, out_channel, downsample, padding="zero", blur_kernel=(1, 3, 3, 1)):
        super().__init__()
        self.conv1 = ConvLayer(in_channel, out_channel, 3, padding=padding)
        self.conv2 = ConvLayer(out_channel, out_channel, 3, downsample=downsample, padding=padding,
                               blur_kernel=blur_kernel)
        if downsample or in_channel != out_channel:
            self.skip = ConvLayer(in_channel, out_channel, 1, downsample=downsample, blur_kernel=blur_kernel,
                                  bias=False, activate=False)
        else:
            self.skip = None

    def _fused_body(self):
        """(conv1's EqualConv2d, its activation, mirror padding, conv2's Blur, EqualConv2d, activation) when the block's body is
        [ReflectionPad2d] conv act -> Blur conv(stride 2) act, the shape op.conv.down_pair runs with the Blur inside the conv kernel."""
        m1, m2 = list(self.conv1), list(self.conv2)
        refl = 0
        if len(m1) == 3 and isinstance(m1[0], nn.ReflectionPad2d):
            refl, m1 = m1[0].padding[0], m1[1:]
        if not (len(m1) == 2 and isinstance(m1[0], EqualConv2d) and isinstance(m1[1], FusedLeakyReLU) and m1[0].bias is None
                and m1[0].stride == 1):
            return None
        if not (len(m2) == 3 and isinstance(m2[0], Blur) and isinstance(m2[1], EqualConv2d) and isinstance(m2[2], FusedLeakyReLU)
                and m2[1].bias is None and m2[1].stride == 2 and m2[1].padding == 0):
            return None
        return m1[0], m1[1], refl, m2[0], m2[1], m2[2]

    def _body_pair_ok(self, x) -> bool:
        """down_pair_ok for this block, memoised per (input shape / dtype, grad mode, conv2 trainable, activation dtype, the module
        switches of op.conv): the decision builds a launch plan and asks the library (ctypes), which the step would otherwise repeat
        in every forward -- also for the blocks that can never fuse."""
        from .op import conv as _cv
        from .precision import activation_dtype
        c1, a1, refl, blur, c2, a2 = self._fused
        key = (tuple(x.shape), x.dtype, str(x.device), torch.is_grad_enabled(), c2.weight.requires_grad, activation_dtype(), _cv.BLUR_CONV,
               _cv.BLUR_CONV_MIN_BLOCKS, _cv.BLUR_CONV_MIN_OW, _cv.MATH)
        memo = self.__dict__.setdefault("_pair_ok_memo", {})
        hit = memo.get(key)
        if hit is None:
            hit = (a1.negative_slope == a2.negative_slope and a1.bias is not None and a2.bias is not None
                   and down_pair_ok(x, c1.weight, c2.weight, blur.kernel, blur.pad, refl if refl else c1.padding))
            memo[key] = hit
        return hit

    def _body_pair(self, x, post_gain: float = 1.0, resid=None):
        c1, a1, refl, blur, c2, a2 = self._fused
        pad1, reflect1 = (refl, True) if refl else (c1.padding, False)
        return down_pair(x, c1.weight, a1.bias, c2.weight, a2.bias, blur.kernel, blur.pad, padding1=pad1, reflect1=reflect1,
                         gain1=c1.scale, gain2=c2.scale, negative_slope=a1.negative_slope, scale1=a1.scale,
                         scale2=a2.scale * post_gain, resid=resid)

    def forward(self, input):
        if FUSE_BLUR_CONV and input.is_cuda:
            if not hasattr(self, "_fused"):
                self._fused = self._fused_body()
            if self._fused is not None and self._body_pair_ok(input):
                # conv1 -> [Blur -> stride-2 conv2] with the Blur inside conv2's kernel (csrc/conv_b3_s2fir.hip); shapes the kernel
                # does not cover (small maps, bf16 activations) take the layer-by-layer path below
                return _res_merge(self, lambda x: x, self._body_pair, input)
        if FUSE_BLUR_BACKWARD and torch.is_grad_enabled() and isinstance(self.conv2[0], Blur) and isinstance(self.conv1[-1], FusedLeakyReLU):
            # downsampling block under autograd: conv1 also applies conv2's blur, so that the backward of the pair is one kernel
            # (blur adjoint + leaky-ReLU mask + bias gradient, op.conv._ConvBiasActBlur)
            blur = self.conv2[0]
            return _res_merge(self, lambda x: self.conv1(x, post_blur=blur), lambda h, **kw: self.conv2(h, skip_blur=True, **kw), input)
        return _res_merge(self, self.conv1, self.conv2, input)


class DisentanglementEncoder(nn.Module):
    """E: image -> (structure [B,8,R/16,R/16], texture [B,2048])."""

    def __init__(self, channel, structure_channel=8, texture_channel=2048, blur_kernel=(1, 3, 3, 1)):
        super().__init__()
        stem = [ConvLayer(3, channel, 1)]
        width = channel
        for i in range(1, 5):
            nxt = channel * (2 ** i)
            stem.append(ResBlock(width, nxt, downsample=True, padding="reflect", blur_kernel=blur_kernel))
            width = nxt
        self.stem = nn.Sequential(*stem)
        self.structure = nn.Sequential(
            ConvLayer(width, width, 1, blur_kernel=blur_kernel),
            ConvLayer(width, structure_channel, 1, blur_kernel=blur_kernel),
        )
        self.texture = nn.Sequential(
            ConvLayer(width, width * 2, 3, downsample=True, padding="valid", blur_kernel=blur_kernel),
            ConvLayer(width * 2, width * 4, 3, downsample=True, padding="valid", blur_kernel=blur_kernel),
            nn.AdaptiveAvgPool2d(1),
            ConvLayer(width * 4, texture_channel, 1, tanh=True, blur_kernel=blur_kernel),
        )

    def forward(self, input):
        feat = self.stem(input)
        return to_f32(self.structure(feat)), to_f32(torch.flatten(self.texture(feat), 1))


class Generator(nn.Module):
    """G: (structure, texture) -> image; 8 StyledResBlocks, the last four upsample."""

    WIDTHS = (4, 8, 12, 16, 16, 16, 8, 4)
    UPSAMPLE = (False, False, False, False, True, True, True, True)

    def __init__(self, channel, structure_channel=8, texture_channel=2048, blur_kernel=(1, 3, 3, 1)):
        super().__init__()
        self.layers = nn.ModuleList()
        width = structure_channel
        for mult, up in zip(self.WIDTHS, self.UPSAMPLE):
            self.layers.append(StyledResBlock(width, channel * mult, texture_channel, up, blur_kernel))
            width = channel * mult
        self.to_rgb = ConvLayer(width, 3, 1, activate=False)

    def forward(self, structure, texture, noises=None):
        out = structure
        # all sixteen modulation layers read `texture`: their styles come from one batched launch (model.styles_for)
        with styles_for([c.conv for layer in self.layers for c in (layer.conv1, layer.conv2)], texture):
            for layer in self.layers:
                out = layer(out, texture, None)
        return to_f32(self.to_rgb(out))


class StructureGenerator(nn.Module):
    """Gstru: secret tensor Z [B,N,h,w] -> structure code."""

    def __init__(self, channel, N=1, structure_channel=8, blur_kernel=(1, 3, 3, 1)):
        super().__init__()
        c = channel
        self.structure = nn.Sequential(
            ConvLayer(N, c, 1, blur_kernel=blur_kernel),
            ResBlock(c, c * 2, downsample=False, padding="reflect", blur_kernel=blur_kernel),
            ResBlock(c * 2, c * 4, downsample=False, padding="reflect", blur_kernel=blur_kernel),
            ResBlock(c * 4, c * 2, downsample=False, padding="reflect", blur_kernel=blur_kernel),
            ConvLayer(c * 2, structure_channel, 1, blur_kernel=blur_kernel),
        )

    def forward(self, noise):
        return to_f32(self.structure(noise))


class ImageLevelDiscriminator(nn.Module):
    """Dreal: image -> logit.  No minibatch-stddev layer (samples stay independent)."""

    def __init__(self, size, channel_multiplier=1, blur_kernel=(1, 3, 3, 1)):
        super().__init__()
        cm = channel_multiplier
        widths = {4: 512, 8: 512, 16: 512, 32: 512, 64: int(256 * cm), 128: int(128 * cm), 256: int(64 * cm),
                  512: int(32 * cm), 1024: int(16 * cm)}
        convs = [ConvLayer(3, widths[size], 1, blur_kernel=blur_kernel)]
        width = widths[size]
        for i in range(int(math.log(size, 2)), 2, -1):
            nxt = widths[2 ** (i - 1)]
            convs.append(ResBlock(width, nxt, downsample=True, blur_kernel=blur_kernel))
            width = nxt
        self.convs = nn.Sequential(*convs)
        self.final_conv = ConvLayer(width, widths[4], 3, blur_kernel=blur_kernel)
        self.final_linear = nn.Sequential(
            EqualLinear(widths[4] * 4 * 4, widths[4], activation="fused_lrelu"),
            EqualLinear(widths[4], 1),
        )

    def forward(self, input):
        out = self.final_conv(self.convs(input))
        return self.final_linear(out.reshape(out.shape[0], -1))


class CooccurenceDiscriminator(nn.Module):
    """Dco: patch vs. averaged reference-patch features -> logit."""

    WIDTHS = (2, 4, 8, 12, 12, 24)
    DOWN = (True, True, True, True, True, False)

    def __init__(self, channel, size=256):
        super().__init__()
        encoder = [ConvLayer(3, channel, 1)]
        width = channel
        for mult, down in zip(self.WIDTHS, self.DOWN):
            encoder.append(ResBlock(width, channel * mult, down))
            width = channel * mult
        k_size, feat_size = (3, 2 * 2) if size > 511 else (2, 1 * 1)
        encoder.append(ConvLayer(width, channel * 12, k_size, padding="valid"))
        self.encoder = nn.Sequential(*encoder)
        self.linear = nn.Sequential(
            EqualLinear(channel * 12 * 2 * feat_size, channel * 32, activation="fused_lrelu"),
            EqualLinear(channel * 32, channel * 32, activation="fused_lrelu"),
            EqualLinear(channel * 32, channel * 16, activation="fused_lrelu"),
            EqualLinear(channel * 16, 1),
        )

    def encode_many(self, *batches):
        """One encoder pass per patch batch (the G phase and R1: one batch needs an input gradient, the other does not; the D phase
        merges its batches in forward_pair)."""
        return tuple(self.encoder(b) for b in batches)

    @staticmethod
    def _ref_mean(ref, ref_batch):
        _, c, h, w = ref.shape
        return ref.reshape(-1, ref_batch, c, h, w).mean(1)

    def forward(self, input, reference=None, ref_batch=None, ref_input=None):
        if ref_input is None:
            out_input, ref = self.encode_many(input, reference)
            ref_input = self._ref_mean(ref, ref_batch)
        else:
            out_input = self.encoder(input)
        out = torch.flatten(torch.cat((out_input, ref_input), 1), 1)
        return self.linear(out), ref_input

    def forward_pair(self, fake, real, reference, ref_batch):
        """``(forward(fake, reference, ref_batch)[0], forward(real, ref_input=...)[0], ref_input)`` -- the two calls of the D phase
        (train.py:88-90) -- with ONE encoder pass over the fake, the real and the reference patches (8B + 8B + 32B samples: the encoder
        has no cross-sample op, so every sample's features are those of a separate pass) and one pass of the linear head.  In the D
        phase no patch batch needs an input gradient, so nothing is computed that three passes would not compute; what changes is the
        launch size: the 8B-sample passes ran their layers at 0.69 of the 32B pass's per-sample rate (tools/probes/dco_census.py).
        Same box, two interleaved runs (profiles/r06_dco_merge_ab.txt, r06_dco_merge3_ab.txt): three passes 400.1 ms, fake + real
        merged 397.8 / 395.8, all three merged 394.5; bf16 150.5 / 148.7 / 147.0.  (Round 3 measured the full merge 0.8 % SLOWER in
        f32 -- on that round's kernels; IDEAS_DCO_MERGE=0 / 1 restore three passes / the fake + real merge for A/B runs.)"""
        mode = DCO_MERGE
        plain = not fake.requires_grad and not real.requires_grad and not reference.requires_grad and fake.shape[1:] == real.shape[1:] == reference.shape[1:]
        nf, nr = fake.shape[0], real.shape[0]
        if plain and mode == "2":
            out = self.encoder(torch.cat((fake, real, reference), 0))
            out_fr, ref = out[:nf + nr], out[nf + nr:]
        elif plain and mode == "1":
            out_fr = self.encoder(torch.cat((fake, real), 0))
            (ref,) = self.encode_many(reference)
        else:
            out_f, out_r, ref = self.encode_many(fake, real, reference)
            out_fr = torch.cat((out_f, out_r), 0)
        ref_input = self._ref_mean(ref, ref_batch)
        pred = self.linear(torch.flatten(torch.cat((out_fr, torch.cat((ref_input, ref_input), 0)), 1), 1))
        return pred[:nf], pred[nf:], ref_input


class DistributionDiscriminator(nn.Module):
    """Ddist: texture code -> logit; four EqualLinear + lrelu (the last one too)."""

    def __init__(self, texture_channel=2048):
        super().__init__()
        t = texture_channel
        self.model = nn.Sequential(
            EqualLinear(t, t // 4, activation="fused_lrelu"),
            EqualLinear(t // 4, t // 16, activation="fused_lrelu"),
            EqualLinear(t // 16, t // 64, activation="fused_lrelu"),
            EqualLinear(t // 64, 1, activation="fused_lrelu"),
        )

    def forward(self, input):
        return self.model(input)


class TensorExtractor(nn.Module):
    """Ex: recovered structure -> secret tensor estimate; its sign carries the bit decision."""

    def __init__(self, channel, N=1, structure_channel=8, blur_kernel=(1, 3, 3, 1)):
        super().__init__()
        c = channel
        self.extract = nn.Sequential(
            ConvLayer(structure_channel, c * 2, 1, blur_kernel=blur_kernel),
            ResBlock(c * 2, c * 4, downsample=False, padding="reflect", blur_kernel=blur_kernel),
            ResBlock(c * 4, c * 2, downsample=False, padding="reflect", blur_kernel=blur_kernel),
            ResBlock(c * 2, c, downsample=False, padding="reflect", blur_kernel=blur_kernel),
            ConvLayer(c, N, 1, blur_kernel=blur_kernel),
        )

    def forward(self, input):
        return to_f32(self.extract(input))


_FACTORY = {
    "DisentanglementEncoder": lambda a: DisentanglementEncoder(a.channel, a.structure_channel, a.texture_channel, a.blur_kernel),
    "Generator": lambda a: Generator(a.channel, a.structure_channel, a.texture_channel, a.blur_kernel),
    "StructureGenerator": lambda a: StructureGenerator(a.channel, a.N, a.structure_channel, a.blur_kernel),
    "ImageLevelDiscriminator": lambda a: ImageLevelDiscriminator(a.image_size, a.channel_multiplier, a.blur_kernel),
    "CooccurenceDiscriminator": lambda a: CooccurenceDiscriminator(a.channel, a.image_size),
    "DistributionDiscriminator": lambda a: DistributionDiscriminator(a.texture_channel),
    "TensorExtractor": lambda a: TensorExtractor(a.channel, a.N, a.structure_channel, a.blur_kernel),
}


def init_model(model: str, args):
    """Factory with the reference's names and ``args`` namespace (models.py:468-513)."""
    try:
        return _FACTORY[model](args)
    except KeyError:
        raise NotImplementedError(model) from None
