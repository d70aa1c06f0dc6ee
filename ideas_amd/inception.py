"""The FID Inception-v3 (the reference's stylegan2/inception.py: pytorch-fid's port of TensorFlow's ``inception-2015-12-05``) on
the HIP ops.

``InceptionV3([3], normalize_input=False)`` is what stylegan2/calc_inception.py and fid.py build: the network up to the final
average pool, returning the feature maps of the selected blocks.  Every conv + BatchNorm + ReLU layer (94 of them) is ONE
``op.conv2d_bias_act(negative_slope=0, scale=1)`` on weights with the eval-mode BatchNorm folded in; the 1x7 / 7x1 / 1x3 / 3x1 layers
use the conv family's rectangular padding; the fourteen 3x3 pools run on ``op.pool3x3`` and the final average on
``op.global_avg_pool``; the bilinear resize to 299x299 is ``patch_resize`` with one whole-image box.  The network always runs with
f32 activations (the metric is not a mixed-precision quantity) and without autograd.

No weights are shipped or fetched: ``weights`` is a path to, or a dict of, the ``pt_inception-2015-12-05-6726825d.pth`` state dict of
pytorch-fid (the keys and shapes of torchvision's ``inception_v3(num_classes=1008, aux_logits=False)``; ``fc.*`` is loaded and not
used).  torchvision's own ImageNet Inception (``use_fid_inception=False``) and fine-tuning (``requires_grad=True``) are not
implemented.
"""
from __future__ import annotations

from typing import Dict, List

import torch
from torch import nn

from . import op, precision
from .op import pool as P
from .op.patchify import patch_resize

FID_WEIGHTS_FILE = "pt_inception-2015-12-05-6726825d.pth"
BN_EPS = 0.001
CL = torch.channels_last


def fold_bn(conv_weight, bn_weight, bn_bias, running_mean, running_var, eps: float = BN_EPS):
    """Eval-mode ``bn(conv(x, w))`` as ``conv(x, w') + b'``: ``w' = w * s``, ``b' = beta - mean * s`` with ``s = gamma / sqrt(var +
    eps)`` per output channel, computed in f64 (-> f64 tensors; the caller rounds once)."""
    s = bn_weight.double() / torch.sqrt(running_var.double() + eps)
    return conv_weight.double() * s.view(-1, 1, 1, 1), bn_bias.double() - running_mean.double() * s


class BasicConv2d(nn.Module):
    """conv (no bias) -> BatchNorm(eps = 0.001, eval statistics) -> ReLU as one kernel.  ``conv`` and ``bn`` hold the parameters
    under torchvision's names and are never called; the folded weight (channels_last, f32) and bias are cached until a parameter or
    statistic changes (``load_state_dict``, a move to another device)."""

    def __init__(self, cin: int, cout: int, kernel_size, stride: int = 1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size=kernel_size, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=BN_EPS)
        self.stride = stride
        self.padding = padding
        self._folded = None

    def _key(self):
        ts = (self.conv.weight, self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var)
        return tuple((t.data_ptr(), t._version) for t in ts) + (str(self.conv.weight.device),)

    def folded(self):
        key = self._key()
        if self._folded is None or self._folded[0] != key:
            with torch.no_grad():
                w, b = fold_bn(self.conv.weight, self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var, self.bn.eps)
                self._folded = (key, w.float().contiguous(memory_format=CL), b.float().contiguous())
        return self._folded[1], self._folded[2]

    def forward(self, x):
        w, b = self.folded()
        return op.conv2d_bias_act(x, w, b, stride=self.stride, padding=self.padding, negative_slope=0.0, scale=1.0)


class _Mixed(nn.Module):
    pool3x3 = staticmethod(P.pool3x3)         # (an attribute so that tools/bench_fid.py can time the torch composition in its place)


class InceptionA(_Mixed):
    def __init__(self, cin: int, pool_features: int):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 64, 1)
        self.branch5x5_1 = BasicConv2d(cin, 48, 1)
        self.branch5x5_2 = BasicConv2d(48, 64, 5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, 1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, 3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, 3, padding=1)
        self.branch_pool = BasicConv2d(cin, pool_features, 1)

    def forward(self, x):
        b1 = self.branch1x1(x)
        b5 = self.branch5x5_2(self.branch5x5_1(x))
        b3 = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        bp = self.branch_pool(self.pool3x3(x, P.AVG_S1P1_VALID))
        return torch.cat([b1, b5, b3, bp], 1)


class InceptionB(_Mixed):
    def __init__(self, cin: int):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, 384, 3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, 1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, 3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, 3, stride=2)

    def forward(self, x):
        b3 = self.branch3x3(x)
        bd = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        return torch.cat([b3, bd, self.pool3x3(x, P.MAX_S2)], 1)


class InceptionC(_Mixed):
    def __init__(self, cin: int, channels_7x7: int):
        super().__init__()
        c = channels_7x7
        self.branch1x1 = BasicConv2d(cin, 192, 1)
        self.branch7x7_1 = BasicConv2d(cin, c, 1)
        self.branch7x7_2 = BasicConv2d(c, c, (1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c, 192, (7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(cin, c, 1)
        self.branch7x7dbl_2 = BasicConv2d(c, c, (7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c, c, (1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c, c, (7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c, 192, (1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(cin, 192, 1)

    def forward(self, x):
        b1 = self.branch1x1(x)
        b7 = self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)))
        bd = self.branch7x7dbl_5(self.branch7x7dbl_4(self.branch7x7dbl_3(self.branch7x7dbl_2(self.branch7x7dbl_1(x)))))
        bp = self.branch_pool(self.pool3x3(x, P.AVG_S1P1_VALID))
        return torch.cat([b1, b7, bd, bp], 1)


class InceptionD(_Mixed):
    def __init__(self, cin: int):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(cin, 192, 1)
        self.branch3x3_2 = BasicConv2d(192, 320, 3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, 192, 1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, (1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, (7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, 3, stride=2)

    def forward(self, x):
        b3 = self.branch3x3_2(self.branch3x3_1(x))
        b7 = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        return torch.cat([b3, b7, self.pool3x3(x, P.MAX_S2)], 1)


class InceptionE(_Mixed):
    """``pool_mode``: ``AVG_S1P1_VALID`` for Mixed_7b (FIDInceptionE_1), ``MAX_S1P1`` for Mixed_7c (FIDInceptionE_2: the max pool
    of the TensorFlow graph the FID statistics were defined on)."""

    def __init__(self, cin: int, pool_mode: int):
        super().__init__()
        self.pool_mode = pool_mode
        self.branch1x1 = BasicConv2d(cin, 320, 1)
        self.branch3x3_1 = BasicConv2d(cin, 384, 1)
        self.branch3x3_2a = BasicConv2d(384, 384, (1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, (3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, 448, 1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, 3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, (1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, (3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, 192, 1)

    def forward(self, x):
        b1 = self.branch1x1(x)
        a = self.branch3x3_1(x)
        d = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        bp = self.branch_pool(self.pool3x3(x, self.pool_mode))
        return torch.cat([b1, self.branch3x3_2a(a), self.branch3x3_2b(a), self.branch3x3dbl_3a(d), self.branch3x3dbl_3b(d), bp], 1)


def _load(obj) -> Dict[str, torch.Tensor]:
    if isinstance(obj, dict):
        return obj
    state = torch.load(obj, map_location="cpu")
    if not isinstance(state, dict):
        raise RuntimeError(f"weights: {obj} does not hold a state dict")
    return state


class InceptionV3(nn.Module):
    """The reference's ``InceptionV3`` (stylegan2/inception.py:16-163): ``forward`` returns the list of the selected block outputs,
    ascending.  Block 0 ends in the first max pool [B, 64, 73, 73], block 1 in the second [B, 192, 35, 35], block 2 is Mixed_5b ..
    Mixed_6e [B, 768, 17, 17], block 3 Mixed_7a .. Mixed_7c and the global average [B, 2048, 1, 1] (sizes for a 299x299 input)."""

    DEFAULT_BLOCK_INDEX = 3
    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}

    def __init__(self, output_blocks=(DEFAULT_BLOCK_INDEX,), resize_input: bool = True, normalize_input: bool = True,
                 requires_grad: bool = False, use_fid_inception: bool = True, weights=None):
        super().__init__()
        if not use_fid_inception:
            raise NotImplementedError("InceptionV3(use_fid_inception=False), torchvision's ImageNet Inception, is not implemented: "
                                      "FID is defined on the FID Inception weights")
        if requires_grad:
            raise NotImplementedError("InceptionV3(requires_grad=True) is not implemented: the network is frozen and forward-only")
        if weights is None:
            raise RuntimeError(f"InceptionV3 needs weights and ships none: pass weights= (the {FID_WEIGHTS_FILE} state dict of "
                               "pytorch-fid, or its path)")
        self.resize_input = resize_input
        self.normalize_input = normalize_input
        self.output_blocks = sorted(output_blocks)
        self.last_needed_block = max(output_blocks)
        assert self.last_needed_block <= 3, "Last possible output block index is 3"
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, 3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, 3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, 3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, 1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, 3)
        self.Mixed_5b = InceptionA(192, 32)
        self.Mixed_5c = InceptionA(256, 64)
        self.Mixed_5d = InceptionA(288, 64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, 128)
        self.Mixed_6c = InceptionC(768, 160)
        self.Mixed_6d = InceptionC(768, 160)
        self.Mixed_6e = InceptionC(768, 192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280, P.AVG_S1P1_VALID)
        self.Mixed_7c = InceptionE(2048, P.MAX_S1P1)
        self.fc = nn.Linear(2048, 1008)          # (part of the file's state dict; the features stop before it)
        self.pool3x3 = P.pool3x3                 # (attributes, as _Mixed.pool3x3)
        self.global_avg_pool = P.global_avg_pool
        self.load_state_dict(_load(weights), strict=True)
        for p in self.parameters():
            p.requires_grad = False
        self.eval()

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        res = super().load_state_dict(state_dict, strict=strict, **kw)
        for m in self.modules():
            if isinstance(m, BasicConv2d):
                m._folded = None
        return res

    def _blocks(self):
        yield lambda x: self.pool3x3(self.Conv2d_2b_3x3(self.Conv2d_2a_3x3(self.Conv2d_1a_3x3(x))), P.MAX_S2)
        yield lambda x: self.pool3x3(self.Conv2d_4a_3x3(self.Conv2d_3b_1x1(x)), P.MAX_S2)

        def block2(x):
            for m in (self.Mixed_5b, self.Mixed_5c, self.Mixed_5d, self.Mixed_6a, self.Mixed_6b, self.Mixed_6c, self.Mixed_6d,
                      self.Mixed_6e):
                x = m(x)
            return x
        yield block2
        yield lambda x: self.global_avg_pool(self.Mixed_7c(self.Mixed_7b(self.Mixed_7a(x))))

    def forward(self, inp: torch.Tensor) -> List[torch.Tensor]:
        """``inp`` [B, 3, H, W], in (0, 1) with ``normalize_input`` and in (-1, 1) without -> the selected block outputs, float32."""
        if inp.dim() != 4 or inp.shape[1] != 3:
            raise RuntimeError(f"InceptionV3 expects a [B, 3, H, W] tensor, got {tuple(inp.shape)}")
        outp = []
        with torch.no_grad(), precision.activations(torch.float32):
            x = inp.detach().float()
            if self.resize_input and tuple(x.shape[2:]) != (299, 299):
                x = patch_resize(x, [(0, 0, x.shape[2], x.shape[3])], (299, 299))
            if self.normalize_input:
                x = 2 * x - 1
            for idx, block in enumerate(self._blocks()):
                x = block(x)
                if idx in self.output_blocks:
                    outp.append(x)
                if idx == self.last_needed_block:
                    break
        return outp
