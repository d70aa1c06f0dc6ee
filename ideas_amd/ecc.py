"""Forward error correction for the payload: between ``stego.frame`` and the secret tensor on the way in, between the extractor's output
and ``stego.unframe`` on the way out.  Every image is one zero-terminated codeword of the K = 7 convolutional code 171 / 133 (octal),
punctured to rate 1/2, 2/3 or 3/4 and interleaved over the image's message bits, so images stay independently decodable; the decoder is
a soft-decision Viterbi that reads reliabilities straight from ``hat_Z``.  DESIGN.md "Payload coding" defines every step.

    code = Code(stego.capacity_bits(args, sigma), "1/2")
    coded = encode(code, info)                     # uint8 [B, code.k_bytes] -> packed message rows for stego.hide
    info, metric = decode(code, soft_bits(hat_Z.reshape(B, -1), sigma))

Device tensors only; everything stays on the device and nothing synchronises.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from .op import ecc as E

RATES = {"1/2": E.RATE_1_2, "2/3": E.RATE_2_3, "3/4": E.RATE_3_4}
# per rate: which outputs (c0, c1) every step of a puncturing period keeps; 3/4 is c0: 1 1 0, c1: 1 0 1
_MASKS = {"1/2": ((1, 1),), "2/3": ((1, 1), (1, 0)), "3/4": ((1, 1), (1, 0), (0, 1))}
MAX_STEPS = 1 << 20


def kept_outputs(steps: int, rate: str) -> int:
    """m(T): the outputs of ``steps`` trellis steps that survive the puncturing of ``rate``."""
    masks = _MASKS[rate]
    full, part = divmod(int(steps), len(masks))
    return full * sum(map(sum, masks)) + sum(map(sum, masks[:part]))


def stride_of(n_bits: int) -> int:
    """The interleaver's stride: the first integer >= max(1, 3 n // 8) that is coprime to n."""
    p = max(1, 3 * n_bits // 8)
    while math.gcd(p, n_bits) != 1:
        p += 1
    return p


class Code:
    """The plan for images of ``n_bits`` message bits at ``rate`` ("1/2", "2/3", "3/4"): ``k_bits`` information bits (the largest
    multiple of 8 whose codeword fits; ``k_bytes`` bytes), ``steps`` = k_bits + 6 trellis steps, ``coded_bits`` = m(steps) kept outputs,
    and the interleaver's ``stride`` with its inverse modulo n_bits, ``stride_inv``.  ``ValueError``: an unknown rate, or an image too
    small for one byte."""

    def __init__(self, n_bits: int, rate: str):
        if rate not in RATES:
            raise ValueError(f"ecc: unknown rate {rate!r} (known: {', '.join(RATES)})")
        n_bits = int(n_bits)
        k = 0
        while k + 8 + E.TAIL <= MAX_STEPS and kept_outputs(k + 8 + E.TAIL, rate) <= n_bits:
            k += 8
        if k < 8:
            raise ValueError(f"ecc: an image of {n_bits} message bits is too small for rate {rate} "
                             f"(one byte needs {kept_outputs(8 + E.TAIL, rate)})")
        self.n_bits, self.rate, self.rate_id = n_bits, rate, RATES[rate]
        self.k_bits, self.k_bytes, self.steps = k, k // 8, k + E.TAIL
        self.coded_bits = kept_outputs(self.steps, rate)
        self.stride = stride_of(n_bits)
        self.stride_inv = pow(self.stride, -1, n_bits)

    def __repr__(self) -> str:
        return f"Code(n_bits={self.n_bits}, rate={self.rate!r}: k_bits={self.k_bits}, coded_bits={self.coded_bits}, stride={self.stride})"


def encode(code: Code, info: torch.Tensor, fill: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None
           ) -> torch.Tensor:
    """``info`` uint8 [B, code.k_bytes] -> packed message rows uint8 [B, ceil(n_bits / 8)] for ``stego.hide``.  The message bits the
    codeword does not reach take ``fill`` (packed rows of the output's shape); without it they are drawn from ``generator``
    (``stego.random_bits``), and are 0 when neither is given."""
    if fill is None and generator is not None:
        from .stego import random_bits
        fill = random_bits(info.shape[0], code.n_bits, generator, info.device)
    return E.ecc_encode(info, code.n_bits, code.k_bits, code.rate_id, code.stride, code.stride_inv, fill)


def soft_bits(z: torch.Tensor, sigma: int, gain: float = 64.0) -> torch.Tensor:
    """The extractor's output ``[B, L]`` -> int8 ``[B, L * sigma]``, one soft value per message bit, positive favours 1."""
    return E.ecc_soft(z, sigma, gain)


def decode(code: Code, soft: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """int8 ``[B, n_bits]`` -> ``(info, metric)``: the decoded rows uint8 [B, code.k_bytes] and the winning path's metric int32 [B]
    (the larger, the closer the soft values are to a codeword).  Codewords above ``op.ecc.LDS_STEPS`` steps get a workspace."""
    ws = None
    if code.steps > E.LDS_STEPS:
        ws = torch.empty((soft.shape[0], code.steps), device=soft.device, dtype=torch.int64)
    return E.ecc_viterbi(soft, code.n_bits, code.k_bits, code.rate_id, code.stride, ws)
