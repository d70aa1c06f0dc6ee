"""The channel between sender and receiver as a value: ``parse("noise:3+jpeg:75")`` is a callable ``attack(u8, generator) -> (u8, y)``
on the uint8 ``[B, H, W, C]`` container bytes, built from the kernels of ``ideas_amd.op.attack`` and ``ideas_amd.op.resample``.

    none          the lossless 8-bit file: the input and ``data.u8_to_f32`` of it
    jpeg:Q        a JPEG file of quality Q (integer, 1..100; 4:4:4)
    jpegfile:Q    the JPEG FILE libjpeg / Pillow writes at quality Q with its defaults, exact to the byte: integer DCT, 4:2:0 chroma,
                  triangle upsampler (what ``Image.save(f, "JPEG", quality=Q)`` stores).  ``jpegfile:Q:444`` keeps 4:4:4 chroma
                  (``subsampling=0``); ``jpegfile:Q:420`` is ``jpegfile:Q``
    noise:S       additive Gaussian noise of standard deviation S >= 0, in 8-bit levels
    sp:P          salt and pepper: a fraction P in [0, 1] of the pixels, half black, half white
    gain:G        intensity: contrast G about mid-grey
    offset:D      intensity: D 8-bit levels brighter
    scale:F       rescaling, 0.25 <= F <= 4: Pillow's 8-bit bilinear resize to (max(1, floor(H F + 0.5)), max(1, floor(W F + 0.5))) --
                  the 8-bit image the channel stores -- and back to (H, W)
    gblur:S       Gaussian filtering of standard deviation S pixels, 0 < S <= 4 (ceil(3 S) taps either side, at most 25 in all)
    median:K      median filtering over K x K pixels, K = 3 or 5, edges replicated

Stages chain with ``+`` and run left to right, each on the bytes the one before it wrote; the chain returns the last stage's ``y``.
``attack.name`` is the spec in canonical spelling: ``parse(a.name).name == a.name``.  A bad spec raises ``ValueError`` naming the stage.
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional, Tuple

import torch

from . import data
from .op import attack as A
from .op import resample as S

Stage = Callable[[torch.Tensor, Optional[torch.Generator]], Tuple[torch.Tensor, torch.Tensor]]


def _number(stage: str, text: str) -> float:
    try:
        v = float(text)
    except ValueError:
        v = math.nan
    if not math.isfinite(v):
        raise ValueError(f"attack stage {stage!r}: {text!r} is not a number")
    return v


def _stage(stage: str) -> Tuple[str, Optional[Stage]]:
    """One ``name[:arg]`` -> (canonical name, callable or None for ``none``)."""
    kind, sep, arg = stage.partition(":")
    if kind == "none":
        if sep:
            raise ValueError(f"attack stage {stage!r}: 'none' takes no argument")
        return "none", None
    if kind == "jpegfile":
        return _jpegfile(stage, sep, arg)
    if kind not in ("jpeg", "noise", "sp", "gain", "offset", "scale", "gblur", "median"):
        raise ValueError(f"attack stage {stage!r}: unknown attack {kind!r} (none, jpeg:Q, jpegfile:Q[:444], noise:S, sp:P, gain:G, offset:D, scale:F, "
                         "gblur:S, median:K)")
    if not sep or not arg:
        raise ValueError(f"attack stage {stage!r}: {kind!r} needs an argument, as in '{kind}:VALUE'")
    v = _number(stage, arg)
    if kind == "jpeg":
        if v != int(v) or not 1 <= v <= 100:
            raise ValueError(f"attack stage {stage!r}: the JPEG quality must be an integer in 1..100")
        q = int(v)
        return f"jpeg:{q}", lambda u8, gen: A.jpeg_roundtrip(u8, q)
    if kind == "noise":
        if v < 0:
            raise ValueError(f"attack stage {stage!r}: the noise's sigma must not be negative")
        return f"noise:{v:g}", lambda u8, gen: A.pixel_attack(u8, sigma=v, generator=gen)
    if kind == "sp":
        if not 0 <= v <= 1:
            raise ValueError(f"attack stage {stage!r}: the salt-and-pepper fraction must lie in [0, 1]")
        return f"sp:{v:g}", lambda u8, gen: A.pixel_attack(u8, sp=v, generator=gen)
    if kind == "gain":
        return f"gain:{v:g}", lambda u8, gen: A.pixel_attack(u8, gain=v)
    if kind == "scale":
        if not 0.25 <= v <= 4:
            raise ValueError(f"attack stage {stage!r}: the scale factor must lie in [0.25, 4]")
        return f"scale:{v:g}", lambda u8, gen: _rescale(u8, v)
    if kind == "gblur":
        if not 0 < v <= 4:
            raise ValueError(f"attack stage {stage!r}: the Gaussian's sigma must lie in (0, 4]")
        return f"gblur:{v:g}", lambda u8, gen: S.gaussian_blur_u8(u8, v)
    if kind == "median":
        if v not in (3, 5):
            raise ValueError(f"attack stage {stage!r}: the median window must be 3 or 5")
        k = int(v)
        return f"median:{k}", lambda u8, gen: S.median_u8(u8, k)
    return f"offset:{v:g}", lambda u8, gen: A.pixel_attack(u8, offset=v)


def _jpegfile(stage: str, sep: str, arg: str) -> Tuple[str, Stage]:
    """``jpegfile:Q[:420|:444]``."""
    if not sep or not arg:
        raise ValueError(f"attack stage {stage!r}: 'jpegfile' needs an argument, as in 'jpegfile:75' or 'jpegfile:75:444'")
    text, colon, suffix = arg.partition(":")
    v = _number(stage, text)
    if v != int(v) or not 1 <= v <= 100:
        raise ValueError(f"attack stage {stage!r}: the JPEG quality must be an integer in 1..100")
    if colon and suffix not in ("420", "444"):
        raise ValueError(f"attack stage {stage!r}: the chroma subsampling must be 420 or 444, as in 'jpegfile:75:444'")
    q, sub = int(v), "4:4:4" if suffix == "444" else "4:2:0"
    return f"jpegfile:{q}" + (":444" if suffix == "444" else ""), lambda u8, gen: A.jpeg_file_roundtrip(u8, q, sub)


def _rescale(u8: torch.Tensor, factor: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """To ``factor`` times the size and back, both ways as Pillow's bilinear resize; the image in between is 8-bit.  Two launches."""
    h, w = int(u8.shape[1]), int(u8.shape[2])
    small = (max(1, math.floor(h * factor + 0.5)), max(1, math.floor(w * factor + 0.5)))
    return S.resize_u8(S.resize_u8(u8, small)[0], (h, w))


class Attack:
    """A chain of stages.  ``attack(u8, generator=None) -> (u8, y)``; the stages' draws come from ``generator`` in chain order."""

    def __init__(self, names: List[str], stages: List[Stage]):
        self.name = "+".join(names)
        self._stages = stages

    def __call__(self, u8: torch.Tensor, generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        y = None
        for stage in self._stages:
            u8, y = stage(u8, generator)
        if y is None:                                        # nothing but 'none': the file as written
            y = data.u8_to_f32(u8.contiguous())
        return u8, y

    def __repr__(self) -> str:
        return f"Attack({self.name!r})"


def parse(spec: str) -> Attack:
    """``"none"``, ``"jpeg:75"``, ``"jpegfile:75"``, ``"jpegfile:75:444"``, ``"noise:5"``, ``"sp:0.02"``, ``"gain:0.8"``, ``"offset:20"``, ``"scale:0.5"``, ``"gblur:1"``,
    ``"median:3"`` or a ``+`` chain of them."""
    if not isinstance(spec, str) or not spec.strip():
        raise ValueError(f"attack spec {spec!r}: expected a string such as 'jpeg:75' or 'noise:3+jpeg:75'")
    names, stages = [], []
    for part in spec.split("+"):
        name, fn = _stage(part.strip())
        names.append(name)
        if fn is not None:
            stages.append(fn)
    return Attack(names, stages)
