"""Using a trained IDEAS checkpoint for its purpose: hide a payload in synthesised images, get it back from image files, and measure
the extraction accuracy (and FID) per jitter width -- the sender / receiver block of train.py:249-286 as a product surface.

    sender     bits -> Z (ideas_bits_to_tensor) -> S2 = Gstru(Z) -> image = G(S2, T2) -> 8-bit file (ideas_image_f32_to_u8)
    receiver   8-bit file -> image (data.u8_to_f32) -> S2' = E(image) -> Z' = Ex(S2') -> bits (ideas_tensor_to_bits)

Messages are PACKED bits (``ideas_amd.op.stego``): uint8 ``[B, capacity_bits / 8]``.  The networks are the EMA copies of a checkpoint
(``load_models``) or of a trainer (``models_of``).  ``frame`` / ``unframe`` put a byte payload into whole images: a 4-byte big-endian
length, the CRC32 of the payload, the payload, random padding.  Everything on the device runs under ``no_grad``.

With a ``Code`` of ``ideas_amd.ecc`` the framed rows are the INFORMATION bits of one codeword per image (``frame_coded``), the receiver
decodes them from soft values of ``hat_Z`` (``extract_coded``), and ``evaluate(code=...)`` counts what survives the decoder.
"""
from __future__ import annotations

import struct
import zlib
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, checkpoint, data, ecc, fid
from .op import stego as S

NETS = ("E", "G", "Gstru", "Ex")
HEADER = 8          # frame: 4 bytes length + 4 bytes CRC32


class PayloadError(ValueError):
    """The extracted rows do not hold a framed payload: impossible length or CRC mismatch."""


def models_of(trainer, ema: bool = True) -> Dict[str, torch.nn.Module]:
    """The four networks of the sender / receiver out of a trainer dict (``train_step.build_trainer``)."""
    return {n: trainer[n + ("_ema" if ema else "")] for n in NETS}


def load_models(ckpt_path: str, device):
    """``(models, args)`` of a checkpoint in the reference's format: E_ema, G_ema, Gstru_ema and Ex_ema built from ``ckpt["args"]``,
    loaded, moved to ``device``, in eval mode."""
    from .models import init_model
    from .train_step import NET_CLASSES
    args = torch.load(ckpt_path, map_location="cpu", weights_only=False)["args"]
    nets = {n + "_ema": init_model(NET_CLASSES[n], args) for n in NETS}
    checkpoint.load(ckpt_path, nets)
    return {n: nets[n + "_ema"].to(device).eval() for n in NETS}, args


def structure_side(args) -> int:
    return int(args.image_size) // 16


def capacity_bits(args, sigma: int) -> int:
    """Message bits one image carries: N * (image_size / 16)^2 elements of sigma bits."""
    return int(args.N) * structure_side(args) ** 2 * int(sigma)


def _rand(shape, generator: Optional[torch.Generator], device) -> torch.Tensor:
    """U[0,1) f32 on ``device``; a generator of another device (a CPU generator for a GPU run) draws there and the result is copied."""
    device = torch.device(device)
    if generator is None or generator.device.type == device.type:
        return torch.rand(shape, generator=generator, device=device)
    return torch.rand(shape, generator=generator, device=generator.device).to(device)


def random_bits(batch: int, n_bits: int, generator: Optional[torch.Generator], device) -> torch.Tensor:
    """Packed uniform bits uint8 ``[batch, ceil(n_bits / 8)]`` with zero pad bits."""
    device = torch.device(device)
    nbytes = S.packed_bytes(n_bits)
    where = device if generator is None or generator.device.type == device.type else generator.device
    bits = torch.randint(0, 256, (batch, nbytes), generator=generator, device=where, dtype=torch.uint8).to(device)
    if n_bits % 8:
        bits[:, -1] &= (0xFF00 >> (n_bits % 8)) & 0xFF
    return bits


@torch.no_grad()
def hide(models, args, bits: torch.Tensor, sigma: int, delta: float, texture: Optional[torch.Tensor] = None,
         jitter: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None):
    """Packed ``bits`` [B, capacity_bits / 8] -> ``(images, Z)``: the containers [B, 3, R, R] and the secret tensor [B, N, R/16, R/16]
    they were grown from.  ``texture``: the texture codes [B, texture_channel] (default: U(-1, 1), train.py:263); ``jitter``: U[0,1)
    [B, N * (R/16)^2] (default with ``delta > 0``: drawn from ``generator``, before the texture)."""
    _lib.require_cuda(bits, texture, jitter)
    side = structure_side(args)
    L = int(args.N) * side * side
    b = bits.shape[0]
    Z = S.bits_to_tensor(bits, L, sigma, delta, jitter=jitter, generator=generator).reshape(b, int(args.N), side, side)
    if texture is None:
        texture = _rand((b, int(args.texture_channel)), generator, bits.device) * 2 - 1
    images = models["G"](models["Gstru"](Z), texture)
    return images, Z


@torch.no_grad()
def extract(models, args, images: torch.Tensor, sigma: int, ref_bits: Optional[torch.Tensor] = None):
    """``images``: float32 / bfloat16 [B, 3, R, R] in [-1, 1], or uint8 [B, R, R, 3] as decoded from image files (normalised on the
    device by ``data.u8_to_f32``).  Returns ``(bits, hat_Z)``, or ``(bits, hat_Z, n_err)`` with ``ref_bits``: the packed decisions, the
    extractor's output [B, N, R/16, R/16], and per image the number of message bits that differ from ``ref_bits``."""
    _lib.require_cuda(images, ref_bits)
    if images.dtype == torch.uint8:
        images = data.u8_to_f32(images.contiguous())
    hat_S, _ = models["E"](images)
    hat_Z = models["Ex"](hat_S)
    out = S.tensor_to_bits(hat_Z.reshape(hat_Z.shape[0], -1), sigma, ref=ref_bits)
    if ref_bits is None:
        return out, hat_Z
    return out[0], hat_Z, out[1]


def _decode_coded(hat_Z: torch.Tensor, sigma: int, code: "ecc.Code"):
    return ecc.decode(code, ecc.soft_bits(hat_Z.reshape(hat_Z.shape[0], -1), sigma))


@torch.no_grad()
def extract_coded(models, args, images: torch.Tensor, sigma: int, code: "ecc.Code"):
    """``extract`` for containers that carry codewords of ``code`` (``frame_coded``): ``(info_rows, hat_Z, metric)``, the decoded
    information rows uint8 [B, code.k_bytes], the extractor's output, and the decoder's final metric int32 [B]."""
    _lib.require_cuda(images)
    if code.n_bits != capacity_bits(args, sigma):
        raise ValueError(f"extract_coded: the code is planned for {code.n_bits} message bits, an image carries {capacity_bits(args, sigma)}")
    if images.dtype == torch.uint8:
        images = data.u8_to_f32(images.contiguous())
    hat_S, _ = models["E"](images)
    hat_Z = models["Ex"](hat_S)
    info, metric = _decode_coded(hat_Z, sigma, code)
    return info, hat_Z, metric


# ---------------------------------------------------------------------------------------------------------------- payload framing
def frame(payload: bytes, capacity_bytes: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """``payload`` -> uint8 [n_img, capacity_bytes] (CPU): length (4 bytes, big-endian), ``zlib.crc32(payload)`` (4 bytes, big-endian),
    the payload, then padding bytes drawn from ``generator`` up to a whole number of images (at least one)."""
    capacity_bytes = int(capacity_bytes)
    if capacity_bytes <= 0:
        raise ValueError("frame: capacity_bytes must be positive")
    payload = bytes(payload)
    if len(payload) >= 1 << 32:
        raise ValueError("frame: the payload length does not fit in 4 bytes")
    body = struct.pack(">II", len(payload), zlib.crc32(payload) & 0xFFFFFFFF) + payload
    n_img = max(1, -(-len(body) // capacity_bytes))
    rows = torch.randint(0, 256, (n_img * capacity_bytes,), generator=generator, dtype=torch.uint8)
    rows[:len(body)] = torch.frombuffer(bytearray(body), dtype=torch.uint8)
    return rows.view(n_img, capacity_bytes)


def frame_coded(payload: bytes, code: "ecc.Code", generator: Optional[torch.Generator] = None, device="cuda") -> torch.Tensor:
    """``frame(payload, code.k_bytes, generator)`` encoded: packed message rows uint8 [n_img, ceil(code.n_bits / 8)] on ``device``, one
    codeword per image; the message bits the codewords do not reach are drawn from ``generator`` after the frame's padding."""
    rows = frame(payload, code.k_bytes, generator).to(device)
    return ecc.encode(code, rows, fill=random_bits(rows.shape[0], code.n_bits, generator, device))


def unframe(rows) -> bytes:
    """The payload of rows written by ``frame`` (uint8 [n_img, capacity_bytes], tensor or array).  ``PayloadError``: fewer than 8
    bytes, a length that does not fill exactly this many rows, or a CRC mismatch."""
    arr = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    if arr.dtype != np.uint8 or arr.ndim != 2:
        raise PayloadError("unframe expects uint8 rows [n_img, capacity_bytes]")
    n_img, cap = arr.shape
    flat = arr.tobytes()
    if len(flat) < HEADER:
        raise PayloadError(f"{len(flat)} bytes cannot hold the {HEADER}-byte header")
    length, crc = struct.unpack(">II", flat[:HEADER])
    if max(1, -(-(HEADER + length) // cap)) != n_img:
        raise PayloadError(f"bad length: the header announces {length} payload bytes, which do not fill {n_img} image(s) of {cap} bytes")
    payload = flat[HEADER:HEADER + length]
    if zlib.crc32(payload) & 0xFFFFFFFF != crc:
        raise PayloadError("CRC mismatch: the extracted bits are not the hidden payload")
    return payload


# ---------------------------------------------------------------------------------------------------------------------- evaluation
@torch.no_grad()
def evaluate(models, args, sigma: int, delta: float, n_sample: int, batch: int, generator: Optional[torch.Generator] = None,
             container: str = "u8", inception=None, attack=None, code: Optional["ecc.Code"] = None) -> dict:
    """Extraction accuracy over ``n_sample`` containers carrying random bits: ``n_sample // batch`` full batches and the remainder (a
    zero remainder is skipped).  Per batch, in this order of draws from ``generator``: the bits, the jitter, the texture codes.
    ``container``: ``"u8"`` sends every image through 8 bits (``quantize_image``), ``"float"`` hands the generator's output to the
    receiver unrounded.  With ``inception`` (``ideas_amd.inception.InceptionV3([3], normalize_input=False)``) the feature statistics of
    the received containers are accumulated too (``fid.feature_statistics``).  ``attack`` (``ideas_amd.attacks.parse(spec)``; None:
    the lossless file) is the channel the 8-bit container travels through: the receiver sees
    ``attack(quantize_image(images)[0], generator)[1]``, the attack's draws come after the texture codes of the same batch, and the
    feature statistics are taken on what the receiver sees.  One host synchronisation, at the end.

    With ``code`` (``ideas_amd.ecc.Code(capacity_bits(args, sigma), rate)``) every container carries one codeword: per batch the draws
    are ``code.k_bytes`` of information per image, the fill bits, then the jitter and the texture codes as above.  ``acc`` / ``n_err``
    then count the channel's errors against the CODED bits, and the soft-decision decoder runs on ``hat_Z``.

    Returns ``acc`` (1 - n_err / n_bits), ``n_bits``, ``n_err``, ``l1`` (mean |hat_Z - Z|), ``stats`` (``fid.FeatureStats`` or None)
    and ``attack`` (the attack's name or None); with ``code`` also ``info_acc`` (1 - n_info_err / n_info_bits), ``n_info_bits``,
    ``n_info_err``, ``n_row_err`` (images with any wrong information bit) and ``rate``."""
    if container not in ("u8", "float"):
        raise ValueError(f"evaluate: container must be 'u8' or 'float', got {container!r}")
    if attack is not None and container != "u8":
        raise ValueError("evaluate: an attack acts on the 8-bit container; container must be 'u8'")
    if n_sample <= 0 or batch <= 0:
        raise ValueError("evaluate: n_sample and batch must be positive")
    device = next(models["G"].parameters()).device
    cap = capacity_bits(args, sigma)
    if code is not None and code.n_bits != cap:
        raise ValueError(f"evaluate: the code is planned for {code.n_bits} message bits, an image carries {cap}")
    err = torch.zeros((), device=device, dtype=torch.int64)
    l1 = torch.zeros((), device=device, dtype=torch.float64)
    info_err = torch.zeros((), device=device, dtype=torch.int64)
    row_err = torch.zeros((), device=device, dtype=torch.int64)

    def batches():
        for b in [batch] * (n_sample // batch) + [n_sample % batch]:
            if b == 0:
                continue
            if code is None:
                bits = random_bits(b, cap, generator, device)
            else:
                info = random_bits(b, code.k_bits, generator, device)
                bits = ecc.encode(code, info, generator=generator)
            images, Z = hide(models, args, bits, sigma, delta, generator=generator)
            if attack is not None:
                received = attack(S.quantize_image(images, dequantize=False)[0], generator)[1]
            else:
                received = S.quantize_image(images)[1] if container == "u8" else images
            _, hat_Z, n_err = extract(models, args, received, sigma, ref_bits=bits)
            err.add_(n_err.sum())
            l1.add_((hat_Z.float() - Z).abs().sum(dtype=torch.float64))
            if code is not None:
                wrong = S.unpack_bits(_decode_coded(hat_Z, sigma, code)[0] ^ info, code.k_bits).sum(1)     # per image, exact in f32
                info_err.add_(wrong.sum(dtype=torch.int64))
                row_err.add_((wrong > 0).sum())
            yield received

    stats = None
    if inception is not None:
        stats = fid.feature_statistics(batches(), inception)
    else:
        for _ in batches():
            pass
    n_bits = n_sample * cap
    if code is None:
        n_err, l1_sum = int(err.item()), float(l1.item())
    else:                                                     # still one synchronisation: the four sums cross together
        n_err, l1_sum, n_info_err, n_row_err = torch.stack((err.double(), l1, info_err.double(), row_err.double())).tolist()
        n_err, n_info_err, n_row_err = int(n_err), int(n_info_err), int(n_row_err)
    res = {"acc": 1.0 - n_err / n_bits, "n_bits": n_bits, "n_err": n_err, "l1": l1_sum / (n_sample * cap // int(sigma)),
           "stats": stats, "attack": None if attack is None else attack.name}
    if code is not None:
        n_info = n_sample * code.k_bits
        res.update(info_acc=1.0 - n_info_err / n_info, n_info_bits=n_info, n_info_err=n_info_err, n_row_err=n_row_err, rate=code.rate)
    return res
