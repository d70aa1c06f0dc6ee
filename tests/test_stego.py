"""Host-side checks of the steganography surface: the C ABI of csrc/stego.hip and its argument errors, the packed-bit helpers, the
payload frame, the capacity rule, the three command lines' parsers, and the arithmetic the kernels are written to -- restated in numpy
f32, one rounding per step, against the reference's own codec vectors (tests/golden/stego.npz, written by
tests/golden/make_golden_stego.py) and against the torch expression of the 8-bit image write.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, Golden

E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
NAMES = ("ideas_bits_to_tensor", "ideas_tensor_to_bits", "ideas_image_f32_to_u8")


@pytest.fixture(scope="module")
def gold():
    return Golden("stego.npz")


# ------------------------------------------------------------------------------------------------- C ABI and errors
def test_c_abi_declares_and_exports_the_three_entry_points():
    from ideas_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ideas_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
    assert re.search(r"#define\s+IDEAS_ABI_VERSION\s+4\b", hdr)
    assert _lib.ABI_VERSION == 4 and _lib.load().ideas_abi_version() == 4        # additive within ABI 4
    assert "stego.hip" in open(os.path.join(ROOT, "ideas_amd", "csrc", "Makefile")).read()


def test_c_abi_argument_checks_run_before_any_launch():
    """NULL pointers, non-positive sizes, sigma outside 1..8, C other than 1 or 3, dtypes / layouts without a kernel and n_err without
    ref_bits are answered in front of the launch (no device needed: the pointers are host buffers a launch would never survive)."""
    from ideas_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    a = ctypes.addressof(buf)

    def enc(z=a, bits=a, jitter=a, B=2, L=4, sigma=1, delta=0.5):
        return lib.ideas_bits_to_tensor(z, bits, jitter, B, L, sigma, delta, None)
    assert enc(z=None) == E_NULL and enc(bits=None) == E_NULL
    assert enc(B=0) == E_SHAPE and enc(L=0) == E_SHAPE and enc(B=-1) == E_SHAPE
    assert enc(sigma=0) == E_UNSUPPORTED and enc(sigma=9) == E_UNSUPPORTED and enc(sigma=-3) == E_UNSUPPORTED

    def dec(bits=a, n_err=a, z=a, ref=a, B=2, L=4, sigma=1, dtype=_lib.F32):
        return lib.ideas_tensor_to_bits(bits, n_err, z, ref, B, L, sigma, dtype, None)
    assert dec(z=None) == E_NULL and dec(bits=None, n_err=None) == E_NULL
    assert dec(ref=None) == E_NULL                                                # n_err needs ref_bits
    assert dec(B=0) == E_SHAPE and dec(L=0) == E_SHAPE
    assert dec(sigma=0) == E_UNSUPPORTED and dec(sigma=9) == E_UNSUPPORTED
    assert dec(dtype=_lib.F16) == E_UNSUPPORTED and dec(dtype=_lib.F64) == E_UNSUPPORTED and dec(dtype=_lib.F32_B3) == E_UNSUPPORTED

    def img(u8=a, y=a, x=a, B=1, C=3, H=2, W=2, layout=_lib.NHWC, dtype=_lib.F32):
        return lib.ideas_image_f32_to_u8(u8, y, x, B, C, H, W, layout, dtype, None)
    assert img(u8=None) == E_NULL and img(x=None) == E_NULL
    assert img(B=0) == E_SHAPE and img(H=0) == E_SHAPE and img(W=-2) == E_SHAPE
    assert img(C=2) == E_SHAPE and img(C=4) == E_SHAPE and img(C=0) == E_SHAPE
    assert img(layout=2) == E_UNSUPPORTED and img(dtype=_lib.F16) == E_UNSUPPORTED and img(dtype=_lib.F64) == E_UNSUPPORTED


def test_ops_refuse_host_tensors():
    from ideas_amd import op
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.bits_to_tensor(torch.zeros(1, 1, dtype=torch.uint8), 4, 1, 0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.tensor_to_bits(torch.zeros(1, 4), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op.quantize_image(torch.zeros(1, 3, 4, 4))


# ------------------------------------------------------------------------------------------------- packed bits
@pytest.mark.parametrize("n", [1, 4, 8, 15, 16, 37])
def test_pack_unpack_round_trip(n):
    from ideas_amd.op import pack_bits, unpack_bits
    g = torch.Generator().manual_seed(n)
    m = torch.randint(0, 2, (3, n), generator=g, dtype=torch.float)
    bits = pack_bits(m)
    assert bits.dtype == torch.uint8 and tuple(bits.shape) == (3, (n + 7) // 8)
    for b in range(3):                                                            # the documented bit order, spelled out
        for j in range(n):
            assert (int(bits[b, j >> 3]) >> (7 - (j & 7))) & 1 == int(m[b, j])
    if n % 8:
        assert int(bits[:, -1].max()) & ((1 << (8 - n % 8)) - 1) == 0             # pad bits are zero
    back = unpack_bits(bits, n)
    assert back.dtype == torch.float32 and torch.equal(back, m)
    assert torch.equal(pack_bits(back), bits)


# ------------------------------------------------------------------------------------------------- frame
CAP = 24


@pytest.mark.parametrize("length,n_img", [(0, 1), (1, 1), (CAP - 8, 1), (CAP - 7, 2), (3 * CAP, 4)])
def test_frame_round_trip(length, n_img):
    from ideas_amd.stego import frame, unframe
    payload = bytes(np.random.default_rng(length).integers(0, 256, length, dtype=np.uint8))
    rows = frame(payload, CAP, torch.Generator().manual_seed(1))
    assert rows.dtype == torch.uint8 and tuple(rows.shape) == (n_img, CAP)
    assert bytes(rows.reshape(-1)[:4].tolist()) == length.to_bytes(4, "big")
    assert unframe(rows) == payload and unframe(rows.numpy()) == payload
    again = frame(payload, CAP, torch.Generator().manual_seed(1))
    assert torch.equal(rows, again)                                               # the padding comes from the generator
    if (8 + length) % CAP:
        other = frame(payload, CAP, torch.Generator().manual_seed(2))
        assert not torch.equal(rows, other) and unframe(other) == payload


def test_unframe_rejects_damage():
    from ideas_amd.stego import PayloadError, frame, unframe
    payload = bytes(range(40))
    rows = frame(payload, CAP, torch.Generator().manual_seed(3))
    assert rows.shape[0] == 2
    bad = rows.clone(); bad[0, 8 + 5] ^= 0x10                                     # a payload bit
    with pytest.raises(PayloadError, match="CRC"):
        unframe(bad)
    bad = rows.clone(); bad[1, 3] ^= 0x01                                         # a payload bit in the second image
    with pytest.raises(PayloadError, match="CRC"):
        unframe(bad)
    for byte, bit in ((3, 0x01), (3, 0x40), (0, 0x80)):                           # length bits: 41, 104 and 2^31 + 40 bytes
        bad = rows.clone(); bad[0, byte] ^= bit
        with pytest.raises(PayloadError):
            unframe(bad)
    with pytest.raises(PayloadError, match="length"):
        unframe(rows[:1])                                                         # a truncated row set
    with pytest.raises(PayloadError):
        unframe(torch.zeros(1, 4, dtype=torch.uint8))                             # no room for the header


def test_capacity_bits():
    from argparse import Namespace
    from ideas_amd.stego import capacity_bits
    assert capacity_bits(Namespace(N=1, image_size=64), 1) == 16
    assert capacity_bits(Namespace(N=2, image_size=64), 3) == 96
    assert capacity_bits(Namespace(N=1, image_size=256), 1) == 256
    assert capacity_bits(Namespace(N=3, image_size=128), 8) == 3 * 64 * 8
    assert capacity_bits(Namespace(N=1, image_size=32), 1) == 4                   # not a whole byte: the command lines refuse it


@pytest.mark.parametrize("name", ["hide", "extract", "evaluate"])
def test_command_line_help_parses(name, capsys):
    mod = __import__(name)
    with pytest.raises(SystemExit) as e:
        mod.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--sigma" in out and ("--ckpt" in out or "CHECKPOINT" in out)


# ------------------------------------------------------------------------------------------------- the kernels' arithmetic, restated
def np_encode(M, sigma, delta, jitter):
    """csrc/stego.hip::bits_to_tensor_kernel in numpy f32: one rounding per step, r rounded once from the double product."""
    f = np.float32
    step = 2.0 / 2 ** sigma
    num = np.zeros((M.shape[0], M.shape[1] // sigma), np.float32)
    for i in range(sigma):
        num += M[:, i::sigma].astype(np.float32) * f(2 ** (sigma - 1 - i))
    v = f(step) * (num + f(0.5)) - f(1.0)
    if jitter is None:
        return v
    r = f(step * delta)
    return v + ((jitter * r) * f(2.0) - r)


def np_decode(z, sigma):
    """csrc/stego.hip::decode1 + the bit order of tensor_to_bits_kernel, as a [B, L * sigma] 0/1 message."""
    f = np.float32
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(z), f(-1.0), np.minimum(np.maximum(z, f(-1.0)), f(1.0))).astype(np.float32)
        n = (c + f(1.0)) * f(2 ** sigma / 2.0)
    q = np.minimum(np.floor(n).astype(np.int64), 2 ** sigma - 1)
    msg = np.zeros((z.shape[0], z.shape[1] * sigma), np.uint8)
    for i in range(sigma):
        msg[:, i::sigma] = (q >> (sigma - 1 - i)) & 1
    return msg


def test_fixture_is_the_codec_of_utils_and_of_the_kernels_arithmetic(gold):
    from ideas_amd import utils as U
    meta = gold.json("meta")
    assert {(c["sigma"], c["delta"]) for c in meta["enc"]} == {(s, d) for s in (1, 2, 3, 5, 8) for d in (0.0, 0.25, 0.5)}
    for c in meta["enc"]:
        M, J, Z = (gold.t(f"enc/{c['tag']}/{k}") for k in ("M", "jitter", "Z"))
        assert Z.dtype == torch.float32 and tuple(Z.shape) == (c["B"], c["L"])
        assert torch.equal(U.message_to_tensor(M.float(), c["sigma"], c["delta"], J), Z), c
        assert np.array_equal(np_encode(M.numpy(), c["sigma"], c["delta"], J.numpy()), Z.numpy()), c
    z = gold.t("dec/z")
    assert z.shape[1] == meta["dec"]["n"] and bool(torch.isnan(z).any()) and bool(torch.isinf(z).any())
    for sigma in meta["dec"]["sigmas"]:
        want = gold.t(f"dec/s{sigma}")
        assert torch.equal(U.tensor_to_message(z, sigma).to(torch.uint8), want), sigma
        assert np.array_equal(np_decode(z.numpy(), sigma), want.numpy()), sigma
    assert int(np_decode(np.array([[-1e-9]], np.float32), 1)[0, 0]) == 1          # the f32 "+ 1" rounds -1e-9 + 1 up to 1.0


def test_encode_restatement_matches_utils_at_delta_03():
    from ideas_amd import utils as U
    for (b, l, sigma) in ((1, 4, 1), (3, 5, 3), (2, 256, 1), (2, 16, 8), (2, 7, 5)):
        g = torch.Generator().manual_seed(100 * l + sigma)
        M = torch.randint(0, 2, (b, l * sigma), generator=g, dtype=torch.float)
        J = torch.rand(b, l, generator=g)
        assert np.array_equal(np_encode(M.numpy(), sigma, 0.3, J.numpy()), U.message_to_tensor(M, sigma, 0.3, J).numpy())


def quantize_reference(x):
    """The bytes torchvision's save_image(normalize=True, range=(-1, 1)) / utils.image_grid write, as a torch expression."""
    return ((x.float().clamp(-1, 1) + 1) / 2 * 255 + 0.5).clamp(0, 255).to(torch.uint8)


def threshold_set():
    """Values around every decision of the 8-bit write: the 256 half-integer thresholds mapped back to [-1, 1] with their f32
    neighbours, every byte's own value, the ends and beyond."""
    k = np.arange(256, dtype=np.float64)
    thr = (((k + 0.5) / 255.0) * 2 - 1).astype(np.float32)
    own = (k / 255.0 * 2 - 1).astype(np.float32)
    parts = [thr, np.nextafter(thr, np.float32(-np.inf)), np.nextafter(thr, np.float32(np.inf)), own,
             np.array([1, -1, 2, -2, -0.0, 0.0, np.inf, -np.inf], np.float32)]
    return torch.from_numpy(np.concatenate(parts))


def test_quantise_restatement_and_byte_round_trip():
    """The kernel's operation order in numpy f32 equals the torch expression on the threshold set, and quantising the dequantised
    value of every byte returns that byte (a received image re-sent is unchanged)."""
    f = np.float32
    x = torch.cat((threshold_set(), torch.rand(5000, generator=torch.Generator().manual_seed(5)) * 2.2 - 1.1))

    def np_quant(v):
        t = np.minimum(np.maximum(v, f(-1.0)), f(1.0))
        t = (t + f(1.0)) / f(2.0)
        t = t * f(255.0)
        t = t + f(0.5)
        return np.minimum(np.maximum(t, f(0.0)), f(255.0)).astype(np.int32).astype(np.uint8)
    want = quantize_reference(x)
    assert np.array_equal(np_quant(x.numpy()), want.numpy())
    assert set(want.tolist()) == set(range(256))
    q = np.arange(256, dtype=np.float32)
    y = (q / f(255.0) - f(0.5)) / f(0.5)
    assert np.array_equal(np_quant(y), np.arange(256, dtype=np.uint8))
    assert torch.equal(quantize_reference(torch.from_numpy(y)), torch.arange(256, dtype=torch.uint8))
