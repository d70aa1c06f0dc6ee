"""Outputs of the f32 JPEG model (ideas_jpeg_roundtrip) pinned to what the library gave BEFORE its kernel was rebuilt from
csrc/u8.hpp and csrc/jpeg_block.hpp (the shared byte I/O, tables, colour conversion, tile walk and block round trip).

The move alters no value.  tests/test_attacks_gpu.py::test_jpeg_roundtrip_against_the_oracle exempts coefficients inside the tie window
of the f32 quantiser, so it would not see a reordered product; this file leaves nothing exempt.  tests/golden/jpeg_pinned.npz
(tests/golden/make_golden_jpeg_pinned.py, run on the parent commit's library) holds, per output of every case below (the bytes `out`,
the received image `y`, the quantised coefficients `coef`), its shape, the SHA-256 of its bytes and its first 16 values; the inputs are
re-made here from seeds on the CPU.  The entry point runs through the C ABI on raw buffers.

Cases: C in {1, 3} x quality in {1, 50, 75, 100} x two images x two placements x five shapes (H, W), B = 1:
  (1, 1)     one pixel, everything replicated
  (13, 21)   byte path, both edges replicated
  (8, 64)    exactly one full tile on the vector path
  (16, 72)   vector path, nine blocks across: the second tile has seven lanes without a block, whose row load clamps to W - 8
  (24, 136)  nine tiles on three workgroups: the last has one live wave and three that repeat the last tile without stores
Images: uniform random bytes; a smooth ramp plus noise of +-3 (most coefficients quantise to zero, the low ones do not).
Placements: aligned; x and out one byte behind an 8-byte boundary, which forces the byte path where W % 8 == 0."""
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "jpeg_pinned.npz")
SHAPES = ((1, 1), (13, 21), (8, 64), (16, 72), (24, 136))
QUALITIES = (1, 50, 75, 100)
IMAGES = ("uniform", "ramp")
PLACEMENTS = (("aligned", 0), ("behind", 1))


def image(kind, seed, H, W, C):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.integers(0, 256, size=(1, H, W, C), dtype=np.uint8)
    yy, xx, cc = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    ramp = 32 + (160 * (xx + yy)) // max(1, H + W - 2) + 16 * cc
    return np.clip(ramp + rng.integers(-3, 4, size=(H, W, C)), 0, 255).astype(np.uint8)[None]


def _bytes_at(n, off, fill=None):
    """n device bytes whose first lies ``off`` bytes behind the (256-byte aligned) start of their buffer"""
    buf = torch.full((n + off,), 0xA5, device="cuda", dtype=torch.uint8)
    v = buf[off:]
    if fill is not None:
        v.copy_(torch.from_numpy(fill.reshape(-1)))
    assert v.data_ptr() % 8 == off
    return v


def _run(C, quality, kind, off, si):
    from ideas_amd import _lib
    H, W = SHAPES[si]
    x = _bytes_at(H * W * C, off, image(kind, 1000 * si + 10 * IMAGES.index(kind) + C, H, W, C))
    out = _bytes_at(H * W * C, off)
    y = torch.full((1, H, W, C), float("nan"), device="cuda", dtype=torch.float32)
    coef = torch.full((1, C, (H + 7) // 8, (W + 7) // 8, 64), -32768, device="cuda", dtype=torch.int16)
    _lib.check(_lib.load().ideas_jpeg_roundtrip(_lib.ptr(out), _lib.ptr(y), _lib.ptr(coef), _lib.ptr(x), 1, C, H, W, quality, _lib.stream_ptr()),
               "ideas_jpeg_roundtrip")
    return [out.view(1, H, W, C), y, coef]


def _cases():
    c = {}
    for C in (1, 3):
        for q in QUALITIES:
            for kind in IMAGES:
                for place, off in PLACEMENTS:
                    for si, (H, W) in enumerate(SHAPES):
                        c["c%d_q%d_%s_%s_%dx%d" % (C, q, kind, place, H, W)] = lambda C=C, q=q, kind=kind, off=off, si=si: _run(C, q, kind, off, si)
    return c


CASES = _cases()


def run_case(name):
    """[(shape, sha256 hex, first 16 values as float32)] of out, y and coef"""
    outs = CASES[name]()
    torch.cuda.synchronize()
    res = []
    for t in outs:
        a = t.contiguous().cpu().numpy()
        assert np.isfinite(a.astype(np.float32)).all(), name
        res.append((tuple(a.shape), hashlib.sha256(a.tobytes()).hexdigest(), a.reshape(-1)[:16].astype(np.float32).copy()))
    return res


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_the_cases_are_the_160_of_the_table():
    assert len(CASES) == 2 * len(QUALITIES) * len(IMAGES) * len(PLACEMENTS) * len(SHAPES) == 160


@pytest.mark.parametrize("name", sorted(CASES))
def test_jpeg_outputs_are_bitwise_the_pinned_ones(name, golden):
    got = run_case(name)
    assert int(golden[name + "/n"]) == len(got) == 3
    for i, (shape, sha, head) in enumerate(got):
        k = "%s/%d" % (name, i)
        assert tuple(golden[k + "/shape"]) == shape, k
        assert np.array_equal(golden[k + "/head"], head), (k, golden[k + "/head"], head)
        assert bytes(golden[k + "/sha256"]).hex() == sha, k
