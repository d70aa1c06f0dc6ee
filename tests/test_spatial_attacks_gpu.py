"""The spatial channel-attack kernels (csrc/attack_spatial.hip) on the GPU against the numpy restatement tests/spatial_ref.py, which is
Pillow byte for byte (tests/test_spatial_attacks.py): resize, Gaussian blur and median, every placement of the operands, hand-made
tables, and ``stego.evaluate`` / ``evaluate.py`` with the new stages on the tiny checkpoint of tests/ckpt_fixture.py.  Every raw call
writes into sentinel-guarded buffers; every comparison is byte for byte."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import spatial_ref as R
from conftest import ROOT, Golden

pytestmark = pytest.mark.gpu

BAND = 64                     # sentinel bytes either side of every buffer
SENT = 0xA5
SHAPES = [(1, 1), (5, 7), (13, 21), (40, 24), (24, 200)]       # the last: four tiles of 64 columns, the last one partial
BATCHED = ((5, 7), (40, 24))                                   # B = 3 there
FACTORS = (0.25, 0.3, 0.5, 0.75, 1.5, 2.0, 3.7)
ALIGNED, BYTES_OFF, WORDS_OFF = (0, 0, 0, 0), (1, 1, 0, 0), (0, 0, 4, 4)      # byte offsets of (x, out, y, tables) from 16-byte alignment
PLACEMENTS = (ALIGNED, BYTES_OFF, WORDS_OFF)


class Guarded:
    """``nbytes`` on the device between two bands of sentinel bytes, ``skew`` bytes off the allocation's 16-byte alignment."""

    def __init__(self, nbytes, skew=0):
        self.n, self.skew = nbytes, skew
        self.buf = torch.full((BAND + skew + nbytes + BAND,), SENT, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[BAND + skew:BAND + skew + nbytes]

    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        lo = BAND + self.skew
        return bool((self.buf[:lo] == SENT).all()) and bool((self.buf[lo + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())

    def get(self, dtype, shape):
        return self.view.clone().view(dtype).view(shape)


def dev(a):
    """A numpy array on the device (through a writable copy: the shared images are read-only)."""
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def place(a, skew):
    """The bytes of the numpy array ``a`` on the device at ``skew`` bytes off 16-byte alignment, guarded."""
    t = dev(a)
    g = Guarded(t.numel() * t.element_size(), skew)
    g.view.copy_(t.view(-1).view(torch.uint8))
    return g


def raw_resample(x, h2, w2, horiz, vert, want_y=True, skew=ALIGNED):
    """ideas_resample_u8 on uint8 numpy [B, H, W, C] with tables (lo, kk) or None per direction -> (out, y or None) as numpy."""
    from ideas_amd import _lib
    b, h, w, c = x.shape
    xin = place(x, skew[0])
    n = b * h2 * w2 * c
    out, y = Guarded(n, skew[1]), Guarded(4 * n, skew[2])
    tabs = [place(t, skew[3]) for d in (horiz, vert) if d is not None for t in d]
    hp = (tabs[0].ptr(), tabs[1].ptr(), horiz[1].shape[1]) if horiz is not None else (None, None, 0)
    vt = tabs[-2:] if vert is not None else None
    vp = (vt[0].ptr(), vt[1].ptr(), vert[1].shape[1]) if vert is not None else (None, None, 0)
    rc = _lib.load().ideas_resample_u8(out.ptr(), y.ptr() if want_y else None, xin.ptr(), b, c, h, w, h2, w2, *hp, *vp, _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert out.intact() and y.intact() and xin.intact() and all(t.intact() for t in tabs)
    assert np.array_equal(xin.get(torch.uint8, x.shape).cpu().numpy(), x)
    assert want_y or y.untouched()
    return finish(out, y, (b, h2, w2, c), want_y)


def raw_median(x, k, want_y=True, skew=ALIGNED):
    from ideas_amd import _lib
    b, h, w, c = x.shape
    xin = place(x, skew[0])
    out, y = Guarded(x.size, skew[1]), Guarded(4 * x.size, skew[2])
    rc = _lib.load().ideas_median_u8(out.ptr(), y.ptr() if want_y else None, xin.ptr(), b, c, h, w, k, _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert out.intact() and y.intact() and xin.intact()
    assert np.array_equal(xin.get(torch.uint8, x.shape).cpu().numpy(), x)
    assert want_y or y.untouched()
    return finish(out, y, x.shape, want_y)


def finish(out, y, shape, want_y):
    """-> (out, y) as numpy, after checking that y is bitwise the receiver's decode of out."""
    from ideas_amd import data
    o = out.get(torch.uint8, shape)
    if not want_y:
        return o.cpu().numpy(), None
    yy = y.get(torch.float32, shape)
    assert torch.equal(yy, data.u8_to_f32(o).permute(0, 2, 3, 1))
    return o.cpu().numpy(), yy.cpu().numpy()


_images = {}


def image(hw, c):
    """uint8 [B, h, w, c], B = 3 on BATCHED: smooth structure plus grain, 0 and 255 among the values; made once per shape."""
    key = (hw, c)
    if key not in _images:
        h, w = hw
        b = 3 if hw in BATCHED else 1
        rng = np.random.default_rng(1000 * h + 10 * w + c)
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        base = 128 + 100 * np.sin(yy[None, :, :, None] / 3.0 + np.arange(b)[:, None, None, None]) * np.cos(xx[None, :, :, None] / 5.0 + 0.5 * np.arange(c))
        img = np.clip(base + rng.normal(0, 25, (b, h, w, c)), 0, 255).astype(np.uint8)
        img.reshape(-1)[:2] = (0, 255)[:img.size]
        img.setflags(write=False)
        _images[key] = img
    return _images[key]


def tables(n_in, n_out):
    return R.bilinear_tables(n_in, n_out) if n_out != n_in else None


def all_placements(run, want):
    """``run(skew, want_y) -> (out, y)``: the same bytes wherever the operands lie, with and without y."""
    first = None
    for skew in PLACEMENTS:
        out, y = run(skew, True)
        assert np.array_equal(out, want), skew
        first = (out, y) if first is None else first
        assert np.array_equal(y, first[1]), skew
    out, y = run(ALIGNED, False)
    assert np.array_equal(out, want) and y is None
    out, _ = run(BYTES_OFF, False)
    assert np.array_equal(out, want)


# ------------------------------------------------------------------------------------------------- resample
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", SHAPES)
def test_resize_is_the_oracle(hw, c):
    from ideas_amd.op import resize_u8
    x = image(hw, c)
    h, w = hw
    targets = sorted({R.scaled_size(h, w, f) for f in FACTORS} | {(h, max(1, w // 2))})      # the last: H2 == H, no vertical tables
    for h2, w2 in targets:
        horiz, vert = tables(w, w2), tables(h, h2)
        want = R.resample_ref(x, horiz, vert)
        assert want.shape == (x.shape[0], h2, w2, c)
        if (h2, w2) in (R.scaled_size(h, w, 0.5), R.scaled_size(h, w, 3.7), (h, max(1, w // 2))):
            all_placements(lambda skew, want_y: raw_resample(x, h2, w2, horiz, vert, want_y, skew), want)
        else:
            assert np.array_equal(raw_resample(x, h2, w2, horiz, vert)[0], want), (h2, w2)
        out, y = resize_u8(dev(x), (h2, w2))
        assert np.array_equal(out.cpu().numpy(), want), (h2, w2)
        assert tuple(y.shape) == (x.shape[0], c, h2, w2) and y.is_contiguous(memory_format=torch.channels_last)


def test_resize_of_the_fixture_images_is_pillows():
    """Straight against the recorded Pillow outputs, through the op: resize, the way back, and one axis up while the other goes down."""
    from ideas_amd.op import resize_u8
    gold, z = Golden("attacks.npz"), Golden("spatial.npz").z

    def pil(key):
        return np.cumsum(z[key], axis=0, dtype=np.uint8)
    for name in ("smooth", "odd", "gray", "noise"):
        img = gold.z[f"img/{name}"]
        h, w = img.shape[:2]
        x = dev(img[None])
        for f in FACTORS:
            small, _ = resize_u8(x, R.scaled_size(h, w, f))
            assert np.array_equal(small[0].cpu().numpy(), pil(f"resize/f{f:g}/{name}")), (name, f)
            assert np.array_equal(resize_u8(small, (h, w))[0][0].cpu().numpy(), pil(f"back/f{f:g}/{name}")), (name, f)
    x = dev(gold.z["img/odd"][None])
    assert np.array_equal(resize_u8(x, (20, 8))[0][0].cpu().numpy(), pil("resize/aniso/odd"))
    want = R.resample_ref(gold.z["img/odd"][None], R.bilinear_tables(21, 8), R.bilinear_tables(13, 20))
    all_placements(lambda skew, want_y: raw_resample(gold.z["img/odd"][None], 20, 8, R.bilinear_tables(21, 8), R.bilinear_tables(13, 20),
                                                     want_y, skew), want)


@pytest.mark.parametrize("c", [1, 3])
def test_resample_with_hand_made_tables(c):
    """Tables no filter makes, whose result is known by hand: the 200 rows shuffled by i -> 97 i mod 200 (the 32 rows of a tile then
    reach rows 0 .. 194, more than a tile keeps in LDS), both axes mirrored (tiles that fit), two taps 31 rows apart in a window
    zero-padded to 32, first inputs far outside the image (clamped to the edge pixel before the load), both directions skipped, and
    coefficients whose sum wraps 32 bits or goes negative."""
    x = np.ascontiguousarray(image((24, 200), c).transpose(0, 2, 1, 3))          # [1, 200, 24, c]
    h, w = 200, 24
    one = np.full((h, 1), 1 << 22, np.int32)
    flip_v = (np.arange(h - 1, -1, -1, dtype=np.int32), one)
    flip_h = (np.arange(w - 1, -1, -1, dtype=np.int32), one[:w])
    shuffle = ((97 * np.arange(h) % h).astype(np.int32), one)
    assert shuffle[0][:32].max() - shuffle[0][:32].min() >= 160
    all_placements(lambda skew, want_y: raw_resample(x, h, w, None, shuffle, want_y, skew), x[:, shuffle[0]])
    all_placements(lambda skew, want_y: raw_resample(x, h, w, flip_h, shuffle, want_y, skew), x[:, shuffle[0], ::-1])
    all_placements(lambda skew, want_y: raw_resample(x, h, w, flip_h, flip_v, want_y, skew), x[:, ::-1, ::-1])
    assert np.array_equal(raw_resample(x, h, w, None, None)[0], x)               # both skipped: a copy (and its y)
    # output row i is the rounded mean of rows i - 8 and i + 23, clamped at both ends: taps 0 and 31 of a window of 32, zeros between
    kk = np.zeros((h, 32), np.int32)
    kk[:, 0] = kk[:, 31] = 1 << 21
    lo = np.arange(h, dtype=np.int32) - 8
    want = R.resample_ref(x, None, (lo, kk))
    rows = np.arange(h)
    by_hand = (x[:, np.clip(rows - 8, 0, h - 1)].astype(np.int64) + x[:, np.clip(rows + 23, 0, h - 1)] + 1) >> 1
    assert np.array_equal(want, by_hand.astype(np.uint8))
    all_placements(lambda skew, want_y: raw_resample(x, h, w, None, (lo, kk), want_y, skew), want)
    # first inputs far outside: every tap clamps to the first or the last pixel
    far = np.where(np.arange(w) % 2 == 0, -(1 << 30), (1 << 31) - 1).astype(np.int32)
    want = np.where((np.arange(w) % 2 == 0)[None, None, :, None], x[:, :, :1], x[:, :, -1:])
    assert np.array_equal(R.resample_ref(x, (far, one[:w]), None), want)
    assert np.array_equal(raw_resample(x, h, w, (far, one[:w]), None)[0], want)
    # sums that wrap or go negative: defined by 32-bit wrapping arithmetic, the signed result clamped
    rng = np.random.default_rng(7)
    wild = (rng.integers(-4, w, w).astype(np.int32), rng.integers(-(1 << 31), 1 << 31, (w, 5)).astype(np.int32))
    want = R.resample_ref(x, wild, None)
    assert 0 in want and 255 in want
    assert np.array_equal(raw_resample(x, h, w, wild, None)[0], want)


@pytest.mark.parametrize("sigma", [0.3, 1.0, 2.5, 4.0])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", SHAPES)
def test_gaussian_blur_is_the_oracle(hw, c, sigma):
    """1x1 and 5x7 have windows wider than the image (sigma 2.5: 8 taps either side; 4: 12)."""
    from ideas_amd.op import gaussian_blur_u8
    x = image(hw, c)
    h, w = hw
    horiz, vert = R.gauss_tables(w, sigma), R.gauss_tables(h, sigma)
    want = R.resample_ref(x, horiz, vert)
    if sigma in (1.0, 4.0):
        all_placements(lambda skew, want_y: raw_resample(x, h, w, horiz, vert, want_y, skew), want)
    else:
        assert np.array_equal(raw_resample(x, h, w, horiz, vert)[0], want)
    out, y = gaussian_blur_u8(dev(x), sigma)
    assert np.array_equal(out.cpu().numpy(), want)
    assert tuple(y.shape) == (x.shape[0], c, h, w) and y.is_contiguous(memory_format=torch.channels_last)


def test_constant_images_stay_constant():
    from ideas_amd.op import gaussian_blur_u8, median_u8, resize_u8
    x = torch.arange(256, dtype=torch.uint8).view(256, 1, 1, 1).expand(256, 5, 7, 1).contiguous().cuda()
    for f in (0.25, 0.3, 3.7):
        assert torch.equal(resize_u8(resize_u8(x, R.scaled_size(5, 7, f))[0], (5, 7))[0], x)
    for s in (0.3, 1.0, 4.0):
        assert torch.equal(gaussian_blur_u8(x, s)[0], x)
    for k in (3, 5):
        assert torch.equal(median_u8(x, k)[0], x)


# ------------------------------------------------------------------------------------------------- median
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", SHAPES)
def test_median_is_the_oracle(hw, c, k):
    from ideas_amd.op import median_u8
    x = image(hw, c)
    want = R.median_ref(x, k)
    all_placements(lambda skew, want_y: raw_median(x, k, want_y, skew), want)
    out, y = median_u8(dev(x), k)
    assert np.array_equal(out.cpu().numpy(), want)
    assert tuple(y.shape) == (x.shape[0], c) + hw and y.is_contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("k", [3, 5])
def test_median_of_sorted_ramps_by_hand(k):
    """v[y, x, ch] = 3 y + x + 20 ch rises along both axes, so away from the edge the window's median is its centre; on the edge the
    replicated window is the window of the clamped ramp.  And every permutation class the network must order: windows of distinct
    values in descending and shuffled order."""
    h, w = 20, 70
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    x = (3 * yy[..., None] + xx[..., None] + 20 * np.arange(3)).astype(np.uint8)[None]
    out, _ = raw_median(x, k)
    r = k // 2
    assert np.array_equal(out[:, r:h - r, r:w - r], x[:, r:h - r, r:w - r])
    assert np.array_equal(out, R.median_ref(x, k))
    assert out[0, 0, 0, 0] == {3: 1, 5: 2}[k]            # k = 3: 0 0 1 0 0 1 3 3 4 -> 1;  k = 5: the 13th of 25 clamped values
    rng = np.random.default_rng(k)
    shuffled = np.stack([rng.permutation(256).astype(np.uint8).reshape(16, 16, 1) for _ in range(3)])
    assert np.array_equal(raw_median(shuffled, k)[0], R.median_ref(shuffled, k))
    down = np.ascontiguousarray(x[:, ::-1, ::-1])
    assert np.array_equal(raw_median(down, k)[0], R.median_ref(down, k))


# ------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """The reference's own checkpoint of tests/golden/ckpt_r256.npz as a file (the discriminator's omitted tensors: zeros)."""
    from ckpt_fixture import build_reference_checkpoint
    raw = build_reference_checkpoint(Golden("ckpt_r256.npz"), lambda key, shape: torch.zeros(shape))
    path = str(tmp_path_factory.mktemp("spatial_ckpt") / "1.pt")
    torch.save(raw, path)
    return path


def test_evaluate_with_spatial_attacks(ckpt):
    from ideas_amd import attacks, stego
    from ideas_amd.op import gaussian_blur_u8, median_u8, quantize_image, resize_u8
    models, args = stego.load_models(ckpt, "cuda")
    sigma, delta = 1, 0.25
    cap = stego.capacity_bits(args, sigma)
    chain = stego.evaluate(models, args, sigma, delta, 3, 2, torch.Generator(device="cuda").manual_seed(31),
                           attack=attacks.parse("gblur:1+scale:0.5+median:3"))
    assert chain["attack"] == "gblur:1+scale:0.5+median:3" and chain["n_bits"] == 3 * cap
    gen = torch.Generator(device="cuda").manual_seed(31)
    n_err = 0
    for b in (2, 1):
        bits = stego.random_bits(b, cap, gen, "cuda")
        images, _ = stego.hide(models, args, bits, sigma, delta, generator=gen)
        u8 = quantize_image(images, dequantize=False)[0]
        h, w = u8.shape[1:3]
        u8, _ = gaussian_blur_u8(u8, 1.0)
        u8, _ = resize_u8(u8, R.scaled_size(h, w, 0.5))
        u8, _ = resize_u8(u8, (h, w))
        u8, y = median_u8(u8, 3)
        n_err += int(stego.extract(models, args, y, sigma, ref_bits=bits)[2].sum())
    assert chain["n_err"] == n_err


def test_evaluate_command_line_prints_a_line_per_attack_and_delta(ckpt):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--delta", "0", "0.5", "--n_sample", "2", "--batch", "2",
                        "--attack", "none", "scale:0.5", ckpt], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 4, r.stdout
    seen = []
    for line in lines:
        m = re.fullmatch(r"sigma=1 delta=(0|50)% attack=(none|scale:0\.5) ACC: [01]\.\d{4}", line)
        assert m, line
        seen.append((m.group(2), m.group(1)))
    assert seen == [("none", "0"), ("none", "50"), ("scale:0.5", "0"), ("scale:0.5", "50")]
