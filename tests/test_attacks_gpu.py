"""The channel-attack kernels (csrc/attack.hip) on the GPU against the numpy restatement tests/attacks_ref.py: the JPEG round trip's
coefficients and bytes (exact outside the tie window TOL, a neighbour inside it; the four rational coefficients and the tie images bit
for bit), edge replication, operand placement, the pixel attacks bit for bit against the f32 restatement, and ``stego.evaluate`` /
``evaluate.py`` with an attack on the tiny checkpoint of tests/ckpt_fixture.py.  Every raw call writes into sentinel-guarded buffers."""
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import attacks_ref as R
from conftest import ROOT, Golden

pytestmark = pytest.mark.gpu

BAND = 64                     # sentinel bytes either side of every buffer
SENT = 0xA5
RATIONAL_IDX = [0, 4, 32, 36]


@pytest.fixture(scope="module")
def gold():
    return Golden("attacks.npz")


class Guarded:
    """``nbytes`` on the device between two bands of sentinel bytes, ``skew`` bytes off the allocation's 16-byte alignment."""

    def __init__(self, nbytes, skew=0):
        self.n, self.skew = nbytes, skew
        self.buf = torch.full((BAND + skew + nbytes + BAND,), SENT, dtype=torch.uint8, device="cuda")
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


def place(t, skew):
    """A copy of the bytes of ``t`` at ``skew`` bytes off 16-byte alignment (guarded: the kernel must not write there either)."""
    g = Guarded(t.numel() * t.element_size(), skew)
    g.view.copy_(t.contiguous().view(-1).view(torch.uint8))
    return g


def raw_jpeg(x, quality, want_y=True, want_coef=True, skew=(0, 0, 0, 0)):
    """ideas_jpeg_roundtrip on uint8 [B, H, W, C]; skew = byte offsets of (x, out, y, coef).  -> (out, y or None, coef or None)."""
    from ideas_amd import _lib
    b, h, w, c = x.shape
    bh, bw = (h + 7) // 8, (w + 7) // 8
    xin = place(x.cuda(), skew[0])
    out, y, coef = Guarded(x.numel(), skew[1]), Guarded(4 * x.numel(), skew[2]), Guarded(2 * b * c * bh * bw * 64, skew[3])
    rc = _lib.load().ideas_jpeg_roundtrip(out.ptr(), y.ptr() if want_y else None, coef.ptr() if want_coef else None, xin.ptr(),
                                          b, c, h, w, quality, _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert out.intact() and y.intact() and coef.intact() and xin.intact()
    assert torch.equal(xin.view.view(x.shape), x.cuda())
    assert want_y or y.untouched()
    assert want_coef or coef.untouched()
    return (out.get(torch.uint8, (b, h, w, c)), y.get(torch.float32, (b, h, w, c)) if want_y else None,
            coef.get(torch.int16, (b, c, bh, bw, 64)) if want_coef else None)


def batch_of(gold, h, w, c, b):
    """``b`` different images [h, w, c] cut from the smooth fixture and its mirror images."""
    s = gold.z["img/smooth"]
    views = (s, s[::-1], s[:, ::-1])
    imgs = [views[i][:h, :w] if c == 3 else views[i][:h, :w, 1:2] for i in range(b)]
    return np.ascontiguousarray(np.stack(imgs))


def check_against_oracle(x, quality, out, coef):
    """The kernel's coefficients against the oracle's, its bytes against the oracle's decode of the KERNEL's coefficients."""
    b, h, w, c = x.shape
    flips = near_c = near_s = 0
    for i in range(b):
        ratio, want = R.encode(x[i], quality)
        ratio = ratio.reshape(want.shape)
        got = coef[i].astype(np.int64)
        assert np.array_equal(got[..., RATIONAL_IDX], want[..., RATIONAL_IDX]), "a rational coefficient differs"
        near = R.near_tie(ratio)
        near[..., RATIONAL_IDX] = False
        assert np.array_equal(got[~near], want[~near]), "a coefficient outside the tie window differs"
        lo = np.sign(ratio) * np.floor(np.abs(ratio))                # inside: either neighbour
        hi = np.sign(ratio) * (np.floor(np.abs(ratio)) + 1)
        assert ((got == lo) | (got == hi))[near].all()
        flips += int((got != want).sum())
        near_c += int(near.sum())
        pre, recon = R.jpeg_from_coef(got, h, w, quality)
        win = R.near_tie(pre)[:, :h, :w].any(0)                       # a pixel with any plane's sample in the window
        d = np.abs(out[i].astype(np.int64) - recon.astype(np.int64))
        assert d.max() <= 1, f"a byte differs by {d.max()} levels"
        assert not d[~win].any(), "a byte outside the tie window differs"
        near_s += int(win.sum())
    return flips, near_c, near_s


SHAPES = [(1, 1), (7, 9), (8, 8), (16, 8), (13, 21), (40, 24)]


@pytest.mark.parametrize("quality", [1, 50, 75, 100])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", SHAPES)
def test_jpeg_roundtrip_against_the_oracle(gold, hw, c, quality):
    from ideas_amd import data
    from ideas_amd.op import jpeg_roundtrip
    h, w = hw
    b = 3 if hw in ((7, 9), (16, 8), (40, 24)) else 1
    x = batch_of(gold, h, w, c, b)
    xd = torch.from_numpy(x)
    out, y, coef = raw_jpeg(xd, quality)
    flips, near_c, near_s = check_against_oracle(x, quality, out.cpu().numpy(), coef.cpu().numpy())
    print(f"{h}x{w}x{c} B={b} q={quality}: {near_c} coefficients and {near_s} pixels in the window, {flips} coefficient(s) took the other neighbour")
    assert torch.equal(y, data.u8_to_f32(out).permute(0, 2, 3, 1))              # bitwise the receiver's decode
    # the optional outputs change nothing
    only, none_y, none_c = raw_jpeg(xd, quality, want_y=False, want_coef=False)
    assert torch.equal(only, out) and none_y is None and none_c is None
    assert torch.equal(raw_jpeg(xd, quality, want_coef=False)[0], out) and torch.equal(raw_jpeg(xd, quality, want_y=False)[2], coef)
    o_out, o_y, o_coef = jpeg_roundtrip(xd.cuda(), quality, return_coef=True)
    assert torch.equal(o_out, out) and torch.equal(o_coef, coef)
    assert tuple(o_y.shape) == (b, c, h, w) and o_y.is_contiguous(memory_format=torch.channels_last) and torch.equal(o_y, data.u8_to_f32(out))
    assert len(jpeg_roundtrip(xd.cuda(), quality)) == 2


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", [(16, 8), (40, 24), (13, 21)])
def test_jpeg_roundtrip_at_odd_byte_offsets(gold, hw, c):
    """x and out one byte, y four bytes, coef two bytes off 16-byte alignment: the byte-wise path, the same results."""
    h, w = hw
    xd = torch.from_numpy(batch_of(gold, h, w, c, 3))
    out, y, coef = raw_jpeg(xd, 75)
    o2, y2, c2 = raw_jpeg(xd, 75, skew=(1, 1, 4, 2))
    assert torch.equal(o2, out) and torch.equal(y2, y) and torch.equal(c2, coef)
    o3, y3, _ = raw_jpeg(xd, 75, skew=(0, 0, 8, 0))                              # only y misplaced for float4
    assert torch.equal(o3, out) and torch.equal(y3, y)
    check_against_oracle(xd.numpy(), 75, o2.cpu().numpy(), c2.cpu().numpy())


def tie_cases(gold):
    for name in ("dc_q50", "sample_q62", "sample_q1", "basis"):
        img = gold.z[f"tie/{name}"]
        for q in sorted({int(gold.z[f"tie/{name}/quality"]), 1, 50, 75, 100}):
            yield name, img, q
    for v in (0, 255):
        for q in (1, 50, 75, 100):
            yield f"all-{v}", np.full((16, 16, 1), v, np.uint8), q


def test_tie_images_match_the_oracle_bit_for_bit(gold):
    """Flat blocks with the DC exactly on a quantiser tie (both signs) or with a dequantised DC that puts every sample on k + 0.5,
    blocks made of the (0,4), (4,0), (4,4) patterns, all-0 and all-255: integers and eighths only, so no window."""
    n = 0
    for name, img, q in tie_cases(gold):
        for x in (img, np.repeat(img, 3, axis=2)):                               # one channel; grey RGB (Cb = Cr = 128)
            want = R.jpeg_ref(x, q)
            out, _, coef = raw_jpeg(torch.from_numpy(x[None]), q)
            assert np.array_equal(coef[0].cpu().numpy(), want["coef"]), (name, q, x.shape)
            assert np.array_equal(out[0].cpu().numpy(), want["out"]), (name, q, x.shape)
            n += 1
    assert n == 2 * (4 + 5 + 4 + 4 + 8)


@pytest.mark.parametrize("c", [1, 3])
def test_edge_replication(gold, c):
    """13x21 equals the top-left 13x21 of its edge-replicated 16x24 version, coefficient for coefficient."""
    img = gold.z["img/odd"][..., :c] if c == 3 else gold.z["img/odd"][..., 1:2]
    padded = np.pad(img, ((0, 3), (0, 3), (0, 0)), mode="edge")
    for q in (1, 50, 75, 100):
        out, y, coef = raw_jpeg(torch.from_numpy(img[None].copy()), q)
        pout, py, pcoef = raw_jpeg(torch.from_numpy(padded[None].copy()), q)
        assert tuple(coef.shape) == tuple(pcoef.shape) == (1, c, 2, 3, 64)
        assert torch.equal(coef, pcoef) and torch.equal(out, pout[:, :13, :21]) and torch.equal(y, py[:, :13, :21])


def test_jpeg_roundtrip_many_tiles():
    """More blocks than one workgroup holds and a last column of blocks that is partly outside a wave's 64 columns: 24 x 200."""
    x = np.random.default_rng(9).integers(0, 256, (2, 24, 200, 3), dtype=np.uint8)
    x = (x.astype(np.int64) // 4 + np.linspace(0, 180, 200)[None, None, :, None]).astype(np.uint8)
    out, _, coef = raw_jpeg(torch.from_numpy(x), 50)
    check_against_oracle(x, 50, out.cpu().numpy(), coef.cpu().numpy())


# ------------------------------------------------------------------------------------------------- pixel_attack
def raw_pixel(x, noise, u, gain, offset, sigma, sp, want_y=True, skew=False):
    from ideas_amd import _lib
    b, h, w, c = x.shape
    xin = place(x.cuda(), 1 if skew else 0)
    nin = place(noise.cuda(), 4 if skew else 0) if noise is not None else None
    uin = place(u.cuda(), 4 if skew else 0) if u is not None else None
    out, y = Guarded(x.numel(), 1 if skew else 0), Guarded(4 * x.numel(), 4 if skew else 0)
    rc = _lib.load().ideas_pixel_attack(out.ptr(), y.ptr() if want_y else None, xin.ptr(), nin.ptr() if nin else None,
                                        uin.ptr() if uin else None, b, c, h, w, gain, offset, sigma, sp, _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert out.intact() and y.intact() and xin.intact() and (nin is None or nin.intact()) and (uin is None or uin.intact())
    assert want_y or y.untouched()
    return out.get(torch.uint8, (b, h, w, c)), y.get(torch.float32, (b, h, w, c)) if want_y else None


GRID = list(itertools.product((0.5, 1.0, 1.5), (-20.0, 0.0, 20.0), (0.0, 5.0), (0.0, 0.1)))


@pytest.mark.parametrize("skew", [False, True])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (16, 16)])
def test_pixel_attack_is_the_f32_restatement(hw, c, skew):
    """Aligned buffers of four pixels or more take the four-pixel path (5x7: 8 groups and a tail of 3), misaligned ones and 1x1 the
    one-pixel path."""
    from ideas_amd import data
    h, w = hw
    g = torch.Generator().manual_seed(100 * h + w + c)
    x = torch.randint(0, 256, (2, h, w, c), generator=g, dtype=torch.uint8)
    x.view(-1)[:2] = torch.tensor([0, 255], dtype=torch.uint8)[:x.numel()]
    noise = torch.randn(2, h, w, c, generator=g)
    u = torch.rand(2, h, w, generator=g)
    u.view(-1)[0] = 0.0
    for gain, offset, sigma, sp in GRID:
        nz, uu = (noise if sigma else None), (u if sp else None)
        want = R.pixel_attack_ref(x.numpy(), gain, offset, sigma, sp, None if nz is None else nz.numpy(), None if uu is None else uu.numpy())
        out, y = raw_pixel(x, nz, uu, gain, offset, sigma, sp, skew=skew)
        assert np.array_equal(out.cpu().numpy(), want), (gain, offset, sigma, sp)
        assert torch.equal(y, data.u8_to_f32(out).permute(0, 2, 3, 1))
    # draws that are given but switched off change nothing; y is optional
    want = R.pixel_attack_ref(x.numpy(), 1.5, -20.0)
    out, _ = raw_pixel(x, noise, u, 1.5, -20.0, 0.0, 0.0, want_y=False, skew=skew)
    assert np.array_equal(out.cpu().numpy(), want)


def test_pixel_attack_nan_noise_and_whole_pixels():
    from ideas_amd.op import pixel_attack
    x = torch.full((1, 4, 8, 3), 200, dtype=torch.uint8)
    noise = torch.zeros(1, 4, 8, 3)
    noise[0, 1, :, 1] = float("nan")
    for skew in (False, True):
        out, _ = raw_pixel(x, noise, None, 1.0, 0.0, 5.0, 0.0, skew=skew)
        assert bool((out[0, 1, :, 1] == 0).all()) and int((out == 200).sum()) == x.numel() - 8
    u = torch.rand(1, 4, 8, generator=torch.Generator().manual_seed(3))
    x = torch.randint(1, 255, (1, 4, 8, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
    for skew in (False, True):
        out, _ = raw_pixel(x, None, u, 1.0, 0.0, 0.0, 0.5, skew=skew)
        pepper, salt = (u < 0.25).cuda(), (u >= 0.75).cuda()
        assert bool(pepper.any()) and bool(salt.any())
        assert bool((out[pepper] == 0).all()) and bool((out[salt] == 255).all())        # the same pixel in all channels
        keep = ~(pepper | salt)
        assert torch.equal(out[keep], x.cuda()[keep])
    # the op draws the noise, then u, from the generator
    gen = torch.Generator(device="cuda").manual_seed(11)
    o1, y1 = pixel_attack(x.cuda(), sigma=4.0, sp=0.2, generator=gen)
    gen = torch.Generator(device="cuda").manual_seed(11)
    nz = torch.randn(1, 4, 8, 3, device="cuda", generator=gen)
    uu = torch.rand(1, 4, 8, device="cuda", generator=gen)
    o2, y2 = pixel_attack(x.cuda(), sigma=4.0, sp=0.2, noise=nz, u=uu)
    assert torch.equal(o1, o2) and torch.equal(y1, y2)
    assert np.array_equal(o1.cpu().numpy(), R.pixel_attack_ref(x.numpy(), sigma=4.0, sp=0.2, noise=nz.cpu().numpy(), u=uu.cpu().numpy()))
    assert tuple(y1.shape) == (1, 3, 4, 8) and y1.is_contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """The reference's own checkpoint of tests/golden/ckpt_r256.npz as a file (the discriminator's omitted tensors: zeros)."""
    from ckpt_fixture import build_reference_checkpoint
    raw = build_reference_checkpoint(Golden("ckpt_r256.npz"), lambda key, shape: torch.zeros(shape))
    path = str(tmp_path_factory.mktemp("attack_ckpt") / "1.pt")
    torch.save(raw, path)
    return path


def test_evaluate_with_attacks(ckpt):
    from ideas_amd import attacks, stego
    from ideas_amd.op import jpeg_roundtrip, pixel_attack, quantize_image
    models, args = stego.load_models(ckpt, "cuda")
    sigma, delta = 1, 0.25
    cap = stego.capacity_bits(args, sigma)

    def run(attack):
        return stego.evaluate(models, args, sigma, delta, 3, 2, torch.Generator(device="cuda").manual_seed(31), attack=attack)
    plain, none = run(None), run(attacks.parse("none"))
    assert plain["attack"] is None and none["attack"] == "none"
    assert none["n_err"] == plain["n_err"] and none["l1"] == plain["l1"] and none["n_bits"] == 3 * cap
    chain = run(attacks.parse("noise:3+jpeg:50"))
    assert chain["attack"] == "noise:3+jpeg:50"
    gen = torch.Generator(device="cuda").manual_seed(31)
    n_err = 0
    for b in (2, 1):
        bits = stego.random_bits(b, cap, gen, "cuda")
        images, _ = stego.hide(models, args, bits, sigma, delta, generator=gen)
        u8 = quantize_image(images, dequantize=False)[0]
        u8, _ = pixel_attack(u8, sigma=3.0, generator=gen)
        u8, y = jpeg_roundtrip(u8, 50)
        n_err += int(stego.extract(models, args, y, sigma, ref_bits=bits)[2].sum())
    assert chain["n_err"] == n_err
    with pytest.raises(ValueError):
        stego.evaluate(models, args, sigma, delta, 3, 2, container="float", attack=attacks.parse("none"))


def test_evaluate_command_line_prints_a_line_per_attack_and_delta(ckpt):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--delta", "0", "0.5", "--n_sample", "2", "--batch", "2",
                        "--attack", "none", "jpeg:75", ckpt], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 4, r.stdout
    seen = []
    for line in lines:
        m = re.fullmatch(r"sigma=1 delta=(0|50)% attack=(none|jpeg:75) ACC: [01]\.\d{4}", line)
        assert m, line
        seen.append((m.group(2), m.group(1)))
    assert seen == [("none", "0"), ("none", "50"), ("jpeg:75", "0"), ("jpeg:75", "50")]
