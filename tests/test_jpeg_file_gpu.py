"""The JPEG file channel (csrc/attack_jpeg.hip) on the GPU against the numpy restatement tests/jpegfile_ref.py, which
tests/test_jpeg_file.py holds to Pillow: bytes, luma and chroma coefficients and the decoded half-resolution chroma in the workspace,
``y``, the recorded Pillow round trips, operand placement, the C ABI's errors, the ``jpegfile:Q`` stage in a chain and in
``stego.evaluate``, and ``hide.py --format jpeg`` end to end.  Everything is integer arithmetic: every comparison is ``torch.equal`` /
``array_equal``, there is no tolerance anywhere.  Every raw call writes into sentinel-guarded buffers."""
import math
import os
import re

import numpy as np
import pytest
import torch

import jpegfile_ref as J
from conftest import Golden

pytestmark = pytest.mark.gpu

BAND = 64                     # sentinel bytes either side of every buffer
SENT = 0xA5
E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
SHAPES = [(1, 1), (4, 4), (5, 3), (16, 2), (8, 8), (15, 9), (16, 16), (17, 23), (31, 16), (33, 40), (2, 50), (9, 129)]


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


def grids(h, w, c, sub):
    """((bh, bw), (cbh, cbw), (ch, cw)): the luma and chroma block grids and the half-resolution chroma size."""
    bh, bw = (h + 7) // 8, (w + 7) // 8
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return (bh, bw), ((bh, bw) if sub == 0 else ((ch + 7) // 8, (cw + 7) // 8)), (ch, cw)


def raw_file(x, quality, sub, want_y=True, want_coef=True, skew=(0, 0, 0, 0, 0, 0)):
    """ideas_jpeg_file_roundtrip on uint8 [B, H, W, C]; skew = byte offsets of (x, out, y, coef_y, coef_c, workspace).
    -> (out, y or None, coef_y or None, coef_c or None, the workspace as uint8 [B, 2, ch, cw] or None)."""
    from ideas_amd import _lib
    lib = _lib.load()
    b, h, w, c = x.shape
    (bh, bw), (cbh, cbw), (ch, cw) = grids(h, w, c, sub)
    nwork = int(lib.ideas_jpeg_file_workspace_bytes(b, c, h, w, sub))
    assert nwork == (2 * b * ch * cw if c == 3 and sub == 2 else 0)
    xin = place(x.cuda(), skew[0])
    out, y = Guarded(x.numel(), skew[1]), Guarded(4 * x.numel(), skew[2])
    coef_y, coef_c = Guarded(2 * b * bh * bw * 64, skew[3]), Guarded(2 * b * 2 * cbh * cbw * 64, skew[4])
    work = Guarded(nwork, skew[5])
    rc = lib.ideas_jpeg_file_roundtrip(out.ptr(), y.ptr() if want_y else None, coef_y.ptr() if want_coef else None,
                                       coef_c.ptr() if want_coef else None, work.ptr() if nwork else None, xin.ptr(), b, c, h, w, quality,
                                       sub, _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert out.intact() and y.intact() and coef_y.intact() and coef_c.intact() and work.intact() and xin.intact()
    assert torch.equal(xin.view.view(x.shape), x.cuda())
    assert want_y or y.untouched()
    assert want_coef or (coef_y.untouched() and coef_c.untouched())
    assert c == 3 or coef_c.untouched()
    return (out.get(torch.uint8, (b, h, w, c)), y.get(torch.float32, (b, h, w, c)) if want_y else None,
            coef_y.get(torch.int16, (b, bh, bw, 64)) if want_coef else None,
            coef_c.get(torch.int16, (b, 2, cbh, cbw, 64)) if want_coef and c == 3 else None,
            work.get(torch.uint8, (b, 2, ch, cw)) if nwork else None)


def images(b, h, w, c, seed=0):
    """``b`` different images uint8 [b, h, w, c]: seeded noise, a ramp with grain, a 0/255 image, in turn."""
    rng = np.random.default_rng(100000 * seed + 1000 * h + 10 * w + c)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for i in range(b):
        if i % 3 == 0:
            out.append(rng.integers(0, 256, (h, w, c), dtype=np.uint8))
        elif i % 3 == 1:
            ramp = np.stack([(3 * yy + 2 * xx + 90 * k) % 256 for k in range(c)], -1)
            out.append(np.clip(ramp + rng.integers(-6, 7, (h, w, c)), 0, 255).astype(np.uint8))
        else:
            out.append((rng.integers(0, 2, (h, w, c)) * 255).astype(np.uint8))
    return np.ascontiguousarray(np.stack(out))


_REF = {}


def ref(x, quality, sub):
    """The restatement of every image of the batch ``x`` (numpy), computed once per (bytes, quality, sub)."""
    key = (x.tobytes(), x.shape, quality, sub)
    if key not in _REF:
        _REF[key] = [J.jpeg_file_ref(img, quality, sub) for img in x]
    return _REF[key]


def check_against_the_restatement(x, quality, sub, got):
    """Bytes, coefficients and the workspace, image by image.  The coefficients tell a forward-side bug from an inverse-side one."""
    out, _, coef_y, coef_c, work = got
    for i, want in enumerate(ref(x, quality, sub)):
        tag = (x.shape, quality, sub, i)
        assert np.array_equal(coef_y[i].cpu().numpy(), want["coef_y"]), ("coef_y", tag)
        if want["coef_c"] is None:
            assert coef_c is None
        else:
            assert np.array_equal(coef_c[i].cpu().numpy(), want["coef_c"]), ("coef_c", tag)
        if want["chroma"] is None:
            assert work is None
        else:
            assert np.array_equal(work[i].cpu().numpy(), want["chroma"]), ("the decoded half-resolution chroma", tag)
        assert np.array_equal(out[i].cpu().numpy(), want["out"]), ("bytes", tag)


# ------------------------------------------------------------------------------------------------- the kernels against the restatement
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", SHAPES)
def test_round_trip_is_the_restatement(hw, c):
    from ideas_amd import data
    from ideas_amd.op import jpeg_file_roundtrip
    h, w = hw
    x = images(2, h, w, c)
    xd = torch.from_numpy(x)
    for quality in (1, 75, 100):
        for sub in (0, 2):
            got = raw_file(xd, quality, sub)
            check_against_the_restatement(x, quality, sub, got)
            out, y, coef_y, coef_c, _ = got
            assert torch.equal(y, data.u8_to_f32(out).permute(0, 2, 3, 1))      # bitwise the receiver's decode
    # the optional outputs change nothing; the op gives the same
    only = raw_file(xd, 75, 2, want_y=False, want_coef=False)
    assert torch.equal(only[0], raw_file(xd, 75, 2)[0]) and only[1] is None and only[2] is None and only[3] is None
    for sub, name in ((0, "4:4:4"), (2, "4:2:0")):
        out, y, coef_y, coef_c, _ = raw_file(xd, 75, sub)
        o_out, o_y, o_cy, o_cc = jpeg_file_roundtrip(xd.cuda(), 75, name, return_coef=True)
        assert torch.equal(o_out, out) and torch.equal(o_cy, coef_y)
        assert (o_cc is None and coef_c is None) if c == 1 else torch.equal(o_cc, coef_c)
        assert tuple(o_y.shape) == (2, c, h, w) and o_y.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(o_y, data.u8_to_f32(out))
        pair = jpeg_file_roundtrip(xd.cuda(), 75, sub)
        assert len(pair) == 2 and torch.equal(pair[0], out)
    assert torch.equal(jpeg_file_roundtrip(xd.cuda(), 75)[0], out)               # 4:2:0 is the default


def test_one_channel_ignores_the_subsampling():
    x = torch.from_numpy(images(2, 17, 23, 1))
    a, b = raw_file(x, 50, 0), raw_file(x, 50, 2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and a[3] is None and b[3] is None and b[4] is None


def test_op_validation_and_empty_input():
    from ideas_amd.op import jpeg_file_roundtrip
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device="cuda")
    for bad in ("4:2:2", 1, "420", None, True):
        with pytest.raises(RuntimeError, match="subsampling"):
            jpeg_file_roundtrip(x, 75, bad)
    for q in (0, 101, 7.5):
        with pytest.raises(RuntimeError, match="quality"):
            jpeg_file_roundtrip(x, q)
    with pytest.raises(RuntimeError, match="uint8"):
        jpeg_file_roundtrip(x.float(), 75)
    out, y, cy, cc = jpeg_file_roundtrip(x[:0], 75, return_coef=True)            # no launch
    assert tuple(out.shape) == (0, 8, 8, 3) and tuple(y.shape) == (0, 3, 8, 8) and tuple(cy.shape) == (0, 1, 1, 64)
    assert tuple(cc.shape) == (0, 2, 1, 1, 64)


@pytest.mark.parametrize("sub", [0, 2])
@pytest.mark.parametrize("quality", [10, 75, 95])
def test_round_trip_is_the_recorded_pillow_round_trip(quality, sub):
    img, pil = Golden("attacks.npz").z, Golden("jpegfile.npz").z
    for name in ("smooth", "odd", "gray", "noise"):
        x = torch.from_numpy(np.ascontiguousarray(img[f"img/{name}"][None]))
        want = np.cumsum(pil[f"rt/q{quality}/s{sub}/{name}"], axis=0, dtype=np.uint8)
        assert np.array_equal(raw_file(x, quality, sub)[0][0].cpu().numpy(), want), name


# ------------------------------------------------------------------------------------------------- placement
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", [(64, 64), (24, 40)])
def test_fast_path_and_byte_path_give_the_same_bytes(hw, c):
    """Aligned with W % 8 == 0: 8-byte words and float4.  x, out and the workspace one byte, y four bytes, the coefficients two bytes
    off 16-byte alignment: byte by byte.  (24 x 40: W % 16 == 8, the last chroma block's right half lies outside the image.)"""
    h, w = hw
    x = images(2, h, w, c, seed=1)
    xd = torch.from_numpy(x)
    for sub in (0, 2):
        fast = raw_file(xd, 75, sub)
        check_against_the_restatement(x, 75, sub, fast)
        slow = raw_file(xd, 75, sub, skew=(1, 1, 4, 2, 2, 1))
        only_y = raw_file(xd, 75, sub, skew=(0, 0, 8, 0, 0, 0))                  # only y misplaced for float4
        only_x = raw_file(xd, 75, sub, skew=(3, 0, 0, 0, 0, 0))                  # only x misplaced
        for other in (slow, only_y, only_x):
            for a, b in zip(fast, other):
                assert (a is None and b is None) or torch.equal(a, b)


def test_many_tiles():
    """B = 3, 72 x 136: 81 luma tiles of 8 blocks (the last of each row 1 block wide) in 21 workgroups, the last with one live wave
    and three that repeat its tile without stores; 45 chroma tiles at 4:2:0."""
    x = images(3, 72, 136, 3, seed=2)
    for sub in (0, 2):
        check_against_the_restatement(x, 50, sub, raw_file(torch.from_numpy(x), 50, sub))


def test_grid_stride_loop_turns_over():
    """The launches are capped at 16384 workgroups of 4 tiles, so only more than 65536 tiles send a workgroup round its loop again:
    65541 images of 8 x 64 (one luma and one chroma tile each; 100 MB), copies of 5 different ones, against the round trip of the 5.
    The first workgroups make a second trip, the last one of them with one live wave."""
    k, b = 5, 4 * 16384 + 5
    small = images(k, 8, 64, 3, seed=4)
    idx = (torch.arange(b) % k).cuda()
    x = torch.from_numpy(small).cuda()[idx]
    for sub in (0, 2):
        want = raw_file(torch.from_numpy(small), 75, sub, want_y=False)
        check_against_the_restatement(small, 75, sub, want)
        got = raw_file(x, 75, sub, want_y=False)
        for g, w in zip(got, want):
            assert (g is None and w is None) or torch.equal(g, w[idx])


# ------------------------------------------------------------------------------------------------- C ABI errors
def test_c_abi_errors_touch_nothing():
    from ideas_amd import _lib
    lib = _lib.load()
    b, c, h, w = 1, 3, 16, 16
    x = place(torch.from_numpy(images(b, h, w, c)).cuda(), 0)
    out, y = Guarded(b * h * w * c), Guarded(4 * b * h * w * c)
    cy, cc, work = Guarded(2 * b * 4 * 64), Guarded(2 * b * 2 * 4 * 64), Guarded(2 * b * 8 * 8)

    def rt(out_=out, x_=x, work_=work, C=c, q=75, sub=2, B=b):
        return lib.ideas_jpeg_file_roundtrip(out_.ptr() if out_ else None, y.ptr(), cy.ptr(), cc.ptr(), work_.ptr() if work_ else None,
                                             x_.ptr() if x_ else None, B, C, h, w, q, sub, _lib.stream_ptr())
    assert rt(out_=None) == E_NULL and rt(x_=None) == E_NULL
    assert rt(C=2) == E_SHAPE and rt(B=0) == E_SHAPE
    assert rt(q=0) == E_UNSUPPORTED and rt(q=101) == E_UNSUPPORTED
    assert rt(sub=1) == E_UNSUPPORTED
    assert rt(work_=None) == E_NULL                                              # NULL workspace at 4:2:0
    torch.cuda.synchronize()
    assert out.untouched() and y.untouched() and cy.untouched() and cc.untouched() and work.untouched() and x.intact()
    assert rt(work_=None, sub=0) == 0 and rt(work_=None, C=1) == 0               # ... which 4:4:4 and C = 1 do not need
    torch.cuda.synchronize()
    assert work.untouched() and not out.untouched() and out.intact()


# ------------------------------------------------------------------------------------------------- the stage
def test_stage_in_a_chain_is_the_two_ops_by_hand():
    from ideas_amd import attacks
    from ideas_amd.op import jpeg_file_roundtrip, pixel_attack
    x = torch.from_numpy(images(2, 33, 40, 3, seed=3)).cuda()
    a = attacks.parse("noise:3+jpegfile:75")
    assert a.name == "noise:3+jpegfile:75"
    u8, y = a(x, torch.Generator(device="cuda").manual_seed(5))
    gen = torch.Generator(device="cuda").manual_seed(5)
    want = jpeg_file_roundtrip(pixel_attack(x, sigma=3.0, generator=gen)[0], 75, "4:2:0")
    assert torch.equal(u8, want[0]) and torch.equal(y, want[1])
    u8, y = attacks.parse("jpegfile:75:444")(x)
    want = jpeg_file_roundtrip(x, 75, "4:4:4")
    assert torch.equal(u8, want[0]) and torch.equal(y, want[1])
    assert not torch.equal(u8, attacks.parse("jpegfile:75")(x)[0])


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """The reference's own checkpoint of tests/golden/ckpt_r256.npz as a file (the discriminator's omitted tensors: zeros)."""
    from ckpt_fixture import build_reference_checkpoint
    raw = build_reference_checkpoint(Golden("ckpt_r256.npz"), lambda key, shape: torch.zeros(shape))
    path = str(tmp_path_factory.mktemp("jpegfile_ckpt") / "1.pt")
    torch.save(raw, path)
    return path


def test_evaluate_behind_a_jpeg_file(ckpt):
    from ideas_amd import attacks, stego
    models, args = stego.load_models(ckpt, "cuda")
    res = stego.evaluate(models, args, 1, 0.25, 3, 2, torch.Generator(device="cuda").manual_seed(31), attack=attacks.parse("jpegfile:75"))
    assert res["attack"] == "jpegfile:75" and res["n_bits"] == 3 * stego.capacity_bits(args, 1)
    assert math.isfinite(res["acc"]) and 0.0 <= res["acc"] <= 1.0


def test_evaluate_command_line_prints_a_line_per_attack(ckpt, capsys):
    import evaluate
    specs = ["jpegfile:75", "jpegfile:75:444", "scale:0.5+jpegfile:75"]
    evaluate.main(["--ecc", "1/2", "--delta", "0.25", "--n_sample", "2", "--batch", "2", "--attack", *specs, ckpt])
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 3, lines
    for line, spec in zip(lines, specs):
        assert re.fullmatch(r"sigma=1 delta=25%% attack=%s ACC: [01]\.\d{4} ECC=1/2 INFO_ACC: [01]\.\d{4} FER: [01]\.\d{4}" % re.escape(spec),
                            line), line


def test_hide_writes_jpeg_files_that_decode_to_the_round_trip(ckpt, tmp_path):
    """``hide.py --format jpeg --jpeg_quality 75``: what Pillow decodes from the .jpg files is ``jpeg_file_roundtrip`` of the bytes hide
    computed -- those of the .png files the same command line writes without ``--format`` (the same seed gives the same containers)."""
    from PIL import Image, features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo: its JPEG files need not be those of the model")
    import hide
    from ideas_amd.op import jpeg_file_roundtrip
    payload = tmp_path / "payload.bin"
    payload.write_bytes(bytes(range(48)))
    common = ["--ckpt", ckpt, "--payload", str(payload), "--seed", "3", "--batch", "2"]
    hide.main(common + ["--out", str(tmp_path / "png")])
    hide.main(common + ["--out", str(tmp_path / "jpg"), "--format", "jpeg", "--jpeg_quality", "75"])
    hide.main(common + ["--out", str(tmp_path / "jpg444"), "--format", "jpeg", "--jpeg_quality", "75", "--jpeg_subsampling", "444"])
    names = sorted(os.listdir(tmp_path / "png"))
    assert names and all(n.endswith(".png") for n in names)
    stems = [n[:-4] for n in names]

    def load(folder, ext):
        assert sorted(os.listdir(tmp_path / folder)) == [s + ext for s in stems]
        arrs = []
        for s in stems:
            with Image.open(tmp_path / folder / (s + ext)) as im:
                assert im.mode == "RGB" and (ext == ".png" or im.format == "JPEG")
                arrs.append(np.asarray(im, dtype=np.uint8).copy())
        return torch.from_numpy(np.stack(arrs))
    sent = load("png", ".png")
    for folder, sub in (("jpg", "4:2:0"), ("jpg444", "4:4:4")):
        got = load(folder, ".jpg")
        want = jpeg_file_roundtrip(sent.cuda(), 75, sub)[0].cpu()
        differing = int((got != want).any(-1).any(-1).any(-1).sum())
        print(f"{folder}: {differing} of {len(stems)} files differ from jpeg_file_roundtrip")
        assert torch.equal(got, want)
