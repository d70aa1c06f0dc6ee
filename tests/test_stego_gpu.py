"""The steganography kernels (csrc/stego.hip) and the surface built on them, on the GPU: the packed-bit codec bit for bit against the
reference's vectors (tests/golden/stego.npz) and the host functions of utils.py, the 8-bit image write against the torch expression and
``data.u8_to_f32``, hide / extract against ``train_step.extraction_test`` on the tiny configuration of ``smoke()``, ``evaluate``
against explicit calls, and the three command lines as child processes."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, Golden, rel_err
from test_stego import quantize_reference, threshold_set

pytestmark = pytest.mark.gpu

BAND = 64                     # sentinel bytes either side of every output buffer
SENT = 0xA5


@pytest.fixture(scope="module")
def gold():
    return Golden("stego.npz")


def guarded(nbytes):
    """A device buffer of ``nbytes`` between two bands of sentinel bytes (the payload keeps the allocation's 16-byte alignment)."""
    buf = torch.full((BAND + nbytes + BAND,), SENT, dtype=torch.uint8, device="cuda")
    return buf, buf[BAND:BAND + nbytes]


def bands_intact(buf, nbytes):
    return bool((buf[:BAND] == SENT).all()) and bool((buf[BAND + nbytes:] == SENT).all())


# ------------------------------------------------------------------------------------------------- bits_to_tensor
def test_bits_to_tensor_is_the_references_encoder(gold):
    from ideas_amd.op import bits_to_tensor, pack_bits
    for c in gold.json("meta")["enc"]:
        M, J, Z = (gold.t(f"enc/{c['tag']}/{k}") for k in ("M", "jitter", "Z"))
        bits = pack_bits(M).cuda()
        got = bits_to_tensor(bits, c["L"], c["sigma"], c["delta"], jitter=J.cuda())
        assert got.dtype == torch.float32 and torch.equal(got.cpu(), Z), c
        if c["delta"] == 0.0:                                 # the NULL-jitter path: the bin centres
            assert torch.equal(bits_to_tensor(bits, c["L"], c["sigma"], 0.0).cpu(), Z), c


@pytest.mark.parametrize("shape", [(1, 4, 1), (3, 5, 3), (2, 256, 1), (2, 16, 8)])
def test_bits_to_tensor_matches_utils_at_delta_03(shape):
    from ideas_amd import utils as U
    from ideas_amd.op import bits_to_tensor, pack_bits
    b, l, sigma = shape
    g = torch.Generator().manual_seed(100 * l + sigma)
    M = torch.randint(0, 2, (b, l * sigma), generator=g, dtype=torch.float)
    J = torch.rand(b, l, generator=g)
    want = U.message_to_tensor(M, sigma, 0.3, J)
    assert torch.equal(bits_to_tensor(pack_bits(M).cuda(), l, sigma, 0.3, jitter=J.cuda()).cpu(), want)
    # without a jitter argument the draw comes from the generator
    dev_gen = torch.Generator(device="cuda").manual_seed(9)
    drawn = bits_to_tensor(pack_bits(M).cuda(), l, sigma, 0.3, generator=dev_gen)
    J2 = torch.rand(b, l, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    assert torch.equal(drawn.cpu(), U.message_to_tensor(M, sigma, 0.3, J2.cpu()))


# ------------------------------------------------------------------------------------------------- tensor_to_bits
def raw_decode(z, sigma, ref=None, want_bits=True):
    """ideas_tensor_to_bits into sentinel-guarded buffers; returns (bits or None, n_err or None)."""
    from ideas_amd import _lib
    b, l = z.shape
    nbytes = (l * sigma + 7) // 8
    bbuf, bits = guarded(b * nbytes)
    ebuf, err = guarded(4 * b)
    z = z.contiguous()
    rc = _lib.load().ideas_tensor_to_bits(bits.data_ptr() if want_bits else None, err.data_ptr() if ref is not None else None,
                                          z.data_ptr(), None if ref is None else ref.data_ptr(), b, l, sigma, _lib.act_dtype(z),
                                          _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bands_intact(bbuf, b * nbytes) and bands_intact(ebuf, 4 * b)
    if not want_bits:
        assert bool((bits == SENT).all())
    if ref is None:
        assert bool((err == SENT).all())
    return (bits.view(b, nbytes).clone() if want_bits else None,
            err.view(torch.int32).clone() if ref is not None else None)


def host_popcount(a, b, n_bits):
    from ideas_amd.op import unpack_bits
    return (unpack_bits(a.cpu(), n_bits) != unpack_bits(b.cpu(), n_bits)).sum(1).to(torch.int32)


@pytest.mark.parametrize("sigma", [1, 2, 3, 5, 8])
def test_tensor_to_bits_is_the_references_decoder(gold, sigma):
    from ideas_amd import utils as U
    from ideas_amd.op import tensor_to_bits, unpack_bits
    z = gold.t("dec/z")
    n = z.shape[1]
    want = gold.t(f"dec/s{sigma}")
    bits, _ = raw_decode(z.cuda(), sigma)
    assert torch.equal(unpack_bits(bits, n * sigma).cpu().to(torch.uint8), want)
    if (n * sigma) % 8:
        assert int(bits[:, -1].max()) & ((1 << (8 - (n * sigma) % 8)) - 1) == 0   # pad bits are written as zero
    assert torch.equal(tensor_to_bits(z.cuda(), sigma), bits)
    zb = z.bfloat16()
    bits_b, _ = raw_decode(zb.cuda(), sigma)
    assert torch.equal(unpack_bits(bits_b, n * sigma).cpu(), U.tensor_to_message(zb.float(), sigma))


def test_tensor_to_bits_rows_straddling_bytes_and_error_counts():
    """B = 3, L = 5, sigma = 3: 15 message bits a row, elements across the byte boundary, one pad bit."""
    from ideas_amd import utils as U
    from ideas_amd.op import pack_bits, tensor_to_bits, unpack_bits
    z = (torch.rand(3, 5, generator=torch.Generator().manual_seed(3)) * 2.4 - 1.2)
    want = U.tensor_to_message(z, 3)
    bits, _ = raw_decode(z.cuda(), 3)
    assert torch.equal(unpack_bits(bits, 15).cpu(), want) and torch.equal(bits.cpu(), pack_bits(want))
    one = bits.clone(); one[1, 0] ^= 0x08
    pads = bits.clone(); pads[:, 1] |= 0x01                   # pad bits set in ref: never counted
    for ref, exp in ((bits, [0, 0, 0]), (one, [0, 1, 0]), (~bits, [15, 15, 15]), (pads, [0, 0, 0])):
        got_bits, n_err = raw_decode(z.cuda(), 3, ref=ref.contiguous())
        assert torch.equal(got_bits, bits) and n_err.tolist() == exp, (n_err.tolist(), exp)
        _, only_err = raw_decode(z.cuda(), 3, ref=ref.contiguous(), want_bits=False)
        assert only_err.tolist() == exp
    got, n_err = tensor_to_bits(z.cuda(), 3, ref=one)
    assert torch.equal(got, bits) and n_err.dtype == torch.int32 and n_err.tolist() == [0, 1, 0]


def test_tensor_to_bits_long_row_runs_the_stride_loop_and_the_cross_wave_sum():
    """B = 1, L = 4096, sigma = 1: 512 bytes, two trips of the 256-thread loop, all four waves contribute to the count."""
    from ideas_amd import utils as U
    from ideas_amd.op import pack_bits
    g = torch.Generator().manual_seed(4096)
    z = torch.randn(1, 4096, generator=g) * 0.7
    ref = torch.randint(0, 256, (1, 512), generator=g, dtype=torch.uint8)
    want = pack_bits(U.tensor_to_message(z, 1))
    bits, n_err = raw_decode(z.cuda(), 1, ref=ref.cuda())
    assert torch.equal(bits.cpu(), want)
    assert n_err.tolist() == host_popcount(want, ref, 4096).tolist() and 1500 < int(n_err[0]) < 2600
    _, all_err = raw_decode(z.cuda(), 1, ref=(~want).cuda())
    assert all_err.tolist() == [4096]


# ------------------------------------------------------------------------------------------------- quantize_image
def raw_quantize(x, want_y=True):
    """ideas_image_f32_to_u8 on ``x`` (NCHW-contiguous or channels_last, as it lies) into sentinel-guarded buffers."""
    from ideas_amd import _lib
    b, c, h, w = x.shape
    layout = _lib.NHWC if x.is_contiguous(memory_format=torch.channels_last) else _lib.NCHW
    assert layout == _lib.NHWC or x.is_contiguous()
    n = x.numel()
    ubuf, u8 = guarded(n)
    ybuf, y = guarded(4 * n)
    rc = _lib.load().ideas_image_f32_to_u8(u8.data_ptr(), y.data_ptr() if want_y else None, x.data_ptr(), b, c, h, w, layout,
                                           _lib.act_dtype(x), _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bands_intact(ubuf, n) and bands_intact(ybuf, 4 * n)
    if not want_y:
        assert bool((y == SENT).all())
    return u8.view(b, h, w, c).clone(), (y.view(torch.float32).view(b, h, w, c).clone() if want_y else None)


def check_quantize(x_dev):
    from ideas_amd import data
    from ideas_amd.op import quantize_image
    want = quantize_reference(x_dev.cpu()).permute(0, 2, 3, 1).contiguous()
    u8, y = raw_quantize(x_dev)
    assert torch.equal(u8.cpu(), want)
    back = data.u8_to_f32(u8)
    assert torch.equal(y, back.permute(0, 2, 3, 1))
    u8_only, _ = raw_quantize(x_dev, want_y=False)
    assert torch.equal(u8_only, u8)
    ou8, oy = quantize_image(x_dev)
    assert torch.equal(ou8, u8) and tuple(oy.shape) == tuple(x_dev.shape) and oy.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(oy, back)
    assert quantize_image(x_dev, dequantize=False)[1] is None


def as_layout(x, dtype, channels_last):
    x = x.to(dtype).cuda()
    return x.contiguous(memory_format=torch.channels_last) if channels_last else x.contiguous()


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_image_on_every_threshold(dtype, channels_last):
    vals = threshold_set()
    filler = torch.rand(4096, generator=torch.Generator().manual_seed(11)) * 2.2 - 1.1
    for shape in ((2, 3, 5, 7), (1, 1, 3, 5)):
        n = int(np.prod(shape))
        for i0 in range(0, vals.numel(), n):                  # the whole set, spread over tensors of this shape
            chunk = torch.cat((vals[i0:i0 + n], filler))[:n].reshape(shape)
            check_quantize(as_layout(chunk, dtype, channels_last))
    for shape in ((1, 3, 64, 64), (1, 3, 41, 51)):            # whole groups of the vector path only; whole and partial groups plus a tail
        big = torch.rand(shape, generator=torch.Generator().manual_seed(12)) * 2.2 - 1.1
        check_quantize(as_layout(big, dtype, channels_last))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_image_unaligned_base_and_strided_views(dtype):
    from ideas_amd.op import quantize_image
    x = as_layout(torch.rand(3, 3, 5, 7, generator=torch.Generator().manual_seed(13)) * 2.2 - 1.1, dtype, True)
    view = x[1:]                                              # base 105 elements in: not 16-byte aligned -> the element-wise path
    assert view.data_ptr() % 16 != 0 and view.is_contiguous(memory_format=torch.channels_last)
    check_quantize(view)
    crop = x[:, :, 1:4, 2:6]                                  # storage-contiguous in neither layout: the op makes it so
    u8, y = quantize_image(crop)
    assert torch.equal(u8.cpu(), quantize_reference(crop.cpu()).permute(0, 2, 3, 1))


def test_quantize_image_nan_is_zero():
    from ideas_amd.op import quantize_image
    x = torch.full((1, 3, 4, 8), float("nan"), device="cuda")
    x[0, 1] = 0.25
    for t in (x, x.contiguous(memory_format=torch.channels_last), x.bfloat16()):
        u8, y = quantize_image(t)
        assert bool((u8[..., 0] == 0).all()) and bool((u8[..., 2] == 0).all()) and bool((u8[..., 1] == 159).all())
        assert bool((y[:, 0] == -1).all())


# ------------------------------------------------------------------------------------------------- pipeline
def tiny_trainer(N):
    from ideas_amd import train_step as TS
    from ideas_amd.models import init_model
    args = TS.default_args(channel=8, texture_channel=128, channel_multiplier=0.25, image_size=64, batch_size=2, N=N, use_dco=False)
    torch.manual_seed(70 + N)
    trainer = TS.build_trainer(args, "cpu", init_model)
    for v in trainer.values():
        if isinstance(v, torch.nn.Module):
            v.cuda()
    return trainer, args


@pytest.fixture(scope="module")
def tiny():
    return {N: tiny_trainer(N) for N in (1, 2)}


@pytest.mark.parametrize("N", [1, 2])
def test_hide_extract_reproduce_the_training_test_block(tiny, N):
    from ideas_amd import stego, train_step as TS, utils as U
    from ideas_amd.op import pack_bits, quantize_image, unpack_bits
    trainer, args = tiny[N]
    models = stego.models_of(trainer)
    cap = stego.capacity_bits(args, 1)
    assert cap == N * 16
    g = torch.Generator().manual_seed(80 + N)
    X = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).cuda()
    M = torch.randint(0, 2, (2, cap), generator=g, dtype=torch.float).cuda()
    J = torch.rand(2, cap, generator=g).cuda()
    T2 = (torch.rand(2, 128, generator=g) * 2 - 1).cuda()
    with torch.no_grad():
        ref_Z, ref_M, _, _ = TS.extraction_test(trainer, args, X, M, T2, use_x3=True, jitter=J)
    bits = pack_bits(M)
    images, Z = stego.hide(models, args, bits, 1, 0.5, texture=T2, jitter=J)
    assert tuple(images.shape) == (2, 3, 64, 64) and tuple(Z.shape) == (2, N, 4, 4)
    assert torch.equal(Z.reshape(2, -1), U.message_to_tensor(M, 1, 0.5, J))
    got_bits, hat_Z = stego.extract(models, args, images, 1)
    e = rel_err(hat_Z, ref_Z)
    print(f"N={N}: float container, hat_Z vs extraction_test: rel err {e:.3e}, bitwise identical: {torch.equal(hat_Z, ref_Z)}")
    assert torch.equal(unpack_bits(got_bits, cap), ref_M), "decisions differ from extraction_test"
    assert e < 1e-5, e
    _, _, n_err = stego.extract(models, args, images, 1, ref_bits=bits)
    assert n_err.tolist() == (unpack_bits(got_bits, cap) != M).sum(1).tolist()

    # the 8-bit container: the receiver's networks on the kernel's own dequantised image
    u8, y = quantize_image(images)
    with torch.no_grad():
        want = U.tensor_to_message(models["Ex"](models["E"](y)[0]).reshape(2, -1).float(), 1)
    bits_u8, _ = stego.extract(models, args, u8, 1)
    bits_y, _ = stego.extract(models, args, y, 1)
    assert torch.equal(unpack_bits(bits_u8, cap), want) and torch.equal(bits_y, bits_u8)


def png_bytes(u8):
    from PIL import Image
    out = []
    for img in u8.cpu().numpy():
        f = io.BytesIO()
        Image.fromarray(img).save(f, format="PNG")
        out.append(f.getvalue())
    return out


def test_same_seed_same_png_bytes(tiny):
    from ideas_amd import stego
    from ideas_amd.op import quantize_image
    trainer, args = tiny[1]
    models = stego.models_of(trainer)
    runs = []
    for seed in (5, 5, 6):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        bits = stego.random_bits(2, stego.capacity_bits(args, 2), torch.Generator(device="cuda").manual_seed(1), "cuda")
        images, _ = stego.hide(models, args, bits, 2, 0.5, generator=gen)
        runs.append(png_bytes(quantize_image(images, dequantize=False)[0]))
    assert runs[0] == runs[1] and runs[0] != runs[2]


# ------------------------------------------------------------------------------------------------- evaluate
class StandInInception(torch.nn.Module):
    """Any module returning ``[features [B, 2048, 1, 1]]``."""

    def forward(self, x):
        f = x.float().mean((2, 3))                            # [B, 3]
        return [f.repeat(1, 683)[:, :2048].reshape(x.shape[0], 2048, 1, 1) * torch.linspace(0.5, 1.5, 2048, device=x.device).view(1, -1, 1, 1)]


@pytest.mark.parametrize("container", ["u8", "float"])
def test_evaluate_counts_what_explicit_calls_count(tiny, container):
    from ideas_amd import stego
    from ideas_amd.op import quantize_image
    trainer, args = tiny[2]
    models = stego.models_of(trainer)
    sigma, delta = 2, 0.25
    cap = stego.capacity_bits(args, sigma)
    res = stego.evaluate(models, args, sigma, delta, 6, 4, torch.Generator(device="cuda").manual_seed(21), container=container,
                         inception=StandInInception())
    assert res["n_bits"] == 6 * cap and res["stats"].n == 6
    gen = torch.Generator(device="cuda").manual_seed(21)
    n_err, l1 = 0, 0.0
    for b in (4, 2):
        bits = stego.random_bits(b, cap, gen, "cuda")
        images, Z = stego.hide(models, args, bits, sigma, delta, generator=gen)
        received = quantize_image(images)[1] if container == "u8" else images
        _, hat_Z, ne = stego.extract(models, args, received, sigma, ref_bits=bits)
        n_err += int(ne.sum())
        l1 += float((hat_Z.float() - Z).abs().double().sum())
    assert res["n_err"] == n_err and 0 <= n_err <= 6 * cap
    assert res["acc"] == 1.0 - n_err / (6 * cap)
    assert abs(res["l1"] - l1 / (6 * cap // sigma)) <= 1e-9 * max(1.0, l1)
    plain = stego.evaluate(models, args, sigma, delta, 6, 4, torch.Generator(device="cuda").manual_seed(21), container=container)
    assert plain["stats"] is None and plain["n_err"] == n_err
    even = stego.evaluate(models, args, sigma, delta, 4, 2, torch.Generator(device="cuda").manual_seed(21), container=container)
    assert even["n_bits"] == 4 * cap                           # a zero remainder is skipped


# ------------------------------------------------------------------------------------------------- command lines
def run_cli(script, *argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, script), *map(str, argv)], capture_output=True, text=True, timeout=300)


def test_command_lines_on_an_untrained_checkpoint(tiny, tmp_path):
    """hide.py writes the containers, extract.py reads them back: the bits are what ``stego.extract`` gives in-process on the files.
    The networks are untrained, so the frame's check must fail: status 1, the CRC message, no payload file."""
    from PIL import Image
    from ideas_amd import checkpoint, stego
    trainer, args = tiny[2]
    ckpt = tmp_path / "0.pt"
    checkpoint.save(str(ckpt), trainer, args, 0)
    payload = tmp_path / "payload.bin"
    payload.write_bytes(bytes(range(40)))
    out_dir = tmp_path / "containers"
    sigma = 2
    cap_bytes = stego.capacity_bits(args, sigma) // 8
    n_img = -(-(8 + 40) // cap_bytes)
    r = run_cli("hide.py", "--ckpt", ckpt, "--payload", payload, "--out", out_dir, "--sigma", sigma, "--seed", 3)
    assert r.returncode == 0, r.stderr[-2000:]
    files = sorted(os.listdir(out_dir))
    assert files == [f"{i:06d}.png" for i in range(n_img)] and f"{n_img} image" in r.stdout
    arrs = []
    for f in files:
        with Image.open(out_dir / f) as img:
            assert img.size == (64, 64) and img.mode == "RGB"
            arrs.append(torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()))

    recovered, dump = tmp_path / "recovered.bin", tmp_path / "bits.npy"
    r = run_cli("extract.py", "--ckpt", ckpt, "--sigma", sigma, "--out", recovered, "--dump_bits", dump, *[out_dir / f for f in files])
    assert r.returncode == 1, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    said = [line for line in r.stderr.splitlines() if line.startswith("extract.py:")]
    assert len(said) == 1 and "CRC" in said[0] and not recovered.exists()
    models, largs = stego.load_models(str(ckpt), "cuda")
    assert largs.N == 2 and not any(m.training for m in models.values())
    bits, _ = stego.extract(models, largs, torch.stack(arrs).cuda(), sigma)
    assert np.array_equal(np.load(dump), bits.cpu().numpy())
    with pytest.raises(stego.PayloadError):
        stego.unframe(bits)
