"""The payload-coding kernels (csrc/ecc.hip) on the GPU against the numpy restatement tests/ecc_ref.py, bit for bit: the encoder, the
soft demapper and the Viterbi decoder through both survivor routes; then the coded pipeline end to end on stand-in networks behind a
noisy channel, ``stego.evaluate(code=...)`` against explicit calls, and the three command lines with ``--ecc``.  Every raw call writes
into sentinel-guarded buffers and must leave its inputs unchanged."""
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ecc_ref as R
from conftest import ROOT
from test_attacks_gpu import Guarded, place

pytestmark = pytest.mark.gpu

RATE_NAMES = sorted(R.RATES)


def rate_id(rate):
    return R.RATES[rate][0]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------- encode
def raw_encode(info, n, k, rate, P, Pinv, fill=None):
    from ideas_amd import _lib
    b, nbytes = info.shape[0], (n + 7) // 8
    iin = place(dev(info), 0)
    fin = place(dev(fill), 0) if fill is not None else None
    out = Guarded(b * nbytes)
    rc = _lib.load().ideas_ecc_encode(out.ptr(), iin.ptr(), fin.ptr() if fin else None, b, n, k, rate_id(rate), P, Pinv, _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert out.intact() and iin.intact() and (fin is None or fin.intact())
    assert np.array_equal(iin.get(torch.uint8, info.shape).cpu().numpy(), info)
    assert fin is None or np.array_equal(fin.get(torch.uint8, fill.shape).cpu().numpy(), fill)
    return out.get(torch.uint8, (b, nbytes)).cpu().numpy()


@pytest.mark.parametrize("n", [28, 29, 100, 256, 2048])
@pytest.mark.parametrize("rate", RATE_NAMES)
def test_encode_is_the_reference_bit_for_bit(rate, n):
    from ideas_amd import ecc
    pl = R.plan(n, rate)
    rng = np.random.default_rng(1000 * rate_id(rate) + n)
    for b in (1, 3):
        info = rng.integers(0, 256, (b, pl["k"] // 8), dtype=np.uint8)
        info[0, 0], info[0, -1] = 0x80, 0x01                  # the first and the last information bit
        fill = R.pack(rng.integers(0, 2, (b, n)))
        for f in (fill, None):
            got = raw_encode(info, n, pl["k"], rate, pl["P"], pl["Pinv"], f)
            assert np.array_equal(got, R.encode(info, n, rate, f)), (b, f is None)
            if n % 8:
                assert not (got[:, -1] & ((1 << (8 - n % 8)) - 1)).any()      # pad bits are written as zero
        code = ecc.Code(n, rate)
        assert np.array_equal(ecc.encode(code, dev(info), fill=dev(fill)).cpu().numpy(), R.encode(info, n, rate, fill))
        assert np.array_equal(ecc.encode(code, dev(info)).cpu().numpy(), R.encode(info, n, rate))


def test_encode_draws_its_fill_like_random_bits():
    from ideas_amd import ecc, stego
    code = ecc.Code(100, "3/4")
    info = stego.random_bits(3, code.k_bits, torch.Generator(device="cuda").manual_seed(5), "cuda")
    got = ecc.encode(code, info, generator=torch.Generator(device="cuda").manual_seed(6))
    fill = stego.random_bits(3, 100, torch.Generator(device="cuda").manual_seed(6), "cuda")
    assert np.array_equal(got.cpu().numpy(), R.encode(info.cpu().numpy(), 100, "3/4", fill.cpu().numpy()))
    assert not torch.equal(got, ecc.encode(code, info))


# ------------------------------------------------------------------------------------------------- soft values
def soft_inputs(sigma):
    """Every bin edge and centre, the float32 neighbours of the edges, +-1, values beyond the clamp, zeros, NaN."""
    step = 2.0 / (1 << sigma)
    edges = (np.arange((1 << sigma) + 1) * step - 1).astype(np.float32)
    centres = ((np.arange(1 << sigma) + 0.5) * step - 1).astype(np.float32)
    extra = np.array([1, -1, 1.5, -1.5, 100, -100, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e-30, -1e-30, 0.3, -0.7], np.float32)
    return np.concatenate((edges, np.nextafter(edges, np.float32(-np.inf)), np.nextafter(edges, np.float32(np.inf)), centres, extra))


def raw_soft(z, sigma, gain):
    from ideas_amd import _lib
    b, L = z.shape
    zin = place(z, 0)
    out = Guarded(b * L * sigma)
    rc = _lib.load().ideas_ecc_soft(out.ptr(), zin.ptr(), b, L, sigma, gain, _lib.act_dtype(z), _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert out.intact() and zin.intact()
    assert torch.equal(zin.get(torch.int8, (z.numel() * z.element_size(),)), z.contiguous().view(-1).view(torch.int8))
    return out.get(torch.int8, (b, L * sigma)).cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("sigma", [1, 2, 3, 8])
def test_soft_values_are_the_f32_restatement(sigma, dtype):
    from ideas_amd import ecc
    L = 37
    vals = torch.from_numpy(soft_inputs(sigma))
    if dtype == torch.bfloat16:                               # the same set in bf16, with the bf16 neighbours of what it rounds to
        v = vals.bfloat16()
        bits = v.view(torch.int16)
        vals = torch.cat((v, (bits + 1).view(torch.bfloat16), (bits - 1).view(torch.bfloat16)))
    rows = -(-vals.numel() // L)
    filler = (torch.rand(rows * L, generator=torch.Generator().manual_seed(sigma)) * 2.4 - 1.2).to(vals.dtype)
    z = torch.cat((vals, filler))[:rows * L].reshape(rows, L).contiguous()
    for gain in (64.0, 7.5):
        want = R.soft(z.float().numpy(), sigma, gain)
        got = raw_soft(z.cuda(), sigma, gain)
        assert got.shape == (rows, L * sigma) and np.array_equal(got, want), (gain, int((got != want).sum()))
    assert np.array_equal(ecc.soft_bits(z.cuda(), sigma).cpu().numpy(), R.soft(z.float().numpy(), sigma))
    assert np.array_equal(ecc.soft_bits(z.cuda(), sigma, gain=7.5).cpu().numpy(), R.soft(z.float().numpy(), sigma, 7.5))


# ------------------------------------------------------------------------------------------------- Viterbi
def raw_viterbi(soft, n, k, rate, P, workspace, want_metric=True):
    """ideas_ecc_viterbi through the LDS route (workspace False) or the global one; -> (info rows, metric or None)."""
    from ideas_amd import _lib
    b, T = soft.shape[0], k + R.TAIL
    sin = place(dev(soft), 0)
    info, met = Guarded(b * (k // 8)), Guarded(4 * b)
    ws = Guarded(8 * b * T) if workspace else None
    rc = _lib.load().ideas_ecc_viterbi(info.ptr(), met.ptr() if want_metric else None, sin.ptr(), ws.ptr() if ws else None, b, n, k,
                                       rate_id(rate), P, _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert info.intact() and met.intact() and sin.intact() and (ws is None or ws.intact())
    assert np.array_equal(sin.get(torch.int8, soft.shape).cpu().numpy(), soft)
    assert want_metric or met.untouched()
    return info.get(torch.uint8, (b, k // 8)).cpu().numpy(), met.get(torch.int32, (b,)).cpu().numpy() if want_metric else None


def soft_kinds(rng, b, n, k, rate, P):
    """Pure noise (many near-ties), all zeros (the tie rule alone decides), all +-127, codewords plus noise."""
    yield "noise", rng.integers(-128, 128, (b, n)).astype(np.int8)
    yield "zeros", np.zeros((b, n), np.int8)
    yield "+127", np.full((b, n), 127, np.int8)
    yield "-127", np.full((b, n), -127, np.int8)
    yield "+-127", (rng.integers(0, 2, (b, n)) * 254 - 127).astype(np.int8)
    info = rng.integers(0, 256, (b, k // 8), dtype=np.uint8)
    coded = R.unpack(R.encode(info, n, rate, R.pack(rng.integers(0, 2, (b, n))), k=k, P=P), n).astype(np.int32)
    yield "codeword+noise", np.clip((coded * 2 - 1) * 24 + np.rint(rng.normal(0, 20, (b, n))), -127, 127).astype(np.int8)


def check_viterbi(soft, n, k, rate, P, tag):
    want_info, want_metric = R.viterbi(soft, n, k, rate, P)
    for workspace in (False, True):
        info, metric = raw_viterbi(soft, n, k, rate, P, workspace)
        assert np.array_equal(metric, want_metric), (tag, workspace, metric.tolist(), want_metric.tolist())
        assert np.array_equal(info, want_info), (tag, workspace)
    return want_info, want_metric


@pytest.mark.parametrize("T", [14, 30, 38, 62, 70, 126, 134])
@pytest.mark.parametrize("rate", RATE_NAMES)
def test_viterbi_is_the_reference_exactly(rate, T):
    """Steps on both sides of the kernel's 64-step chunk, and n three bits above the codeword so that fill positions exist."""
    k = T - R.TAIL
    n = R.kept(T, rate) + 3
    pl = R.plan(n, rate)
    assert pl["k"] == k
    rng = np.random.default_rng(100 * T + rate_id(rate))
    for b in (1, 5):
        for kind, soft in soft_kinds(rng, b, n, k, rate, pl["P"]):
            check_viterbi(soft, n, k, rate, pl["P"], (kind, b))
    soft = rng.integers(-128, 128, (2, n)).astype(np.int8)                       # the metric is optional
    assert np.array_equal(raw_viterbi(soft, n, k, rate, pl["P"], False, want_metric=False)[0], R.viterbi(soft, n, k, rate, pl["P"])[0])


@pytest.mark.parametrize("rate,n", [("1/2", 256), ("2/3", 256), ("3/4", 256), ("3/4", 2048)])
def test_decode_recovers_noisy_codewords(rate, n):
    from ideas_amd import ecc
    code = ecc.Code(n, rate)
    rng = np.random.default_rng(n + rate_id(rate))
    info = rng.integers(0, 256, (5, code.k_bytes), dtype=np.uint8)
    coded = R.unpack(R.encode(info, n, rate), n).astype(np.int32)
    soft = np.clip((coded * 2 - 1) * 40 + np.rint(rng.normal(0, 14, coded.shape)), -127, 127).astype(np.int8)
    want_info, want_metric = check_viterbi(soft, n, code.k_bits, rate, code.stride, rate)
    assert np.array_equal(want_info, info)
    got, metric = ecc.decode(code, dev(soft))
    assert got.dtype == torch.uint8 and metric.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy(), info) and np.array_equal(metric.cpu().numpy(), want_metric)


def test_viterbi_long_codewords_take_the_workspace():
    """T = 4094 is the longest codeword in LDS (and runs both routes); n = 20000 gives T = 9998, which ``decode`` sends through a
    workspace of its own and the raw call refuses without one."""
    from ideas_amd import _lib, ecc
    from ideas_amd.op.ecc import LDS_STEPS
    rng = np.random.default_rng(20000)
    code = ecc.Code(8188, "1/2")
    assert code.steps == 4094 <= LDS_STEPS
    soft = rng.integers(-128, 128, (1, 8188)).astype(np.int8)
    check_viterbi(soft, 8188, code.k_bits, "1/2", code.stride, "lds cap")
    code = ecc.Code(20000, "1/2")
    assert code.steps == 9998 > LDS_STEPS
    info = rng.integers(0, 256, (1, code.k_bytes), dtype=np.uint8)
    coded = R.unpack(R.encode(info, 20000, "1/2"), 20000).astype(np.int32)
    soft = np.clip((coded * 2 - 1) * 32 + np.rint(rng.normal(0, 16, coded.shape)), -127, 127).astype(np.int8)
    print(f"n=20000: {int(((soft > 0) != (coded > 0)).sum())} of 20000 hard decisions wrong")
    want_info, want_metric = R.viterbi(soft, 20000, code.k_bits, "1/2", code.stride)
    got, metric = ecc.decode(code, dev(soft))
    assert np.array_equal(got.cpu().numpy(), want_info) and np.array_equal(metric.cpu().numpy(), want_metric)
    assert np.array_equal(want_info, info)
    s = dev(soft)
    out = torch.empty(1, code.k_bytes, dtype=torch.uint8, device="cuda")
    rc = _lib.load().ideas_ecc_viterbi(out.data_ptr(), None, s.data_ptr(), None, 1, 20000, code.k_bits, 0, code.stride, _lib.stream_ptr())
    assert rc == -3


@pytest.mark.parametrize("rate", ["1/2", "3/4"])
def test_long_interleaver_takes_the_64_bit_products(rate):
    """Above n = 65536 message bits the de-interleaver's i * P no longer fits 32 bits and the kernel takes the 64-bit product, as the
    encoder's (kb * 8) * Pinv does: n = 120000 (N = 3, sigma = 8 at 1024 x 1024 gives 98304) has (m - 1) P >= 2^32, so a product
    truncated to 32 bits lands on another position.  The encoder, the raw decoder with a workspace and ``ecc.decode`` are compared
    with the REFERENCE's output, not with ``info`` (at 3/4 with this noise the code does not recover it); row 1 of the soft values is
    pure noise."""
    from ideas_amd import ecc
    n, b = 120_000, 2
    pl = R.plan(n, rate)
    k, P = pl["k"], pl["P"]
    assert n > 65536 and (pl["m"] - 1) * P >= 2 ** 32 and ((n + 7) // 8 * 8 - 8) * pl["Pinv"] >= 2 ** 32
    rng = np.random.default_rng(n + rate_id(rate))
    info = rng.integers(0, 256, (b, k // 8), dtype=np.uint8)
    fill = R.pack(rng.integers(0, 2, (b, n)))
    want = R.encode(info, n, rate, fill)
    assert np.array_equal(raw_encode(info, n, k, rate, P, pl["Pinv"], fill), want)
    coded = R.unpack(want, n).astype(np.int32)
    soft = np.clip((coded * 2 - 1) * 32 + np.rint(rng.normal(0, 16, coded.shape)), -127, 127).astype(np.int8)
    soft[1] = rng.integers(-128, 128, n).astype(np.int8)
    want_info, want_metric = R.viterbi(soft, n, k, rate, P)
    got_info, got_metric = raw_viterbi(soft, n, k, rate, P, True)
    assert np.array_equal(got_metric, want_metric), (got_metric.tolist(), want_metric.tolist())
    assert np.array_equal(got_info, want_info)
    code = ecc.Code(n, rate)
    assert (code.k_bits, code.stride) == (k, P)
    dec_info, dec_metric = ecc.decode(code, dev(soft))
    assert np.array_equal(dec_info.cpu().numpy(), want_info) and np.array_equal(dec_metric.cpu().numpy(), want_metric)


# ------------------------------------------------------------------------------------------------- end to end on stand-in networks
BLOCK = 16
E2E = SimpleNamespace(N=1, image_size=256, texture_channel=8)          # 16 x 16 elements: n = 256 message bits at sigma = 1
# chosen with tests/ecc_ref.py on the CPU (same draws: the generator is a CPU one): noise of 300 levels on every pixel leaves 7 to 14
# wrong bits of 256 in every image of seeds 0..7 (about 4 %), the plain frame fails and the reference decoder returns every row
E2E_NOISE, E2E_SEED, E2E_PAYLOAD = 300, 4, bytes(range(101, 138))


def stand_in_models():
    """``Gstru`` and ``Ex`` are the identity, ``G`` paints every element of Z as a 16 x 16 block of grey, ``E`` averages the blocks."""
    def G(s, texture):
        return s.repeat_interleave(BLOCK, 2).repeat_interleave(BLOCK, 3).expand(-1, 3, -1, -1).contiguous()

    def E(x):
        return torch.nn.functional.avg_pool2d(x.float().mean(1, keepdim=True), BLOCK), None
    return {"Gstru": lambda z: z, "G": G, "E": E, "Ex": lambda s: s}


def send(models, rows, gen, device):
    """Packed message rows through hide -> 8-bit container -> noise; the jitter, then the channel's noise, from the CPU generator."""
    from ideas_amd import attacks, stego
    from ideas_amd.op import quantize_image
    b = rows.shape[0]
    jitter = torch.rand(b, 256, generator=gen).to(device)
    images, _ = stego.hide(models, E2E, rows, 1, 0.5, texture=torch.zeros(b, 8, device=device), jitter=jitter)
    u8 = quantize_image(images, dequantize=False)[0]
    return attacks.parse(f"noise:{E2E_NOISE}")(u8, gen)[1]


def test_coded_payload_survives_a_channel_that_breaks_the_plain_frame():
    from ideas_amd import ecc, stego
    models = stand_in_models()
    code = ecc.Code(stego.capacity_bits(E2E, 1), "1/2")
    assert code.n_bits == 256 and code.k_bytes == 15

    # without the code: wrong bits, and the frame's check refuses them
    gen = torch.Generator().manual_seed(E2E_SEED)
    plain = stego.frame(E2E_PAYLOAD, 32, gen).cuda()
    bits, _, n_err = stego.extract(models, E2E, send(models, plain, gen, "cuda"), 1, ref_bits=plain)
    print(f"plain frame: {n_err.tolist()} wrong bits of 256 an image")
    assert int(n_err.sum()) > 0
    with pytest.raises(stego.PayloadError):
        stego.unframe(bits)

    # with it: the hard decisions are as wrong, the decoded rows are the frame
    gen = torch.Generator().manual_seed(E2E_SEED)
    coded = stego.frame_coded(E2E_PAYLOAD, code, gen, "cuda")
    assert tuple(coded.shape) == (3, 32)
    received = send(models, coded, gen, "cuda")
    hard, hat_Z, n_err = stego.extract(models, E2E, received, 1, ref_bits=coded)
    print(f"coded: {n_err.tolist()} wrong bits of 256 an image before decoding")
    assert int(n_err.min()) > 0
    with pytest.raises(stego.PayloadError):
        stego.unframe(hard)
    info, hat_Z2, metric = stego.extract_coded(models, E2E, received, 1, code)
    assert torch.equal(hat_Z2, hat_Z) and tuple(info.shape) == (3, 15) and tuple(metric.shape) == (3,)
    assert stego.unframe(info) == E2E_PAYLOAD
    # the reference decoder on the same soft values: the same rows, the same metrics
    soft = ecc.soft_bits(hat_Z.reshape(3, -1), 1)
    assert np.array_equal(soft.cpu().numpy(), R.soft(hat_Z.reshape(3, -1).cpu().numpy(), 1))
    want_info, want_metric = R.decode(soft.cpu().numpy(), 256, "1/2")
    assert np.array_equal(info.cpu().numpy(), want_info) and np.array_equal(metric.cpu().numpy(), want_metric)
    assert stego.unframe(want_info) == E2E_PAYLOAD


# ------------------------------------------------------------------------------------------------- evaluate
@pytest.fixture(scope="module")
def tiny():
    from test_stego_gpu import tiny_trainer
    return tiny_trainer(2)


def test_evaluate_with_a_code_counts_what_explicit_calls_count(tiny):
    from ideas_amd import attacks, ecc, stego
    from ideas_amd.op import quantize_image, unpack_bits
    trainer, args = tiny
    models = stego.models_of(trainer)
    sigma, delta = 8, 0.25
    cap = stego.capacity_bits(args, sigma)
    assert cap == 256
    code = ecc.Code(cap, "2/3")
    res = stego.evaluate(models, args, sigma, delta, 5, 3, torch.Generator(device="cuda").manual_seed(41), code=code)
    gen = torch.Generator(device="cuda").manual_seed(41)
    n_err = n_info_err = n_row_err = 0
    l1 = 0.0
    for b in (3, 2):
        info = stego.random_bits(b, code.k_bits, gen, "cuda")
        fill = stego.random_bits(b, cap, gen, "cuda")
        bits = ecc.encode(code, info, fill=fill)
        images, Z = stego.hide(models, args, bits, sigma, delta, generator=gen)
        _, hat_Z, ne = stego.extract(models, args, quantize_image(images)[1], sigma, ref_bits=bits)
        n_err += int(ne.sum())
        l1 += float((hat_Z.float() - Z).abs().double().sum())
        soft = R.soft(hat_Z.reshape(b, -1).float().cpu().numpy(), sigma)
        wrong = (R.unpack(R.decode(soft, cap, "2/3")[0], code.k_bits) != unpack_bits(info, code.k_bits).cpu().numpy()).sum(1)
        n_info_err += int(wrong.sum())
        n_row_err += int((wrong > 0).sum())
    assert (res["n_err"], res["n_bits"]) == (n_err, 5 * cap) and res["acc"] == 1.0 - n_err / (5 * cap)
    assert (res["n_info_err"], res["n_info_bits"], res["n_row_err"]) == (n_info_err, 5 * code.k_bits, n_row_err)
    assert res["info_acc"] == 1.0 - n_info_err / (5 * code.k_bits) and res["rate"] == "2/3"
    assert abs(res["l1"] - l1 / (5 * cap // sigma)) <= 1e-9 * max(1.0, l1)
    assert 0 < n_row_err <= 5                                   # untrained networks: the decoder has nothing to work with
    chained = stego.evaluate(models, args, sigma, delta, 5, 3, torch.Generator(device="cuda").manual_seed(41), code=code,
                             attack=attacks.parse("none"))
    assert chained["n_info_err"] == n_info_err and chained["attack"] == "none"
    with pytest.raises(ValueError, match="message bits"):
        stego.evaluate(models, args, sigma, delta, 5, 3, code=ecc.Code(128, "1/2"))


def test_evaluate_without_a_code_is_unchanged(tiny):
    from ideas_amd import stego
    from ideas_amd.op import quantize_image
    trainer, args = tiny
    models = stego.models_of(trainer)
    sigma, delta = 8, 0.25
    cap = stego.capacity_bits(args, sigma)
    res = stego.evaluate(models, args, sigma, delta, 5, 3, torch.Generator(device="cuda").manual_seed(41), code=None)
    assert sorted(res) == ["acc", "attack", "l1", "n_bits", "n_err", "stats"]
    gen = torch.Generator(device="cuda").manual_seed(41)
    n_err, l1 = 0, 0.0
    for b in (3, 2):
        bits = stego.random_bits(b, cap, gen, "cuda")
        images, Z = stego.hide(models, args, bits, sigma, delta, generator=gen)
        _, hat_Z, ne = stego.extract(models, args, quantize_image(images)[1], sigma, ref_bits=bits)
        n_err += int(ne.sum())
        l1 += float((hat_Z.float() - Z).abs().double().sum())
    assert res["n_err"] == n_err and abs(res["l1"] - l1 / (5 * cap // sigma)) <= 1e-9 * max(1.0, l1)
    assert res == stego.evaluate(models, args, sigma, delta, 5, 3, torch.Generator(device="cuda").manual_seed(41))


# ------------------------------------------------------------------------------------------------- command lines
def run_cli(script, *argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, script), *map(str, argv)], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def ckpt(tiny, tmp_path_factory):
    from ideas_amd import checkpoint
    trainer, args = tiny
    path = str(tmp_path_factory.mktemp("ecc_ckpt") / "0.pt")
    checkpoint.save(path, trainer, args, 0)
    return path


def test_hide_and_extract_with_ecc_on_an_untrained_checkpoint(tiny, ckpt, tmp_path):
    """As the plain command-line test: hide.py --ecc writes the containers, extract.py --ecc decodes them to what ``extract_coded``
    gives in-process; untrained networks, so status 1, the CRC line and no payload file."""
    from PIL import Image
    from ideas_amd import ecc, stego
    trainer, args = tiny
    payload = tmp_path / "payload.bin"
    payload.write_bytes(bytes(range(40)))
    out_dir = tmp_path / "containers"
    sigma = 8
    code = ecc.Code(stego.capacity_bits(args, sigma), "1/2")
    n_img = -(-(8 + 40) // code.k_bytes)
    r = run_cli("hide.py", "--ckpt", ckpt, "--payload", payload, "--out", out_dir, "--sigma", sigma, "--seed", 3, "--ecc", "1/2")
    assert r.returncode == 0, r.stderr[-2000:]
    files = sorted(os.listdir(out_dir))
    assert files == [f"{i:06d}.png" for i in range(n_img)] and f"{n_img} image" in r.stdout
    assert f"ECC 1/2: {code.k_bytes} info bytes" in r.stdout
    arrs = []
    for f in files:
        with Image.open(out_dir / f) as img:
            arrs.append(torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()))

    recovered, dump = tmp_path / "recovered.bin", tmp_path / "bits.npy"
    r = run_cli("extract.py", "--ckpt", ckpt, "--sigma", sigma, "--out", recovered, "--dump_bits", dump, "--ecc", "1/2",
                *[out_dir / f for f in files])
    assert r.returncode == 1, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    said = [line for line in r.stderr.splitlines() if line.startswith("extract.py:")]
    assert len(said) == 1 and "CRC" in said[0] and not recovered.exists()
    models, largs = stego.load_models(str(ckpt), "cuda")
    info, _, _ = stego.extract_coded(models, largs, torch.stack(arrs).cuda(), sigma, code)
    assert np.load(dump).shape == (n_img, code.k_bytes) and np.array_equal(np.load(dump), info.cpu().numpy())
    with pytest.raises(stego.PayloadError):
        stego.unframe(info)


def test_evaluate_command_line_with_ecc_appends_the_decoders_figures(ckpt):
    sigma = 8
    r = run_cli("evaluate.py", "--sigma", sigma, "--delta", "0.5", "--n_sample", "2", "--batch", "2", "--ecc", "1/2", ckpt)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and re.fullmatch(r"sigma=8 delta=50% ACC: [01]\.\d{4} ECC=1/2 INFO_ACC: [01]\.\d{4} FER: [01]\.\d{4}", lines[0]), r.stdout
