"""Every capped-grid kernel sent round its loop a second time (tests/grid_caps.py names the launches and their caps).

The method is that of tests/test_jpeg_file_gpu.py::test_grid_stride_loop_turns_over.  All of these kernels treat samples, rows, pixels or
planes independently, so: K = 5 distinct small items go through the kernel and are checked against the reference and with the tolerance
(or byte equality) of the module that owns the kernel; then the kernel runs on ``small[arange(B) % K]`` with B just past ``cap x units``
of the launch, and the big output must be BITWISE ``small_out[arange(B) % K]``.  No new tolerance: a difference between the first trip
and the second is a finding.  What only shows from the second trip on: the stride expression, index arithmetic narrowed to 32 bits, a
partial last trip, and the barrier at the top of a loop that re-stages LDS (csrc/attack_spatial.hip).

Every call goes through the C ABI on raw sentinel-guarded buffers and checks its return code and the guard bands.  Every big tensor is
made on the device by one index gather straight into its buffer and compared on the device by torch.equal, in pieces of 64 MiB; nothing
of size B crosses to the host.  Each test asserts from its row of the table that its work exceeds ``cap x units`` and by how much, and
states the device memory it holds (buffers of the call plus one piece of the comparison)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attacks_ref
import ecc_ref
import grid_caps
import spatial_ref
from conftest import rel_err
from test_attacks_gpu import Guarded, check_against_oracle

pytestmark = pytest.mark.gpu

K = 5
F32, BF = torch.float32, torch.bfloat16
PIECE = 1 << 26                # bytes of the expected rows made at a time for the comparison


def lib():
    from ideas_amd import _lib
    return _lib


def enum(dtype):
    return lib().BF16 if dtype == BF else lib().F32


def beyond(key, work):
    """Units of ``work`` past what the capped grid of row ``key`` covers in its first trip; asserted positive and small."""
    row = grid_caps.CAPS[key]
    first = row.cap * row.units
    assert work > first, (key, work, first)
    assert work - first <= 8 * max(row.units, 2), (key, work - first, "the last trip is meant to be a handful of threads or workgroups")
    return work - first


def byte_rows(t):
    """[k, ...] of any dtype -> uint8 [k, bytes of an item]"""
    t = t.contiguous()
    return t.view(t.shape[0], -1).view(torch.uint8)


def gather(small, idx, skew=0):
    """``small[idx]`` made on the device by one index gather straight into a guarded buffer, ``skew`` bytes off 16-byte alignment."""
    rows = byte_rows(small)
    g = Guarded(idx.numel() * rows.shape[1], skew)
    torch.index_select(rows, 0, idx, out=g.view.view(idx.numel(), rows.shape[1]))
    return g


def fixed(t, skew=0):
    """An operand that is the same for every item (tables, FIR), guarded."""
    return gather(t.reshape((1,) + tuple(t.shape)), torch.zeros(1, dtype=torch.int64, device="cuda"), skew)


def call(name, *args):
    rc = getattr(lib().load(), name)(*args, lib().stream_ptr())
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()


def settled(*buffers):
    for g in buffers:
        assert g is None or g.intact()


def rows_of(g, n):
    return g.view.view(n, -1)


def same_rows(big, small, idx):
    """On the device: row i of the big buffer is bitwise row idx[i] of the small one."""
    want, got = rows_of(small, K), rows_of(big, idx.numel())
    assert got.shape[1] == want.shape[1]
    step = max(1, PIECE // want.shape[1])
    return all(torch.equal(got[i:i + step], want[idx[i:i + step]]) for i in range(0, idx.numel(), step))


def second_trip(b, run, check):
    """``run(idx) -> {name: guarded output}`` on the K items (checked by ``check``) and on B copies of them."""
    first = torch.arange(K, device="cuda")
    small = run(first)
    check(small)
    idx = torch.arange(b, device="cuda") % K
    big = run(idx)
    assert sorted(big) == sorted(small)
    for name in sorted(big):
        assert same_rows(big[name], small[name], idx), name
    del big
    torch.cuda.empty_cache()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def decode_of(u8):
    """what the receiver makes of NHWC bytes, as NHWC floats"""
    from ideas_amd import data
    return data.u8_to_f32(u8).permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------- pad.hip
@pytest.mark.parametrize("dtype,c", [(F32, 1), (BF, 8)], ids=["f32-c1-element", "bf16-c8-vector"])
def test_reflect_fold(dtype, c):
    """B = 167 773 samples of 5 x 5 with pad 2: 4 194 325 channel vectors (one a pixel in both cases) against 16384 x 256, 21 threads
    on the second trip.  f32, C = 1: 71 MB; bf16, C = 8: 285 MB.  Small items against autograd of F.pad(mode="reflect") in f64 with the
    bounds of tests/test_ops_gpu.py: 1e-6 of the largest element in f32; 2^-8 |ref| + 2^-20 mag in bf16."""
    h = w = 5
    pad, b = 2, 167_773
    assert beyond("pad.reflect_fold", b * h * w * 1) == 21                     # one vector (bf16, C = 8) or one element (C = 1) a pixel
    gp = torch.randn(K, c, h + 2 * pad, w + 2 * pad, generator=gen(1)).to(dtype).double()
    x = torch.zeros(K, c, h, w, dtype=torch.float64, requires_grad=True)
    padded = F.pad(x, [pad] * 4, mode="reflect")
    (ref,) = torch.autograd.grad(padded, x, gp, retain_graph=True)
    (mag,) = torch.autograd.grad(padded, x, gp.abs())
    small_in = gp.permute(0, 2, 3, 1).to(dtype).cuda()
    esize = 2 if dtype == BF else 4

    def run(idx):
        n = idx.numel()
        gpad, gx = gather(small_in, idx), Guarded(n * h * w * c * esize)
        call("ideas_reflect_fold", gx.ptr(), gpad.ptr(), n, h, w, c, pad, enum(dtype))
        settled(gx, gpad)
        return {"gx": gx}

    def check(small):
        got = small["gx"].get(dtype, (K, h, w, c)).permute(0, 3, 1, 2).double().cpu()
        if dtype == BF:
            assert bool(((got - ref).abs() <= 2.0 ** -8 * ref.abs() + 2.0 ** -20 * mag).all())
        else:
            assert rel_err(got, ref) < 1e-6
    second_trip(b, run, check)


# ------------------------------------------------------------------------------------------------- image_io.hip
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flips"])
def test_image_u8_to_f32(flip):
    """B = 46 604 images of 3 x 5 x 3: 2 097 180 bytes against 8192 x 256, 28 threads on the second trip; 13 MB.  The per-sample flip
    bytes follow the same pattern.  Small items: bitwise ((v / 255) - 0.5) / 0.5 in f32 on the host."""
    h, w, c, b = 3, 5, 3, 46_604
    assert beyond("image_io.u8_to_f32", b * h * w * c) == 28
    x = torch.randint(0, 256, (K, h, w, c), generator=gen(2), dtype=torch.uint8)
    x.view(-1)[:2] = torch.tensor([0, 255], dtype=torch.uint8)
    flags = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8).view(K, 1)
    small_x, small_f = x.cuda(), flags.cuda()

    def run(idx):
        n = idx.numel()
        xin, fin = gather(small_x, idx), (gather(small_f, idx) if flip else None)
        y = Guarded(4 * n * h * w * c)
        call("ideas_image_u8_to_f32", y.ptr(), xin.ptr(), fin.ptr() if fin else None, n, h, w, c, 0.5, 0.5)
        settled(y, xin, fin)
        return {"y": y}

    def check(small):
        src = torch.where(flags.view(K, 1, 1, 1).bool(), x.flip(2), x) if flip else x
        want = ((src.float() / 255.0) - 0.5) / 0.5
        assert torch.equal(small["y"].get(F32, (K, h, w, c)).cpu(), want)
    second_trip(b, run, check)


# ------------------------------------------------------------------------------------------------- stego.hip
@pytest.mark.parametrize("jitter", [False, True], ids=["centres", "jitter"])
def test_bits_to_tensor(jitter):
    """B = 113 360 rows of L = 37 elements at sigma = 3 (14 bytes a row): 4 194 320 elements against 16384 x 256, 16 threads on the
    second trip; 35 MB.  Small items: bitwise utils.message_to_tensor on the host."""
    from ideas_amd import utils as U
    from ideas_amd.op import pack_bits
    L, sigma, delta, b = 37, 3, 0.3, 113_360
    assert beyond("stego.bits_to_tensor", b * L) == 16
    M = torch.randint(0, 2, (K, L * sigma), generator=gen(3), dtype=torch.float)
    J = torch.rand(K, L, generator=gen(4))
    small_bits, small_j = pack_bits(M).cuda(), J.cuda()
    assert tuple(small_bits.shape) == (K, 14)

    def run(idx):
        n = idx.numel()
        bits, jit = gather(small_bits, idx), (gather(small_j, idx) if jitter else None)
        z = Guarded(4 * n * L)
        call("ideas_bits_to_tensor", z.ptr(), bits.ptr(), jit.ptr() if jit else None, n, L, sigma, delta)
        settled(z, bits, jit)
        return {"z": z}

    def check(small):
        want = U.message_to_tensor(M, sigma, delta if jitter else 0.0, J)
        assert torch.equal(small["z"].get(F32, (K, L)).cpu(), want)
    second_trip(b, run, check)


def quantize_case(key, work, excess, small_nchw, channels_last, b, skew=0):
    """ideas_image_f32_to_u8 on K items [K, C, H, W] (as NHWC memory when ``channels_last``), x ``skew`` bytes off 16-byte alignment."""
    from test_stego import quantize_reference
    assert beyond(key, work) == excess
    k, c, h, w = small_nchw.shape
    dtype = small_nchw.dtype
    mem = small_nchw.permute(0, 2, 3, 1).contiguous() if channels_last else small_nchw.contiguous()
    small_x = mem.cuda()

    def run(idx):
        n = idx.numel()
        xin = gather(small_x, idx, skew)
        u8, y = Guarded(n * c * h * w), Guarded(4 * n * c * h * w)
        call("ideas_image_f32_to_u8", u8.ptr(), y.ptr(), xin.ptr(), n, c, h, w, lib().NHWC if channels_last else lib().NCHW, enum(dtype))
        settled(u8, y, xin)
        return {"u8": u8, "y": y}

    def check(small):
        got = small["u8"].get(torch.uint8, (K, h, w, c))
        assert torch.equal(got.cpu(), quantize_reference(small_nchw).permute(0, 2, 3, 1))
        assert torch.equal(small["y"].get(F32, (K, h, w, c)), decode_of(got))
    second_trip(b, run, check)


def quantize_items(dtype, seed):
    x = (torch.rand(K, 3, 5, 7, generator=gen(seed)) * 2.2 - 1.1).to(dtype)
    x.view(-1)[:2] = torch.tensor([-1.0, 1.0]).to(dtype)
    return x


def test_image_f32_to_u8_flat_vector():
    """bf16 NHWC, B = 639 133 images of 5 x 7 x 3: n = 67 108 965 elements, n % 4 = 1.  A workgroup takes 256 x 4 quads a trip, so
    16 777 241 quads against 16384 x 1024 leave 25 quads for the second trip -- a partial last group, after the whole groups of the
    first -- and the element tail of one.  x 134 MB, u8 67 MB, y 268 MB, a piece of the comparison 134 MB: 0.6 GB."""
    b = 639_133
    n = b * 105
    assert n % 4 == 1
    quantize_case("stego.image_flat_vec", n >> 2, 25, quantize_items(BF, 5), True, b)


def test_image_f32_to_u8_flat_element():
    """f32 NHWC with x one element off 16-byte alignment, B = 39 946: 4 194 330 elements against 16384 x 256, 26 threads on the second
    trip; 38 MB."""
    b = 39_946
    quantize_case("stego.image_flat_elem", b * 105, 26, quantize_items(F32, 6), True, b, skew=4)


def test_image_f32_to_u8_planar():
    """f32 NCHW, C = 3, B = 119 838 images of 5 x 7: 4 194 330 pixels against 16384 x 256, 26 threads on the second trip; 113 MB."""
    b = 119_838
    quantize_case("stego.image_planar", b * 35, 26, quantize_items(F32, 7), False, b)


# ------------------------------------------------------------------------------------------------- attack.hip
def smooth_images(k, h, w, c, seed):
    """Different images with structure (a ramp each way and grain), 0 and 255 among the values."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    base = 30.0 * np.arange(1, k + 1)[:, None, None, None] * (yy / h - xx / w)[None, :, :, None] + 40.0 * np.arange(c) + 60
    img = np.clip(base + rng.normal(0, 30, (k, h, w, c)), 0, 255).astype(np.uint8)
    img.reshape(-1)[:2] = (0, 255)
    return img


@pytest.mark.parametrize("w", [9, 8], ids=["8x9-bytes", "8x8-vector"])
def test_jpeg_roundtrip(w):
    """B = 65 541 images of 8 x W x 3, one tile each (at W = 9 its second block is partial): 65 541 tiles against 16384 x 4, two
    workgroups on the second trip, the last with one live wave.  W = 9 takes the byte path, W = 8 the 8-byte one.  out, y and coef are
    compared.  W = 9: 107 MB.  Small items: the oracle's coefficients and decode, as tests/test_attacks_gpu.py."""
    h, c, q, b = 8, 3, 75, 65_541
    bw = (w + 7) // 8
    assert beyond("attack.jpeg", b * 1 * 1) == 5
    x = smooth_images(K, h, w, c, 8)
    small_x = torch.from_numpy(x).cuda()

    def run(idx):
        n = idx.numel()
        xin = gather(small_x, idx)
        out, y, coef = Guarded(n * h * w * c), Guarded(4 * n * h * w * c), Guarded(2 * n * c * bw * 64)
        assert xin.ptr() % 8 == 0 and out.ptr() % 8 == 0 and y.ptr() % 16 == 0            # so W % 8 alone chooses the path
        call("ideas_jpeg_roundtrip", out.ptr(), y.ptr(), coef.ptr(), xin.ptr(), n, c, h, w, q)
        settled(out, y, coef, xin)
        return {"out": out, "y": y, "coef": coef}

    def check(small):
        out = small["out"].get(torch.uint8, (K, h, w, c))
        check_against_oracle(x, q, out.cpu().numpy(), small["coef"].get(torch.int16, (K, c, 1, bw, 64)).cpu().numpy())
        assert torch.equal(small["y"].get(F32, (K, h, w, c)), decode_of(out))
    second_trip(b, run, check)


def pixel_case(key, work, excess, c, b, skew):
    h, w = 5, 7
    gain, offset, sigma, sp = 1.5, -20.0, 5.0, 0.1
    assert beyond(key, work) == excess
    x = torch.randint(0, 256, (K, h, w, c), generator=gen(9 + c), dtype=torch.uint8)
    x.view(-1)[:2] = torch.tensor([0, 255], dtype=torch.uint8)
    noise, u = torch.randn(K, h, w, c, generator=gen(10)), torch.rand(K, h, w, generator=gen(11))
    u.view(-1)[0] = 0.0
    small_x, small_n, small_u = x.cuda(), noise.cuda(), u.cuda()

    def run(idx):
        n = idx.numel()
        xin, nin, uin = gather(small_x, idx, 1 if skew else 0), gather(small_n, idx, 4 if skew else 0), gather(small_u, idx, 4 if skew else 0)
        out, y = Guarded(n * h * w * c, 1 if skew else 0), Guarded(4 * n * h * w * c, 4 if skew else 0)
        call("ideas_pixel_attack", out.ptr(), y.ptr(), xin.ptr(), nin.ptr(), uin.ptr(), n, c, h, w, gain, offset, sigma, sp)
        settled(out, y, xin, nin, uin)
        return {"out": out, "y": y}

    def check(small):
        out = small["out"].get(torch.uint8, (K, h, w, c))
        want = attacks_ref.pixel_attack_ref(x.numpy(), gain, offset, sigma, sp, noise.numpy(), u.numpy())
        assert np.array_equal(out.cpu().numpy(), want)
        assert torch.equal(small["y"].get(F32, (K, h, w, c)), decode_of(out))
    second_trip(b, run, check)


def test_pixel_attack_vector():
    """C = 1, aligned, B = 479 350 images of 5 x 7: 16 777 250 pixels, four a thread, against 16384 x 1024: 8 quads on the second trip
    and a tail of 2 pixels.  Noise and u follow the same pattern.  x and out 17 MB each, noise, u and y 67 MB each: 0.3 GB."""
    b = 479_350
    pixel_case("attack.pixel_vec", b * 35, 34, 1, b, False)


def test_pixel_attack_element():
    """C = 3, every pointer off its alignment, B = 119 838 images of 5 x 7: 4 194 330 pixels against 16384 x 256, 26 threads on the
    second trip; 0.2 GB."""
    b = 119_838
    pixel_case("attack.pixel_elem", b * 35, 26, 3, b, True)


# ------------------------------------------------------------------------------------------------- attack_spatial.hip
def spatial_images(h, w, c, seed):
    """K images that differ strongly from one to the next (independent noise on different levels), so that a row or a table left in LDS
    by the tile before changes bytes."""
    rng = np.random.default_rng(seed)
    img = np.clip(rng.integers(0, 256, (K, h, w, c)) // 2 + 32 * np.arange(K)[:, None, None, None], 0, 255).astype(np.uint8)
    img.reshape(-1)[:2] = (0, 255)
    assert all(np.abs(img[i].astype(int) - img[i + 1]).mean() > 20 for i in range(K - 1))
    return img


def resample_case(x, h2, w2, horiz, vert, b, tiles_each, excess):
    """ideas_resample_u8 on uint8 numpy [K, H, W, C] with tables (lo, kk) or None per direction."""
    k, h, w, c = x.shape
    assert beyond("attack_spatial.resample", b * tiles_each) == excess
    small_x = torch.from_numpy(x).cuda()

    def run(idx):
        n = idx.numel()
        xin = gather(small_x, idx)
        out, y = Guarded(n * h2 * w2 * c), Guarded(4 * n * h2 * w2 * c)
        tabs = [fixed(torch.from_numpy(np.ascontiguousarray(t)).cuda()) for d in (horiz, vert) if d is not None for t in d]
        hp = (tabs[0].ptr(), tabs[1].ptr(), horiz[1].shape[1]) if horiz is not None else (None, None, 0)
        vp = (tabs[-2].ptr(), tabs[-1].ptr(), vert[1].shape[1]) if vert is not None else (None, None, 0)
        call("ideas_resample_u8", out.ptr(), y.ptr(), xin.ptr(), n, c, h, w, h2, w2, *hp, *vp)
        settled(out, y, xin, *tabs)
        return {"out": out, "y": y}

    def check(small):
        out = small["out"].get(torch.uint8, (K, h2, w2, c))
        assert np.array_equal(out.cpu().numpy(), spatial_ref.resample_ref(x, horiz, vert))
        assert torch.equal(small["y"].get(F32, (K, h2, w2, c)), decode_of(out))
    second_trip(b, run, check)


@pytest.mark.parametrize("c", [1, 3])
def test_resample(c):
    """B = 65 541 images of 5 x 7 resized to 4 x 5, one tile each: 65 541 tiles against 65536 workgroups, five of which go round again
    and meet the barrier at the top of the loop with the tables and rows of their first tile in LDS.  C = 3: 28 MB."""
    x = spatial_images(5, 7, c, 12 + c)
    resample_case(x, 4, 5, spatial_ref.bilinear_tables(7, 5), spatial_ref.bilinear_tables(5, 4), 65_541, 1, 5)


def test_resample_tile_that_does_not_fit_lds():
    """The route that takes its sums from x directly: images of 200 x 3 with the rows shuffled by i -> 97 i mod 200 (a tile's 32 rows
    reach more rows than LDS keeps), 7 tiles a sample, B = 9 364: 65 548 tiles, 12 on the second trip; 28 MB."""
    h, w = 200, 3
    x = spatial_images(h, w, 1, 15)
    shuffle = ((97 * np.arange(h) % h).astype(np.int32), np.full((h, 1), 1 << 22, np.int32))
    assert shuffle[0][:32].max() - shuffle[0][:32].min() >= 160
    assert np.array_equal(spatial_ref.resample_ref(x, None, shuffle), x[:, shuffle[0]])
    resample_case(x, h, w, None, shuffle, 9_364, 7, 12)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("k", [3, 5])
def test_median(k, c):
    """B = 65 541 images of 5 x 7, one tile each: five workgroups stage a second tile over the first.  C = 3: 41 MB."""
    h, w, b = 5, 7, 65_541
    assert beyond("attack_spatial.median", b * 1) == 5
    x = spatial_images(h, w, c, 16 + k + c)
    small_x = torch.from_numpy(x).cuda()

    def run(idx):
        n = idx.numel()
        xin = gather(small_x, idx)
        out, y = Guarded(n * h * w * c), Guarded(4 * n * h * w * c)
        call("ideas_median_u8", out.ptr(), y.ptr(), xin.ptr(), n, c, h, w, k)
        settled(out, y, xin)
        return {"out": out, "y": y}

    def check(small):
        out = small["out"].get(torch.uint8, (K, h, w, c))
        assert np.array_equal(out.cpu().numpy(), spatial_ref.median_ref(x, k))
        assert torch.equal(small["y"].get(F32, (K, h, w, c)), decode_of(out))
    second_trip(b, run, check)


# ------------------------------------------------------------------------------------------------- ecc.hip
@pytest.mark.parametrize("fill", [False, True], ids=["zeros", "fill"])
@pytest.mark.parametrize("rate", sorted(ecc_ref.RATES))
def test_ecc_encode(rate, fill):
    """n = 29 message bits (4 bytes a row), B = 1 048 580: 4 194 320 coded bytes against 16384 x 256, 16 threads on the second trip;
    12 MB.  Small items: bit for bit tests/ecc_ref.py."""
    n, b = 29, 1_048_580
    assert beyond("ecc.encode", b * 4) == 16
    pl = ecc_ref.plan(n, rate)
    rng = np.random.default_rng(17 + ecc_ref.RATES[rate][0])
    info = rng.integers(0, 256, (K, pl["k"] // 8), dtype=np.uint8)
    frows = ecc_ref.pack(rng.integers(0, 2, (K, n)))
    small_i, small_f = torch.from_numpy(info).cuda(), torch.from_numpy(frows).cuda()

    def run(idx):
        m = idx.numel()
        iin, fin = gather(small_i, idx), (gather(small_f, idx) if fill else None)
        coded = Guarded(4 * m)
        call("ideas_ecc_encode", coded.ptr(), iin.ptr(), fin.ptr() if fin else None, m, n, pl["k"], ecc_ref.RATES[rate][0], pl["P"], pl["Pinv"])
        settled(coded, iin, fin)
        return {"coded": coded}

    def check(small):
        got = small["coded"].get(torch.uint8, (K, 4)).cpu().numpy()
        assert np.array_equal(got, ecc_ref.encode(info, n, rate, frows if fill else None))
    second_trip(b, run, check)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_ecc_soft(dtype):
    """L = 37 elements at sigma = 3, B = 37 800: 4 195 800 message bits against 16384 x 256, 1496 threads (six workgroups) on the second
    trip; 10 MB.  Small items: bit for bit the f32 restatement."""
    L, sigma, gain, b = 37, 3, 64.0, 37_800
    assert beyond("ecc.soft", b * L * sigma) == 1496
    z = (torch.rand(K, L, generator=gen(18)) * 2.4 - 1.2).to(dtype)
    small_z = z.cuda()

    def run(idx):
        m = idx.numel()
        zin, soft = gather(small_z, idx), Guarded(m * L * sigma)
        call("ideas_ecc_soft", soft.ptr(), zin.ptr(), m, L, sigma, gain, enum(dtype))
        settled(soft, zin)
        return {"soft": soft}

    def check(small):
        assert np.array_equal(small["soft"].get(torch.int8, (K, L * sigma)).cpu().numpy(), ecc_ref.soft(z.float().numpy(), sigma, gain))
    second_trip(b, run, check)


# ------------------------------------------------------------------------------------------------- pool.hip
POOL_CASES = {       # mode name: (H, W, C, dtype, B) -- OW stays within one run of a row, so a sample is OH runs of C / VW vectors
    "MAX_S1P1": (2, 2, 1, F32, 8_388_609),
    "AVG_S1P1_VALID": (2, 2, 8, BF, 8_388_609),
    "MAX_S2": (3, 3, 1, BF, 16_777_217),
}


@pytest.mark.parametrize("mode", sorted(POOL_CASES))
def test_pool3x3(mode):
    """65536 x 256 threads, each a channel vector of a run of an output row.  MAX_S1P1: f32, C = 1, 2 x 2, B = 8 388 609 -- two rows a
    sample, 2 threads on the second trip, 0.33 GB.  AVG_S1P1_VALID: bf16, C = 8 (one 16-byte vector a pixel: the vector path), the same
    B, 1.2 GB.  MAX_S2: bf16, C = 1, 3 x 3 (one window), B = 16 777 217, 1 thread on the second trip, 0.4 GB.  Small items against the
    F.* calls in f64 on the same rounded operands, as tests/test_fid_gpu.py: the maxima exact, the bf16 average within close_bf16."""
    from ideas_amd.op import pool as P
    from test_bf16_gpu import close_bf16
    h, w, c, dtype, b = POOL_CASES[mode]
    m = getattr(P, mode)
    oh, ow = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if mode == "MAX_S2" else (h, w)
    assert ow <= 4 and c in (1, 8)
    assert beyond("pool.pool3x3", b * oh * 1 * 1) == (1 if mode == "MAX_S2" else 2)
    x = torch.randn(K, c, h, w, generator=gen(19)).to(dtype)
    small_x = x.permute(0, 2, 3, 1).contiguous().cuda()
    esize = 2 if dtype == BF else 4

    def run(idx):
        n = idx.numel()
        xin, y = gather(small_x, idx), Guarded(n * oh * ow * c * esize)
        call("ideas_pool3x3_fwd", y.ptr(), xin.ptr(), n, c, h, w, m, enum(dtype))
        settled(y, xin)
        return {"y": y}

    def check(small):
        got = small["y"].get(dtype, (K, oh, ow, c)).permute(0, 3, 1, 2)
        ref = P.pool3x3_composition(x.double(), m)
        if mode == "AVG_S1P1_VALID":
            close_bf16(got, ref, "avg")
        else:
            assert torch.equal(got.double().cpu(), ref)
    second_trip(b, run, check)


def test_global_avg_pool():
    """f32, C = 1, H W = 2, B = 16 777 217: one thread a sample against 65536 x 256, 1 thread on the second trip; 0.27 GB.  Small
    items against F.adaptive_avg_pool2d in f64 at the 1e-5 of tests/test_fid_gpu.py."""
    h, w, c, b = 1, 2, 1, 16_777_217
    assert beyond("pool.global_avg", b * 1) == 1
    x = torch.randn(K, c, h, w, generator=gen(20))
    small_x = x.permute(0, 2, 3, 1).contiguous().cuda()

    def run(idx):
        n = idx.numel()
        xin, out = gather(small_x, idx), Guarded(4 * n * c)
        call("ideas_global_avg_pool", out.ptr(), xin.ptr(), n, c, h, w, enum(F32))
        settled(out, xin)
        return {"out": out}

    def check(small):
        assert rel_err(small["out"].get(F32, (K, c, 1, 1)), F.adaptive_avg_pool2d(x.double(), 1)) <= 1e-5
    second_trip(b, run, check)


# ------------------------------------------------------------------------------------------------- lpips.hip: the 2x2 max pool
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_maxpool2x2_fwd(dtype):
    """C = 1, 2 x 2, B = 2 097 153: one output a sample against 8192 x 256, 1 thread on the second trip; 50 MB.  Small items equal to
    F.max_pool2d."""
    h = w = 2
    b = 2_097_153
    assert beyond("lpips.maxpool_fwd", b * 1) == 1
    x = torch.randn(K, 1, h, w, generator=gen(21)).to(dtype)
    small_x = x.permute(0, 2, 3, 1).contiguous().cuda()
    esize = 2 if dtype == BF else 4

    def run(idx):
        n = idx.numel()
        xin, y = gather(small_x, idx), Guarded(n * esize)
        call("ideas_maxpool2x2_fwd", y.ptr(), xin.ptr(), n, 1, h, w, enum(dtype))
        settled(y, xin)
        return {"y": y}

    def check(small):
        assert torch.equal(small["y"].get(dtype, (K, 1, 1, 1)).double().cpu(), F.max_pool2d(x.double(), 2, 2))
    second_trip(b, run, check)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_maxpool2x2_bwd(dtype):
    """C = 1, 3 x 3, B = 524 289: the odd edge gives ceil(3 / 2)^2 = 4 windows a sample, one whole and three cut, 2 097 156 against
    8192 x 256, 4 threads on the second trip; 40 MB.  Small items equal to autograd of F.max_pool2d."""
    h = w = 3
    b = 524_289
    assert beyond("lpips.maxpool_bwd", b * 2 * 2) == 4
    x = torch.randn(K, 1, h, w, generator=gen(22)).to(dtype)
    gy = torch.randn(K, 1, 1, 1, generator=gen(23)).to(dtype)
    small_x, small_g = x.permute(0, 2, 3, 1).contiguous().cuda(), gy.permute(0, 2, 3, 1).contiguous().cuda()
    esize = 2 if dtype == BF else 4

    def run(idx):
        n = idx.numel()
        xin, gin, gx = gather(small_x, idx), gather(small_g, idx), Guarded(n * h * w * esize)
        call("ideas_maxpool2x2_bwd", gx.ptr(), gin.ptr(), xin.ptr(), n, 1, h, w, enum(dtype))
        settled(gx, gin, xin)
        return {"gx": gx}

    def check(small):
        ref_in = x.double().requires_grad_(True)
        (ref,) = torch.autograd.grad(F.max_pool2d(ref_in, 2, 2), ref_in, gy.double())
        assert torch.equal(small["gx"].get(dtype, (K, h, w, 1)).permute(0, 3, 1, 2).double().cpu(), ref)
    second_trip(b, run, check)


# ------------------------------------------------------------------------------------------------- upfirdn2d.hip: the generic kernel
def test_upfirdn2d_generic():
    """NCHW f32, a random 3 x 5 FIR (wider than the tiled kernel takes), up = down = 1: 16 385 planes of 32 x 32 outputs, 16 778 240
    against 65536 x 256 -- the last plane, four workgroups, on the second trip; 0.14 GB.  Small planes against
    oracle.torch_ref.upfirdn2d in f64 at the 1e-5 of tests/test_ops_gpu.py."""
    import oracle.torch_ref as O
    ih, iw, oh, ow, kh, kw, b = 32, 34, 32, 32, 3, 5, 16_385
    assert beyond("upfirdn2d.generic", b * oh * ow) == 1024
    x = torch.randn(K, 1, ih, iw, generator=gen(24))
    fir = torch.randn(kh, kw, generator=gen(25))
    small_x, fir_d = x.cuda(), fir.cuda()

    def run(idx):
        n = idx.numel()
        xin, taps, y = gather(small_x, idx), fixed(fir_d), Guarded(4 * n * oh * ow)
        call("ideas_upfirdn2d", y.ptr(), xin.ptr(), taps.ptr(), n, 1, ih, iw, oh, ow, kh, kw, 1, 1, 1, 1, 1, 1, 1.0, 1, lib().NCHW, lib().F32)
        settled(y, xin, taps)
        return {"y": y}

    def check(small):
        ref = O.upfirdn2d(x.double(), fir.double(), pad=(1, 1))
        assert tuple(ref.shape) == (K, 1, oh, ow)
        assert rel_err(small["y"].get(F32, (K, 1, oh, ow)), ref) < 1e-5
    second_trip(b, run, check)


# ------------------------------------------------------------------------------------------------- bias_act.hip
def bias_act_case(key, c, pixels_each, b, work, excess):
    """ideas_fused_bias_act forward (bias + leaky ReLU) on NHWC f32 items of ``pixels_each`` pixels of C channels."""
    assert beyond(key, work) == excess
    alpha, scale = 0.2, 2.0 ** 0.5
    x = torch.randn(K, pixels_each, c, generator=gen(30 + c))
    bias = torch.randn(c, generator=gen(31)) * 0.5
    small_x, bias_d = x.cuda(), bias.cuda()

    def run(idx):
        n = idx.numel() * pixels_each * c
        xin, bin_, y = gather(small_x, idx), fixed(bias_d), Guarded(4 * n)
        call("ideas_fused_bias_act", y.ptr(), xin.ptr(), bin_.ptr(), None, None, n, c, 1, lib().NHWC, 3, 0, alpha, scale, lib().F32)
        settled(y, xin, bin_)
        return {"y": y}

    def check(small):
        v = x.double() + bias.double()
        assert rel_err(small["y"].get(F32, (K, pixels_each, c)), torch.where(v > 0, v, v * alpha) * scale) < 1e-5
    second_trip(b, run, check)


def test_bias_act_vector_not_tiled():
    """C = 2048 (a 1024-float row is no multiple of C, so not the tiled variant), one pixel an item, B = 8 193: 4 194 816 float4
    against 4096 x 256 threads of four float4 a trip, 512 on the second trip; 0.14 GB.  Small items against f64 at 1e-5."""
    b = 8_193
    bias_act_case("bias_act.vec", 2048, 1, b, b * 512, 512)


def test_bias_act_scalar():
    """C = 3 (no vector of four channels), seven pixels an item, B = 99 865: 2 097 165 elements against 8192 x 256, 13 threads on
    the second trip; 17 MB."""
    b = 99_865
    bias_act_case("bias_act.scalar", 3, 7, b, b * 21, 13)


def counts_of(idx):
    return torch.bincount(idx, minlength=K).to(torch.int64)


def test_channel_sum():
    """A sum over what is replicated: values in {-1, 0, 1}, so every f32 partial sum is an exact integer below 2^24 whatever the
    order of the atomics, compared with the count in int64 on the device.  C = 3, items of four pixels, B = 699 051: 8 388 612
    elements; the grid is one workgroup per 4096 elements (16 a thread: the loop runs at every size), capped at 2048 -- 4 elements past
    the size where the cap binds; 34 MB."""
    c, b = 3, 699_051
    assert beyond("bias_act.channel_sum", b * 12) == 4
    x = torch.randint(-1, 2, (K, 4, c), generator=gen(32)).float()
    small_x = x.cuda()
    idx = torch.arange(b, device="cuda") % K
    xin, out = gather(small_x, idx), Guarded(4 * c)
    out.view.view(F32).fill_(7.0)                                   # clear = 1: overwritten
    call("ideas_channel_sum", out.ptr(), xin.ptr(), b * 12, c, 1, lib().F32)
    settled(out, xin)
    want = (counts_of(idx).view(K, 1) * small_x.to(torch.int64).sum(1)).sum(0)
    assert int(want.abs().max()) < 2 ** 24
    assert torch.equal(out.get(F32, (c,)).to(torch.int64), want)


# ------------------------------------------------------------------------------------------------- conv_direct.hip: forward
DIRECT_CASES = {       # kernel: (row, Cin, Cout, k, H, W, B, work per sample, units past the first trip)
    "direct": ("conv_direct.direct", 3, 8, 3, 7, 9, 33_289, 7 * 9 * 8, 440),
    "smallk_vec": ("conv_direct.smallk_vec", 3, 16, 1, 1, 5, 838_861, 5, 1),
    "smallk": ("conv_direct.smallk", 5, 6, 1, 1, 3, 917_505, 3, 3),
    "rowdot": ("conv_direct.rowdot", 32, 4, 1, 1, 3, 174_763, 3, 1),
}


@pytest.mark.parametrize("kernel", sorted(DIRECT_CASES))
def test_conv_direct_forward(kernel):
    """The four VALU kernels behind ideas_conv_direct, f32, with bias; samples are independent.
    direct (3 x 3, 3 -> 8, 7 x 9): one output a thread, B = 33 289, 16 777 656 outputs against 65536 x 256; 92 MB.
    The pointwise kernels size their grids for several trips of a workgroup (8, 8 and 4), so their loops turn at every size; the cases
    are the first sizes at which the caps bind and one more trip is made.  smallk_vec (3 -> 16, 64 pixels a trip): 4 194 305 pixels
    against 8192 x 512, 0.32 GB; smallk (5 -> 6, 42 pixels a trip): 2 752 515 against 8192 x 336, 0.12 GB; rowdot (32 -> 4, 32 pixels a
    trip): 524 289 against 4096 x 128, 76 MB.  Small items against F.conv2d in f64 at the 1e-5 of tests/test_ops_gpu.py."""
    import ctypes
    import ideas_amd.op.conv as CV
    from ideas_amd.op.conv_plan import ConvGeom, plan_fwd
    from test_conv_epilogue_pinned_gpu import _direct_kernel
    key, ci, co, k, h, w, b, each, excess = DIRECT_CASES[kernel]
    assert beyond(key, b * each) == excess
    gain = 0.21
    x = torch.randn(K, ci, h, w, generator=gen(40 + ci))
    wt = torch.randn(co, ci, k, k, generator=gen(41))
    bias = torch.randn(co, generator=gen(42)) * 0.3
    small_x = x.permute(0, 2, 3, 1).contiguous().cuda()
    wd, bias_d = wt.cuda().contiguous(memory_format=torch.channels_last), bias.cuda()

    def run(idx):
        n = idx.numel()
        L = plan_fwd((n, ci, h, w), wd, ConvGeom(k, k, 1, k // 2, False))
        p = CV._params(L, gain)
        assert _direct_kernel(p) == kernel and (L.YH, L.YW, L.Cout) == (h, w, co)
        xin, bin_, y = gather(small_x, idx), fixed(bias_d), Guarded(4 * n * h * w * co)
        call("ideas_conv_direct", y.ptr(), xin.ptr(), lib().ptr(L.wmat), None, None, bin_.ptr(), None, ctypes.byref(p), lib().F32)
        settled(y, xin, bin_)
        return {"y": y}

    def check(small):
        ref = F.conv2d(x.double(), wt.double(), padding=k // 2) * gain + bias.double().view(1, -1, 1, 1)
        assert rel_err(small["y"].get(F32, (K, h, w, co)).permute(0, 3, 1, 2), ref) < 1e-5
    second_trip(b, run, check)


# ------------------------------------------------------------------------------------------------- conv_direct.hip: weight gradients
WGRAD_CASES = {        # kernel: (row, Cin, Cout, k, H, W, B, pixels past the size where the cap binds)
    "wgrad_vec": ("conv_direct.wgrad_vec", 32, 3, 1, 1, 3, 1_398_102, 2),
    "small_wgrad": ("conv_direct.small_wgrad", 5, 6, 1, 1, 3, 21_846, 2),
    "wgrad_direct": ("conv_direct.wgrad_direct", 3, 5, 3, 7, 9, 8_323, 61),
}


@pytest.mark.parametrize("kernel", sorted(WGRAD_CASES))
def test_conv_wgrad_direct(kernel):
    """The three launchers of ideas_conv_wgrad_direct give every workgroup a run of pixels -- 2048, 64 and 256 by design -- and a
    capped grid makes the runs longer: the cases are the first sizes past cap x run.  A weight gradient sums over what is replicated, so
    x and gy hold values in {-1, 0, 1}: every f32 partial sum is an exact integer below 2^24 whatever the order of the atomics, and the
    result is compared for equality with sum_k count_k gw_k in int64 on the device, gw_k being autograd's (exact in f64) for item k.
    wgrad_vec (1 x 1, 32 -> 3): 4 194 306 pixels, 0.6 GB; small_wgrad (5 -> 6): 65 538 pixels; wgrad_direct (3 x 3, 3 -> 5, 7 x 9):
    524 349 pixels, 17 MB."""
    import ctypes
    import ideas_amd.op.conv as CV
    from ideas_amd.op.conv_plan import ConvGeom, plan_wgrad
    key, ci, co, k, h, w, b, excess = WGRAD_CASES[kernel]
    assert beyond(key, b * h * w) == excess and b * h * w < 2 ** 24
    x = torch.randint(-1, 2, (K, ci, h, w), generator=gen(50 + ci)).double()
    gy = torch.randint(-1, 2, (K, co, h, w), generator=gen(51)).double()
    per_item = []
    for i in range(K):
        wt = torch.zeros(co, ci, k, k, dtype=torch.float64, requires_grad=True)
        (g,) = torch.autograd.grad(F.conv2d(x[i:i + 1], wt, padding=k // 2), wt, gy[i:i + 1])
        per_item.append(g.permute(0, 2, 3, 1))                      # OHWI, as the kernel stores it
    per_item = torch.stack(per_item).to(torch.int64).cuda()
    idx = torch.arange(b, device="cuda") % K
    xin = gather(x.permute(0, 2, 3, 1).float().contiguous().cuda(), idx)
    gin = gather(gy.permute(0, 2, 3, 1).float().contiguous().cuda(), idx)
    gw = Guarded(4 * co * k * k * ci)
    gw.view.zero_()
    L = plan_wgrad((b, ci, h, w), (b, co, h, w), ConvGeom(k, k, 1, k // 2, False))
    p = CV._params(L, 1.0)
    call("ideas_conv_wgrad_direct", gw.ptr(), gin.ptr(), xin.ptr(), None, None, ctypes.byref(p), lib().F32)
    settled(gw, gin, xin)
    want = (counts_of(idx).view(K, 1, 1, 1, 1) * per_item).sum(0)
    assert int(want.abs().max()) < 2 ** 24 and int(want.abs().max()) > 0
    assert torch.equal(gw.get(F32, (co, k, k, ci)).to(torch.int64), want)


# ------------------------------------------------------------------------------------------------- conv_wino.hip: the fold
def test_wino_wgrad_fold():
    """dU [4][Cout][3][Cin] folded onto the 3 x 3 taps and ADDED into gw, element by element: Cout = 1366, Cin = 256 is 1 049 088
    elements against 4096 x 256, 512 on the second trip; the rows o follow the pattern.  With ``clear`` the scratch is zeroed behind the
    read, on the second trip too.  36 MB.  Small rows against f64 at 1e-5."""
    co, ci = 1366, 256
    assert beyond("conv_wino.fold", co * 3 * ci) == 512
    gu = torch.randn(4, K, 3, ci, generator=gen(60))
    gw0 = torch.randn(K, 3, 3, ci, generator=gen(61))
    gu_d, gw0_d = gu.cuda(), gw0.cuda()

    def run(idx):
        n = idx.numel()
        scratch = Guarded(4 * 4 * n * 3 * ci)
        torch.index_select(gu_d, 1, idx, out=scratch.view.view(F32).view(4, n, 3, ci))
        gw = gather(gw0_d, idx)
        call("ideas_wino_wgrad_fold", gw.ptr(), scratch.ptr(), n, ci, 9 * ci, 3 * ci, ci, 1, 1)
        settled(gw, scratch)
        assert not bool(scratch.view.any())                         # cleared behind the read
        return {"gw": gw}

    def check(small):
        u = gu.double()
        half = (u[1] + u[2]) * 0.5
        ref = gw0.double() + torch.stack((u[0] + half, (u[1] - u[2]) * 0.5, half + u[3]), 2)
        assert rel_err(small["gw"].get(F32, (K, 3, 3, ci)), ref) < 1e-5
    second_trip(co, run, check)
