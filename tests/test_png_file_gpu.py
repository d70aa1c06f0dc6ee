"""The PNG file written on the device (csrc/png_bytes.hip) against the numpy restatement tests/png_ref.py, which tests/test_png_file.py
holds to zlib's inflate and Pillow's reader: byte for byte, through the C ABI with guard bands round every buffer and a dirty
workspace, through the op, and through ``hide.py --png_encoder device``.  Files are compared as ``bytes``: there is no tolerance
anywhere.  ``files[b, nbytes[b]:]`` is unspecified and not asserted, but for the guard band behind each row at its stride."""
import io
import os

import numpy as np
import pytest
import torch

import png_ref as R
from conftest import Golden

pytestmark = pytest.mark.gpu

BAND = 64                     # sentinel bytes either side of every buffer
SENT = 0xA5
E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3


class Guarded:
    """``nbytes`` on the device between two bands of sentinel bytes, ``skew`` bytes off the allocation's alignment."""

    def __init__(self, nbytes, skew=0, fill=SENT):
        self.n, self.skew = nbytes, skew
        self.buf = torch.full((BAND + skew + nbytes + BAND,), SENT, dtype=torch.uint8, device="cuda")
        self.view = self.buf[BAND + skew:BAND + skew + nbytes]
        self.view.fill_(fill)

    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        lo = BAND + self.skew
        return bool((self.buf[:lo] == SENT).all()) and bool((self.buf[lo + self.n:] == SENT).all())


def raw_encode(x, extra_stride=37, skew=(0, 0, 0, 0), work=None):
    """ideas_png_file_encode on the numpy batch ``x`` uint8 [B, H, W, C]; skew = byte offsets of (files, nbytes, u8, workspace).  Every
    buffer is guarded, the rows of ``files`` carry ``extra_stride`` sentinel bytes behind the bound.  -> (files as bytes, nbytes)."""
    from ideas_amd import _lib
    lib = _lib.load()
    b, h, w, c = x.shape
    bound = int(lib.ideas_png_file_max_bytes(c, h, w))
    assert bound == R.max_bytes(c, h, w) > 0
    stride = bound + extra_stride
    nwork = int(lib.ideas_png_file_encode_workspace_bytes(b, c, h, w))
    assert nwork > 0
    files, nbytes = Guarded(b * stride, skew[0]), Guarded(4 * b, 4 * skew[1])
    src = Guarded(x.size, skew[2])
    src.view.copy_(torch.from_numpy(np.ascontiguousarray(x)).view(-1))
    if work is None:
        work = Guarded(nwork, skew[3], fill=0xFF)             # never zeros: the call clears what it needs
    assert work.n >= nwork
    rc = lib.ideas_png_file_encode(files.ptr(), nbytes.ptr(), stride, src.ptr(), work.ptr(), b, c, h, w, _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert files.intact() and nbytes.intact() and src.intact() and work.intact()
    assert np.array_equal(src.view.cpu().numpy().reshape(x.shape), x)            # the input is only read
    n = nbytes.view.cpu().numpy().view(np.int32).tolist()
    rows = files.view.cpu().numpy().reshape(b, stride)
    assert all(0 < v <= bound for v in n), n
    assert (rows[:, bound:] == SENT).all()                                       # the guard band behind each row, at its stride
    return [rows[i, :v].tobytes() for i, v in enumerate(n)], n


def check(x, **kw):
    got, n = raw_encode(x, **kw)
    want = [R.png_file(img)[0] for img in x]
    assert n == [len(f) for f in want], (n, [len(f) for f in want])
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            first = next(k for k in range(len(a)) if a[k] != b[k])
            raise AssertionError(f"image {i} of {x.shape}: first difference at byte {first} of {len(b)}")
    return got


# ------------------------------------------------------------------------------------------------- the writer against the restatement
@pytest.mark.parametrize("name", ["one_grey", "one_rgb", "smooth_grey", "stripe_32", "stripe_33", "stripe_70", "wide", "flat", "fibonacci",
                                  "noise_64", "pink_64_grey"])
def test_files_are_the_restatement(name):
    """The fixtures of tests/png_ref.py, one image a call: 1 x 1; H below a stripe; H = 32, 33 and 70 at W = 33 (exactly one stripe, one
    row into the second, a short last stripe of three); ``wide``: 2 x 1400 x 3, rows of 4200 bytes against the 256 a workgroup of the
    filter kernel covers a trip (17 trips) and stripes of 8402 bytes against the 4096 of the packing kernel (3 trips); a flat image (the
    two-symbol code); the length-limit fixture; uniform noise (codes near 8 bits, the header near its largest); 1/f noise."""
    check(R.fixture(name)[None])


def test_batches_of_odd_shapes():
    """(2, 13, 21, 3) and (1, 40, 24, 1): odd sizes, H below a stripe and a stripe and a quarter."""
    check(np.stack([R.make_image("noise", 13, 21, 3), R.make_image("smooth", 13, 21, 3)]))
    check(R.make_image("noise", 40, 24, 1)[None])


def test_a_batch_of_three_different_images():
    """64 x 48 x 3, noise, smooth and flat: three lengths, so per-image offsets and the lengths column show."""
    x = np.stack([R.make_image(kind, 64, 48, 3) for kind in ("noise", "smooth", "flat")])
    got = check(x, skew=(3, 1, 5, 7), extra_stride=0)
    assert len({len(f) for f in got}) == 3


def test_dirty_workspace_and_repeated_calls():
    """One workspace, never cleared by the caller: noise (every word of the bit buffer in use), then a small flat image whose bits are
    ORed into what the first call left unless the call clears it; and the same call twice."""
    from ideas_amd import _lib
    big = np.stack([R.make_image("noise", 64, 64, 3, seed=s) for s in range(2)])
    work = Guarded(int(_lib.load().ideas_png_file_encode_workspace_bytes(2, 3, 64, 64)), fill=0xFF)
    first = check(big, work=work)
    assert check(big, work=work) == first
    check(R.make_image("flat", 33, 33, 3)[None], work=work)


def test_rows_past_two_gigabytes():
    """The caller chooses row_stride: 2100 images of 2 x 2 x 1 in rows of 2^20 bytes put the last rows past byte 2^31 of ``files``, where
    a 32-bit row offset would land in the first rows (or outside).  Copies of 3 different images; checked on the device, but for the
    bound's bytes of every row."""
    from ideas_amd import _lib
    lib = _lib.load()
    b, stride, bound = 2100, 1 << 20, R.max_bytes(1, 2, 2)
    x = np.stack([R.make_image("noise", 2, 2, 1, seed=s) for s in range(3)])
    x[2] = 9                                                                     # a flat one: another length
    want = [R.png_file(img)[0] for img in x]
    assert len({len(f) for f in want}) >= 2 and int(lib.ideas_png_file_max_bytes(1, 2, 2)) == bound
    xd = torch.from_numpy(x).cuda()[torch.arange(b, device="cuda") % 3].contiguous()
    buf = torch.full((BAND + b * stride + BAND,), SENT, dtype=torch.uint8, device="cuda")
    nbytes = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    work = torch.empty(int(lib.ideas_png_file_encode_workspace_bytes(b, 1, 2, 2)), dtype=torch.uint8, device="cuda")
    rc = lib.ideas_png_file_encode(buf.data_ptr() + BAND, nbytes.data_ptr(), stride, xd.data_ptr(), work.data_ptr(), b, 1, 2, 2,
                                   _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    rows = buf[BAND:BAND + b * stride].view(b, stride)
    assert nbytes.cpu().tolist() == [len(want[i % 3]) for i in range(b)]
    head = rows[:, :bound].cpu().numpy()
    for k in range(3):
        assert (head[k::3, :len(want[k])] == np.frombuffer(want[k], np.uint8)).all(), k
    assert bool((rows[:, bound:] == SENT).all()) and bool((buf[:BAND] == SENT).all()) and bool((buf[-BAND:] == SENT).all())


def test_pillow_opens_the_device_files_to_the_input():
    pytest.importorskip("PIL")
    from PIL import Image
    from ideas_amd.op import png_file_encode, png_files_to_host
    for h, w, c in ((33, 40, 3), (17, 23, 1), (70, 64, 3)):
        x = np.stack([R.make_image(kind, h, w, c) for kind in ("noise", "smooth", "pink")])
        files, nbytes = png_file_encode(torch.from_numpy(x).cuda())
        assert files.dtype == torch.uint8 and tuple(files.shape) == (3, R.max_bytes(c, h, w))
        assert nbytes.dtype == torch.int32 and tuple(nbytes.shape) == (3,)
        for i, data in enumerate(png_files_to_host(files, nbytes)):
            with Image.open(io.BytesIO(data)) as im:
                assert im.format == "PNG" and im.size == (w, h) and im.mode == ("RGB" if c == 3 else "L")
                assert np.array_equal(np.asarray(im, dtype=np.uint8).reshape(h, w, c), x[i]), (h, w, c, i)


def test_op_writes_the_recorded_files():
    """Through the op, against tests/golden/png_pinned.npz."""
    from ideas_amd.op import png_file_encode, png_files_to_host
    z = Golden("png_pinned.npz").z
    for name in ("odd_rgb", "pink_256"):
        got = png_files_to_host(*png_file_encode(torch.from_numpy(R.fixture(name)[None]).cuda()))
        assert got == [z["file/" + name].tobytes()], name


def test_op_validation_and_empty_input():
    from ideas_amd.op import png_file_encode, png_files_to_host
    x = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="uint8"):
        png_file_encode(x.float())
    with pytest.raises(RuntimeError, match="C = 1 or 3"):
        png_file_encode(x[..., :2])
    with pytest.raises(RuntimeError, match="HIP device"):
        png_file_encode(x.cpu())
    with pytest.raises(RuntimeError, match="png_file_encode: a file holds"):
        png_file_encode(x[:, :0])
    files, nbytes = png_file_encode(x[:0])                                        # no launch
    assert tuple(files.shape) == (0, R.max_bytes(3, 8, 8)) and tuple(nbytes.shape) == (0,)
    assert png_files_to_host(files, nbytes) == []
    files, nbytes = png_file_encode(x)
    with pytest.raises(RuntimeError, match="png_files_to_host expects uint8"):
        png_files_to_host(files.int(), nbytes)
    with pytest.raises(RuntimeError, match="a file holds"):                      # a bound beyond 2^31 - 1 bytes: refused by shape alone
        png_file_encode(torch.empty(0, 40000, 40000, 1, dtype=torch.uint8, device="cuda"))


def test_c_abi_refuses_by_return_code():
    """Nothing is launched: every pointer but the ones under test is a real buffer, the refusals come first."""
    from ideas_amd import _lib
    lib = _lib.load()
    bound = int(lib.ideas_png_file_max_bytes(3, 8, 8))
    assert bound == R.max_bytes(3, 8, 8)
    f, n, x, w = (Guarded(k) for k in (bound + 8, 4, 8 * 8 * 4, int(lib.ideas_png_file_encode_workspace_bytes(1, 3, 8, 8))))

    def call(files=f.ptr(), nbytes=n.ptr(), stride=bound, u8=x.ptr(), work=w.ptr(), b=1, c=3, h=8, w_=8):
        return lib.ideas_png_file_encode(files, nbytes, stride, u8, work, b, c, h, w_, _lib.stream_ptr())

    for name in ("files", "nbytes", "u8", "work"):
        assert call(**{name: None}) == E_NULL, name
    for c in (2, 4):
        assert call(c=c) == E_UNSUPPORTED and lib.ideas_png_file_max_bytes(c, 8, 8) == 0
        assert lib.ideas_png_file_encode_workspace_bytes(1, c, 8, 8) == 0
    for kw in ({"b": 0}, {"b": -1}, {"h": 0}, {"w_": -3}, {"c": 0}):
        assert call(**kw) == E_SHAPE, kw
    assert call(stride=bound - 1) == E_SHAPE
    assert lib.ideas_png_file_max_bytes(1, 40000, 40000) == 0 and call(c=1, h=40000, w_=40000) == E_SHAPE
    torch.cuda.synchronize()
    for g in (f, n, x, w):
        assert g.intact() and bool((g.view == SENT).all())                       # and nothing was written
    assert call() == 0                                                           # the same arguments, unrefused
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """The reference's own checkpoint of tests/golden/ckpt_r256.npz as a file (the discriminator's omitted tensors: zeros)."""
    from ckpt_fixture import build_reference_checkpoint
    raw = build_reference_checkpoint(Golden("ckpt_r256.npz"), lambda key, shape: torch.zeros(shape))
    path = str(tmp_path_factory.mktemp("png_ckpt") / "1.pt")
    torch.save(raw, path)
    return path


def test_hide_with_the_device_encoder_extracts_like_the_default(ckpt, tmp_path, capsys):
    """``hide.py --png_encoder device`` against the default, same seed: other bytes, the same pixels; and ``extract.py`` reads out of the
    device's files what it reads out of Pillow's -- the same bits (``--dump_bits``), the same exit status, the same payload file.  The
    fixture's networks are untrained (as in tests/test_jpeg_decode_gpu.py), so the frame's check fails on either directory: measured,
    status 1 and no payload file; wherever the default path recovers the payload, the device path must recover it too."""
    pytest.importorskip("PIL")
    from PIL import Image
    import extract
    import hide
    data = bytes(range(48))
    payload = tmp_path / "payload.bin"
    payload.write_bytes(data)
    common = ["--ckpt", ckpt, "--payload", str(payload), "--seed", "3", "--batch", "2"]
    hide.main(common + ["--out", str(tmp_path / "pillow")])
    assert "bytes" not in capsys.readouterr().out.strip().splitlines()[-1]      # the closing line of today's path stays as it is
    hide.main(common + ["--out", str(tmp_path / "device"), "--png_encoder", "device"])
    closing = capsys.readouterr().out.strip().splitlines()[-1]
    names = sorted(os.listdir(tmp_path / "pillow"))
    assert names and all(n.endswith(".png") for n in names) and sorted(os.listdir(tmp_path / "device")) == names
    total = 0
    for n in names:
        with Image.open(tmp_path / "pillow" / n) as a, Image.open(tmp_path / "device" / n) as b:
            assert a.format == b.format == "PNG" and a.mode == b.mode and np.array_equal(np.asarray(a), np.asarray(b)), n
        total += os.path.getsize(tmp_path / "device" / n)
    assert closing.endswith(f", {total} bytes"), closing
    rcs = {}
    for who in ("pillow", "device"):
        rcs[who] = extract.main(["--ckpt", ckpt, "--out", str(tmp_path / (who + ".bin")), "--dump_bits", str(tmp_path / (who + ".npy")),
                                 "--batch", "2"] + [str(tmp_path / who / n) for n in names])
    print("exit status:", rcs)
    assert rcs["device"] == rcs["pillow"]
    assert np.array_equal(np.load(tmp_path / "device.npy"), np.load(tmp_path / "pillow.npy"))
    assert (tmp_path / "device.bin").exists() == (tmp_path / "pillow.bin").exists() == (rcs["pillow"] == 0)
    if rcs["pillow"] == 0:
        assert (tmp_path / "device.bin").read_bytes() == data
