"""The JPEG file written on the device (csrc/jpeg_bytes.hip) against the Python restatement tests/jpegbytes_ref.py, which
tests/test_jpeg_bytes.py holds to Pillow's files: through the C ABI from the restatement's own coefficients (so that a difference is the
coder's), on batches whose files differ in length, on scans of many chunks, with guard bands round every buffer, a dirty workspace
and a coefficient without a code; and end to end through the op and ``hide.py --jpeg_encoder device`` against Pillow's recorded and
live files.  Files are compared as ``bytes``: there is no tolerance anywhere."""
import io
import os

import numpy as np
import pytest
import torch

import jpegbytes_ref as R
from conftest import Golden

pytestmark = pytest.mark.gpu

BAND = 64                     # sentinel bytes either side of every buffer
SENT = 0xA5
SHAPES = [(1, 1), (9, 129), (17, 33), (24, 40), (23, 7)]


class Guarded:
    """``nbytes`` on the device between two bands of sentinel bytes, ``skew`` bytes off the allocation's 16-byte alignment; the
    payload starts as ``fill``."""

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


def place(a, skew=0):
    """The bytes of the numpy array ``a`` on the device, guarded."""
    t = torch.from_numpy(np.ascontiguousarray(a)).view(-1).view(torch.uint8)
    g = Guarded(t.numel(), skew)
    g.view.copy_(t)
    return g


def coefs_of(x, quality, sub):
    """The restatement's coefficients of the batch ``x`` uint8 [B, H, W, C]: (coef_y int16 [B, bh, bw, 64], coef_c [B, 2, cbh, cbw, 64]
    or None)."""
    res = [R.jpeg_file_ref(img, quality, sub) for img in x]
    cy = np.stack([r["coef_y"] for r in res])
    return cy, (np.stack([r["coef_c"] for r in res]) if x.shape[3] == 3 else None)


def raw_encode(cy, cc, h, w, quality, sub, extra_stride=37, skew=(0, 0, 0, 0, 0), work=None):
    """ideas_jpeg_file_encode on coefficient arrays; skew = byte offsets of (files, nbytes, coef_y, coef_c, workspace); ``work``: a
    Guarded workspace to use as it is (dirty).  Every buffer is guarded.  -> (list of files as bytes, None where nbytes is -1; nbytes as
    a list; the row of every image as a uint8 array)."""
    from ideas_amd import _lib
    lib = _lib.load()
    b, c = cy.shape[0], 1 if cc is None else 3
    bound = int(lib.ideas_jpeg_file_max_bytes(c, h, w, sub))
    assert bound == R.max_bytes(c, h, w, sub)
    stride = bound + extra_stride
    nwork = int(lib.ideas_jpeg_file_encode_workspace_bytes(b, c, h, w, sub))
    assert nwork > 0
    files, nbytes = Guarded(b * stride, skew[0]), Guarded(4 * b, 4 * skew[1])
    gy, gc = place(cy, 2 * skew[2]), (place(cc, 2 * skew[3]) if cc is not None else None)
    if work is None:
        work = Guarded(nwork, skew[4], fill=0xFF)                                # never zeros: the call clears what it needs
    assert work.n >= nwork
    rc = lib.ideas_jpeg_file_encode(files.ptr(), nbytes.ptr(), stride, gy.ptr(), gc.ptr() if gc else None, work.ptr(), b, c, h, w, quality,
                                    sub, _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert files.intact() and nbytes.intact() and gy.intact() and work.intact() and (gc is None or gc.intact())
    assert np.array_equal(gy.view.cpu().numpy().view(np.int16).reshape(cy.shape), cy)          # the inputs are only read
    n = nbytes.view.cpu().numpy().view(np.int32).tolist()
    rows = files.view.cpu().numpy().reshape(b, stride)
    assert all(v == -1 or 0 < v <= bound for v in n), n
    assert (rows[:, bound:] == SENT).all()                                       # nothing behind the bound, inside the row
    return [None if v < 0 else rows[i, :v].tobytes() for i, v in enumerate(n)], n, rows


def batch(kinds, h, w, c):
    return np.stack([R.make_image(kind, h, w, c) for kind in kinds])


# ------------------------------------------------------------------------------------------------- the coder against the restatement
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", SHAPES)
def test_files_are_the_restatement(hw, c):
    """B = 3 in one call, a noise, a flat and a 0/255 image: three lengths.  Shapes with odd block grids (dummy luma blocks at 4:2:0)."""
    h, w = hw
    x = batch(("noise", "flat", "binary"), h, w, c)
    for quality in (1, 75, 100):
        for sub in (0, 2):
            cy, cc = coefs_of(x, quality, sub)
            got, n, _ = raw_encode(cy, cc, h, w, quality, sub)
            want = [R.encode_coefs(cy[i], None if cc is None else cc[i], h, w, c, quality, sub)[0] for i in range(3)]
            for i in range(3):
                assert got[i] == want[i], (hw, c, quality, sub, i, n[i], len(want[i]))
            assert n == [len(f) for f in want]
            assert quality == 1 or h * w == 1 or len(set(n)) == 3, n             # (at quality 1 every tiny image is its DC alone)


@pytest.mark.parametrize("shape,sub", [((200, 264, 3), 2), ((256, 256, 1), 0)])
def test_scans_of_many_chunks(shape, sub):
    """Noise at quality 100.  200 x 264 at 4:2:0: 1326 blocks (the prefix sum of the bit counts takes two trips) and about 95 KB of
    scan (24 trips of the stuffing pass, hundreds of stuffed bytes); 256 x 256 x 1: 1024 blocks, exactly one trip."""
    h, w, c = shape
    x = batch(("noise",), h, w, c)
    cy, cc = coefs_of(x, 100, sub)
    got, n, _ = raw_encode(cy, cc, h, w, 100, sub, skew=(1, 1, 1, 1, 3))
    want, stats = R.encode_coefs(cy[0], None if cc is None else cc[0], h, w, c, 100, sub)
    print(shape, n, stats)
    assert stats["blocks"] == (1326 if c == 3 else 1024) and stats["stuffed"] > 100 and len(want) > 16 * 4096
    assert n == [len(want)] and got[0] == want


def test_placement_changes_nothing():
    """Every buffer off its alignment (the coefficients by 2 bytes: the 16-byte loads give way to 2-byte ones)."""
    x = batch(("noise", "smooth"), 24, 40, 3)
    cy, cc = coefs_of(x, 75, 2)
    a = raw_encode(cy, cc, 24, 40, 75, 2)
    b = raw_encode(cy, cc, 24, 40, 75, 2, extra_stride=0, skew=(3, 1, 1, 3, 5))
    assert a[0] == b[0] and a[1] == b[1] and a[0][0] == R.encode_coefs(cy[0], cc[0], 24, 40, 3, 75, 2)[0]


def test_dirty_workspace_and_repeated_calls():
    """One workspace, never cleared by the caller: a batch of noise (long files: every word of the bit buffer gets used), then a
    small flat batch whose bits are ORed into what the first call left unless the call clears it; and the same call twice."""
    from ideas_amd import _lib
    big = batch(("noise", "noise", "binary", "noise"), 64, 64, 3)
    big[1] = big[1][::-1]
    cy, cc = coefs_of(big, 100, 0)
    work = Guarded(int(_lib.load().ideas_jpeg_file_encode_workspace_bytes(4, 3, 64, 64, 0)), fill=0xFF)
    first, _, rows1 = raw_encode(cy, cc, 64, 64, 100, 0, work=work)
    assert first == [R.encode_coefs(cy[i], cc[i], 64, 64, 3, 100, 0)[0] for i in range(4)]
    again, _, rows2 = raw_encode(cy, cc, 64, 64, 100, 0, work=work)
    assert again == first
    for i, f in enumerate(first):
        assert np.array_equal(rows1[i, :len(f)], rows2[i, :len(f)])
    small = batch(("flat", "smooth"), 17, 33, 3)
    sy, sc = coefs_of(small, 75, 2)
    got, _, _ = raw_encode(sy, sc, 17, 33, 75, 2, work=work)
    assert got == [R.encode_coefs(sy[i], sc[i], 17, 33, 3, 75, 2)[0] for i in range(2)]


@pytest.mark.parametrize("k,v", [(9, 1024), (63, -1024), (0, 4000)])
def test_an_image_without_a_code_is_flagged_alone(k, v):
    """Image 1 of 3 gets a coefficient that has no Huffman code (an AC of +-1024; a DC of 4000, more than 2047 from any DC an encoder
    produces): its length is -1, its row stays inside its bound, and images 0 and 2 are the files they were."""
    x = batch(("noise", "smooth", "binary"), 24, 40, 3)
    cy, cc = coefs_of(x, 75, 2)
    want, clean, _ = raw_encode(cy, cc, 24, 40, 75, 2)
    cy = cy.copy()
    cy[1, 1, 2, k] = v
    assert R.encode_coefs(cy[1], cc[1], 24, 40, 3, 75, 2)[0] is None
    got, n, _ = raw_encode(cy, cc, 24, 40, 75, 2)
    assert n == [clean[0], -1, clean[2]] and got[0] == want[0] and got[2] == want[2] and got[1] is None


def test_rows_past_two_gigabytes():
    """The caller chooses row_stride: 2100 one-block images in rows of 2^20 bytes put the last rows past byte 2^31 of ``files``, where
    a 32-bit row offset would land in the first rows (or outside).  Copies of 3 different images; checked on the device, but for the
    first 747 bytes (the bound) of every row."""
    from ideas_amd import _lib
    lib = _lib.load()
    b, stride, bound = 2100, 1 << 20, 328 + 416 + 3
    cy, _ = coefs_of(batch(("noise", "binary", "smooth"), 8, 8, 1), 75, 0)
    want = [R.encode_coefs(cy[i], None, 8, 8, 1, 75, 0)[0] for i in range(3)]
    assert len({len(f) for f in want}) == 3 and int(lib.ideas_jpeg_file_max_bytes(1, 8, 8, 0)) == bound
    cyd = torch.from_numpy(cy).cuda()[torch.arange(b, device="cuda") % 3].contiguous()
    buf = torch.full((BAND + b * stride + BAND,), SENT, dtype=torch.uint8, device="cuda")
    nbytes = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    work = torch.empty(int(lib.ideas_jpeg_file_encode_workspace_bytes(b, 1, 8, 8, 0)), dtype=torch.uint8, device="cuda")
    rc = lib.ideas_jpeg_file_encode(buf.data_ptr() + BAND, nbytes.data_ptr(), stride, cyd.data_ptr(), None, work.data_ptr(), b, 1, 8, 8, 75,
                                    0, _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    rows = buf[BAND:BAND + b * stride].view(b, stride)
    assert nbytes.cpu().tolist() == [len(want[i % 3]) for i in range(b)]
    head = rows[:, :bound].cpu().numpy()
    for k in range(3):
        assert (head[k::3, :len(want[k])] == np.frombuffer(want[k], np.uint8)).all(), k
    assert bool((rows[:, bound:] == SENT).all()) and bool((buf[:BAND] == SENT).all()) and bool((buf[-BAND:] == SENT).all())


# ------------------------------------------------------------------------------------------------- end to end
def test_op_writes_the_recorded_pillow_files():
    """From the image bytes, through the round trip's coefficient outputs and the coder: Pillow's files, recorded."""
    from ideas_amd.op import jpeg_file_encode, jpeg_file_roundtrip, jpeg_files_to_host
    z = Golden("jpegfile_bytes.npz").z
    groups = {}
    for key in z.files:
        if key.startswith("file/"):
            _, shape, kind, q, s = key.split("/")
            groups.setdefault((shape, int(q[1:]), int(s[1:])), []).append((kind, key))
    assert len(groups) == 5 * (1 + 2) * 3
    for (shape, q, s), members in sorted(groups.items()):
        h, w, c = (int(v) for v in shape.split("x"))
        x = torch.from_numpy(batch([kind for kind, _ in members], h, w, c)).cuda()
        files, nbytes, out, y = jpeg_file_encode(x, q, s, return_decoded=True)
        assert files.dtype == torch.uint8 and tuple(files.shape) == (len(members), R.max_bytes(c, h, w, s))
        assert nbytes.dtype == torch.int32 and tuple(nbytes.shape) == (len(members),)
        got = jpeg_files_to_host(files, nbytes)
        for (kind, key), data in zip(members, got):
            assert data == z[key].tobytes(), key
        o2, y2 = jpeg_file_roundtrip(x, q, s)
        assert torch.equal(out, o2) and torch.equal(y, y2)
    pair = jpeg_file_encode(x, 75, "4:2:0")
    assert len(pair) == 2 and jpeg_files_to_host(*pair) == jpeg_files_to_host(*jpeg_file_encode(x, 75))      # 4:2:0 is the default


def test_pillow_decodes_the_files_to_the_round_trip():
    pytest.importorskip("PIL")
    from PIL import Image, features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo: its decoder need not be that of the model")
    from ideas_amd.op import jpeg_file_encode, jpeg_files_to_host
    for h, w, c in ((33, 40, 3), (17, 23, 1), (64, 64, 3)):
        x = torch.from_numpy(batch(("noise", "smooth", "binary"), h, w, c)).cuda()
        for sub in ("4:2:0", "4:4:4"):
            files, nbytes, out, _ = jpeg_file_encode(x, 75, sub, return_decoded=True)
            for i, data in enumerate(jpeg_files_to_host(files, nbytes)):
                with Image.open(io.BytesIO(data)) as im:
                    assert im.format == "JPEG" and im.size == (w, h) and im.mode == ("RGB" if c == 3 else "L")
                    got = np.asarray(im, dtype=np.uint8).reshape(h, w, c)
                assert np.array_equal(got, out[i].cpu().numpy()), (h, w, c, sub, i)


def test_op_validation_empty_input_and_uncodable_files():
    from ideas_amd.op import jpeg_file_encode, jpeg_files_to_host
    x = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device="cuda")
    for bad in ("4:2:2", 1, None, True):
        with pytest.raises(RuntimeError, match="jpeg_file_encode: subsampling"):
            jpeg_file_encode(x, 75, bad)
    for q in (0, 101, 7.5):
        with pytest.raises(RuntimeError, match="jpeg_file_encode: quality"):
            jpeg_file_encode(x, q)
    with pytest.raises(RuntimeError, match="uint8"):
        jpeg_file_encode(x.float(), 75)
    files, nbytes, out, y = jpeg_file_encode(x[:0], 75, return_decoded=True)     # no launch
    assert tuple(files.shape) == (0, 623 + 416 * 6 + 3) and tuple(nbytes.shape) == (0,) and tuple(out.shape) == (0, 8, 8, 3)
    assert jpeg_files_to_host(files, nbytes) == []
    files, nbytes = jpeg_file_encode(x, 75)
    with pytest.raises(RuntimeError, match="uint8"):
        jpeg_files_to_host(files.int(), nbytes)
    nbytes[1] = -1
    with pytest.raises(RuntimeError, match=r"image\(s\) \[1\]"):
        jpeg_files_to_host(files, nbytes)


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """The reference's own checkpoint of tests/golden/ckpt_r256.npz as a file (the discriminator's omitted tensors: zeros)."""
    from ckpt_fixture import build_reference_checkpoint
    raw = build_reference_checkpoint(Golden("ckpt_r256.npz"), lambda key, shape: torch.zeros(shape))
    path = str(tmp_path_factory.mktemp("jpegbytes_ckpt") / "1.pt")
    torch.save(raw, path)
    return path


def test_hide_writes_the_same_files_with_either_encoder(ckpt, tmp_path, capsys):
    """``hide.py --format jpeg --jpeg_encoder device`` against ``--jpeg_encoder pillow``, same seed: the same directory, byte for byte."""
    pytest.importorskip("PIL")
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo: its JPEG files need not be those of the model")
    import hide
    payload = tmp_path / "payload.bin"
    payload.write_bytes(bytes(range(48)))
    common = ["--ckpt", ckpt, "--payload", str(payload), "--seed", "3", "--batch", "2", "--format", "jpeg", "--jpeg_quality", "75"]
    for sub in ("420", "444"):
        hide.main(common + ["--out", str(tmp_path / ("pillow" + sub)), "--jpeg_subsampling", sub])
        assert "bytes" not in capsys.readouterr().out.strip().splitlines()[-1]  # the closing line of today's path stays as it is
        hide.main(common + ["--out", str(tmp_path / ("device" + sub)), "--jpeg_subsampling", sub, "--jpeg_encoder", "device"])
        closing = capsys.readouterr().out.strip().splitlines()[-1]
        names = sorted(os.listdir(tmp_path / ("pillow" + sub)))
        assert names and all(n.endswith(".jpg") for n in names) and sorted(os.listdir(tmp_path / ("device" + sub))) == names
        total = 0
        for n in names:
            a, b = (tmp_path / ("pillow" + sub) / n).read_bytes(), (tmp_path / ("device" + sub) / n).read_bytes()
            assert a == b, (sub, n, len(a), len(b))
            total += len(b)
        assert closing.endswith(f", {total} bytes"), closing
