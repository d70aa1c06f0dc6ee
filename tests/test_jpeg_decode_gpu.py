"""The JPEG file read on the device (csrc/jpeg_decode.hip) against the Python restatement tests/jpegdecode_ref.py, which
tests/test_jpeg_decode.py holds to Pillow's pixels: through the C ABI on batches whose scans differ in length, on scans of many
subsequences and many rounds of the synchronise loop, on a stream that never re-synchronises early, on the device's own files with no
host in the loop, on Pillow's recorded and live files through the op, on corrupt input, with a dirty workspace, and end to end through
``extract.py --jpeg_decoder device``.  Everything is compared with ``array_equal`` / ``torch.equal``: there is no tolerance anywhere.
Every raw call writes into sentinel-guarded buffers."""
import io
import os

import numpy as np
import pytest
import torch

import jpegbytes_ref as R
import jpegdecode_ref as D
from attacks_ref import quant_tables
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

    def untouched(self):
        return bool((self.buf == SENT).all())

    def get(self, dtype, shape):
        return self.view.clone().view(dtype).view(shape)


def place(a, skew=0):
    """The bytes of the numpy array ``a`` on the device, guarded."""
    t = torch.from_numpy(np.ascontiguousarray(a)).view(-1).view(torch.uint8)
    g = Guarded(t.numel(), skew)
    g.view.copy_(t)
    return g


def grids(h, w, c, sub):
    bh, bw = (h + 7) // 8, (w + 7) // 8
    return (bh, bw), ((bh, bw) if sub == 0 else ((h + 15) // 16, (w + 15) // 16))


def raw_decode(files, extra_stride=37, skew=(0,) * 10, work=None, want_y=True, want_coef=True, lie=None):
    """ideas_jpeg_file_decode on files that share shape, subsampling and Huffman tables; skew = byte offsets of (out, y, coef_y,
    coef_c, status, scans, nbytes, qt, huff, workspace); ``work``: a Guarded workspace to use as it is (dirty).  The rows of ``scans``
    are filled with sentinel bytes behind their data; ``lie``: {image: the length to claim for it}.  -> dict(out, y, coef_y, coef_c,
    status)."""
    from ideas_amd import _lib
    lib = _lib.load()
    infos = [D.parse(f) for f in files]
    c, h, w, sub = (infos[0][k] for k in ("c", "h", "w", "subsampling"))
    for info in infos:
        assert (info["c"], info["h"], info["w"], info["subsampling"]) == (c, h, w, sub) and np.array_equal(info["huff"], infos[0]["huff"])
    b = len(files)
    (bh, bw), (cbh, cbw) = grids(h, w, c, sub)
    scans = [f[info["scan_offset"]:] for f, info in zip(files, infos)]
    stride = max(max(len(s) for s in scans), 1) + extra_stride
    rows = np.full((b, stride), SENT, np.uint8)
    for i, s in enumerate(scans):
        rows[i, :len(s)] = np.frombuffer(s, np.uint8)
    lengths = np.array([len(s) for s in scans], np.int32)
    for i, n in (lie or {}).items():
        lengths[i] = n
    qt = np.stack([info["qt"] for info in infos]).astype(np.uint16)
    nwork = int(lib.ideas_jpeg_file_decode_workspace_bytes(b, c, h, w, sub, stride))
    assert nwork > 0
    out, y = Guarded(b * h * w * c, skew[0]), Guarded(4 * b * h * w * c, 4 * skew[1])
    coef_y, coef_c = Guarded(2 * b * bh * bw * 64, 2 * skew[2]), Guarded(2 * b * 2 * cbh * cbw * 64, 2 * skew[3])
    status = Guarded(4 * b, 4 * skew[4])
    g_scans, g_n, g_qt, g_huff = place(rows, skew[5]), place(lengths, 4 * skew[6]), place(qt, 2 * skew[7]), place(infos[0]["huff"], skew[8])
    if work is None:
        work = Guarded(nwork, skew[9], fill=0xFF)                                # never zeros: the call clears what it needs
    assert work.n >= nwork
    rc = lib.ideas_jpeg_file_decode(out.ptr(), y.ptr() if want_y else None, coef_y.ptr() if want_coef else None,
                                    coef_c.ptr() if want_coef and c == 3 else None, status.ptr(), g_scans.ptr(), g_n.ptr(), stride,
                                    g_qt.ptr(), g_huff.ptr(), work.ptr(), b, c, h, w, sub, _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for g in (out, y, coef_y, coef_c, status, g_scans, g_n, g_qt, g_huff, work):
        assert g.intact()
    assert np.array_equal(g_scans.view.cpu().numpy().reshape(b, stride), rows) and np.array_equal(g_n.get(torch.int32, (b,)).cpu().numpy(), lengths)
    assert np.array_equal(g_qt.get(torch.int16, qt.shape).cpu().numpy().view(np.uint16), qt)      # the inputs are only read
    assert np.array_equal(g_huff.view.cpu().numpy(), infos[0]["huff"].reshape(-1))
    assert want_y or y.untouched()
    assert want_coef or coef_y.untouched()
    assert (want_coef and c == 3) or coef_c.untouched()
    return dict(out=out.get(torch.uint8, (b, h, w, c)), y=y.get(torch.float32, (b, h, w, c)) if want_y else None,
                coef_y=coef_y.get(torch.int16, (b, bh, bw, 64)) if want_coef else None,
                coef_c=coef_c.get(torch.int16, (b, 2, cbh, cbw, 64)) if want_coef and c == 3 else None,
                status=status.get(torch.int32, (b,)).cpu().tolist())


_REF = {}


def ref(data):
    """The restatement's answer for one file, computed once."""
    if data not in _REF:
        _REF[data] = D.decode_ref(data)
    return _REF[data]


def check(files, got, tag=()):
    """Status, coefficients, bytes and ``y`` of every file of the batch against the restatement."""
    from ideas_amd import data as Data
    for i, f in enumerate(files):
        want = ref(f)
        assert got["status"][i] == want["status"] == 0, ("status", tag, i, got["status"])
        if got["coef_y"] is not None:
            assert np.array_equal(got["coef_y"][i].cpu().numpy(), want["coef_y"]), ("coef_y", tag, i)
        if got["coef_c"] is not None:
            assert np.array_equal(got["coef_c"][i].cpu().numpy(), want["coef_c"]), ("coef_c", tag, i)
        assert np.array_equal(got["out"][i].cpu().numpy(), want["out"]), ("bytes", tag, i)
    if got["y"] is not None:
        assert torch.equal(got["y"], Data.u8_to_f32(got["out"]).permute(0, 2, 3, 1)), ("y", tag)      # bitwise the receiver's decode


def files_of(kinds, h, w, c, quality, sub):
    return [R.jpeg_bytes_ref(R.make_image(kind, h, w, c), quality, sub)[0] for kind in kinds]


# ------------------------------------------------------------------------------------------------- the kernels against the restatement
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("hw", SHAPES)
def test_pixels_and_coefficients_are_the_restatement(hw, c):
    """B = 3 in one call, a noise, a flat and a 0/255 image: three scan lengths.  Shapes with odd block grids (dummy luma blocks at
    4:2:0)."""
    h, w = hw
    for quality in (1, 75, 100):
        for sub in (0, 2):
            files = files_of(("noise", "flat", "binary"), h, w, c, quality, sub)
            check(files, raw_decode(files), (hw, c, quality, sub))
    only = raw_decode(files, want_y=False, want_coef=False)                       # the optional outputs change nothing
    check(files, only)


def test_many_subsequences_and_many_rounds():
    """Noise at quality 100.  200 x 264 x 3 at 4:2:0: 734 subsequences, more than the workgroup has threads, and 137 rounds of the
    synchronise loop (asserted >= 3 on the schedule run in Python); 256 x 256 x 1: 1024 blocks."""
    f = files_of(("noise",), 200, 264, 3, 100, 2)
    rounds, nsub = D.sync_rounds(f[0])
    print("200x264x3:", rounds, "rounds,", nsub, "subsequences")
    assert rounds >= 3 and nsub > 256
    check(f, raw_decode(f, skew=(1, 1, 1, 1, 1, 3, 1, 1, 5, 7)), "200x264x3")
    g = files_of(("noise",), 256, 256, 1, 100, 0)
    assert D.sync_rounds(g[0])[1] > 256
    check(g, raw_decode(g), "256x256x1")


@pytest.mark.parametrize("sub", [0, 2])
def test_a_flat_image_never_resynchronises_early(sub):
    """Flat 256 x 256 x 3: every block is the same few bits, so a speculative start in the wrong phase can stay wrong to the end of its
    subsequence; the loop's bound carries it."""
    f = files_of(("flat",), 256, 256, 3, 75, sub)
    print("flat:", D.sync_rounds(f[0]))
    check(f, raw_decode(f), ("flat", sub))


def test_placement_changes_nothing():
    files = files_of(("noise", "smooth"), 24, 40, 3, 75, 2)
    a = raw_decode(files)
    b = raw_decode(files, extra_stride=0, skew=(3, 1, 1, 3, 1, 5, 1, 1, 7, 9))
    check(files, a)
    check(files, b)


def test_dirty_workspace_and_repeated_calls():
    """One workspace, 0xFF-filled and skewed, never cleared by the caller: a batch of noise, the same call again, then a small batch."""
    from ideas_amd import _lib
    big = files_of(("noise", "binary", "noise", "smooth"), 64, 64, 3, 100, 0)
    stride = max(len(f) - 623 for f in big) + 37
    work = Guarded(int(_lib.load().ideas_jpeg_file_decode_workspace_bytes(4, 3, 64, 64, 0, stride)), skew=5, fill=0xFF)
    check(big, raw_decode(big, work=work))
    check(big, raw_decode(big, work=work))
    small = files_of(("flat", "smooth"), 17, 33, 3, 75, 2)
    check(small, raw_decode(small, work=work))


# ------------------------------------------------------------------------------------------------- no host in the loop
def standard_huff(c):
    t = np.zeros((c, 2, 272), np.uint8)
    for k in range(c):
        i = 1 if k else 0
        for j, (bits, vals) in enumerate(((R.DC_BITS[i], R.DC_VALS[i]), (R.AC_BITS[i], R.AC_VALS[i]))):
            t[k, j, :16], t[k, j, 16:16 + len(vals)] = bits, vals
    return t


@pytest.mark.parametrize("shape", [(4, 64, 64, 3), (2, 256, 256, 3), (3, 40, 24, 1)])
def test_the_devices_own_files_decode_to_the_round_trip(shape):
    """``jpeg_file_encode`` writes files on the device; their scans are decoded where they lie (row b of ``files`` behind the header
    of known size) and give the round trip's bytes, ``y`` and coefficients."""
    from ideas_amd import _lib
    from ideas_amd.op import jpeg_file_encode, jpeg_file_roundtrip
    lib = _lib.load()
    b, h, w, c = shape
    x = torch.from_numpy(np.stack([R.make_image(R.KINDS[i % 3], h, w, c) for i in range(b)])).cuda()
    hdr = 623 if c == 3 else 328
    for quality in (50, 90):
        for sub in ((0, 2) if c == 3 else (0,)):
            files, nbytes, out, y = jpeg_file_encode(x, quality, sub, return_decoded=True)
            _, _, coef_y, coef_c = jpeg_file_roundtrip(x, quality, sub, return_coef=True)
            stride = files.shape[1]
            qt = torch.from_numpy(np.tile(quant_tables(quality).reshape(2, 64)[[0, 1, 1][:c]].astype(np.int16), (b, 1, 1))).cuda()
            huff = torch.from_numpy(standard_huff(c)).cuda()
            lengths = nbytes - hdr
            work = torch.empty(int(lib.ideas_jpeg_file_decode_workspace_bytes(b, c, h, w, sub, stride)), dtype=torch.uint8, device="cuda")
            o2, y2, cy2 = torch.empty_like(out), torch.empty_like(y), torch.empty_like(coef_y)
            cc2 = torch.empty_like(coef_c) if c == 3 else None
            status = torch.full((b,), 7, dtype=torch.int32, device="cuda")
            rc = lib.ideas_jpeg_file_decode(o2.data_ptr(), y2.data_ptr(), cy2.data_ptr(), _lib.ptr(cc2), status.data_ptr(),
                                            files.data_ptr() + hdr, lengths.data_ptr(), stride, qt.data_ptr(), huff.data_ptr(),
                                            work.data_ptr(), b, c, h, w, sub, _lib.stream_ptr())
            assert rc == 0, rc
            tag = (shape, quality, sub)
            assert status.tolist() == [0] * b, tag
            assert torch.equal(cy2, coef_y), tag
            assert c == 1 or torch.equal(cc2, coef_c), tag
            assert torch.equal(o2, out) and torch.equal(y2, y), tag
            assert y2.is_contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------------- the op on Pillow's files
def test_op_reads_the_recorded_pillow_files():
    from ideas_amd.op import jpeg_file_decode, jpeg_file_decode_grouped
    z = Golden("jpegdecode.npz").z
    tags = [k[5:] for k in z.files if k.startswith("file/")]
    assert len(tags) == 9
    for tag in tags:
        data = z["file/" + tag].tobytes()
        assert torch.equal(jpeg_file_decode_grouped([data])[0].cpu(), torch.from_numpy(z["pixels/" + tag])), tag
    # the 60 standard files, a shape and channel count at a time: qualities and subsamplings mixed in one call to the grouping op
    old = Golden("jpegfile_bytes.npz").z
    by_shape = {}
    for key in old.files:
        if key.startswith("file/"):
            by_shape.setdefault(key.split("/")[1], []).append(old[key].tobytes())
    assert sum(len(v) for v in by_shape.values()) == 60
    for shape, files in sorted(by_shape.items()):
        got = jpeg_file_decode_grouped(files).cpu().numpy()
        for i, f in enumerate(files):
            assert np.array_equal(got[i], ref(f)["out"]), (shape, i)
    # per-image tables: qualities 30, 75 and 95 in ONE call
    mixed = [R.jpeg_bytes_ref(R.make_image("noise", 24, 40, 3), q, 2)[0] for q in (30, 75, 95)]
    out, y, status = jpeg_file_decode(mixed)
    assert status.tolist() == [0, 0, 0] and tuple(y.shape) == (3, 3, 24, 40) and y.is_contiguous(memory_format=torch.channels_last)
    for i, f in enumerate(mixed):
        assert np.array_equal(out[i].cpu().numpy(), ref(f)["out"]), i
    # two groups, results in input order: a file with Huffman tables of its own between two standard ones
    own = z["file/opt95/17x33x3/noise"].tobytes()
    std = [R.jpeg_bytes_ref(R.make_image(kind, 17, 33, 3), 75, 2)[0] for kind in ("smooth", "binary")]
    with pytest.raises(RuntimeError, match="file 1 differs"):
        jpeg_file_decode([std[0], own, std[1]])
    got = jpeg_file_decode_grouped([std[0], own, std[1]]).cpu().numpy()
    assert np.array_equal(got[0], ref(std[0])["out"]) and np.array_equal(got[2], ref(std[1])["out"])
    assert np.array_equal(got[1], z["pixels/opt95/17x33x3/noise"])
    out, y, status, cy, cc = jpeg_file_decode(std, return_coef=True)
    assert np.array_equal(cy[1].cpu().numpy(), ref(std[1])["coef_y"]) and np.array_equal(cc[0].cpu().numpy(), ref(std[0])["coef_c"])


@pytest.mark.parametrize("hw", SHAPES[1:])
def test_op_reads_live_pillow_files(hw):
    pytest.importorskip("PIL")
    from PIL import Image, features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo: its decoder need not be that of the model")
    from ideas_amd.op import jpeg_file_decode_grouped
    h, w = hw
    options = (dict(quality=75, subsampling=2), dict(quality=30, subsampling=0), dict(quality=95, optimize=True),
               dict(quality=100, optimize=True, subsampling=0), dict(qtables=[list(range(1, 65)), [3] * 64]), dict(quality=1))
    for c in (1, 3):
        files, want = [], []
        for kind in R.KINDS:
            img = R.make_image(kind, h, w, c)
            for kw in options:
                buf = io.BytesIO()
                Image.fromarray(img[..., 0] if c == 1 else img).save(buf, "JPEG", **kw)
                files.append(buf.getvalue())
                with Image.open(io.BytesIO(files[-1])) as im:
                    want.append(np.asarray(im, dtype=np.uint8).reshape(h, w, c))
        got = jpeg_file_decode_grouped(files).cpu().numpy()
        differing = [i for i in range(len(files)) if not np.array_equal(got[i], want[i])]
        assert not differing, (hw, c, differing)


# ------------------------------------------------------------------------------------------------- corrupt input
def damaged():
    """Three files of 24 x 40 x 3 at quality 75, 4:2:0; the middle one (upside-down noise: 1159 bytes, its scan 534 bytes behind a
    623-byte header) is the one the tests damage."""
    files = files_of(("noise", "smooth", "binary"), 24, 40, 3, 75, 2)
    files[1] = R.jpeg_bytes_ref(R.make_image("noise", 24, 40, 3)[::-1].copy(), 75, 2)[0]
    assert len(files[1]) == 1159
    return files


def test_a_truncated_scan_is_flagged_alone():
    """The middle file's scan cut to half (267 bytes, no EOI): status [0, -1, 0], both neighbours exact, bands intact."""
    files = damaged()
    cut = files[1][:623 + 267]
    assert D.decode_coefs(D.parse(cut), cut[623:])[2] == -1
    got = raw_decode([files[0], cut, files[2]])
    assert got["status"] == [0, -1, 0]
    for i in (0, 2):
        want = ref(files[i])
        assert np.array_equal(got["out"][i].cpu().numpy(), want["out"]) and np.array_equal(got["coef_y"][i].cpu().numpy(), want["coef_y"])
        assert np.array_equal(got["coef_c"][i].cpu().numpy(), want["coef_c"])


@pytest.mark.parametrize("pos,status", [(245, 0), (229, -1)])
def test_a_flipped_byte_gives_the_restatements_answer(pos, status):
    """Bit 0 of one byte in the middle of the middle file's scan, chosen on the CPU.  Byte 245: the restatement decodes other
    coefficients and status 0 (the stream re-synchronises and still fills every block); byte 229: status -1 (a symbol without a code).
    The device gives the same status and, where it is 0, the same coefficients; the neighbours are exact."""
    files = damaged()
    bad = bytearray(files[1])
    bad[623 + pos] ^= 1
    bad = bytes(bad)
    cy, cc, want = D.decode_coefs(D.parse(bad), bad[623:])
    assert want == status
    got = raw_decode([files[0], bad, files[2]])
    assert got["status"] == [0, status, 0]
    if status == 0:
        assert not np.array_equal(cy, ref(files[1])["coef_y"])
        assert np.array_equal(got["coef_y"][1].cpu().numpy(), cy) and np.array_equal(got["coef_c"][1].cpu().numpy(), cc)
    for i in (0, 2):
        assert np.array_equal(got["out"][i].cpu().numpy(), ref(files[i])["out"])


@pytest.mark.parametrize("claimed", [-1, 1 << 30])
def test_a_length_outside_its_row_is_flagged_alone(claimed):
    """The lengths live on the device, so the host cannot refuse them: nbytes[1] below 0 or beyond row_stride flags image 1, nothing
    outside its row is read or written (the bands hold), and the neighbours are exact."""
    files = damaged()
    got = raw_decode(files, lie={1: claimed})
    assert got["status"] == [0, -1, 0]
    for i in (0, 2):
        assert np.array_equal(got["out"][i].cpu().numpy(), ref(files[i])["out"])
        assert np.array_equal(got["coef_y"][i].cpu().numpy(), ref(files[i])["coef_y"])


def test_op_names_a_corrupt_file():
    from ideas_amd.op import jpeg_file_decode_grouped
    files = damaged()
    files[1] = files[1][:623 + 267]
    with pytest.raises(RuntimeError, match=r"file\(s\) \[1\] are corrupt"):
        jpeg_file_decode_grouped(files)


# ------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """The reference's own checkpoint of tests/golden/ckpt_r256.npz as a file (the discriminator's omitted tensors: zeros)."""
    from ckpt_fixture import build_reference_checkpoint
    raw = build_reference_checkpoint(Golden("ckpt_r256.npz"), lambda key, shape: torch.zeros(shape))
    path = str(tmp_path_factory.mktemp("jpegdecode_ckpt") / "1.pt")
    torch.save(raw, path)
    return path


def test_extract_reads_the_same_bits_with_either_decoder(ckpt, tmp_path, capsys):
    """``hide.py --format jpeg`` writes .jpg files; ``extract.py --jpeg_decoder device`` gets the bits the Pillow path gets
    (``--dump_bits``), the same exit status and the same payload file.  The fixture's networks are untrained, so neither path recovers
    the payload: measured, both end with status 1; the payload's bytes are compared wherever the Pillow path has them."""
    pytest.importorskip("PIL")
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo: its decoder need not be that of the model")
    import extract
    import hide
    payload = tmp_path / "payload.bin"
    payload.write_bytes(bytes(range(48)))
    folder = tmp_path / "jpg"
    hide.main(["--ckpt", ckpt, "--payload", str(payload), "--seed", "3", "--batch", "2", "--format", "jpeg", "--jpeg_quality", "100",
               "--jpeg_subsampling", "444", "--jpeg_encoder", "device", "--out", str(folder)])
    names = [str(folder / n) for n in sorted(os.listdir(folder))]
    assert names and all(n.endswith(".jpg") for n in names)
    capsys.readouterr()
    rcs = {}
    for decoder in ("pillow", "device"):
        rcs[decoder] = extract.main(["--ckpt", ckpt, "--out", str(tmp_path / (decoder + ".bin")), "--dump_bits", str(tmp_path / (decoder + ".npy")),
                                     "--batch", "2", "--jpeg_decoder", decoder] + names)
    print("exit status:", rcs)
    assert "falls back" not in capsys.readouterr().err
    assert rcs["device"] == rcs["pillow"]
    assert np.array_equal(np.load(tmp_path / "device.npy"), np.load(tmp_path / "pillow.npy"))
    # (the fixture's networks are untrained, as in tests/test_ecc_gpu.py: measured, both decoders end with status 1, the frame's CRC
    # line and no payload file.  Whatever the Pillow path recovers, the device path recovers.)
    assert (tmp_path / "device.bin").exists() == (tmp_path / "pillow.bin").exists() == (rcs["pillow"] == 0)
    if rcs["pillow"] == 0:
        assert (tmp_path / "device.bin").read_bytes() == (tmp_path / "pillow.bin").read_bytes() == payload.read_bytes()
