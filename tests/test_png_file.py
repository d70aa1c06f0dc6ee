"""The PNG file of include/ideas_hip.h ("The PNG file, written") as tests/png_ref.py restates it, held on the CPU to the readers that
matter -- zlib's inflate and Pillow's ``Image.open`` -- to its recorded files, and to the size of a measurable Huffman-only coder.
tests/test_png_file_gpu.py holds the device (csrc/png_bytes.hip) to the same restatement byte for byte."""
import io
import struct
import zlib

import numpy as np
import pytest

import png_ref as R
from conftest import Golden


@pytest.fixture(scope="module")
def files():
    """name -> (image, file, filtered bytes), made once."""
    out = {}
    for name in R.FIXTURES:
        img = R.fixture(name)
        out[name] = (img,) + R.png_file(img)
    return out


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_files_are_valid(files, name):
    """Three chunks with correct CRCs, a zlib stream that inflates to the filtered bytes, filtered bytes that undo to the pixels (by
    Pillow's reader), and a length inside the bound."""
    pytest.importorskip("PIL")
    from PIL import Image
    img, data, filtered = files[name]
    h, w, c = img.shape
    chunks = R.split_chunks(data)
    assert [k for k, _, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    for kind, payload, crc in chunks:
        assert crc == zlib.crc32(kind + payload), kind
    assert chunks[0][1] == struct.pack(">IIBBBBB", w, h, 8, 0 if c == 1 else 2, 0, 0, 0) and chunks[2][1] == b""
    idat = chunks[1][1]
    assert idat[:2] == b"\x78\x01" and zlib.decompress(idat) == filtered and len(filtered) == h * (w * c + 1)
    assert struct.unpack(">I", idat[-4:])[0] == zlib.adler32(filtered)
    with Image.open(io.BytesIO(data)) as im:
        assert im.format == "PNG" and im.size == (w, h) and im.mode == ("RGB" if c == 3 else "L")
        assert np.array_equal(np.asarray(im, dtype=np.uint8).reshape(h, w, c), img)
    assert 0 < len(data) <= R.max_bytes(c, h, w)


def test_every_filter_type_is_chosen_somewhere(files):
    seen = np.zeros(5, int)
    for img, _, filtered in files.values():
        seen += np.bincount(np.frombuffer(filtered, np.uint8).reshape(img.shape[0], -1)[:, 0], minlength=5)
    assert (seen > 0).all(), seen


def test_length_limit_fixture_needs_the_limit(files):
    """The plain Huffman tree of the fibonacci fixture's one stripe is deeper than 15 (without that the fixture proves nothing); the
    code the file uses is not, is complete, and still inflates (test_files_are_valid)."""
    img, _, filtered = files["fibonacci"]
    assert img.shape[0] == R.STRIPE_ROWS
    freq = np.bincount(np.frombuffer(filtered, np.uint8), minlength=257)
    freq[256] = 1
    depth = R.plain_huffman_depth(freq)
    print("plain Huffman depth", depth)
    assert depth > 15
    lens = R.limited_lengths(freq, 15)
    assert lens.max() == 15 and ((lens > 0) == (freq > 0)).all()
    assert sum(2.0 ** -int(v) for v in lens if v) == 1.0
    order = sorted((int(f), s) for s, f in enumerate(freq) if f)
    assert all(lens[a[1]] >= lens[b[1]] for a, b in zip(order, order[1:]))       # a lighter symbol never has the shorter code


def test_code_length_code_is_limited_to_seven_bits():
    """258 lengths whose counts run like Fibonacci numbers: the plain tree over the code-length symbols is deeper than 7."""
    freq = np.zeros(19, int)
    freq[:12] = [1, 1, 3, 5, 9, 15, 25, 41, 67, 40, 30, 21]
    assert freq.sum() == 258 and R.plain_huffman_depth(freq) > 7
    lens = R.limited_lengths(freq, 7)
    assert lens.max() == 7 and sum(2.0 ** -int(v) for v in lens if v) == 1.0


def test_flat_stripe_gets_two_codes_of_length_one():
    freq = np.zeros(257, int)
    freq[2], freq[256] = 32 * 100, 1
    lens = R.limited_lengths(freq, 15)
    assert lens[2] == 1 and lens[256] == 1 and lens.sum() == 2
    codes = R.canonical_codes(lens, 15)
    assert codes[2] == 0 and codes[256] == 1


def test_files_are_the_recorded_ones(files):
    """tests/golden/png_pinned.npz (tests/golden/make_golden_png.py): a change of the contract shows here."""
    z = Golden("png_pinned.npz").z
    assert sorted(z.files) == sorted("file/" + name for name in R.FIXTURES)
    for name, (_, data, _) in files.items():
        assert data == z["file/" + name].tobytes(), name


# the restatement's own ratios on the CPU, rounded up to the next whole percent
SIZE_BOUND = {"pink_256": 1.01, "pink_64_grey": 1.03}


@pytest.mark.parametrize("name", R.CONTENT_LIKE)
def test_size_against_a_huffman_only_zlib(files, name):
    """On content-like fixtures (seeded 1/f noise) IDAT is compared with ``zlib.compressobj(6, DEFLATED, 15, 8, Z_HUFFMAN_ONLY)`` over
    the same filtered bytes.  Measured here on the CPU: 256 x 256 x 3: 168035 / 167989 = 1.0003 -> bound 1.01 (the file is 0.972 of
    Pillow's default file of the same pixels); 64 x 64 x 1: 3782 / 3696 = 1.0233 -> bound 1.03 (two block headers on 4 KB; 1.003 of
    Pillow's file)."""
    _, data, filtered = files[name]
    idat = R.split_chunks(data)[1][1]
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    ref = co.compress(filtered) + co.flush()
    print(name, len(idat), len(ref), len(idat) / len(ref))
    assert len(idat) <= SIZE_BOUND[name] * len(ref)


def test_bound_and_refusals():
    assert R.max_bytes(3, 256, 256) == 43 + (8 * 1895 + 15 * 256 * 769 + 7) // 8 + 20
    assert R.max_bytes(2, 8, 8) == 0 and R.max_bytes(1, 0, 8) == 0 and R.max_bytes(3, 65536, 65536) == 0
