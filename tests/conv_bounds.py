"""Banded operands for tests/test_conv_bounds_gpu.py: a tensor placed inside a larger device buffer with a guard band on each side,
so that a kernel's memory footprint can be read off afterwards -- without any access of the test's own outside the buffer.

Three kinds of band (``Band(t, kind)``):

``"out"``     outputs written by plain stores (y, gx, xb).  Bands AND payload hold the bit pattern of
              test_ops_gpu.py::test_pointwise_flat_gemm_kernel_never_writes_past_its_output, 0x7fc0dead (bf16: 0x7fc0 pairs), a NaN:
              a store of any computed value changes it, and a pixel the launch was to leave alone still shows it bit for bit.
``"atomic"``  outputs written by floating-point atomics (the gw of every weight-gradient kernel).  A NaN band must NOT be used here:
              NaN + v keeps the NaN's payload, so a stray atomicAdd would leave the band looking intact.  Zero hides a stray plain
              store of zero, and a large finite value absorbs small additions (v + eps == v).  The bands therefore hold a small
              finite pattern, the bits 0x35A5A5A5 (about 1.2e-6): adding any contribution of a gradient of randn operands (never
              exactly 0, many orders above the pattern's last place) changes it, and so does a store of 0.  The payload is zeroed,
              which is what the kernels' contract asks of the caller.
``"in"``      operands that are only read.  The payload is the data, the bands are NaN (f32 or bf16): a load that strays into a band
              and reaches an accumulator makes the output non-finite.

Each band is at least 256 pixel-rows of the tensor (256 x C elements) and at least 4 KiB, rounded up to 256 bytes, so the payload
keeps the buffer's 16-byte alignment (asserted).  ``arm()`` takes the copy the later comparisons are made against."""
import torch

CL = torch.channels_last
BF = torch.bfloat16
PATTERN = {"out": {4: bytes.fromhex("addec07f"), 2: bytes.fromhex("c07f")},        # little-endian 0x7fc0dead / 0x7fc0
           "atomic": {4: bytes.fromhex("a5a5a535")},                                # 0x35A5A5A5
           "in": {4: bytes.fromhex("0000c07f"), 2: bytes.fromhex("c07f")}}          # quiet NaN


def _mem(t):
    """The tensor in its memory order: NHWC for a 4-D (channels_last) tensor, itself otherwise."""
    if t.dim() == 4:
        assert t.is_contiguous(memory_format=CL), (t.shape, t.stride())
        return t.permute(0, 2, 3, 1)
    assert t.is_contiguous(), (t.shape, t.stride())
    return t


def fill_pattern(t):
    """The "out" pattern over an ordinary tensor (any strides)."""
    if t.element_size() == 4:
        t.view(torch.int32).fill_(0x7fc0dead)
    else:
        t.view(torch.int16).fill_(0x7fc0)
    return t


def is_pattern(t):
    """Elementwise: does the element still hold the "out" pattern, bit for bit."""
    return (t.view(torch.int32) == 0x7fc0dead) if t.element_size() == 4 else (t.view(torch.int16) == 0x7fc0)


class Band:
    def __init__(self, t, kind, keep=False):
        """``t``: a device tensor that gives shape, dtype, layout and -- for "in", or with ``keep`` -- the payload's values."""
        mem = _mem(t)
        esz = t.element_size()
        self.kind = kind
        self.row_bytes = (mem.shape[-1] if mem.dim() > 1 else 16) * esz       # one pixel-row: C elements (flat tensors: a 16-element row)
        self.band = -(-max(256 * self.row_bytes, 4096) // 256) * 256
        self.n = mem.numel() * esz
        assert self.band >= 4096 and self.band >= 256 * self.row_bytes and self.band % 256 == 0
        pat = PATTERN[kind][esz]
        total = 2 * self.band + self.n
        assert self.n % esz == 0 and self.band % esz == 0
        self.buf = torch.tensor(list(pat), dtype=torch.uint8).repeat(total // esz).to(t.device)
        assert self.buf.numel() == total
        payload = self.buf[self.band:self.band + self.n].view(t.dtype).view(mem.shape)
        if kind == "in" or keep:
            payload.copy_(mem)
        elif kind == "atomic":
            payload.zero_()
        self.view = payload.permute(0, 3, 1, 2) if t.dim() == 4 else payload
        assert self.view.shape == t.shape and self.view.data_ptr() % 16 == 0
        assert all(a == b for a, b, n in zip(self.view.stride(), t.stride(), t.shape) if n > 1)
        assert self.view.data_ptr() == self.buf.data_ptr() + self.band
        self.snap = None

    def arm(self):
        self.snap = self.buf.clone()
        return self

    def changed(self, shrink_rows=0):
        """Does either band differ from the copy ``arm`` took?  ``shrink_rows``: as if the payload ended that many pixel-rows early,
        so that its last legitimate rows count as band (the sensitivity check: the comparison must then report a violation)."""
        end = self.band + self.n - shrink_rows * self.row_bytes
        return not (torch.equal(self.buf[:self.band], self.snap[:self.band]) and torch.equal(self.buf[end:], self.snap[end:]))

    def intact(self):
        """Bands and payload bit-identical to the armed copy (operands that are only read)."""
        return torch.equal(self.buf, self.snap)


class Placer:
    """Hands a case its operands: ordinary tensors (``banded=False``) or banded ones.  ``poison``: "x" / "w" puts NaN into the last
    pixel-row of the activation operand that the geometry reads / the last output-channel row of the weights (read-side check)."""

    def __init__(self, banded, poison=None):
        self.banded, self.poison = banded, poison
        self.ins, self.outs = {}, {}

    def _name(self, d, name):
        k, i = name, 1
        while k in d:
            i += 1
            k = "%s#%d" % (name, i)
        return k

    def inp(self, name, t):
        if t is None or not self.banded:
            return t
        b = Band(t, "in").arm()
        self.ins[self._name(self.ins, name)] = b
        return b.view

    def act(self, name, t, last=None, key="x"):
        """An activation operand: ``last`` = (iy, ix) of the last pixel the geometry reads (default: the tensor's last pixel);
        ``key``: the poison that selects it ("w" for the gy of a weight gradient, which has no weight operand)."""
        if self.poison == key:
            t = t.clone()
            iy, ix = last if last is not None else (t.shape[2] - 1, t.shape[3] - 1)
            t[-1, :, iy, ix] = float("nan")
        return self.inp(name, t)

    def weight(self, w, out_axis=0):
        """The parameter (never banded itself: the launchers read derived forms of it, which are)."""
        if self.poison == "w":
            w = w.clone()
            w.select(out_axis, w.shape[out_axis] - 1).fill_(float("nan"))
        return w

    def out(self, name, t, keep=False, kind="out"):
        """An output of ``t``'s shape / dtype / layout: pattern-filled ("out") or zeroed ("atomic"), or (``keep``) holding ``t``'s
        values -- accumulation into an existing tensor."""
        if not self.banded:
            y = t.clone()
            if not keep:
                fill_pattern(y) if kind == "out" else y.zero_()
            return y
        b = Band(t, kind, keep).arm()
        self.outs[self._name(self.outs, name)] = b
        return b.view
