"""The 16-byte stores of conv_b3_tphase_kernel's epilogue (csrc/conv_b3_tphase.hip) against its one-dword stores.

Per phase a wave passes its 64 positions x 32 channels through LDS so that a lane holds four consecutive channels of one
output pixel; gain and out_scale are applied before, with the same roundings in the same order, so the output must be
BITWISE that of the old epilogue.  IDEAS_B3_TPHASE_STORE=0 (read per call) keeps the old epilogue; the new one needs
Cout % 4 == 0 and a 16-byte aligned output.  IDEAS_B3_TPHASE=1 makes the plain launches take the kernel as well."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
CL = torch.channels_last
GAIN = 0.05


def _store16(y_ptr, cout):
    """1 when the kernel writing ``cout`` channels at ``y_ptr`` takes the 16-byte stores under the present environment."""
    from ideas_amd import _lib
    fn = _lib.load().ideas_b3_tphase_store16
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    return int(fn(y_ptr, cout))


def _inputs(B, cin, cout, h, w, mod, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, h, w, generator=g).cuda().contiguous(memory_format=CL)
    wt = torch.randn(cin, cout, 3, 3, generator=g).cuda().contiguous(memory_format=CL)
    lin = (torch.rand(B, cin, generator=g) + 0.5).cuda() if mod else None
    lout = (torch.rand(B, cout, generator=g) + 0.5).cuda() if mod else None
    return x, wt, lin, lout


def _launch_into(y, x, wt, lin, lout):
    """The four phases of the transposed conv written into ``y`` (logical [B, Cout, 2H+1, 2W+1], NHWC memory at any address):
    what op/conv.py::launch_multi does, with the output tensor given."""
    import ideas_amd.op.conv as CV
    from ideas_amd import _lib
    from ideas_amd.op.conv_plan import ConvGeom, plan_dgrad
    launches, need_zero = plan_dgrad(x.shape, wt, ConvGeom(3, 3, 2, 0, False), (y.shape[2], y.shape[3]))
    assert len(launches) == 4 and not need_zero
    launches = sorted(launches, key=lambda L: -(L.TY * L.TX * L.OH * L.OW))
    ps = (_lib.ConvParams * 4)(*[CV._params(L, GAIN) for L in launches])
    planes = [CV.b3_planes(L) for L in launches]
    ws = (C.c_void_p * 4)(*[_lib.ptr(pl) for pl in planes])
    rc = _lib.load().ideas_conv_igemm_multi(4, _lib.ptr(y), _lib.ptr(x), ws, _lib.ptr(lin), _lib.ptr(lout), ps, _lib.F32_B3,
                                            _lib.stream_ptr())
    _lib.check(rc, "ideas_conv_igemm_multi")
    torch.cuda.synchronize()


def _both(B, cin, cout, h, w, mod, monkeypatch):
    import ideas_amd.op.conv as CV
    from ideas_amd.op.conv_plan import ConvGeom
    x, wt, lin, lout = _inputs(B, cin, cout, h, w, mod, seed=B + cin + cout + h * w + mod)
    monkeypatch.setenv("IDEAS_B3_TPHASE", "1")
    out = {}
    for flag in ("0", None):
        if flag is None:
            monkeypatch.delenv("IDEAS_B3_TPHASE_STORE", raising=False)
        else:
            monkeypatch.setenv("IDEAS_B3_TPHASE_STORE", flag)
        y = CV.conv_dgrad_raw(x, wt, ConvGeom(3, 3, 2, 0, False), (2 * h + 1, 2 * w + 1), GAIN, lin=lin, lout=lout)
        torch.cuda.synchronize()
        out[flag] = (y, _store16(y.data_ptr(), cout))
    return out


# exact patch and one chunk; ragged rows and columns with a half-empty second N tile; several patches and three chunks
@pytest.mark.parametrize("shape", [(2, 16, 128, 4, 16), (2, 32, 192, 5, 18), (1, 48, 128, 8, 32)])
@pytest.mark.parametrize("mod", [False, True])
def test_store16_is_bitwise_the_one_dword_epilogue(shape, mod, monkeypatch):
    B, cin, cout, h, w = shape
    out = _both(B, cin, cout, h, w, mod, monkeypatch)
    (old, old16), (new, new16) = out["0"], out[None]
    assert old16 == 0 and new16 == 1                       # the default takes the new epilogue here, the switch the old one
    assert torch.isfinite(new).all() and float(new.abs().max()) > 0
    assert torch.equal(old, new), float((old - new).abs().max())


@pytest.mark.parametrize("mod", [False, True])
def test_cout_not_a_multiple_of_four_keeps_the_old_epilogue(mod, monkeypatch):
    """Cout = 130: the geometry is the kernel's (Cout > 64), a channel quad would straddle pixels: one-dword stores either way."""
    out = _both(2, 16, 130, 4, 16, mod, monkeypatch)
    (old, old16), (new, new16) = out["0"], out[None]
    assert old16 == 0 and new16 == 0
    assert torch.equal(old, new)


@pytest.mark.parametrize("offset", [8, 5])
def test_store16_into_a_view_leaves_the_guard_bands_alone(offset, monkeypatch):
    """The output is a window of a sentinel-filled buffer: at a 16-byte aligned offset (8 floats) the new epilogue runs, at an
    unaligned one (5 floats) the dispatch keeps the old one; either way exactly the window is written, with the values of a
    fresh output tensor.  Ragged patches and a half-empty second N tile, modulated."""
    B, cin, cout, h, w = 2, 32, 192, 5, 18
    x, wt, lin, lout = _inputs(B, cin, cout, h, w, True, seed=99)
    monkeypatch.setenv("IDEAS_B3_TPHASE", "1")
    monkeypatch.setenv("IDEAS_B3_TPHASE_STORE", "0")
    ref = torch.empty((B, cout, 2 * h + 1, 2 * w + 1), device="cuda", memory_format=CL)
    _launch_into(ref, x, wt, lin, lout)
    monkeypatch.delenv("IDEAS_B3_TPHASE_STORE", raising=False)
    n, guard, sentinel = ref.numel(), 4096, -12345.0
    buf = torch.full((guard + n + guard,), sentinel, device="cuda")
    assert buf.data_ptr() % 16 == 0
    y = buf[offset:offset + n].view(B, 2 * h + 1, 2 * w + 1, cout).permute(0, 3, 1, 2)
    assert _store16(y.data_ptr(), cout) == (1 if offset % 4 == 0 else 0)
    _launch_into(y, x, wt, lin, lout)
    assert torch.equal(y, ref)
    assert bool((buf[:offset] == sentinel).all()) and bool((buf[offset + n:] == sentinel).all())
