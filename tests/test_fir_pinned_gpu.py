"""Outputs of the FIR kernels (csrc/upfirdn2d.hip) pinned to what the library gave BEFORE its kernels were rebuilt from shared
pieces (one tap staging, one factorisation, one tile decode, one masked row loader, one fused stage; one body per scheme).

The rebuild alters no value: every scheme keeps its arithmetic and its order.  tests/golden/fir_pinned.npz
(tests/golden/make_golden_fir_pinned.py, run on the parent commit's library, which also checks every output against the f64
oracle) holds, per output tensor of every case below, its shape, the SHA-256 of its bytes and its first 16 values (one row of four packed
arrays each); the inputs are
re-made here from seeds on the CPU.  B = 2 and a few tens of pixels everywhere.  The geometries:
  unit blur   (9, 20) pad (1, 1) -> 8 x 19: an odd out_w, so the last column pair has one column;
              (33, 31) pad (2, 2) -> 34 x 32: three row segments of 16, 16 and 2 rows;
              (33, 31) pad (2, 1) -> 33 x 31: both, and a lone last row behind the two-rows-per-trip loop;
  down = 2    (10, 6) pad (0, 3) -> 5 x 3 and (33, 31) pad (2, 2) -> 17 x 16 (three segments of 8 rows);
  up = 2      (5, 7) pad (3, 2) -> 12 x 16, (9, 9) pad (1, 1) -> 17 x 17 (odd pad0, odd outputs: a half 2 x 2 block at both
              ends) and (6, 5) pad (2, 1) -> 12 x 10 (even pad0, the model's own).
Channels choose the kernel: f32 C % 4 == 0, bf16 / f16 C % 8 == 0 (8 channels per thread), bf16 C % 8 == 4 (4 per thread).  A
random 4 x 4 FIR has rank > 1 and takes the direct loops of the separable kernels.  The fused stages (ideas_blur_fused) pin y
only: bias_grad is summed with f32 atomics in varying order, and is compared with the f64 sum of y instead."""
import hashlib
import importlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CL = torch.channels_last
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fir_pinned.npz")
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f64": torch.float64}
TOL = {"f32": 2e-6, "bf16": 6e-3, "f16": 6e-3, "f64": 1e-12}       # against the f64 oracle (tests/test_ops_gpu.py's, f64: its own rounding)
ALPHA, SCALE = 0.2, 2 ** 0.5


def _U():
    return importlib.import_module("ideas_amd.op.upfirdn2d")       # (ideas_amd.op.upfirdn2d the attribute is the function)


class _Rng:
    """CPU generator (the same stream on every machine); tensors go to the device afterwards."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def n(self, *s):
        return torch.randn(*s, generator=self.g)


def _fir(r, random_fir):
    from ideas_amd.model import make_kernel
    return r.n(4, 4) if random_fir else make_kernel((1, 3, 3, 1))


def _x(r, dt, shape, cl=True):
    """(device tensor in the storage dtype, the same values in f64 on the CPU)"""
    x = r.n(*shape).to(DT[dt])
    return (x.cuda().contiguous(memory_format=CL) if cl else x.cuda().contiguous()), x.double()


def _lrelu(v, sel):
    return torch.where(sel > 0, v, v * ALPHA) * SCALE


def _fir_case(seed, dt, C, hw, pad, up, down, random_fir, resid=False, cl=True, fir_hw=None):
    """upfirdn2d_raw (fir_up2_add_raw with `resid`) -> ([y], [f64 oracle])"""
    import oracle.torch_ref as O
    U, r = _U(), _Rng(seed)
    fir = _fir(r, random_fir) if fir_hw is None else r.n(*fir_hw)
    x, x64 = _x(r, dt, (2, C) + hw, cl)
    pad4, out_hw, _ = U._geometry(hw, fir, up, down, pad)
    ref = O.upfirdn2d(x64, fir.double(), up, down, pad)
    if resid:
        rs, rs64 = _x(r, dt, (2, C) + out_hw)
        return [U.fir_up2_add_raw(x, fir.cuda(), pad4, out_hw, True, rs)], [ref + rs64]
    return [U.upfirdn2d_raw(x, fir.cuda(), (up, up), (down, down), pad4, out_hw, flip=True)], [ref]


def _fused_case(seed, dt, C, hw, pad):
    """ideas_blur_fused, both modes, in the geometry of a layer: blur + bias + leaky ReLU from hw, and the blur's adjoint + leaky-ReLU
    backward back to hw -> ([y_fwd, y_bwd, bias_grad], [f64 oracles, bias_grad's being the f64 sum of y_bwd itself])"""
    import oracle.torch_ref as O
    U, r = _U(), _Rng(seed)
    fir = _fir(r, False)
    x, x64 = _x(r, dt, (2, C) + hw)
    bias = r.n(C)
    pad4, out_hw, g_pad = U.blur_geometry(hw, fir, pad)
    g, g64 = _x(r, dt, (2, C) + out_hw)
    y1, y164 = _x(r, dt, (2, C) + hw)
    cv = C // 8 if (dt != "f32" and C % 8 == 0) else C // 4
    cols = hw[1] if (dt == "bf16" and C % 8) else (hw[1] + 1) // 2
    assert (2 * ((hw[0] + 15) // 16) * cols * cv) % 256 != 0            # threads past the end run the ACT_BWD stage masked off
    fd = fir.cuda()
    y_fwd = U.blur_fused_raw(x, fd, pad4, out_hw, True, U.BLUR_BIAS_ACT, bias=bias.cuda(), alpha=ALPHA, scale=SCALE)
    bg = torch.full((C,), 3.0, device="cuda")
    y_bwd = U.blur_fused_raw(g, fd, g_pad, hw, False, U.BLUR_ACT_BWD, ref=y1, bias_grad=bg, alpha=ALPHA, scale=SCALE)
    v = O.upfirdn2d(x64, fir.double(), 1, 1, pad) + bias.double().view(1, -1, 1, 1)
    assert g_pad[0] == g_pad[2] and g_pad[1] == g_pad[3]
    w = O.upfirdn2d(g64, torch.flip(fir.double(), [0, 1]), 1, 1, (g_pad[0], g_pad[1]))
    return [y_fwd, y_bwd, bg - 3.0], [_lrelu(v, v), _lrelu(w, y164), y_bwd.double().sum((0, 2, 3)).cpu()]


BLUR_GEOMS = (((9, 20), (1, 1)), ((33, 31), (2, 2)), ((33, 31), (2, 1)))
DOWN_GEOMS = (((10, 6), (0, 3)), ((33, 31), (2, 2)))
UP_GEOMS = (((5, 7), (3, 2)), ((9, 9), (1, 1)), ((6, 5), (2, 1)))
CASES = {}        # name -> thunk returning (outputs, f64 oracles)
_seed = 100
for _gi, (_hw, _pad) in enumerate(BLUR_GEOMS):
    for _dt, _c, _rnd in (("f32", 8, 0), ("bf16", 16, 0), ("f16", 16, 0), ("bf16", 12, 0), ("f32", 8, 1), ("bf16", 16, 1), ("bf16", 12, 1)):
        _seed += 1
        CASES["blur%d_%s_c%d%s" % (_gi, _dt, _c, "_rnd" if _rnd else "")] = (
            lambda s=_seed, d=_dt, c=_c, h=_hw, p=_pad, q=_rnd: _fir_case(s, d, c, h, p, 1, 1, bool(q)))
for _gi, (_hw, _pad) in ((0, BLUR_GEOMS[0]), (2, BLUR_GEOMS[2])):
    for _dt, _c in (("f32", 8), ("bf16", 16), ("bf16", 12)):
        _seed += 1
        CASES["fused%d_%s_c%d" % (_gi, _dt, _c)] = lambda s=_seed, d=_dt, c=_c, h=_hw, p=_pad: _fused_case(s, d, c, h, p)
for _kind, _geoms, _ud in (("down", DOWN_GEOMS, (1, 2)), ("up", UP_GEOMS, (2, 1))):
    for _gi, (_hw, _pad) in enumerate(_geoms):
        for _dt, _c, _rnd in (("f32", 4, 0), ("bf16", 12, 0), ("bf16", 16, 0), ("f16", 16, 0), ("bf16", 16, 1)):
            _seed += 1
            CASES["%s%d_%s_c%d%s" % (_kind, _gi, _dt, _c, "_rnd" if _rnd else "")] = (
                lambda s=_seed, d=_dt, c=_c, h=_hw, p=_pad, u=_ud, q=_rnd: _fir_case(s, d, c, h, p, u[0], u[1], bool(q)))
for _dt, _c in (("f32", 4), ("bf16", 16), ("bf16", 12)):
    _seed += 1
    CASES["up1_resid_%s_c%d" % (_dt, _c)] = lambda s=_seed, d=_dt, c=_c: _fir_case(s, d, c, (9, 9), (1, 1), 2, 1, False, resid=True)
# the two kernels left as they were: the NCHW tile kernel (2 x 2 tiles of 16 x 64) and the generic one (f64, 3 x 5 FIR, up 2, down 3)
CASES["nchw_f32"] = lambda: _fir_case(901, "f32", 3, (18, 66), (2, 1), 1, 1, False, cl=False)
CASES["generic_f64"] = lambda: _fir_case(902, "f64", 3, (7, 9), (3, 2), 2, 3, False, cl=False, fir_hw=(3, 5))
FUSED = [k for k in CASES if k.startswith("fused")]


def _host(t):
    """the tensor in its memory order (NHWC for channels-last), on the CPU"""
    t = t.detach()
    return (t.permute(0, 2, 3, 1) if t.dim() == 4 and t.is_contiguous(memory_format=CL) else t).contiguous().cpu()


def run_case(name):
    """([(shape, sha256 hex, first 16 values as float64)] of the case's outputs, the outputs, their f64 oracles)"""
    outs, refs = CASES[name]()
    torch.cuda.synchronize()
    res = []
    for t in outs:
        h = _host(t)
        assert bool(torch.isfinite(h).all()), name
        raw = h.view(torch.int16 if h.element_size() == 2 else torch.int32 if h.element_size() == 4 else torch.int64).numpy()
        res.append((tuple(h.shape), hashlib.sha256(raw.tobytes()).hexdigest(), h.double().reshape(-1)[:16].numpy().copy()))
    return res, outs, refs


def pinned(name, res):
    """the outputs that are pinned: all but the atomically summed bias gradient"""
    return res[:2] if name in FUSED else res


def bias_grad_tol(name):
    return 2e-3 if "bf16" in name else 1e-5          # test_blur_fused_stages_equal_the_two_kernel_chain's


@pytest.fixture(scope="module")
def golden():
    """{"case/i": (shape, sha256 hex, head)} from the packed arrays of the file (one row per pinned tensor)"""
    z = np.load(GOLDEN)
    return {str(k): (tuple(int(v) for v in s), bytes(h).hex(), f) for k, s, h, f in zip(z["keys"], z["shape"], z["sha256"], z["head"])}


@pytest.mark.parametrize("name", sorted(CASES))
def test_fir_outputs_are_bitwise_the_pinned_ones(name, golden):
    from conftest import rel_err
    res, outs, refs = run_case(name)
    got = pinned(name, res)
    assert sorted(k for k in golden if k.rsplit("/", 1)[0] == name) == ["%s/%d" % (name, i) for i in range(len(got))]
    for i, (shape, sha, head) in enumerate(got):
        k = "%s/%d" % (name, i)
        g_shape, g_sha, g_head = golden[k]
        assert g_shape == shape, k
        assert np.array_equal(g_head, head), (k, g_head, head)
        assert g_sha == sha, k
    if name in FUSED:
        err = rel_err(outs[2], refs[2])
        print(name, "bias_grad against the f64 sum of y: %.3g" % err)
        assert err < bias_grad_tol(name), err
