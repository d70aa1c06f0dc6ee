"""Outputs of the streaming kernels pinned to what the library gave BEFORE they were moved onto csrc/stream.hpp (the shared
channel-vector I/O, fixed-order sums, width / lane-group rules and (dtype, width) dispatch) and before reflect_fold_kernel was
rewritten on it.

The move alters no value.  tests/golden/stream_pinned.npz (tests/golden/make_golden_stream_pinned.py, run on the parent commit's
library) holds, per output tensor of every case below, its shape, the SHA-256 of its bytes and its first 16 values; the inputs
are re-made here from seeds on the CPU.  Every entry point of noise_act, lpips (2x2 max pool and head), pool, augment,
minibatch_stddev and pad runs through the C ABI on raw channels-innermost buffers, in f32 and bf16, on the 16-byte vector path and
on the element path (a channel count that is no multiple of the vector, or a buffer that starts one element behind a 16-byte
boundary), at the smallest shapes that reach every branch.

Left out of the hashes, because the sources document them as summed by floating-point atomics in no fixed order:
  * gbias of ideas_noise_bias_act_bwd (the kernel still receives the buffer, so the branch runs); bounded against f64 by
    tests/test_stylegan2_gen_gpu.py::test_op_f32_vs_f64_restatement;
  * gx of ideas_affine_warp_bwd for a general theta; bounded by tests/test_non_leaking_gpu.py::test_affine_warp_general_f32 and
    ::test_affine_warp_backward_under_atomic_load.  It IS pinned for a whole-pixel shift, where every input pixel receives at
    most one non-zero contribution and the order cannot matter."""
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F32 = torch.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "stream_pinned.npz")
DT = {"f32": F32, "bf16": BF}


class _Rng:
    """CPU generator (the same stream on every machine); tensors go to the device afterwards."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def n(self, *s):
        return torch.randn(*s, generator=self.g)

    def u(self, *s):
        return torch.rand(*s, generator=self.g)


def _dev(t, dtype=F32, off=0):
    """``t`` on the device as ``dtype``, its first element ``off`` elements behind the (256-byte aligned) start of its buffer."""
    buf = torch.empty(t.numel() + off, device="cuda", dtype=dtype)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (off * v.element_size()) % 16
    return v


def _out(shape, dtype=F32, off=0):
    return _dev(torch.zeros(shape), dtype, off)


def _call(name, *args):
    from ideas_amd import _lib
    _lib.check(getattr(_lib.load(), name)(*[_lib.ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args], _lib.stream_ptr()),
               name)


def _enum(dtype):
    from ideas_amd import _lib
    return _lib.BF16 if dtype == BF else _lib.F32


def _noise_act(seed, dtype, shape, nb, off=0):
    """forward -> out; backward on that out -> gx, gnw, gnoise ([nb, P]: nb = 1 sums the per-sample rows over b)."""
    from ideas_amd import _lib
    B, C, H, W = shape
    r, P = _Rng(seed), H * W
    x, gy = _dev(r.n(B, P, C), dtype, off), _dev(r.n(B, P, C), dtype, off)
    noise, nw, bias = _dev(r.n(nb, P)), _dev(r.n(1)), _dev(r.n(C) * 0.3)
    out, gx = _out((B, P, C), dtype, off), _out((B, P, C), dtype, off)
    _call("ideas_noise_bias_act", out, x, noise, nw, bias, B, C, H, W, nb, 0.2, 2 ** 0.5, _enum(dtype))
    gbias, gnw, gnoise = _out((C,)), _out((1,)), _out((nb, P))
    ws = torch.empty(_lib.NOISE_ACT_MAX_PARTIALS + (B * P + 1) // 2, device="cuda", dtype=torch.float64)
    _call("ideas_noise_bias_act_bwd", gx, gbias, gnw, gnoise, ws, gy, out, noise, nw, B, C, H, W, nb, 0.2, 2 ** 0.5, _enum(dtype))
    return [out, gx, gnw, gnoise]


def _lpips_head(seed, dtype, shape, off=0):
    from ideas_amd import _lib
    B, C, H, W = shape
    r = _Rng(seed)
    f0, f1 = _dev(r.n(B, H, W, C), dtype, off), _dev(r.n(B, H, W, C), dtype, off)
    w, gd = _dev(r.u(C)), _dev(r.n(B))
    d, g0, g1 = _out((B,)), _out((B, H, W, C), dtype, off), _out((B, H, W, C), dtype, off)
    ws = torch.empty(B * _lib.LPIPS_MAX_PARTIALS, device="cuda", dtype=torch.float64)
    _call("ideas_lpips_layer_fwd", d, ws, f0, f1, w, B, C, H, W, _enum(dtype))
    _call("ideas_lpips_layer_bwd", g0, g1, gd, f0, f1, w, B, C, H, W, _enum(dtype))
    return [d, g0, g1]


def _maxpool(seed, dtype, shape, off=0):
    B, C, H, W = shape
    r = _Rng(seed)
    x, gy = _dev(r.n(B, H, W, C), dtype, off), _dev(r.n(B, H // 2, W // 2, C), dtype, off)
    y, gx = _out((B, H // 2, W // 2, C), dtype, off), _out((B, H, W, C), dtype, off)
    _call("ideas_maxpool2x2_fwd", y, x, B, C, H, W, _enum(dtype))
    _call("ideas_maxpool2x2_bwd", gx, gy, x, B, C, H, W, _enum(dtype))
    return [y, gx]


def _pool3(seed, dtype, shape, off=0):
    """the three 3x3 windows and the global average of one input"""
    from ideas_amd import _lib
    B, C, H, W = shape
    x = _dev(_Rng(seed).n(B, H, W, C), dtype, off)
    outs = []
    for mode in (_lib.POOL_MAX_S2, _lib.POOL_MAX_S1P1, _lib.POOL_AVG_S1P1_VALID):
        oh, ow = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if mode == _lib.POOL_MAX_S2 else (H, W)
        y = _out((B, oh, ow, C), dtype, off)
        _call("ideas_pool3x3_fwd", y, x, B, C, H, W, mode, _enum(dtype))
        outs.append(y)
    g = _out((B, C), F32, off)
    _call("ideas_global_avg_pool", g, x, B, C, H, W, _enum(dtype))
    return outs + [g]


def _warp(seed, dtype, C, nhwc, off=0):
    """affine warp 6 x 7 -> 5 x 9 with a general theta (one sample's rows reach outside the image), and the adjoint of a
    whole-pixel shift (weights 1 and 0: no two contributions meet in one input pixel)"""
    from ideas_amd import _lib
    B, H, W, OH, OW = 2, 6, 7, 5, 9
    r = _Rng(seed)
    layout = _lib.NHWC if nhwc else _lib.NCHW
    x = _dev(r.n(B, H, W, C) if nhwc else r.n(B, C, H, W), dtype, off)
    gy = _dev(r.n(B, OH, OW, C) if nhwc else r.n(B, C, OH, OW), dtype, off)
    theta = _dev(torch.tensor([[0.9, 0.2, 0.5, -0.15, 1.1, -0.7], [1.05, -0.3, 1.25, 0.25, 0.8, 2.5]]))
    shift = _dev(torch.tensor([[1.0, 0.0, -1.0, 0.0, 1.0, 1.0], [1.0, 0.0, 2.0, 0.0, 1.0, -2.0]]))
    y, gx = _out(gy.shape, dtype, off), _out(x.shape, F32)
    _call("ideas_affine_warp", y, x, theta, B, C, H, W, OH, OW, layout, _enum(dtype))
    _call("ideas_affine_warp_bwd", gx, gy, shift, B, C, H, W, OH, OW, 1, layout, _enum(dtype))
    return [y, gx]


def _color(seed, dtype, nhwc):
    from ideas_amd import _lib
    B, H, W = 2, 5, 7
    r = _Rng(seed)
    x, m = _dev(r.n(B, H, W, 3) if nhwc else r.n(B, 3, H, W), dtype), _dev(r.n(B, 12))
    y = _out(x.shape, dtype)
    _call("ideas_color_affine", y, x, m, B, H, W, _lib.NHWC if nhwc else _lib.NCHW, _enum(dtype))
    return [y]


def _mbstd(seed, dtype, shape, group, feat):
    """forward -> out; backward -> gx, a; backward of the backward -> dgout, dx"""
    from ideas_amd import _lib
    B, C, H, W = shape
    r, m = _Rng(seed), B // min(B, group)
    x, gout, ggx = _dev(r.n(B, H, W, C), dtype), _dev(r.n(B, H, W, C + feat), dtype), _dev(r.n(B, H, W, C), dtype)
    out, gx, a = _out((B, H, W, C + feat), dtype), _out((B, H, W, C), dtype), _out((m * feat,))
    dgout, dx = _out((B, H, W, C + feat), dtype), _out((B, H, W, C), dtype)
    ws = torch.empty(m * feat * _lib.MBSTD_MAX_PARTIALS, device="cuda", dtype=torch.float64)
    _call("ideas_mbstd_fwd", out, ws, x, B, C, H, W, group, feat, 1e-8, _enum(dtype))
    _call("ideas_mbstd_bwd", gx, a, gout, x, B, C, H, W, group, feat, 1e-8, _enum(dtype))
    _call("ideas_mbstd_bwd2", dgout, dx, ws, ggx, x, a, B, C, H, W, group, feat, 1e-8, _enum(dtype))
    return [out, gx, a, dgout, dx]


def _fold(seed, dtype, shape, pad):
    B, C, H, W = shape
    gp = _dev(_Rng(seed).n(B, H + 2 * pad, W + 2 * pad, C), dtype)
    gx = _out((B, H, W, C), dtype)
    _call("ideas_reflect_fold", gx, gp, B, H, W, C, pad, _enum(dtype))
    return [gx]


def _cases():
    c = {}
    for dn, dt in DT.items():
        # noise_act: C = 132 -> f32 33 vectors (G = 64), bf16 132 elements (> 64 a pixel); C = 16 -> G = 4 / 2; off: G = 16 elements
        for C in (132, 16):
            for nb in (1, 2):
                c["noise_act_%s_c%d_nb%d" % (dn, C, nb)] = lambda dt=dt, C=C, nb=nb: _noise_act(300 + C + nb, dt, (2, C, 5, 7), nb)
        c["noise_act_%s_c16_nb2_unaligned" % dn] = lambda dt=dt: _noise_act(321, dt, (2, 16, 5, 7), 2, off=1)
        for C in (64, 33):
            c["lpips_head_%s_c%d" % (dn, C)] = lambda dt=dt, C=C: _lpips_head(330 + C, dt, (2, C, 5, 7))
        c["lpips_head_%s_c64_unaligned" % dn] = lambda dt=dt: _lpips_head(331, dt, (2, 64, 5, 7), off=1)
        for C in (16, 5):
            c["maxpool2x2_%s_c%d" % (dn, C)] = lambda dt=dt, C=C: _maxpool(340 + C, dt, (2, C, 7, 5))
            c["pool3x3_%s_c%d" % (dn, C)] = lambda dt=dt, C=C: _pool3(350 + C, dt, (2, C, 9, 11))
        c["maxpool2x2_%s_c16_unaligned" % dn] = lambda dt=dt: _maxpool(341, dt, (2, 16, 7, 5), off=1)
        c["pool3x3_%s_c16_unaligned" % dn] = lambda dt=dt: _pool3(351, dt, (2, 16, 9, 11), off=1)
        c["warp_%s_nhwc_c8" % dn] = lambda dt=dt: _warp(360, dt, 8, True)
        c["warp_%s_nhwc_c3" % dn] = lambda dt=dt: _warp(361, dt, 3, True)
        c["warp_%s_nchw_c3" % dn] = lambda dt=dt: _warp(362, dt, 3, False)
        c["warp_%s_nhwc_c8_unaligned" % dn] = lambda dt=dt: _warp(363, dt, 8, True, off=1)
        c["color_%s_nhwc" % dn] = lambda dt=dt: _color(364, dt, True)
        c["color_%s_nchw" % dn] = lambda dt=dt: _color(365, dt, False)
        c["mbstd_%s_g4_f1" % dn] = lambda dt=dt: _mbstd(370, dt, (4, 8, 4, 4), 4, 1)
        c["mbstd_%s_g2_f2" % dn] = lambda dt=dt: _mbstd(371, dt, (4, 8, 4, 4), 2, 2)
        c["mbstd_%s_g8_f1" % dn] = lambda dt=dt: _mbstd(372, dt, (8, 8, 4, 4), 8, 1)       # the 16-slot instantiation
        for i, (shape, pad) in enumerate((((2, 8, 6, 9), 1), ((1, 32, 34, 34), 1), ((2, 4, 5, 4), 2))):
            c["reflect_fold_%s_%d" % (dn, i)] = lambda dt=dt, i=i, shape=shape, pad=pad: _fold(380 + i, dt, shape, pad)
    return c


CASES = _cases()


def run_case(name):
    """[(shape, sha256 hex, first 16 values as float32)] of the case's outputs (bf16 hashed as stored)."""
    outs = CASES[name]()
    torch.cuda.synchronize()
    res = []
    for t in outs:
        t = t.detach().contiguous()
        a = t.float().cpu().numpy()
        assert np.isfinite(a).all() and float(np.abs(a).max()) > 0, name
        raw = (t.view(torch.int16) if t.dtype == BF else t).cpu().numpy()
        res.append((tuple(a.shape), hashlib.sha256(raw.tobytes()).hexdigest(), a.reshape(-1)[:16].astype(np.float32).copy()))
    return res


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", sorted(CASES))
def test_stream_outputs_are_bitwise_the_pinned_ones(name, golden):
    got = run_case(name)
    assert int(golden[name + "/n"]) == len(got)
    for i, (shape, sha, head) in enumerate(got):
        k = "%s/%d" % (name, i)
        assert tuple(golden[k + "/shape"]) == shape, k
        assert np.array_equal(golden[k + "/head"], head), (k, golden[k + "/head"], head)
        assert bytes(golden[k + "/sha256"]).hex() == sha, k
