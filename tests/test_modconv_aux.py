"""The bounds of tests/modconv_aux_ref.py discriminate, and the argument checks of csrc/modconv_aux.hip (no GPU).

Discrimination: for every bound an evaluation in the kernel's own operation order with the library's accumulator types stays within it
against the long-double reference; with f32 accumulators (ideas_pixel_dot) or f32 algebra (ideas_demod_bwd) -- the forms the file's
header rules out -- the same evaluation exceeds it at least 100 times.  So tests/test_modconv_aux_gpu.py, which asserts the same bounds
on the kernels, fails if they ever stop working in double.

Argument errors: every check of the entry points comes before any launch, so the library answers here with dummy non-null pointers,
as tests/test_op_dtypes.py relies on."""
import ctypes
import os

import numpy as np
import pytest
import torch

import modconv_aux_ref as R

F32, F64 = np.float32, np.float64
E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = -1, -2, -3, -4


def _wide():
    if not R.WIDE:
        pytest.skip("numpy.longdouble is no wider than float64 here: a float64 evaluation cannot be judged against it")


def _ratio(got, ref, bound):
    """max over elements of |got - ref| / bound (bound > 0 everywhere)."""
    err = np.abs(R.ld(got) - R.ld(ref))
    assert np.all(np.asarray(bound) > 0)
    return float(np.max(err / bound))


# ---------------------------------------------------------------------------------------------------------------- pixel_dot
def _positive(rng, shape):
    return (0.5 + rng.random(shape)).astype(F32)


def test_pixel_dot_f64_order_within_bound():
    _wide()
    rng = np.random.default_rng(1)
    for B, P, C, pos in [(1, 16384, 8, True), (2, 70, 16, False), (3, 130, 24, False), (2, 33, 7, False), (2, 3, 1028, False)]:
        a, g = (_positive(rng, (B, P, C)), _positive(rng, (B, P, C))) if pos else (rng.standard_normal((B, P, C)).astype(F32),
                                                                                 rng.standard_normal((B, P, C)).astype(F32))
        ref, absum = R.pixel_dot_ref(a, g)
        out = R.pixel_dot_eval(a, g, F64)
        assert _ratio(out, ref, R.pixel_dot_bound(P, absum)) < 1, (B, P, C)
        out0 = rng.standard_normal((B, C))
        ref, absum = R.pixel_dot_ref(a, g, out0)
        assert _ratio(R.pixel_dot_eval(a, g, F64, out0), ref, R.pixel_dot_bound(P, absum)) < 1, (B, P, C, "out0")


def test_pixel_dot_f32_accumulators_exceed_bound_100x():
    rng = np.random.default_rng(2)
    B, P, C = 1, 16384, 8
    a, g = _positive(rng, (B, P, C)), _positive(rng, (B, P, C))
    ref, absum = R.pixel_dot_ref(a, g)
    r = _ratio(R.pixel_dot_eval(a, g, F32), ref, R.pixel_dot_bound(P, absum))
    print("pixel_dot f32 accumulators: error / bound =", r)
    assert r > 100, r


# ---------------------------------------------------------------------------------------------------------------- act_bwd_dot
def _act_data(rng, B, P, C, exact):
    gy = rng.standard_normal((B, P, C)).astype(F32)
    if exact:
        out, bias = R.exact_grid(rng, (B, P, C)), R.exact_grid(rng, (C,))
    else:
        out, bias = rng.standard_normal((B, P, C)).astype(F32), (0.3 * rng.standard_normal(C)).astype(F32)
    out[0, 0, 0], out[0, 0, 1] = 0.0, -0.0
    return gy, out, bias


def test_gpre_is_bitwise_the_torch_f32_expression_and_bf16_rounding_is_torchs():
    rng = np.random.default_rng(3)
    gy, out, _ = _act_data(rng, 2, 37, 12, False)
    gs = (0.5 + rng.random((2, 12))).astype(F32)
    for kw in (R.EXACT, R.REALISTIC):
        gp, stored = R.gpre_f32(gy, out, gpre_scale=gs, **kw)
        tgy, tout = torch.from_numpy(gy), torch.from_numpy(out)
        t = torch.where(tout > 0, tgy, tgy * kw["alpha"]) * kw["act_gain"]
        assert np.array_equal(t.numpy().view(np.uint32), gp.view(np.uint32))
        ts = t * torch.from_numpy(gs)[:, None, :]
        assert np.array_equal(ts.numpy().view(np.uint32), stored.view(np.uint32))
        assert np.array_equal(ts.to(torch.bfloat16).float().numpy().view(np.uint32), R.bf16_round(stored).view(np.uint32))
    assert gp[0, 0, 0] == F32(gy[0, 0, 0] * F32(0.2)) * F32(2 ** 0.5) and gp[0, 0, 1] == F32(gy[0, 0, 1] * F32(0.2)) * F32(2 ** 0.5)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
def test_act_bwd_dot_kernel_order_within_bounds(fused, with_bias):
    _wide()
    rng = np.random.default_rng(4 + fused + 2 * with_bias)
    for B, P, C in [(2, 70, 16), (3, 130, 24), (1, 321, 4)]:
        dot0, bg0 = rng.standard_normal((B, C)), rng.standard_normal(C).astype(F32)
        # exact set: pre is exact whatever is contracted, so dot obeys the pixel_dot bound
        gy, out, bias = _act_data(rng, B, P, C, True)
        bias = bias if with_bias else None
        ref = R.act_bwd_dot_ref(gy, out, bias, dot0=dot0, bg0=bg0, **R.EXACT)
        _, dot, bg = R.act_bwd_dot_eval(gy, out, bias, fused=fused, dot0=dot0, bg0=bg0, **R.EXACT)
        assert _ratio(dot, ref["dot"], R.act_dot_exact_bound(P, ref["dot_abs"])) < 1
        assert _ratio(bg, ref["bg"], R.bias_grad_bound(B, P, ref["bg_abs"])) < 1
        # realistic set
        gy, out, bias = _act_data(rng, B, P, C, False)
        bias = bias if with_bias else None
        ref = R.act_bwd_dot_ref(gy, out, bias, **R.REALISTIC)
        _, dot, bg = R.act_bwd_dot_eval(gy, out, bias, fused=fused, **R.REALISTIC)
        assert _ratio(dot, ref["dot"], R.act_dot_realistic_bound(ref["dot_scale"])) < 1
        assert _ratio(bg, ref["bg"], R.bias_grad_bound(B, P, ref["bg_abs"])) < 1


def test_chunking_rule():
    # (B, P) -> (pixels per block, blocks): the cases tests/test_modconv_aux_gpu.py names after their block counts
    assert R.chunking(2, 70) == (35, 2) and R.chunking(1, 321) == (54, 6) and R.chunking(2049, 3) == (3, 1)
    assert R.chunking(1, 64) == (64, 1) and R.chunking(1, 65) == (33, 2) and R.chunking(1, 16384) == (64, 256)


# ---------------------------------------------------------------------------------------------------------------- demodulation
@pytest.mark.parametrize("case", R.CANCEL_CASES)
def test_demod_bwd_f64_within_f32_exceeds_on_cancellation(case):
    """What the double contract bounds is the ALGEBRA: gs before its one rounding to f32 (gs_algebra_bound, relative to T) and the
    double gq the kernel leaves in dot_d (gq_bound without the float copy).  An f32 evaluation errs by 1e-7 .. 6e-7 of T and of |gq|
    and exceeds both at least 100 times in every case.  The stored f32 gs adds 2^-24 |gs| to its bound, and the GPU sees only that
    one: against it the f32 algebra stands out by as much as the two terms cancel, |gs| / T -- a million times at Cin = 1, where
    the cancellation is complete, a hundred at Cin = 2, still above 1 where |gs| ~ T (printed).  The double gq is bounded without
    any f32 term, so the GPU test's check of dot_d fails an f32 evaluation by ~1e7 at every size."""
    B, Cin, Cout = case
    c = R.cancel_case(B, Cin, Cout)
    gs_ref, gq_ref, T = R.demod_bwd_ref(**c)
    if Cin == 1:          # complete cancellation: what is left of gs is the rounding of d32 (2^-24 relative) and eps
        assert float(np.max(np.abs(gs_ref) / T)) < 2.0 ** -22
    gs32, gq32 = R.demod_bwd_eval(dt=F32, **c)
    r32 = _ratio(gs32, gs_ref, R.gs_algebra_bound(Cin, Cout, T))
    r32_stored = _ratio(gs32, gs_ref, R.gs_bound(Cin, Cout, gs_ref, T))
    rq32 = _ratio(gq32, gq_ref, R.gq_bound(Cin, gq_ref, False))
    print(case, "f32 algebra: error / bound gs (algebra), gs (stored), gq64 =", r32, r32_stored, rq32)
    assert r32 > 100 and rq32 > 100 and r32_stored > 1, (r32, rq32, r32_stored)
    if Cin == 1:
        assert r32_stored > 100, r32_stored
    _wide()
    gs64, gq64 = R.demod_bwd_eval(dt=F64, **c)
    ra = _ratio(gs64, gs_ref, R.gs_algebra_bound(Cin, Cout, T))
    r64 = _ratio(gs64.astype(F32), gs_ref, R.gs_bound(Cin, Cout, gs_ref, T))
    rq = _ratio(gq64, gq_ref, R.gq_bound(Cin, gq_ref, False))
    rqf = _ratio(gq64.astype(F32), gq_ref, R.gq_bound(Cin, gq_ref, True))
    print(case, "f64 algebra: error / bound gs (algebra), gs (stored), gq64, gq32 =", ra, r64, rq, rqf)
    assert ra < 1 and r64 < 1 and rq < 1 and rqf < 1, (ra, r64, rq, rqf)


def test_demod_bwd_without_demodulation_is_the_direct_term():
    _wide()
    c = R.cancel_case(3, 65, 5)
    c["s"][1, 3] = 0
    gs_ref, gq_ref, T = R.demod_bwd_ref(c["dot_s"], None, None, c["s"], None, c["eps"])
    gs, gq = R.demod_bwd_eval(c["dot_s"], None, None, c["s"], None, c["eps"])
    assert gq is None and gq_ref is None and gs_ref[1, 3] == 0 and gs[1, 3] == 0
    assert float(np.max(np.abs(R.ld(gs.astype(F32)) - gs_ref) - R.gs_bound(65, 5, gs_ref, T))) <= 0


@pytest.mark.parametrize("Cin", [1, 2, 4, 63, 64, 65, 130])
def test_f32_demodulation_kernels_in_kernel_order_within_bounds(Cin):
    rng = np.random.default_rng(Cin)
    for Cout, B, (KH, KW) in [(1, 1, (3, 3)), (3, 3, (1, 1)), (5, 3, (1, 3)), (40, 1, (3, 3))]:
        w = rng.standard_normal((Cout, Cin, KH, KW)).astype(F32)
        scale2 = 1.0 / (Cin * KH * KW)
        ref = R.weight_sqsum_ref(w, F32(scale2))
        assert _ratio(R.weight_sqsum_eval(w, scale2, F32), ref, R.weight_sqsum_bound(KH, KW, ref, False)) < 1
        if R.WIDE:
            ref64 = R.weight_sqsum_ref(w, scale2)
            assert _ratio(R.weight_sqsum_eval(w, scale2, F64), ref64, R.weight_sqsum_bound(KH, KW, ref64, True)) < 1
        s = (1 + 0.5 * rng.standard_normal((B, Cin))).astype(F32)
        s[0, 0] = 0
        wsq = R.weight_sqsum_eval(w, scale2, F32)
        dref = R.demod_ref(s, wsq, 1e-8)
        assert _ratio(R.demod_eval(s, wsq, 1e-8), dref, R.demod_bound(Cin, dref)) < 1
        gq, gw0 = rng.standard_normal((B, Cout)).astype(F32), rng.standard_normal(w.shape).astype(F32)
        coef = 2 * scale2
        gref, gscale = R.demod_wgrad_ref(gw0, w, gq, s, coef)
        err = np.abs(R.ld(R.demod_wgrad_eval(gw0, w, gq, s, coef)) - gref)
        assert np.all(err <= R.demod_wgrad_bound(B, gscale, gref))


# ---------------------------------------------------------------------------------------------------------------- argument errors
@pytest.fixture(scope="module")
def lib():
    from ideas_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build libideas_hip.so first (__graft_entry__.build())"
    return _lib.load()


OK16, OFF4 = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4)      # never dereferenced: every call below fails a check first


def test_pixel_dot_argument_errors(lib):
    from ideas_amd import _lib
    f = lib.ideas_pixel_dot
    assert f(OK16, OK16, OK16, 1, 4, 6148, _lib.F32, None) == E_SHAPE          # C > 6144
    assert f(OK16, OK16, OK16, 65536, 4, 8, _lib.F32, None) == E_SHAPE         # B > 65535 (grid.y)
    assert f(OK16, OK16, OK16, 1, 0, 8, _lib.F32, None) == E_SHAPE
    for C in (3, 6, 7):
        assert f(OK16, OK16, OK16, 1, 4, C, _lib.BF16, None) == E_ALIGN        # bf16 has no element-wise path
    assert f(OK16, OFF4, OK16, 1, 4, 8, _lib.F32, None) == E_ALIGN             # float4 reads of a
    assert f(OK16, OK16, OFF4, 1, 4, 8, _lib.BF16, None) == E_ALIGN
    assert f(OK16, OK16, OK16, 1, 4, 8, _lib.F16, None) == E_UNSUPPORTED
    assert f(OK16, OK16, OK16, 1, 4, 8, _lib.F64, None) == E_UNSUPPORTED
    assert f(None, OK16, OK16, 1, 4, 8, _lib.F32, None) == E_NULL


def test_act_bwd_dot_argument_errors(lib):
    from ideas_amd import _lib
    f = lib.ideas_act_bwd_dot
    p = OK16

    def call(gpre=p, bg=p, dot=p, gy=p, out=p, bias=p, gscale=None, B=1, P=4, C=8, dtype=_lib.F32):
        return f(gpre, bg, dot, gy, out, bias, gscale, B, P, C, 0.2, 1.5, dtype, None)
    assert call(C=3076) == E_SHAPE                  # C > 3072
    assert call(B=65536) == E_SHAPE
    assert call(C=6) == E_ALIGN
    assert call(dot=None) == E_NULL
    assert call(dtype=_lib.F16) == E_UNSUPPORTED
    assert call(bias=OFF4) == E_ALIGN
    for dt in (_lib.F32, _lib.BF16):
        assert call(gscale=OFF4, dtype=dt) == E_ALIGN          # read as float4, like bias
        assert call(gscale=OFF4, bias=None, dtype=dt) == E_ALIGN


def test_demod_bwd_argument_errors(lib):
    f = lib.ideas_demod_bwd
    p = OK16

    def call(gs=p, gq=p, dot_s=p, dot_d=p, d=p, s=p, wsq=p, B=1, Cin=4, Cout=4):
        return f(gs, gq, dot_s, dot_d, d, s, wsq, B, Cin, Cout, 1e-8, None)
    assert call(gq=None) == E_NULL and call(dot_d=None) == E_NULL and call(wsq=None) == E_NULL
    assert call(gs=None) == E_NULL and call(dot_s=None) == E_NULL and call(s=None) == E_NULL
    assert call(B=65536) == E_SHAPE and call(Cin=0) == E_SHAPE
