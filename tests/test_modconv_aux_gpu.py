"""The reductions of csrc/modconv_aux.hip against their long-double restatements (tests/modconv_aux_ref.py), through the C ABI, to
the DERIVED bounds of that file -- tests/test_modconv_aux.py shows without a GPU that an evaluation with f32 accumulators or f32
algebra exceeds them a hundredfold -- and the ``needs_input_grad`` subsets of the modulated-conv Functions through the modules.

Every kernel path of the file is reached: the C4 <= 256 / C4 > 256 forms, 256 % C4 != 0, the element path, one and several blocks
per sample, P below / at / across a block edge, B > 2048, the documented channel limits, accumulation into non-zero outputs,
``gpre_scale``, both weight memory orders and offset views, d == NULL.  Each test prints the largest error / bound ratio it saw.

Largest error / bound on an MI355X (the module prints them at the end; the whole file runs in under 3 s):
    pixel_dot 0.36, act_bwd_dot dot 0.25 (exact set) / 0.55 (realistic set), bias_grad 0.61, demod 0.19, weight_sqsum 0.96,
    weight_sqsum_f64 0.63, demod_wgrad 0.999, demod_bwd gq in double 0.12, gq as float 0.97, gs 0.99 (0.95 on the cancellation cases).
Those near 1 are the outputs whose bound IS one rounding of the result to f32, 2^-24 |ref|: half an ulp reaches that when |ref| sits
just above a power of two, and among ~10^5 elements some do (gs, gq as float, demod_wgrad, whose other term is ~1e-2 of it); the
double gq, which has no such term, uses at most 12 % of its bound.  weight_sqsum at 1x1 has exactly the two roundings it is
charged, weight_sqsum_f64 at 1x3 three of four; bias_grad at one block two of three.  The realistic dot reaches 0.55 on columns of
two or three pixels that are all negative, where five roundings meet the 4 charged and no positive element brings slack."""
import itertools
import math

import numpy as np
import pytest
import torch

import oracle.torch_ref as O
from conftest import rel_err
import modconv_aux_ref as R

pytestmark = pytest.mark.gpu
CL = torch.channels_last
BF = torch.bfloat16
F32, F64 = np.float32, np.float64
GTOL = 1e-4             # gradient tolerance of tests/test_ops_gpu.py::test_modconv_golden
RATIO = {}              # kernel output -> the largest error / bound seen in this module
SENTINEL, GUARD = 12345.0, 64


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nlargest error / bound per output:", {k: float("%.3g" % v) for k, v in sorted(RATIO.items())})


@pytest.fixture(scope="module")
def L():
    from ideas_amd import _lib
    _lib.load()
    return _lib


def _within(name, got, ref, bound):
    err = np.abs(R.ld(got) - R.ld(ref))
    bound = np.broadcast_to(np.asarray(bound), err.shape)
    assert np.all(np.isfinite(np.asarray(got, F64))), name
    ratio = float(np.max(np.where(err == 0, 0, err / np.where(bound > 0, bound, 1e-300))))
    RATIO[name] = max(RATIO.get(name, 0.0), ratio)
    assert ratio < 1, (name, ratio)
    return ratio


def _dev(a, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(BF) if bf16 else t          # (exact: bf16 operands are rounded on the host first)


class _Guarded:
    """A device tensor between two sentinel bands (GUARD elements: a multiple of 16 bytes in every dtype used, so the view keeps the
    alignment of the allocation); ``intact()``: nothing outside the view was written."""

    def __init__(self, shape, dtype, init=None):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(shape)
        if init is None:
            self.t.zero_()
        else:
            self.t.copy_(init)

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())

    def np(self):
        t = self.t.detach()
        return (t.float() if t.dtype == BF else t).cpu().numpy().copy()


# ---------------------------------------------------------------------------------------------------------------- pixel_dot
PD_CASES = [(2, 70, 16),        # two blocks of 35 pixels per sample: 64 pixel rows per pass, the second pass ragged
            (3, 130, 24),       # 256 % C4 != 0: 42 pixel rows x 6 quads = 252 threads work, 4 idle
            (1, 5, 1020),       # C4 = 255
            (1, 5, 1024),       # C4 = 256: one pixel row per pass
            (2, 3, 1028),       # C4 = 257: the loop path with a one-element second trip
            (1, 2, 6144),       # the channel limit (48 KiB of LDS accumulators)
            (1, 1, 8), (1, 64, 8), (1, 65, 8),          # P = 1; one full block; one pixel across the block edge
            (1, 321, 4),        # six blocks
            (2049, 3, 4)]       # B > 2048: one block per sample
PD_ELEMENT = [(2, 130, 3), (2, 33, 7)]          # C % 4 != 0: the f32 element path
PD_PARAMS = [(c, d) for c in PD_CASES for d in ("f32", "bf16")] + [(c, "f32") for c in PD_ELEMENT]


def _pixel_dot_case(L, B, P, C, bf16, positive, seed):
    rng = np.random.default_rng(seed)

    def draw():
        v = (0.5 + rng.random((B, P, C))) if positive else rng.standard_normal((B, P, C))
        return R.bf16_round(v.astype(F32)) if bf16 else v.astype(F32)
    out = _Guarded((B, C), torch.float64)
    prev = None
    for call in range(2):             # the second call adds into the non-zero result of the first
        a, g = draw(), draw()
        da, dg = _dev(a, bf16), _dev(g, bf16)
        L.check(L.load().ideas_pixel_dot(L.ptr(out.t), L.ptr(da), L.ptr(dg), B, P, C, L.BF16 if bf16 else L.F32, L.stream_ptr()), "ideas_pixel_dot")
        torch.cuda.synchronize()
        got = out.np()
        ref, absum = R.pixel_dot_ref(a, g, prev)
        r = _within("pixel_dot", got, ref, R.pixel_dot_bound(P, absum))
        print("pixel_dot", (B, P, C), "bf16" if bf16 else "f32", "call", call, "error / bound", r)
        prev = got
    assert out.intact()


@pytest.mark.parametrize("case,dtype", PD_PARAMS)
def test_pixel_dot(L, case, dtype):
    B, P, C = case
    per, chunks = R.chunking(B, P)
    assert (case != (2, 70, 16) or (per, chunks) == (35, 2)) and (case != (1, 321, 4) or chunks == 6) and (B <= 2048 or chunks == 1)
    _pixel_dot_case(L, B, P, C, dtype == "bf16", False, 100 + B + P + C)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_pixel_dot_long_positive_sum(L, dtype):
    """P = 16384 positive terms, C = 8: 256 blocks of 64 pixels.  f32 accumulators miss this bound by more than 1e4
    (tests/test_modconv_aux.py::test_pixel_dot_f32_accumulators_exceed_bound_100x)."""
    _pixel_dot_case(L, 1, 16384, 8, dtype == "bf16", True, 7)


# ---------------------------------------------------------------------------------------------------------------- act_bwd_dot
ACT_CASES = [c for c in PD_CASES if c[2] <= 3072] + [(1, 2, 3072)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("case", ACT_CASES)
def test_act_bwd_dot(L, case, exact, dtype):
    B, P, C = case
    bf16 = dtype == "bf16"
    rng = np.random.default_rng(200 + B + P + C + exact)
    kw = R.EXACT if exact else R.REALISTIC
    rnd = (lambda v: R.bf16_round(v)) if bf16 else (lambda v: v)
    gy = rnd(rng.standard_normal((B, P, C)).astype(F32))
    if exact:
        out, bias = rnd(R.exact_grid(rng, (B, P, C))), R.exact_grid(rng, (C,))
    else:
        out, bias = rnd(rng.standard_normal((B, P, C)).astype(F32)), (0.3 * rng.standard_normal(C)).astype(F32)
    out.reshape(-1)[0], out.reshape(-1)[1] = 0.0, -0.0            # both take the alpha branch (out > 0 is false)
    if P * B > 2:
        out[B - 1, P - 1, C - 1] = 0.0
    gscale = (0.5 + rng.random((B, C))).astype(F32)
    dgy, dout, dbias, dgscale = _dev(gy, bf16), _dev(out, bf16), _dev(bias), _dev(gscale)
    tgy, tout = torch.from_numpy(gy), torch.from_numpy(out)
    for with_bias, with_scale in itertools.product((False, True), (False, True)):
        bg0 = rng.standard_normal(C).astype(F32)                  # the wrapper sums into the parameter's .grad
        dot0 = rng.standard_normal((B, C)) if exact else None     # (the realistic bound has no term for a previous value)
        gpre = _Guarded((B, P, C), BF if bf16 else torch.float32)
        bg = _Guarded((C,), torch.float32, _dev(bg0))
        dot = _Guarded((B, C), torch.float64, None if dot0 is None else _dev(dot0))
        rc = L.load().ideas_act_bwd_dot(L.ptr(gpre.t), L.ptr(bg.t), L.ptr(dot.t), L.ptr(dgy), L.ptr(dout), L.ptr(dbias) if with_bias else None,
                                        L.ptr(dgscale) if with_scale else None, B, P, C, kw["alpha"], kw["act_gain"],
                                        L.BF16 if bf16 else L.F32, L.stream_ptr())
        L.check(rc, "ideas_act_bwd_dot")
        torch.cuda.synchronize()
        assert gpre.intact() and bg.intact() and dot.intact()
        # gpre: two or three f32 multiplications, bitwise torch's; bf16: that value rounded once to nearest-even
        exp = torch.where(tout > 0, tgy, tgy * kw["alpha"]) * kw["act_gain"]
        if with_scale:
            exp = exp * torch.from_numpy(gscale)[:, None, :]
        got = gpre.t.cpu()
        if bf16:
            assert torch.equal(got.view(torch.int16), exp.to(BF).view(torch.int16)), (case, with_bias, with_scale)
        else:
            assert torch.equal(got.view(torch.int32), exp.view(torch.int32)), (case, with_bias, with_scale)
        r = R.act_bwd_dot_ref(gy, out, bias if with_bias else None, dot0=dot0, bg0=bg0, **kw)
        if exact:
            rd = _within("act_bwd_dot.dot (exact set)", dot.np(), r["dot"], R.act_dot_exact_bound(P, r["dot_abs"]))
        else:
            rd = _within("act_bwd_dot.dot (realistic set)", dot.np(), r["dot"], R.act_dot_realistic_bound(r["dot_scale"]))
        rb = _within("act_bwd_dot.bias_grad", bg.np(), r["bg"], R.bias_grad_bound(B, P, r["bg_abs"]))
        print("act_bwd_dot", case, dtype, "exact" if exact else "realistic", with_bias, with_scale, "error / bound dot, bias_grad", rd, rb)


# ---------------------------------------------------------------------------------------------------------------- demodulation
def _weight_forms(w):
    """The same [Cout,Cin,KH,KW] values: dense, (o, ky, kx, i) and (i, ky, kx, o) memory orders, and a dense view at a storage offset
    of one element (4-byte aligned only)."""
    t = torch.from_numpy(w).cuda()
    flat = torch.empty(t.numel() + 1, device="cuda")
    off = flat[1:].view(t.shape)
    off.copy_(t)
    forms = {"dense": t.contiguous(), "o_kk_i": t.contiguous(memory_format=CL),
             "i_kk_o": t.transpose(0, 1).contiguous(memory_format=CL).transpose(0, 1), "offset": off}
    assert forms["offset"].storage_offset() == 1 and (min(t.shape) == 1 or forms["i_kk_o"].stride(0) < forms["i_kk_o"].stride(1))
    assert all(torch.equal(f, t) for f in forms.values())
    return forms


def _demod_bwd(L, c, with_d=True):
    """One ideas_demod_bwd call on the operands of ``c`` -> (gs f32, gq f32, dot_d on return) as numpy."""
    B, Cin = c["s"].shape
    Cout = c["wsq"].shape[0]
    gs = _Guarded((B, Cin), torch.float32)
    gq = _Guarded((B, Cout), torch.float32)
    dd = _Guarded((B, Cout), torch.float64, _dev(c["dot_d"]))
    ds, s, d32, wsq = _dev(c["dot_s"]), _dev(c["s"]), _dev(c["d32"]), _dev(c["wsq"])
    if with_d:
        rc = L.load().ideas_demod_bwd(L.ptr(gs.t), L.ptr(gq.t), L.ptr(ds), L.ptr(dd.t), L.ptr(d32), L.ptr(s), L.ptr(wsq), B, Cin, Cout,
                                      c["eps"], L.stream_ptr())
    else:
        rc = L.load().ideas_demod_bwd(L.ptr(gs.t), None, L.ptr(ds), None, None, L.ptr(s), None, B, Cin, Cout, c["eps"], L.stream_ptr())
    L.check(rc, "ideas_demod_bwd")
    torch.cuda.synchronize()
    assert gs.intact() and gq.intact() and dd.intact()
    return gs.np(), gq.np(), dd.np()


def _check_demod_bwd(L, c, tag):
    B, Cin = c["s"].shape
    Cout = c["wsq"].shape[0]
    gs_ref, gq_ref, T = R.demod_bwd_ref(**c)
    gs, gq, gq64 = _demod_bwd(L, c)
    r1 = _within("demod_bwd.gs" + tag, gs, gs_ref, R.gs_bound(Cin, Cout, gs_ref, T))
    r2 = _within("demod_bwd.gq (float)", gq, gq_ref, R.gq_bound(Cin, gq_ref, True))
    r3 = _within("demod_bwd.gq (double, in dot_d)", gq64, gq_ref, R.gq_bound(Cin, gq_ref, False))
    assert np.array_equal(gq64.astype(F32), gq)                   # dot_d on return IS gq in double
    gs_b, gq_b, gq64_b = _demod_bwd(L, c)                         # no atomics: two runs agree bitwise
    assert np.array_equal(gs.view(np.uint32), gs_b.view(np.uint32)) and np.array_equal(gq.view(np.uint32), gq_b.view(np.uint32))
    assert np.array_equal(gq64.view(np.uint64), gq64_b.view(np.uint64))
    return r1, r2, r3


@pytest.mark.parametrize("case", R.CANCEL_CASES)
def test_demod_bwd_cancellation(L, case):
    """The operands a real demodulated layer produces: the two terms of gs cancel (completely at Cin = 1, where |gs| ~ 1e-7 T)."""
    B, Cin, Cout = case
    print("demod_bwd cancellation", case, "error / bound gs, gq, gq64", _check_demod_bwd(L, R.cancel_case(B, Cin, Cout), " (cancellation)"))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Cout", [1, 3, 5, 40])
@pytest.mark.parametrize("Cin", [1, 2, 4, 63, 64, 65, 130])
def test_demodulation_kernels(L, Cin, Cout, B):
    rng = np.random.default_rng(300 + 7 * Cin + 3 * Cout + B)
    lib = L.load()
    s = (1 + 0.5 * rng.standard_normal((B, Cin))).astype(F32)
    s[B - 1, Cin // 2] = 0.0                                       # one style exactly 0
    ds = _dev(s)
    wsq_np = {}
    for KH, KW in ((3, 3), (1, 1), (1, 3)):
        w = rng.standard_normal((Cout, Cin, KH, KW)).astype(F32)
        scale = 1.0 / math.sqrt(Cin * KH * KW)
        scale2_32, scale2_64 = float(F32(scale * scale)), scale * scale
        gq = rng.standard_normal((B, Cout)).astype(F32)
        dgq = _dev(gq)
        ref32, ref64 = R.weight_sqsum_ref(w, F32(scale2_32)), R.weight_sqsum_ref(w, scale2_64)
        for name, wt in _weight_forms(w).items():
            o32, o64 = _Guarded((Cout, Cin), torch.float32), _Guarded((Cout, Cin), torch.float64)
            L.check(lib.ideas_weight_sqsum(L.ptr(o32.t), L.ptr(wt), Cout, Cin, KH, KW, *wt.stride(), scale2_32, L.stream_ptr()), "ideas_weight_sqsum")
            L.check(lib.ideas_weight_sqsum_f64(L.ptr(o64.t), L.ptr(wt), Cout, Cin, KH, KW, *wt.stride(), scale2_64, L.stream_ptr()),
                    "ideas_weight_sqsum_f64")
            # gw in ANOTHER memory order than w: (o, ky, kx, i) unless w has it, then dense
            gw0 = rng.standard_normal(w.shape).astype(F32)
            gw = torch.from_numpy(gw0).cuda()
            gw = gw.contiguous() if name == "o_kk_i" else gw.contiguous(memory_format=CL)
            coef = float(F32(2.0 * scale * scale))
            L.check(lib.ideas_demod_wgrad(L.ptr(gw), L.ptr(wt), L.ptr(dgq), L.ptr(ds), B, Cout, Cin, KH, KW, *wt.stride(), *gw.stride(), coef,
                                          L.stream_ptr()), "ideas_demod_wgrad")
            torch.cuda.synchronize()
            assert o32.intact() and o64.intact()
            _within("weight_sqsum", o32.np(), ref32, R.weight_sqsum_bound(KH, KW, ref32, False))
            _within("weight_sqsum_f64", o64.np(), ref64, R.weight_sqsum_bound(KH, KW, ref64, True))
            gref, gscale = R.demod_wgrad_ref(gw0, w, gq, s, coef)
            _within("demod_wgrad", gw.cpu().numpy(), gref, R.demod_wgrad_bound(B, gscale, gref))
            wsq_np[(KH, KW)] = (o32.np(), o64.np())
    # ideas_demod on the f32 table, ideas_demod_bwd on the double one (3x3 weight), random uncorrelated dots
    wsq32, wsq64 = wsq_np[(3, 3)]
    d = _Guarded((B, Cout), torch.float32)
    L.check(lib.ideas_demod(L.ptr(d.t), L.ptr(ds), L.ptr(_dev(wsq32)), B, Cin, Cout, 1e-8, L.stream_ptr()), "ideas_demod")
    torch.cuda.synchronize()
    assert d.intact()
    dref = R.demod_ref(s, wsq32, 1e-8)
    _within("demod", d.np(), dref, R.demod_bound(Cin, dref))
    c = dict(dot_s=rng.standard_normal((B, Cin)), dot_d=rng.standard_normal((B, Cout)), d32=d.np(), s=s, wsq=wsq64, eps=1e-8)
    _check_demod_bwd(L, c, "")
    # d == NULL: the direct term only (0 where s == 0), nothing else touched
    gs, gq_untouched, dd_untouched = _demod_bwd(L, c, with_d=False)
    ref0, _, T0 = R.demod_bwd_ref(c["dot_s"], None, None, s, None, 1e-8)
    _within("demod_bwd.gs (d == NULL)", gs, ref0, R.gs_bound(Cin, Cout, ref0, T0))
    assert gs[B - 1, Cin // 2] == 0 and not gq_untouched.any() and np.array_equal(dd_untouched, c["dot_d"])


# ---------------------------------------------------------------------------------------------------------------- subsets
STYLE_DIM = 24
LAYERS = {      # name -> (Cin, Cout, k, upsample, demodulate, styled)
    "same_demod": (16, 32, 3, False, True, False),
    "same_plain": (32, 16, 3, False, False, False),
    "up_demod": (32, 16, 3, True, True, False),
    "up_plain": (16, 32, 3, True, False, False),
    "to_rgb": (16, 3, 1, False, False, False),
    "styled": (16, 32, 3, False, True, True),
}
# what requires grad; "bias" = the activation bias where the layer has one, else the modulation's (a style gradient without an input one)
SUBSETS = [("x",), ("style",), ("weight",), ("x", "style"), ("weight", "bias")]


def _build(name):
    from ideas_amd.model import ModulatedConv2d, StyledConv_without_noise
    ci, co, k, up, demod, styled = LAYERS[name]
    torch.manual_seed(sum(map(ord, name)))
    if styled:
        layer = StyledConv_without_noise(ci, co, k, STYLE_DIM, demodulate=demod)
        layer.activate.bias.data.normal_(0, 0.3)
        conv = layer.conv
    else:
        layer = conv = ModulatedConv2d(ci, co, k, STYLE_DIM, demodulate=demod, upsample=up)
    x = torch.randn(2, ci, 8, 8, dtype=torch.float64)
    st = torch.randn(2, STYLE_DIM, dtype=torch.float64)
    # f64 reference gradients of everything, once
    x64, st64 = x.clone().requires_grad_(True), st.clone().requires_grad_(True)
    P = [p.detach().double().requires_grad_(True) for p in (conv.weight, conv.modulation.weight, conv.modulation.bias)]
    y = O.modulated_conv2d(x64, st64, *P, demodulate=demod, upsample=up)
    names = ["x", "style", "weight", "mod_weight", "mod_bias"]
    if styled:
        P.append(layer.activate.bias.detach().double().requires_grad_(True))
        y = O.fused_leaky_relu(y, P[-1])
        names.append("act_bias")
    gy = torch.randn_like(y)
    ref = dict(zip(names, torch.autograd.grad(y, [x64, st64] + P, gy)))
    return layer.cuda(), conv, x, st, gy, ref


@pytest.fixture(scope="module")
def layers():
    return {n: _build(n) for n in LAYERS}


def _run(layer, conv, x, st, gy, want):
    """Forward + backward with exactly the tensors named in ``want`` requiring grad.  -> {name: gradient}, all tensors by name."""
    styled = conv is not layer
    t = {"x": x.float().cuda().contiguous(memory_format=CL), "style": st.float().cuda(), "weight": conv.weight,
         "mod_weight": conv.modulation.weight, "mod_bias": conv.modulation.bias}
    if styled:
        t["act_bias"] = layer.activate.bias
    for n, v in t.items():
        v.requires_grad_(n in want)
    y = layer(t["x"], t["style"])
    grads = torch.autograd.grad(y, [t[n] for n in want], gy.float().cuda().contiguous(memory_format=CL), retain_graph=True)
    return dict(zip(want, grads)), t, y


@pytest.mark.parametrize("arena", [False, True])
@pytest.mark.parametrize("name", sorted(LAYERS))
def test_needs_input_grad_subsets(layers, name, arena):
    """Every gradient of a subset run equals the f64 reference at GTOL and the all-inputs run within 1e-6 (gx and the style gradient
    bitwise: the same reproducible kernels run in both), and a tensor that did not require grad has no gradient.  ``arena``: with
    the scratch arena on, where ideas_demod_bwd overwrites dot_d in place on an arena view."""
    from ideas_amd.op import scratch
    layer, conv, x, st, gy, ref = layers[name]
    styled = conv is not layer
    everything = list(ref)
    if arena:
        scratch.begin(torch.device("cuda", torch.cuda.current_device()))
    try:
        full, _, _ = _run(layer, conv, x, st, gy, everything)
        for n in everything:
            assert rel_err(full[n], ref[n]) < GTOL, (name, "all", n, rel_err(full[n], ref[n]))
        for sub in SUBSETS:
            want = [("act_bias" if styled else "mod_bias") if n == "bias" else n for n in sub]
            got, t, y = _run(layer, conv, x, st, gy, want)
            for n in want:
                e64, efull = rel_err(got[n], ref[n]), rel_err(got[n], full[n])
                assert e64 < GTOL and efull < 1e-6, (name, sub, n, e64, efull)
                if n in ("x", "style"):
                    assert torch.equal(got[n], full[n]), (name, sub, n, efull)
            frozen = [n for n in everything if n not in want]
            assert not any(t[n].requires_grad for n in frozen)
            with pytest.raises(RuntimeError):
                torch.autograd.grad(y, [t[frozen[0]]], gy.float().cuda().contiguous(memory_format=CL))
    finally:
        if arena:
            scratch.end()
        for p in layer.parameters():
            p.requires_grad_(True)
