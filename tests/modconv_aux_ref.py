"""References and error bounds for the reductions of csrc/modconv_aux.hip (no GPU code here).

Every reference is the plain restatement of one operation on the operands the kernel actually reads (f32, or bf16 widened to f32),
evaluated in ``numpy.longdouble`` where that is wider than float64 (x86: 64-bit significand), else in float64.  Each ``*_ref``
returns the value and the absolute-term sum its bound is relative to; each ``*_bound`` is derived, in the comment above it, from the
number formats and the operation count of the kernel -- never from what a kernel returned.  U24 / U53 are the unit roundoffs of
f32 / f64 (half an ulp relative: 2^-24, 2^-53).

The ``*_eval`` functions restate a kernel in ITS operation order with a chosen accumulator type.  tests/test_modconv_aux.py uses them
without a GPU to show that an evaluation in double stays within each bound and that one with f32 accumulators / f32 algebra exceeds
the bounds that guard the file's double-precision contract by two orders of magnitude: the evidence that the GPU tests
(tests/test_modconv_aux_gpu.py) can fail.  numpy has no fused multiply-add, so an fma of the kernel is a rounded product and a rounded
sum here (for f32 operands in double the product is exact, and the two forms coincide); the bounds below count an fma as two roundings
wherever that matters.
"""
import numpy as np

WIDE = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
LD = np.longdouble if WIDE else np.float64
U24, U53 = 2.0 ** -24, 2.0 ** -53
F32, F64 = np.float32, np.float64


def ld(a):
    return np.asarray(a).astype(LD)


def bf16_round(a):
    """f32 -> the nearest bf16 (ties to even), returned widened to f32: what torch's .to(bfloat16) and v_cvt_pk_bf16_f32 do."""
    u = np.ascontiguousarray(a, dtype=F32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(F32).reshape(np.shape(a))


def chunking(B, P):
    """(pixels per block, blocks per sample) of ideas_pixel_dot / ideas_act_bwd_dot:
    chunks = clamp(ceil(2048 / B), 1, ceil(P / 64)); per = ceil(P / chunks); chunks = ceil(P / per)."""
    chunks = max(1, min(-(-2048 // B), -(-P // 64)))
    per = -(-P // chunks)
    return per, -(-P // per)


# ---------------------------------------------------------------------------------------------------------------- pixel_dot
def pixel_dot_ref(a, g, out0=None):
    """out[b,c] = out0[b,c] + sum_p a[b,p,c] g[b,p,c]; a, g [B,P,C] f32.  -> (value, out0| + sum_p |a g|)."""
    prod = ld(a) * ld(g)
    val, absum = prod.sum(1), np.abs(prod).sum(1)
    if out0 is not None:
        val, absum = val + ld(out0), absum + np.abs(ld(out0))
    return val, absum


# The product of two f32 (24-bit significands) has at most 48 bits: exact in double, and fma(a, g, acc) is then one rounded
# addition.  The result is the sum of P exact terms and out0 by SOME tree of rounded additions (a thread's chain, the LDS atomics of
# its block, the global atomics; additions to an exact zero cost nothing): a leaf passes through at most P additions, each of
# relative error <= U53, so |err| <= ((1 + U53)^P - 1) * sum|leaf| <= (P + 2) * U53 * sum|leaf| for P * U53 << 1.
def pixel_dot_bound(P, absum):
    return (P + 2) * U53 * absum


def _rows_sum(prod_terms, per, chunks, C, acc, fma_operands=None):
    """The blocks' partial sums [chunks, B, C] in the kernels' order.  Thread (pr, c4) adds the pixels p0 + pr, p0 + pr + R, ... of
    its block in that order; the threads' partials are then added to the block's LDS accumulator (atomics: any order; here pr
    ascending).  ``prod_terms`` [B,P,C] in double = the exact products; with acc == float32 and fma_operands == (a, g) the chain is
    fmaf(a, g, acc) instead (product and sum rounded once, emulated through double)."""
    B, P, _ = prod_terms.shape
    if C % 4 == 0:
        C4 = C // 4
        R = 256 // C4 if C4 <= 256 else 1
    else:
        R = None
    part = np.zeros((chunks, B, C), acc)
    for k in range(chunks):
        p0, p1 = k * per, min(P, (k + 1) * per)
        if R is None:         # element path: every element is one LDS atomic, in some order; here ascending p
            blk = np.zeros((B, C), acc)
            for p in range(p0, p1):
                blk = (blk + prod_terms[:, p].astype(acc)).astype(acc)
            part[k] = blk
            continue
        rows = []
        for pr in range(min(R, p1 - p0)):
            t = np.zeros((B, C), acc)
            for p in range(p0 + pr, p1, R):
                if fma_operands is not None and acc == F32:
                    a, g = fma_operands
                    t = (a[:, p].astype(F64) * g[:, p].astype(F64) + t.astype(F64)).astype(F32)
                else:
                    t = (t + prod_terms[:, p].astype(acc)).astype(acc)
            rows.append(t)
        blk = np.zeros((B, C), acc)
        for t in rows:
            blk = (blk + t).astype(acc)
        part[k] = blk
    return part


def pixel_dot_eval(a, g, acc=F64, out0=None):
    """ideas_pixel_dot in the kernel's operation order with accumulators of type ``acc`` (the library's: float64)."""
    B, P, C = a.shape
    per, chunks = chunking(B, P)
    prod = a.astype(F64) * g.astype(F64)
    part = _rows_sum(prod, per, chunks, C, acc, (a, g))
    out = np.zeros((B, C), acc) if out0 is None else np.array(out0, acc)
    for k in range(chunks):           # global atomics: any order; here block index ascending
        out = (out + part[k]).astype(acc)
    return out


# ---------------------------------------------------------------------------------------------------------------- act_bwd_dot
def gpre_f32(gy, out, alpha, act_gain, gpre_scale=None):
    """(gpre as the kernel uses it for dot / bias_grad, gpre as it is stored before any narrowing), f32 arithmetic: two or three
    multiplications and no addition, so nothing can be contracted and the result is bitwise torch's
    where(out > 0, gy, gy * alpha) * act_gain [* gpre_scale].  out == 0 and out == -0.0 take the alpha branch."""
    gy, out = np.asarray(gy, F32), np.asarray(out, F32)
    gp = (np.where(out > 0, gy, (gy * F32(alpha)).astype(F32)) * F32(act_gain)).astype(F32)
    stored = gp if gpre_scale is None else (gp * np.asarray(gpre_scale, F32)[:, None, :]).astype(F32)
    return gp, stored


def act_bwd_dot_ref(gy, out, bias, alpha, act_gain, dot0=None, bg0=None):
    """-> dict: dot [B,C] = dot0 + sum_p gpre * pre with pre = inverse_act(out) - bias in exact arithmetic on the f32 operands
    (t = out / act_gain; pre = (t > 0 ? t : t / alpha) - bias), its |.|-sum, the sum the realistic bound is relative to
    (sum_p |gpre| (|t / alpha| + |bias|)), bias_grad [C] = bg0 + sum_{b,p} gpre and its |.|-sum."""
    gp, _ = gpre_f32(gy, out, alpha, act_gain)
    B, P, C = gp.shape
    t = ld(out) / LD(F32(act_gain))
    bv = np.zeros(C, LD) if bias is None else ld(bias)
    pre = np.where(t > 0, t, t / LD(F32(alpha))) - bv
    terms = ld(gp) * pre
    r = {"dot": terms.sum(1), "dot_abs": np.abs(terms).sum(1),
         "dot_scale": (np.abs(ld(gp)) * (np.abs(t / LD(F32(alpha))) + np.abs(bv))).sum(1),
         "bg": ld(gp).sum((0, 1)), "bg_abs": np.abs(ld(gp)).sum((0, 1))}
    if dot0 is not None:
        r["dot"], r["dot_abs"] = r["dot"] + ld(dot0), r["dot_abs"] + np.abs(ld(dot0))
    if bg0 is not None:
        r["bg"], r["bg_abs"] = r["bg"] + ld(bg0), r["bg_abs"] + np.abs(ld(bg0))
    return r


EXACT = dict(alpha=0.25, act_gain=2.0)          # with out / bias on the 2^-8 grid within +-8 (exact_grid)
REALISTIC = dict(alpha=0.2, act_gain=2 ** 0.5)


def exact_grid(rng, shape):
    """Multiples of 2^-8 in [-8, 8] as f32: out * (1/2), * (1/0.25) and - bias are then exact in f32 (at most 8 + 6 fraction/integer
    bits), fused or not, so pre is the exact value and gpre = gy * 0.25 * 2 is exact too."""
    return (rng.integers(-2048, 2049, size=shape) / 256.0).astype(F32)


# Exact data set: pre and gpre are exact f32 values, their product is exact in double, and dot is a pixel_dot of (gpre, pre):
def act_dot_exact_bound(P, dot_abs):
    return pixel_dot_bound(P, dot_abs)


# Realistic data set (alpha = 0.2, gain = sqrt 2; neither reciprocal is a power of two).  With u = U24 the kernel computes
# inv_gain = fl(1 / gain) (u), t = fl(out * inv_gain) (u), inv_alpha = fl(1 / alpha) (u), for t <= 0 fl(t * inv_alpha) (u), and the
# subtraction of the bias, rounded once whether or not the compiler fuses it with that product: u (|x| + |bias|), x = the
# pre-activation.  Per element |pre - exact| <= 3u|t| + u|bias| for out > 0 and 5u|x| + u|bias| for out <= 0 (x = t / alpha), the
# accumulation in double adds (P + 2) U53 of the same sum, and sign(t) == sign(out) because gain > 0.  The bound charges EVERY element
# 4u (|t / alpha| + |bias|) = 2^-22 (...): that is 20u|t| for the positive ones, so a column needs more than 15/16 of its weight on
# negative elements whose five roundings all fall the same way before 5u > the 4u charged could show.
def act_dot_realistic_bound(dot_scale):
    return 2.0 ** -22 * dot_scale


# bias_grad[c]: each of the nblocks = chunks * B blocks adds its partial (accumulated in double: P * U53, far below one f32 rounding)
# rounded ONCE to f32, by an f32 atomic, into the running value that started as the caller's bias_grad: one rounding per partial
# (together at most u * sum|gpre|) and one per atomic (each at most u * (|bg0| + sum|gpre|)), so (nblocks + 1) u; + 1 covers the
# double accumulation.  nblocks follows the entry point's rule, restated in chunking():
#   chunks = clamp(ceil(2048 / B), 1, ceil(P / 64)); per = ceil(P / chunks); chunks = ceil(P / per).
def bias_grad_bound(B, P, bg_abs):
    return (chunking(B, P)[1] * B + 2) * U24 * bg_abs


def act_bwd_dot_eval(gy, out, bias, alpha, act_gain, fused, dot0=None, bg0=None):
    """ideas_act_bwd_dot in the kernel's order: f32 steps for gpre and pre (``fused``: the compiler contracts t * inv_alpha - bias
    into one fma), double block accumulators, one f32 rounding per block partial of bias_grad and f32 atomics."""
    gp, _ = gpre_f32(gy, out, alpha, act_gain)
    B, P, C = gp.shape
    inv_gain, inv_alpha = F32(1.0) / F32(act_gain), F32(1.0) / F32(alpha)
    bv = np.zeros(C, F32) if bias is None else np.asarray(bias, F32)
    t = (np.asarray(out, F32) * inv_gain).astype(F32)
    if fused:
        neg = (t.astype(F64) * F64(inv_alpha) - bv.astype(F64)).astype(F32)
    else:
        neg = ((t * inv_alpha).astype(F32) - bv).astype(F32)
    pre = np.where(t > 0, (t - bv).astype(F32), neg)
    per, chunks = chunking(B, P)
    pd = _rows_sum(gp.astype(F64) * pre.astype(F64), per, chunks, C, F64)
    pb = _rows_sum(gp.astype(F64), per, chunks, C, F64)
    dot = np.zeros((B, C), F64) if dot0 is None else np.array(dot0, F64)
    bg = np.zeros(C, F32) if bg0 is None else np.array(bg0, F32)
    for k in range(chunks):
        dot = dot + pd[k]
        for b in range(B):
            bg = (bg + pb[k, b].astype(F32)).astype(F32)
    return gp, dot, bg


# ---------------------------------------------------------------------------------------------------------------- demodulation
def weight_sqsum_ref(w, scale2):
    """wsq[o,i] = scale2 * sum_k W[o,i,k]^2 of an f32 [Cout,Cin,KH,KW] weight (all terms positive: the value is its own |.|-sum)."""
    return LD(scale2) * (ld(w) ** 2).sum((2, 3))


# f32: KH*KW accumulations fmaf(v, v, acc) (hipcc contracts v * v + acc) and the multiplication by scale2, one rounding each, all
# terms positive.  f64: v * v is exact, KH*KW rounded additions and the multiplication.
def weight_sqsum_bound(KH, KW, ref, f64):
    return (KH * KW + 1) * (U53 if f64 else U24) * np.abs(ref)


def weight_sqsum_eval(w, scale2, acc):
    w = np.asarray(w, F32)
    out = np.zeros(w.shape[:2], acc)
    for ky in range(w.shape[2]):
        for kx in range(w.shape[3]):
            v = w[:, :, ky, kx].astype(F64)
            out = (v * v + out.astype(F64)).astype(acc)
    return (out * acc(scale2)).astype(acc)


def _wave_sum(v):
    """common.hpp::wave_sum: v += shfl_xor(v, o) for o = 32 .. 1 on the last axis (64 lanes); every lane ends with the same tree."""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lanes ^ o]).astype(v.dtype)
    return v[..., 0]


def _lane_chain(s, wsq, dt):
    """q[b,o] of demod_kernel / demod_gq_kernel: lane l runs acc = fma(s_i * s_i, wsq[o,i], acc) over i = l, l + 64, ..., then the
    64-lane butterfly."""
    B, Cin = s.shape
    Cout = wsq.shape[0]
    n = -(-Cin // 64)
    sp = np.zeros((B, n * 64), dt)
    sp[:, :Cin] = s
    wp = np.zeros((Cout, n * 64), dt)
    wp[:, :Cin] = wsq
    acc = np.zeros((B, Cout, 64), dt)
    for j in range(n):
        sv = sp[:, j * 64:(j + 1) * 64]
        acc = ((sv * sv).astype(dt)[:, None, :] * wp[None, :, j * 64:(j + 1) * 64] + acc).astype(dt)
    return _wave_sum(acc)


def demod_ref(s, wsq, eps):
    """d[b,o] = (sum_i s^2 wsq + eps)^(-1/2) for f32 s [B,Cin], f32 wsq [Cout,Cin], f32 eps."""
    q = (ld(s) ** 2)[:, None, :] * ld(wsq)[None]
    return 1 / np.sqrt(q.sum(2) + LD(F32(eps)))


# ideas_demod, f32, all terms positive (wsq >= 0): a term carries the rounding of s * s, the n = ceil(Cin / 64) roundings of its lane's
# fma chain, the 6 of the butterfly and the one of + eps: q + eps has relative error <= (n + 8) u.  d = (q + eps)^(-1/2) halves it, and
# rsqrtf adds at most 2 ulp <= 2 * 2^-23 = 4u relative.
def demod_bound(Cin, ref):
    return ((-(-Cin // 64) + 8) / 2 + 4) * U24 * np.abs(ref)


def demod_eval(s, wsq, eps):
    q = _lane_chain(np.asarray(s, F32), np.asarray(wsq, F32), F32)
    return (F32(1) / np.sqrt((q + F32(eps)).astype(F32), dtype=F32)).astype(F32)        # two roundings for rsqrtf's <= 2 ulp


def demod_bwd_ref(dot_s, dot_d, d32, s, wsq, eps):
    """ideas_demod_bwd on (double dot_s [B,Cin], double dot_d [B,Cout], f32 d32, f32 s, double wsq [Cout,Cin], f32 eps):
    gq = -0.5 (dot_d / d32) dt^3 with dt = (sum_i s^2 wsq + eps)^(-1/2) and dL/dd = dot_d / d32, d32 the f32 factor the forward
    multiplied by; gs = (s != 0 ? dot_s / s : 0) + 2 s sum_o gq wsq.  d32 = None: the first term only.
    -> (gs, gq, T) with T = |dot_s / s| + 2 |s| sum_o |gq wsq|."""
    S = ld(s)
    safe = np.where(S != 0, S, LD(1))
    direct = np.where(S != 0, ld(dot_s) / safe, LD(0))
    if d32 is None:
        return direct, None, np.abs(direct)
    W = ld(wsq)
    q = ((S ** 2)[:, None, :] * W[None]).sum(2)
    dt = 1 / np.sqrt(q + LD(F32(eps)))
    gq = LD(-0.5) * (ld(dot_d) / ld(d32)) * dt ** 3
    gs = direct + 2 * S * (gq @ W)
    T = np.abs(direct) + 2 * np.abs(S) * (np.abs(gq) @ np.abs(W))
    return gs, gq, T


# gq, in double (v = U53): q is a sum of Cin positive terms, each s * s exact (48 bits), one rounding for the product with wsq and at
# most ceil(Cin / 64) - 1 + min(6, ceil(log2 Cin)) additions to a non-zero partner on its path (adding an exact zero costs nothing),
# so rel(q) <= (Cin + 2) v at every Cin; + eps, 1 / x, sqrt, the division by d32
# and three multiplications add 7 v; d^3 = d2 sqrt(d2) carries 1.5 rel(q).  Together <= (1.5 (Cin + 2) + 7) v = (0.75 Cin + 5) 2^-52
# <= (Cin + 16) 2^-52 of |gq|.  The float copy adds one rounding to f32.
def gq_bound(Cin, ref, f32_copy):
    return ((U24 if f32_copy else 0.0) + (Cin + 16) * 2 * U53) * np.abs(ref)


# gs: the o-sum has Cout terms gq wsq, each with gq's error above, a product rounding and at most ceil(Cout / 4) + 2 additions; the
# factor 2 s is exact and the closing fma rounds once; dot_s / s is one division.  Every piece is relative to its own term of T, so
# |err| <= (Cin + 16 + Cout / 2 + 4) 2^-52 T <= (Cin + Cout + 32) 2^-52 T before the one rounding of the result to f32, U24 |gs|.
def gs_algebra_bound(Cin, Cout, T):
    """The double-algebra part: what gs may be off by BEFORE its one rounding to f32."""
    return (Cin + Cout + 32) * 2 * U53 * T


def gs_bound(Cin, Cout, ref, T):
    return U24 * np.abs(ref) + gs_algebra_bound(Cin, Cout, T)


def demod_bwd_eval(dot_s, dot_d, d32, s, wsq, eps, dt=F64):
    """ideas_demod_bwd in the kernels' operation order with all algebra in ``dt`` (the library's: float64; float32 = the round-2
    form the file's header rules out).  -> (gs before the f32 store, gq before the f32 store)."""
    s_, B, Cin = np.asarray(s, dt), s.shape[0], s.shape[1]
    safe = np.where(s_ != 0, s_, dt(1))
    g = np.where(s_ != 0, (np.asarray(dot_s, dt) / safe).astype(dt), dt(0))
    if d32 is None:
        return g, None
    W = np.asarray(wsq, dt)
    Cout = W.shape[0]
    q = _lane_chain(s_, W, dt)
    d2 = (dt(1) / (q + dt(F32(eps))).astype(dt)).astype(dt)
    gq = (((dt(-0.5) * (np.asarray(dot_d, dt) / np.asarray(d32, dt)).astype(dt)).astype(dt) * d2).astype(dt) * np.sqrt(d2, dtype=dt)).astype(dt)
    part = np.zeros((4, B, Cin), dt)
    for o in range(Cout):                     # slice og = o % 4 runs o = og, og + 4, ... in order
        part[o % 4] = ((gq[:, o:o + 1] * W[o][None, :]).astype(dt) + part[o % 4]).astype(dt)
    osum = (((part[0] + part[1]).astype(dt)) + ((part[2] + part[3]).astype(dt))).astype(dt)
    gs = (((dt(2) * s_).astype(dt) * osum).astype(dt) + g).astype(dt)
    return gs, gq


def demod_wgrad_ref(gw0, w, gq, s, coef):
    """gw[o,i,k] = gw0 + coef W[o,i,k] sum_b gq[b,o] s[b,i]^2 (f32 operands, f32 coef).
    -> (value, |coef W| sum_b |gq| s^2)."""
    acc = np.einsum("bo,bi->oi", ld(gq), ld(s) ** 2)
    aabs = np.einsum("bo,bi->oi", np.abs(ld(gq)), ld(s) ** 2)
    cw = LD(F32(coef)) * ld(w)
    return ld(gw0) + cw * acc[:, :, None, None], np.abs(cw) * aabs[:, :, None, None]


# acc = sum_b fmaf(gq, s * s, acc): the rounding of s * s and at most B of the chain per term, then * coef, one rounding:
# (B + 2) u of |coef| sum_b |gq| s^2, times |W|; the closing fmaf(acc, W, gw) rounds its result once: u |gw_after|.  + 1 u spare.
def demod_wgrad_bound(B, scale, ref):
    return (B + 3) * U24 * scale + U24 * np.abs(ref)


def demod_wgrad_eval(gw0, w, gq, s, coef):
    gq, s, w = np.asarray(gq, F32), np.asarray(s, F32), np.asarray(w, F32)
    acc = np.zeros(w.shape[:2], F32)
    for b in range(s.shape[0]):
        sv2 = (s[b] * s[b]).astype(F32)
        acc = (gq[b][:, None].astype(F64) * sv2[None, :].astype(F64) + acc.astype(F64)).astype(F32)
    acc = (acc * F32(coef)).astype(F32)
    return (acc[:, :, None, None].astype(F64) * w.astype(F64) + np.asarray(gw0, F64)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------- cancellation
CANCEL_CASES = [(2, 1, 40), (3, 2, 40), (3, 4, 7), (3, 72, 40), (2, 130, 5)]      # (B, Cin, Cout)


def cancel_case(B, Cin, Cout, seed=0, eps=1e-8):
    """Operands of ideas_demod_bwd as a real demodulated layer produces them, for one pixel of x = 1 and a 1x1 weight A:
    y[b,o] = d32[b,o] sum_i A[o,i] s[b,i], upstream gradient t, so dot_d = <t, y> = t y and dot_s = <x, gx> = s ((t d32) @ A).
    y does not change when s[b,:] is rescaled (up to eps), so sum_i s_i gs_i ~ 0: the two terms of gs cancel, completely for
    Cin = 1, where |gs| is ~1e-7 of T (what is left is the rounding of d32 to f32)."""
    rng = np.random.default_rng(1000 * seed + 100 * B + 10 * Cin + Cout)
    A = rng.standard_normal((Cout, Cin))
    t = rng.standard_normal((B, Cout))
    s = (1 + 0.5 * rng.standard_normal((B, Cin))).astype(F32)
    wsq = A * A
    s64 = s.astype(F64)
    d32 = (1 / np.sqrt((s64 * s64) @ wsq.T + F64(F32(eps)))).astype(F32)
    y = d32.astype(F64) * (s64 @ A.T)
    return dict(dot_s=s64 * ((t * d32.astype(F64)) @ A), dot_d=t * y, d32=d32, s=s, wsq=wsq, eps=eps)
