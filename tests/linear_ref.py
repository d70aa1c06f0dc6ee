"""Plain float64 restatements of the four C contracts of csrc/linear.hip and csrc/optim.hip, written from the formulas of
include/ideas_hip.h (not from the kernels), and the cases tests/test_linear_abi_gpu.py / tests/test_adam_ema_abi_gpu.py run.

    fwd     y_s[m][j]   = scale_s * sum_k x[m][k] w_s[j][k] + bias_mul_s * bias_s[j]
    bwd_x   gx[m][k]    = sum_s scale_s * sum_j g_s[m][j] w_s[j][k]
    bwd_w   gw_s[j][k] (+)= scale_s * sum_m g_s[m][j] x[m][k];     gb_s[j] (+)= bias_mul_s * sum_m g_s[m][j]
    adam    v = beta2 v + (1 - beta2) g g;   p -= lr g / (sqrt(v) / sqrt(bc2) + eps);   ema = d ema + (1 - d) p

Every function returns the value AND ``S``, the sum of the absolute values of all addends of each element: the quantity every
summation error bound is stated in.  The float parameters enter as the float32 values the ABI receives (``f32``).

Two kinds of data per case (``make_case``), seeded on the CPU:
  * "exact":  integers in [-4, 4], power-of-two scales.  Every addend is then a multiple of a power of two q, and any partial sum, in
    any association, is a multiple of q of magnitude <= S: it is a float32 number as long as S / q < 2^24 (``exact_in_f32``).  A
    correct f32 kernel therefore reproduces the f64 reference BIT FOR BIT, and a dropped, doubled or misplaced term cannot.
  * "random": N(0, 1) drawn in float32, the product's scales 1/sqrt(K) (1 + 0.5 i) and bias_mul in {1, 0.25}; the bound is
    ``gamma(3 T + 80) * S`` per element (``bound``), T = the number of terms of the element's sum.
"""
import math
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of float32
F64 = torch.float64


def f32(v):
    """The float32 value a C ``float`` argument receives, as a Python float."""
    return float(np.float32(v))


def gamma(n):
    """n u / (1 - n u): the standard bound on the relative error of n chained roundings."""
    return n * U / (1.0 - n * U)


def bound(terms, S):
    """Elementwise error bound of a float32 sum of ``terms`` products in ANY association: up to three roundings a term (the scaling
    of g, the product, the add -- so it holds whether or not the compiler or the matrix unit fuses them), plus 80 for up to 64 split
    folds and the epilogue (scale, bias product, bias add, accumulate)."""
    return gamma(3 * terms + 80) * S


def exact_in_f32(value, S, quantum):
    """Every addend is a multiple of ``quantum`` (a power of two) and their absolute values sum to ``S``: is every partial sum, in any
    order, a float32 number (fewer than 24 significant bits, no exponent trouble), and does ``value`` survive float32 unchanged?"""
    m, e = math.frexp(quantum)
    if m != 0.5 or not -100 < e < 100:
        return False
    return bool((S / quantum < 2.0 ** 24).all()) and bool((value.float().double() == value).all())


# a layer: w [n][K], b [n] or None, g [M][n] (the incoming gradient; None in the forward), scale, bias_mul
Seg = namedtuple("Seg", "w b g scale bias_mul")


def _d(t):
    return None if t is None else t.to(F64)


def fwd(x, segs):
    """[(y_s, S_s)] for every segment."""
    x = _d(x)
    out = []
    for s in segs:
        sc, bm, w = f32(s.scale), f32(s.bias_mul), _d(s.w)
        y, S = sc * (x @ w.t()), abs(sc) * (x.abs() @ w.abs().t())
        if s.b is not None:
            y, S = y + bm * _d(s.b), S + (bm * _d(s.b)).abs()
        out.append((y, S))
    return out


def bwd_x(segs):
    """(gx, S): ONE tensor, the sum over the segments."""
    gx = S = 0.0
    for s in segs:
        sc = f32(s.scale)
        gx = gx + sc * (_d(s.g) @ _d(s.w))
        S = S + abs(sc) * (_d(s.g).abs() @ _d(s.w).abs())
    return gx, S


def bwd_w(x, segs, old, accumulate):
    """[((gw_s, S), (gb_s, S) or None)]; ``old`` = [(gw_old, gb_old or None)] is added (and its magnitude joins S) when ``accumulate``;
    gb_s is None for a segment without a bias."""
    x = _d(x)
    out = []
    for i, s in enumerate(segs):
        sc, bm, g = f32(s.scale), f32(s.bias_mul), _d(s.g)
        gw, Sw = sc * (g.t() @ x), abs(sc) * (g.abs().t() @ x.abs())
        gb, Sb = bm * g.sum(0), abs(bm) * g.abs().sum(0)
        if accumulate:
            gw, Sw = gw + _d(old[i][0]), Sw + _d(old[i][0]).abs()
            if old[i][1] is not None:
                gb, Sb = gb + _d(old[i][1]), Sb + _d(old[i][1]).abs()
        out.append(((gw, Sw), (gb, Sb) if s.b is not None else None))
    return out


def adam_ema(p, g, v, ema, lr, beta2, eps, bc2, decay):
    """One step on float64 copies of the float32 state (any device).  1 - beta2, 1 - decay and sqrt(bc2) are formed in float32, as
    csrc/optim.hip does (the first two in the kernel, the root on the host); everything after that is float64.
    -> dict: p, v, ema (None without one), update, and the magnitudes the bounds are stated in: S_p = |p_old| + |update|, S_v = v,
    S_ema = |ema_old| + |p|."""
    lr, beta2, eps, bc2, decay = (np.float32(a) for a in (lr, beta2, eps, bc2, decay))
    omb, omd, sbc = float(np.float32(1) - beta2), float(np.float32(1) - decay), float(np.sqrt(bc2))
    lr, beta2, eps, decay = float(lr), float(beta2), float(eps), float(decay)
    p, g, v = _d(p), _d(g), _d(v)
    v1 = beta2 * v + omb * g * g
    upd = lr * (g / (v1.sqrt() / sbc + eps))
    p1 = p - upd
    res = {"p": p1, "v": v1, "ema": None, "update": upd, "S_p": p.abs() + upd.abs(), "S_v": v1, "S_ema": None}
    if ema is not None:
        res["ema"] = decay * _d(ema) + omd * p1
        res["S_ema"] = _d(ema).abs() + p1.abs()
    return res


# --------------------------------------------------------------------------------------------------------------------- the cases
# M, K, ns: the shape; pad*: row stride minus row length, in floats (per segment where the matrix is per segment); nobias: segments
# without bias / bias gradient; kinds: which data the case runs with.  The smallest shapes that reach each branch of the kernels:
BOTH, RANDOM = ("exact", "random"), ("random",)
FWD_CASES = {
    # one K step (steps = 1): waves 0-2 get no step, wave 3 only the odd tail; row and column clamps; n = 1
    "m1_k8_n1": dict(M=1, K=8, ns=(1,), kinds=BOTH),
    # 3 steps (0/1/1/1 per wave); two m tiles, the second with one live row; n < 32; n = 33 spans two j tiles; every stride padded:
    # ldx = K + 4, ldw = K + 8; ldy = n + 3 = 10 (rows not 16-byte aligned), ldy = n = 33 (odd and dense), ldy = 64
    "m33_k24_n7_33_64": dict(M=33, K=24, ns=(7, 33, 64), padx=4, padw=(8, 8, 8), pady=(3, 0, 0), nobias=(1,), kinds=BOTH),
    # 5 steps (1/1/1/2): the pair loop and the tail in one launch
    "m32_k40_n32": dict(M=32, K=40, ns=(32,), kinds=BOTH),
    # a full table (IDEAS_LINEAR_MAX_SEGMENTS), every scale different: find_seg over 32 entries
    "m5_k16_32seg": dict(M=5, K=16, ns=(8,) * 32, kinds=BOTH),
    # the product's shapes
    "m96_k2048_n8_512": dict(M=96, K=2048, ns=(8, 512), nobias=(1,), kinds=RANDOM),
}
BWD_X_CASES = {
    # one group, one split, one slab: only lane 0 of wave 0 holds live columns
    "m1_k4_n8": dict(M=1, K=4, ns=(8,), kinds=BOTH),
    # two m tiles with clamped rows; the second k slab has 8 live columns; splits = groups = 4; ldgx, ldy and ldw padded
    "m33_k520_n8_24": dict(M=33, K=520, ns=(8, 24), padgx=4, pady=(4, 4), padw=(4, 4), kinds=BOTH),
    # three k slabs (the last with 4 live columns); 26 groups = 26 splits
    "m40_k1028_n64_8_136": dict(M=40, K=1028, ns=(64, 8, 136), kinds=BOTH),
    # 9 groups over 8 splits: the last split holds groups 7 and 8, which belong to different segments
    "m256_k4096_n8_16_40_8": dict(M=256, K=4096, ns=(8, 16, 40, 8), kinds=BOTH),
    # M K / 4 = 266240 float4 for the fold kernel's 1024 blocks x 256 threads = 262144: its grid-stride loop takes a second trip
    # (256 x 4096 above is the last size that does not); two splits to fold
    "m260_k4096_n8_8": dict(M=260, K=4096, ns=(8, 8), kinds=BOTH),
}
BWD_W_CASES = {
    # odd M: the missing second row of the pair adds zeros; n = 1
    "m1_k4_n1": dict(M=1, K=4, ns=(1,), kinds=BOTH),
    # ragged j tile (33 = 32 + 1); second k slab; ldgw = K + 4, ldx = K + 4, ldy = 33 (odd); a bias gradient on segment 0 only
    "m7_k520_n33_8": dict(M=7, K=520, ns=(33, 8), padx=4, padgw=(4, 4), nobias=(1,), kinds=BOTH),
    # the product's shapes
    "m96_k2048_n8_512": dict(M=96, K=2048, ns=(8, 512), nobias=(1,), kinds=RANDOM),
}
CASES = {"fwd": FWD_CASES, "bwd_x": BWD_X_CASES, "bwd_w": BWD_W_CASES}
PARAMS = {e: [(n, k) for n, c in cs.items() for k in c["kinds"]] for e, cs in CASES.items()}

Case = namedtuple("Case", "M K ns x segs old spec")


def make_case(entry, name, kind):
    """The case's data as float32 CPU tensors: x [M][K]; per segment w, b (None where the case has none), g, the scales; ``old`` =
    [(gw_old, gb_old or None)], the non-zero contents the accumulating weight gradient adds to."""
    spec = CASES[entry][name]
    M, K, ns = spec["M"], spec["K"], spec["ns"]
    gen = torch.Generator().manual_seed(1000 * sorted(CASES).index(entry) + sorted(CASES[entry]).index(name))
    if kind == "exact":
        draw = lambda *s: torch.randint(-4, 5, s, generator=gen).float()
    else:
        draw = lambda *s: torch.randn(*s, generator=gen)
    x = draw(M, K)
    segs, old = [], []
    for i, n in enumerate(ns):
        if kind == "exact":
            # powers of two; with 32 segments all different, and bias_mul kept within 2 bits of scale so the sum stays short
            scale, bias_mul = (2.0 ** (i - 16), 2.0 ** (i - 14)) if len(ns) > 4 else (2.0 ** -i, 1.0 if i % 2 == 0 else 0.25)
        else:
            scale, bias_mul = 1 / math.sqrt(K) * (1 + 0.5 * i), 1.0 if i % 2 == 0 else 0.25
        has_b = i not in spec.get("nobias", ())
        w, b, g = draw(n, K), draw(n), draw(M, n)
        segs.append(Seg(w, b if has_b else None, g, scale, bias_mul))
        old.append((draw(n, K), draw(n) if has_b else None))
    return Case(M, K, ns, x, segs, old, spec)


def quanta(case):
    """Per segment, the power of two every addend of an "exact" case is a multiple of, for (y, gw with accumulation, gb with
    accumulation); for gx it is the smallest scale of all segments (the sum runs over them)."""
    return [(min(f32(s.scale), f32(s.bias_mul)), min(f32(s.scale), 1.0), min(f32(s.bias_mul), 1.0)) for s in case.segs]


# ----------------------------------------------------------------------------------------------------------------- Adam + EMA
ADAM_LR, ADAM_BETA2, ADAM_EPS, ADAM_DECAY = 0.002 * 16 / 17, 0.99 ** (16 / 17), 1e-8, 0.5 ** (32 / 10000)
ADAM_STEPS = (1, 7, 5000)
ADAM_BIG = 8192 * 256 * 4 + 8           # the grid is capped at 8192 blocks of 256 float4 lanes: the first n with a second loop trip


def adam_bc2(t):
    return 1.0 - ADAM_BETA2 ** t


def adam_case(n, seed):
    """float32 CPU state: p, ema ~ N(0, 1); |g| log-uniform in [1e-8, 1e3] with random sign; v = 0 on a quarter of the elements and
    log-uniform in [1e-12, 1e4] otherwise; the first element of every block of 16 has g = 0 where v = 0 (update exactly 0)."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda: torch.rand(n, generator=gen, dtype=F64)
    p, ema = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    g = 10.0 ** (r() * 11 - 8) * torch.where(r() < 0.5, -1.0, 1.0)
    v = torch.where(r() < 0.25, torch.zeros(n, dtype=F64), 10.0 ** (r() * 16 - 12))
    idx = torch.arange(n)
    v[idx % 16 == 1] = 0.0
    g[(idx % 16 == 0) & (v == 0)] = 0.0
    g[1] = 0.0                                    # (n = 4 has the pair too: element 1 has v = 0 by the line above)
    return p, g.float(), v.float(), ema
