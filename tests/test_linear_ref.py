"""tests/linear_ref.py is what the ABI tests of csrc/linear.hip and csrc/optim.hip are judged by; here it is checked itself, without
a GPU: against autograd of F.linear and against torch.optim.Adam + utils.accumulate in float64, that every "exact" case really is
exact in float32 (so the GPU equality test can be met by a correct f32 kernel, and only by one), and that the elementwise bound of
the "random" cases holds for a plain float32 evaluation with room to spare while a single dropped term breaks it."""
import math

import pytest
import torch
import torch.nn.functional as F

import linear_ref as R

F64 = torch.float64
ALL = [(e, n, k) for e in sorted(R.CASES) for n, k in R.PARAMS[e]]
EXACT = [(e, n) for e, n, k in ALL if k == "exact"]
SMALL = [(e, n, k) for e, n, k in ALL if R.CASES[e][n]["M"] * R.CASES[e][n]["K"] <= 64 * 1028]


@pytest.mark.parametrize("entry,name,kind", SMALL)
def test_reference_equals_autograd_of_f_linear(entry, name, kind):
    """fwd / bwd_x / bwd_w against F.linear(x, w * scale, b * bias_mul) and its autograd in float64 (the float32-rounded scales)."""
    c = R.make_case(entry, name, kind)
    x = c.x.double().requires_grad_(True)
    ws = [s.w.double().requires_grad_(True) for s in c.segs]
    bs = [None if s.b is None else s.b.double().requires_grad_(True) for s in c.segs]
    ys = [F.linear(x, w * R.f32(s.scale), None if b is None else b * R.f32(s.bias_mul)) for s, w, b in zip(c.segs, ws, bs)]
    leaves = [x] + ws + [b for b in bs if b is not None]
    grads = list(torch.autograd.grad(ys, leaves, [s.g.double() for s in c.segs]))
    close = lambda a, b, S: bool(((a - b).abs() <= 1e-13 * S + 1e-300).all())
    for (y, S), y_ref in zip(R.fwd(c.x, c.segs), ys):
        assert y.shape == y_ref.shape and close(y, y_ref.detach(), S)
    gx, S = R.bwd_x(c.segs)
    assert gx.shape == x.shape and close(gx, grads[0], S)
    gbs = iter(grads[1 + len(ws):])
    for i, ((gw, Sw), gb) in enumerate(R.bwd_w(c.x, c.segs, c.old, False)):
        assert close(gw, grads[1 + i], Sw)
        assert (gb is None) == (bs[i] is None)
        if gb is not None:
            assert close(gb[0], next(gbs), gb[1])
    for i, ((gw, Sw), gb) in enumerate(R.bwd_w(c.x, c.segs, c.old, True)):
        assert close(gw, grads[1 + i] + c.old[i][0].double(), Sw)
        assert bool((Sw >= c.old[i][0].double().abs()).all())


def test_adam_reference_equals_torch_adam_and_accumulate():
    """Three steps of torch.optim.Adam(betas=(0, beta2)) + utils.accumulate on float64 parameters.  Adam forms 1 - beta2 and
    sqrt(1 - beta2^t) in double; the reference, as the kernel, takes bc2 as a float32 and roots it in float32 (1 - beta2 and
    1 - decay are exact in float32 for beta2, decay in [0.5, 1]).  That is one rounding of bc2 (half of it after the root) and one of
    the root: each update differs by less than 2^-23 of itself, the parameter by that of the updates so far, v not at all."""
    from ideas_amd.utils import accumulate
    n = 512
    p0, g0, v0, e0 = R.adam_case(n, 5)
    lr, b2, eps, decay = (R.f32(a) for a in (R.ADAM_LR, R.ADAM_BETA2, R.ADAM_EPS, R.ADAM_DECAY))
    assert 1 - b2 == R.f32(1 - b2) and 1 - decay == R.f32(1 - decay)
    net, net_ema = torch.nn.Linear(1, 1, bias=False).double(), torch.nn.Linear(1, 1, bias=False).double()
    net.weight.data, net_ema.weight.data = p0.double().clone().view(1, n), e0.double().clone().view(1, n)
    opt = torch.optim.Adam(net.parameters(), lr=lr, betas=(0.0, b2), eps=eps)
    p, v, ema = p0.double(), torch.zeros(n, dtype=F64), e0.double()
    moved = torch.zeros(n, dtype=F64)
    gen = torch.Generator().manual_seed(6)
    for t in (1, 2, 3):
        g = g0.double() * torch.rand(n, generator=gen, dtype=F64)
        net.weight.grad = g.clone().view(1, n)
        opt.step()
        accumulate(net_ema, net, decay)
        r = R.adam_ema(p, g, v, ema, lr, b2, eps, 1.0 - b2 ** t, decay)
        p, v, ema = r["p"], r["v"], r["ema"]
        moved += r["update"].abs()
        tol = 2.0 ** -23 * moved + 1e-15 * r["S_p"]
        assert bool(((p - net.weight.data.view(-1)).abs() <= tol).all())
        assert bool(((v - opt.state[net.weight]["exp_avg_sq"].view(-1)).abs() <= 1e-15 * v).all())
        assert bool(((ema - net_ema.weight.data.view(-1)).abs() <= tol + 1e-15 * r["S_ema"]).all())
        assert bool((r["S_p"] >= p.abs()).all()) and r["S_v"] is v
    assert float(moved.min()) >= 0 and float(moved.max()) > 0


def test_adam_reference_zero_gradient_on_zero_moment_moves_nothing():
    for n in (4, 1028):
        p, g, v, ema = R.adam_case(n, n)
        both = (g == 0) & (v == 0)
        assert bool(both[1]) and int(both.sum()) >= 1 and int((v == 0).sum()) >= n // 8
        r = R.adam_ema(p, g, v, ema, R.ADAM_LR, R.ADAM_BETA2, R.ADAM_EPS, R.adam_bc2(1), R.ADAM_DECAY)
        assert bool((r["update"][both] == 0).all()) and bool((r["p"][both] == p.double()[both]).all())
        assert bool(torch.isfinite(r["p"]).all()) and bool(torch.isfinite(r["v"]).all())
        # no float32 subnormals anywhere the kernel computes: g*g, v
        tiny = 2.0 ** -126
        gg = (g.double() ** 2)[g != 0]
        assert float(gg.min()) * (1 - R.f32(R.ADAM_BETA2)) > tiny and float(r["v"][r["v"] > 0].min()) > tiny


@pytest.mark.parametrize("entry,name", EXACT)
def test_exact_cases_are_exact_in_float32(entry, name):
    """Integer data in [-4, 4] and power-of-two scales: every addend is a multiple of a power of two q and S / q < 2^24, so every
    partial sum in every association -- before and after the scale, the bias and the accumulate step -- is a float32 number, and
    the float64 reference is one too."""
    c = R.make_case(entry, name, "exact")
    for t in [c.x] + [u for s in c.segs for u in (s.w, s.b, s.g) if u is not None] + [u for o in c.old for u in o if u is not None]:
        assert bool((t == t.round()).all()) and float(t.abs().max()) <= 4
    for s in c.segs:
        assert math.frexp(s.scale)[0] == 0.5 and math.frexp(s.bias_mul)[0] == 0.5
    q = R.quanta(c)
    if entry == "fwd":
        assert len({s.scale for s in c.segs}) == len(c.segs)
        for (y, S), (qy, _, _), s in zip(R.fwd(c.x, c.segs), q, c.segs):
            assert R.exact_in_f32(y, S, qy)
            # the unscaled sum the kernel holds before its epilogue: integers
            xd, wd = c.x.double(), s.w.double()
            assert R.exact_in_f32(xd @ wd.t(), xd.abs() @ wd.abs().t(), 1.0)
    elif entry == "bwd_x":
        gx, S = R.bwd_x(c.segs)
        assert R.exact_in_f32(gx, S, min(R.f32(s.scale) for s in c.segs))
    else:
        for acc in (False, True):
            for ((gw, Sw), gb), (_, qw, qb) in zip(R.bwd_w(c.x, c.segs, c.old, acc), q):
                assert R.exact_in_f32(gw, Sw, qw)
                if gb is not None:
                    assert R.exact_in_f32(gb[0], gb[1], qb)


def test_exact_in_f32_refuses_what_is_not():
    one = torch.ones(1, dtype=F64)
    assert R.exact_in_f32(one * (2.0 ** 24 - 1), one * (2.0 ** 24 - 1), 1.0)
    assert not R.exact_in_f32(one * 2.0 ** 24, one * 2.0 ** 24, 1.0)               # a partial sum may need 25 bits
    assert not R.exact_in_f32(one * (1 + 2.0 ** -30), one * 2, 1.0)                # the value itself is no float32
    assert not R.exact_in_f32(one, one, 0.3)                                       # not a power of two
    assert not R.exact_in_f32(one, one * 4, 2.0 ** -23)                            # 4 / 2^-23 = 2^25 quanta


@pytest.mark.parametrize("entry,name,kind", [(e, n, k) for e, n, k in SMALL if k == "random"])
def test_random_bound_holds_for_float32_and_notices_a_lost_term(entry, name, kind):
    """A float32 evaluation on the CPU (another association than the kernel's) stays far inside gamma(3 T + 80) S, while some
    single term of the first element's sum is larger than that element's bound: losing it would show."""
    c = R.make_case(entry, name, kind)
    sc = [torch.tensor(s.scale, dtype=torch.float32) for s in c.segs]
    if entry == "fwd":
        T = c.K
        got = [sc_ * (c.x @ s.w.t()) + (0 if s.b is None else s.b * torch.tensor(s.bias_mul)) for s, sc_ in zip(c.segs, sc)]
        ref = R.fwd(c.x, c.segs)
        lost = c.x[0].double() * c.segs[0].w[0].double() * R.f32(c.segs[0].scale)
    elif entry == "bwd_x":
        T = sum(c.ns)
        got = [sum((s.g * sc_) @ s.w for s, sc_ in zip(c.segs, sc))]
        ref = [R.bwd_x(c.segs)]
        lost = c.segs[0].g[0].double() * c.segs[0].w[:, 0].double() * R.f32(c.segs[0].scale)
    else:
        T = c.M
        got = [sc_ * (s.g.t() @ c.x) for s, sc_ in zip(c.segs, sc)]
        ref = [r[0] for r in R.bwd_w(c.x, c.segs, c.old, False)]
        lost = c.segs[0].g[:, 0].double() * c.x[:, 0].double() * R.f32(c.segs[0].scale)
    worst = 0.0
    for a, (r, S) in zip(got, ref):
        assert a.dtype == torch.float32
        worst = max(worst, float(((a.double() - r).abs() / R.bound(T, S)).max()))
    print(entry, name, "float32 on the CPU: worst err / bound", worst)
    assert worst < 0.1
    r, S = ref[0]
    assert float(lost.abs().max()) > R.bound(T, S)[0, 0]


def test_gamma_and_bound():
    assert R.gamma(1) == pytest.approx(2.0 ** -24, rel=1e-6) and R.gamma(1) > 2.0 ** -24
    assert float(R.bound(8, torch.ones(1, dtype=F64))) == R.gamma(104)
    assert R.f32(0.1) != 0.1 and R.f32(0.25) == 0.25
