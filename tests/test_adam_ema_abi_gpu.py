"""ideas_adam_ema (csrc/optim.hip) through the C ABI on raw buffers against tests/linear_ref.py::adam_ema, ELEMENTWISE:

    |p' - p| <= 16 u (|p_old| + |update|),      |v' - v| <= 16 u v,      |ema' - ema| <= 16 u (|ema_old| + |p|),      u = 2^-24.

Each quantity is at most 8 correctly rounded float32 operations on same-sign or bounded terms (v: two products, a square, an add;
the update: root, two divides, an add, a product; then one subtract; the EMA two products and an add); the bound doubles that.  The
build has no fast-math and the device code uses the correctly rounded divide and square root.

The gradient spans eleven decades and a quarter of the second moments are zero -- a whole-tensor max|a - b| / max|b| sees only the
largest elements of such data -- and g = 0 on v = 0 must leave p bitwise alone.  Sizes: n = 4 (one lane), n = 1028 with and without
EMA (both instantiations; p and v must not depend on which), and n = 8192 * 256 * 4 + 8, the first size at which the grid-stride
loop (the grid is capped at 8192 blocks) takes a second trip; that one is compared on the device.

Largest error / bound seen on an MI355X: p 0.26, v 0.18, ema 0.062 (all three at the 8.4 M element size).
"""
import pytest
import torch

import linear_ref as R

pytestmark = pytest.mark.gpu
NULL, SHAPE, ALIGN = -1, -2, -4
RATIO = {}


@pytest.fixture(scope="module")
def L():
    from ideas_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nlargest error / bound per output:", {k: float("%.3g" % v) for k, v in sorted(RATIO.items())})


def _dev(t, off=0):
    """``t`` on the device as float32, its first element ``off`` floats behind the (256-byte aligned) start of its buffer"""
    buf = torch.empty(t.numel() + off, device="cuda", dtype=torch.float32)
    v = buf[off:]
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


def _call(L, p, g, v, ema, n, t, over=()):
    a = dict(p=L.ptr(p), g=L.ptr(g), v=L.ptr(v), ema=L.ptr(ema), n=n, lr=R.ADAM_LR, beta2=R.ADAM_BETA2, eps=R.ADAM_EPS,
             bc2=R.adam_bc2(t), decay=R.ADAM_DECAY)
    a.update(over)
    rc = L.load().ideas_adam_ema(a["p"], a["g"], a["v"], a["ema"], a["n"], a["lr"], a["beta2"], a["eps"], a["bc2"], a["decay"],
                                 L.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _step(L, n, t, with_ema, seed, device_compare=False):
    """one call on fresh state -> (p', v', ema') as left on the device, judged against the reference"""
    p0, g0, v0, e0 = R.adam_case(n, seed)
    p, g, v, ema = _dev(p0), _dev(g0), _dev(v0), (_dev(e0) if with_ema else None)
    where = (lambda x: x.cuda()) if device_compare else (lambda x: x)
    ref = R.adam_ema(where(p0), where(g0), where(v0), where(e0) if with_ema else None, R.ADAM_LR, R.ADAM_BETA2, R.ADAM_EPS,
                     R.adam_bc2(t), R.ADAM_DECAY)
    assert _call(L, p, g, v, ema, n, t) == 0
    back = (lambda x: x) if device_compare else (lambda x: x.cpu())
    assert torch.equal(back(g), where(g0)), "the gradient is an input"
    worst = {}
    for key, got in (("p", p), ("v", v), ("ema", ema)):
        if got is None:
            continue
        got = back(got).double()
        assert bool(torch.isfinite(got).all()), key
        err, bnd = (got - ref[key]).abs(), 16 * R.U * ref["S_" + key]
        worst[key] = float(torch.where(err == 0, torch.zeros_like(err), err / bnd.clamp_min(1e-300)).max())
        RATIO[key] = max(RATIO.get(key, 0.0), worst[key])
        assert bool((err <= bnd).all()), (key, n, t, "worst error / bound", worst[key])
    still = where((g0 == 0) & (v0 == 0))
    assert int(still.sum()) >= 1
    assert torch.equal(back(p)[still], where(p0)[still]) and bool((back(v)[still] == 0).all()), "g = 0 on v = 0 moved a parameter"
    print("adam_ema n", n, "t", t, "ema", with_ema, "worst error / bound", worst)
    return p, v, ema


@pytest.mark.parametrize("t", R.ADAM_STEPS)
@pytest.mark.parametrize("n", [4, 1028])
def test_adam_ema_elementwise(L, n, t):
    p, v, ema = _step(L, n, t, True, 100 + n)
    p2, v2, none = _step(L, n, t, False, 100 + n)
    assert none is None
    assert torch.equal(p.view(torch.int32), p2.view(torch.int32)) and torch.equal(v.view(torch.int32), v2.view(torch.int32)), \
        "p and v depend on whether an EMA is kept"


def test_adam_ema_second_trip_of_the_grid_stride_loop(L):
    """n / 4 = 8192 * 256 + 2 lanes of work for 8192 * 256 threads: two of them run the loop twice"""
    assert R.ADAM_BIG == 8388616 and (R.ADAM_BIG // 4 - 1) // 256 + 1 > 8192 and (R.ADAM_BIG - 8) // 4 // 256 == 8192
    _step(L, R.ADAM_BIG, 7, True, 9, device_compare=True)


REFUSALS = {
    "p NULL": (NULL, lambda s: dict(p=None)),
    "g NULL": (NULL, lambda s: dict(g=None)),
    "v NULL": (NULL, lambda s: dict(v=None)),
    "n 0": (SHAPE, lambda s: dict(n=0)),
    "n negative": (SHAPE, lambda s: dict(n=-4)),
    "n 6": (SHAPE, lambda s: dict(n=6)),
    "p 4 bytes off": (ALIGN, lambda s: dict(p=s["p_off"].data_ptr())),
    "g 4 bytes off": (ALIGN, lambda s: dict(g=s["g_off"].data_ptr())),
    "v 4 bytes off": (ALIGN, lambda s: dict(v=s["v_off"].data_ptr())),
    "ema 4 bytes off": (ALIGN, lambda s: dict(ema=s["ema_off"].data_ptr())),
    "bc2 0": (SHAPE, lambda s: dict(bc2=0.0)),
    "bc2 negative": (SHAPE, lambda s: dict(bc2=-0.5)),
    "bc2 NaN": (SHAPE, lambda s: dict(bc2=float("nan"))),
}


@pytest.mark.parametrize("fault", sorted(REFUSALS))
def test_adam_ema_refusals_leave_the_buffers_alone(L, fault):
    """One fault at a time in an otherwise valid call of n = 8 (the misaligned pointers lie inside their own 9-float allocations):
    the documented code, and no buffer changed -- the check came before the launch."""
    n = 8
    host = dict(zip(("p", "g", "v", "ema"), R.adam_case(n, 3)))
    s = {k: _dev(t) for k, t in host.items()}
    s.update({k + "_off": _dev(t, off=1) for k, t in host.items()})
    code, edit = REFUSALS[fault]
    assert _call(L, s["p"], s["g"], s["v"], s["ema"], n, 7, edit(s)) == code
    for k, t in host.items():
        assert torch.equal(s[k].cpu().view(torch.int32), t.view(torch.int32)), (fault, k)
        assert torch.equal(s[k + "_off"].cpu().view(torch.int32), t.view(torch.int32)), (fault, k)
    if fault == sorted(REFUSALS)[0]:
        assert _call(L, s["p"], s["g"], s["v"], s["ema"], n, 7) == 0       # and without a fault the same call is accepted
        assert not torch.equal(s["p"].cpu(), host["p"])
