"""ideas_linear_fwd / _bwd_x / _bwd_w (csrc/linear.hip) through the C ABI on raw buffers, against the float64 restatements of
tests/linear_ref.py: the segment table up to IDEAS_LINEAR_MAX_SEGMENTS, every row stride (ldx / ldw / ldy / ldgw / ldgx) larger than
the row, ``accumulate`` on and off, the caller-sized workspace, and every refusal -- what op/linear.py, which always passes dense
tensors, never asks of the kernels.

Every matrix lives in a [rows][ld] buffer whose padding columns hold a sentinel bit pattern (a quiet NaN: read as data it poisons
the sum, written over it shows); after every call the padding of EVERY operand, inputs included, and 256 bytes behind the workspace
are compared bitwise with it.  Outputs start as the sentinel too, so an element the kernel does not write fails.

Each case (linear_ref.CASES, the smallest shapes that reach each branch) runs with two kinds of data:
  exact   integers in [-4, 4], power-of-two scales: the result must EQUAL the reference (tests/test_linear_ref.py shows a correct
          float32 kernel can).  A dropped, doubled or misplaced term, a wrong row clamp or a wrong stride cannot pass.
  random  N(0, 1): |got - ref| <= gamma(3 T + 80) S per element (linear_ref.bound), T = the terms of the sum: derived, not measured.
and twice: the two runs must agree bit for bit (fixed summation order, no atomics).

Largest error / bound seen on an MI355X (printed per case and at the end of the module):
    fwd 0.020, bwd_x 0.026, bwd_w 0.033 (gw) / 0.011 (gb); every exact case equal.  The whole file runs in about a second.
"""
import ctypes as C

import pytest
import torch

import linear_ref as R

pytestmark = pytest.mark.gpu
SENT = 0x7FC5A5A5           # a quiet NaN with a recognisable payload
TAIL = 256                  # sentinel bytes behind the workspace
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


class _Mat:
    """``data`` [rows][cols] inside a [rows][ld] float32 device buffer (``off`` floats behind its 256-byte aligned start); everything
    else holds SENT.  Without data the matrix itself is SENT as well (an output, or the NaN the non-accumulating gradient must not
    read)."""

    def __init__(self, rows, cols, ld=None, data=None, off=0):
        self.rows, self.cols, self.ld, self.data = rows, cols, ld or cols, data
        self.bits = torch.empty(off + rows * self.ld, dtype=torch.int32, device="cuda")
        self.grid = self.bits[off:].view(rows, self.ld)
        self.t = self.grid.view(torch.float32)[:, :cols]
        self.reset()
        assert self.ptr % 16 == (4 * off) % 16

    def reset(self):
        self.bits.fill_(SENT)
        if self.data is not None:
            self.t.copy_(self.data.view(self.rows, self.cols))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def pad_intact(self):
        return bool((self.grid[:, self.cols:] == SENT).all()) and bool((self.bits[:self.bits.numel() - self.grid.numel()] == SENT).all())

    def untouched(self):
        """bitwise what reset() left"""
        if self.data is None:
            return bool((self.bits == SENT).all())
        return self.pad_intact() and torch.equal(self.t.cpu().view(torch.int32), self.data.view(self.rows, self.cols).view(torch.int32))

    def host(self):
        return self.t.cpu().clone()


def _vec(data=None, n=None):
    """a vector (bias, bias gradient) with 4 sentinel floats behind it"""
    n = data.numel() if data is not None else n
    return _Mat(1, n, n + 4, data)


class _Setup:
    """The device operands of one case: x, per segment w / bias / y (output or incoming gradient) / gw / gb, gx and the workspace;
    ``table()`` builds the segment array from them.  ``pad(name, i)`` = the case's stride padding."""

    def __init__(self, L, c, entry, accumulate=False):
        self.L, self.c, self.entry = L, c, entry
        sp = c.spec
        pad = lambda key, i=None: (sp.get(key, 0) if i is None else sp.get(key, (0,) * len(c.ns))[i])
        M, K = c.M, c.K
        self.x = _Mat(M, K, K + pad("padx"), c.x)
        self.w, self.b, self.y, self.gw, self.gb = [], [], [], [], []
        for i, (s, n) in enumerate(zip(c.segs, c.ns)):
            self.w.append(_Mat(n, K, K + pad("padw", i), s.w))
            self.b.append(None if s.b is None else _vec(s.b))
            self.y.append(_Mat(M, n, n + pad("pady", i), None if entry == "fwd" else s.g))
            if entry == "bwd_w":
                self.gw.append(_Mat(n, K, K + pad("padgw", i), c.old[i][0] if accumulate else None))
                self.gb.append(None if s.b is None else _vec(c.old[i][1] if accumulate else None, n))
        self.gx = self.ws = None
        if entry == "bwd_x":
            self.gx = _Mat(M, K, K + pad("padgx"))
            self.ws_bytes = int(L.load().ideas_linear_bwd_x_workspace(sum(c.ns), M, K))
            assert self.ws_bytes > 0 and self.ws_bytes % 16 == 0
            self.ws = _Mat(1, self.ws_bytes // 4, (self.ws_bytes + TAIL) // 4)
        self.seg = self.table()

    def table(self, count=None):
        count = count or len(self.c.ns)
        sg = (self.L.LinearSeg * count)()
        for j in range(count):
            i = j % len(self.c.ns)
            s = self.c.segs[i]
            sg[j].w, sg[j].y = self.w[i].ptr, self.y[i].ptr
            sg[j].bias = None if self.b[i] is None or self.entry != "fwd" else self.b[i].ptr
            sg[j].n, sg[j].ldw, sg[j].ldy = self.c.ns[i], self.w[i].ld, self.y[i].ld
            sg[j].scale, sg[j].bias_mul = s.scale, s.bias_mul
            sg[j].tile0, sg[j].pad_ = -12345, 777                   # scratch of the library: any value
            if self.entry == "bwd_w":
                sg[j].gw, sg[j].ldgw = self.gw[i].ptr, self.gw[i].ld
                sg[j].gb = None if self.gb[i] is None else self.gb[i].ptr
        return sg

    def everything(self):
        return [self.x] + self.w + [b for b in self.b if b is not None] + self.y + self.gw + [g for g in self.gb if g is not None] + \
            [m for m in (self.gx, self.ws) if m is not None]

    def outputs(self):
        return {"fwd": self.y, "bwd_x": [self.gx, self.ws], "bwd_w": self.gw + [g for g in self.gb if g is not None]}[self.entry]

    def call(self, accumulate=0, **over):
        """the entry point with this setup's arguments, any of them replaced by ``over``"""
        lib, c = self.L.load(), self.c
        a = dict(segs=self.seg, nseg=len(self.seg), x=self.x.ptr, M=c.M, K=c.K, ldx=self.x.ld)
        if self.entry == "bwd_x":
            a.update(gx=self.gx.ptr, ldgx=self.gx.ld, ws=self.ws.ptr, ws_bytes=self.ws_bytes)
        a.update(over)
        st = self.L.stream_ptr()
        if self.entry == "fwd":
            rc = lib.ideas_linear_fwd(a["segs"], a["nseg"], a["x"], a["M"], a["K"], a["ldx"], st)
        elif self.entry == "bwd_x":
            rc = lib.ideas_linear_bwd_x(a["segs"], a["nseg"], a["gx"], a["M"], a["K"], a["ldgx"], a["ws"], a["ws_bytes"], st)
        else:
            rc = lib.ideas_linear_bwd_w(a["segs"], a["nseg"], a["x"], a["M"], a["K"], a["ldx"], accumulate, st)
        torch.cuda.synchronize()
        return rc


def _judge(tag, kind, got, ref, S, terms):
    """exact: equality with the float64 reference; random: the elementwise summation bound.  -> error / bound"""
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), tag
    if kind == "exact":
        bad = (got.double() != ref).nonzero()
        assert bad.numel() == 0, (tag, "first differing element", bad[0].tolist(), "of", int(bad.shape[0]))
        return 0.0
    err, bnd = (got.double() - ref).abs(), R.bound(terms, S)
    ratio = float((err / bnd.clamp_min(1e-300)).max())
    key = tag.split(" ")[0]
    RATIO[key] = max(RATIO.get(key, 0.0), ratio)
    assert bool((err <= bnd).all()), (tag, "worst error / bound", ratio)
    return ratio


def _run_twice(su, outs, accumulate=0):
    """two calls from the same start: status 0, no padding touched, bitwise the same results -> the first run's results"""
    res = []
    for run in range(2):
        for m in su.everything():
            m.reset()
        assert su.call(accumulate) == 0
        assert all(m.pad_intact() for m in su.everything()), "a padding column, or the tail behind the workspace, was written"
        res.append([m.host() for m in outs])
    for a, b in zip(*res):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two runs differ: the summation order is not fixed"
    return res[0]


@pytest.mark.parametrize("name,kind", R.PARAMS["fwd"])
def test_fwd(L, name, kind):
    c = R.make_case("fwd", name, kind)
    su = _Setup(L, c, "fwd")
    got = _run_twice(su, su.y)
    worst = max(_judge("fwd %s seg %d" % (name, i), kind, g, y, S, c.K) for i, (g, (y, S)) in enumerate(zip(got, R.fwd(c.x, c.segs))))
    print("fwd", name, kind, "worst error / bound", worst)


def _splits(L, c):
    """(splits, groups, [group range of every split]) of the launcher's plan, from the workspace size alone"""
    nbytes = int(L.load().ideas_linear_bwd_x_workspace(sum(c.ns), c.M, c.K))
    mtiles, groups = (c.M + 31) // 32, sum(c.ns) // 8
    splits = nbytes // (mtiles * 32 * c.K * 4)
    assert splits * mtiles * 32 * c.K * 4 == nbytes and 1 <= splits <= groups
    return splits, groups, [(sp * groups // splits, (sp + 1) * groups // splits) for sp in range(splits)]


@pytest.mark.parametrize("name,kind", R.PARAMS["bwd_x"])
def test_bwd_x(L, name, kind):
    c = R.make_case("bwd_x", name, kind)
    splits, groups, ranges = _splits(L, c)
    if name == "m33_k520_n8_24":
        assert splits == groups == 4
    if name == "m256_k4096_n8_16_40_8":
        # the case is here for a split whose groups belong to two segments: make sure the plan still has one
        edges = [sum(c.ns[:i]) // 8 for i in range(1, len(c.ns))]
        assert any(g0 < e < g1 for g0, g1 in ranges for e in edges), (splits, ranges, edges)
    if name == "m260_k4096_n8_8":
        assert splits == 2 and c.M * (c.K // 4) > 1024 * 256          # more float4 than the fold kernel's largest grid has threads
    su = _Setup(L, c, "bwd_x")
    (got, _), (ref, S) = _run_twice(su, [su.gx, su.ws]), R.bwd_x(c.segs)
    print("bwd_x", name, kind, "splits", splits, "worst error / bound", _judge("bwd_x %s" % name, kind, got, ref, S, sum(c.ns)))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("name,kind", R.PARAMS["bwd_w"])
def test_bwd_w(L, name, kind, accumulate):
    """accumulate = 0 onto NaN: the plain gradient (the old contents are not read); accumulate = 1: old + gradient."""
    c = R.make_case("bwd_w", name, kind)
    su = _Setup(L, c, "bwd_w", bool(accumulate))
    gbs = [g for g in su.gb if g is not None]
    got = _run_twice(su, su.gw + gbs, accumulate)
    ref = R.bwd_w(c.x, c.segs, c.old, bool(accumulate))
    worst, gb_got = 0.0, iter(got[len(su.gw):])
    for i, ((gw, Sw), gb) in enumerate(ref):
        worst = max(worst, _judge("bwd_w_gw %s seg %d acc %d" % (name, i, accumulate), kind, got[i], gw, Sw, c.M))
        assert (gb is None) == (su.gb[i] is None)
        if gb is not None:
            worst = max(worst, _judge("bwd_w_gb %s seg %d acc %d" % (name, i, accumulate), kind, next(gb_got).view(-1), gb[0], gb[1], c.M))
    print("bwd_w", name, kind, "accumulate", accumulate, "worst error / bound", worst)


# ------------------------------------------------------------------------------------------------------------------ refusals
NULL, SHAPE, ALIGN = -1, -2, -4
REFUSE_CASE = {"fwd": "m33_k24_n7_33_64", "bwd_x": "m33_k520_n8_24", "bwd_w": "m7_k520_n33_8"}


def _seg_edit(su, i, count=None, **fields):
    sg = su.table(count)
    for k, v in fields.items():
        setattr(sg[i], k, v)
    return dict(segs=sg, nseg=len(sg))


def _off4(su, like):
    """a copy of ``like`` that starts 4 bytes behind a 16-byte boundary, inside its own allocation"""
    m = _Mat(like.rows, like.cols, like.ld, like.data, off=1)
    su.keep = getattr(su, "keep", []) + [m]
    return m


REFUSALS = {
    "fwd": {
        "segs NULL": (NULL, lambda su: dict(segs=None)),
        "nseg 0": (SHAPE, lambda su: dict(nseg=0)),
        "nseg 33": (SHAPE, lambda su: _seg_edit(su, 0, count=33)),
        "n 0": (SHAPE, lambda su: _seg_edit(su, 1, n=0)),
        "n negative": (SHAPE, lambda su: _seg_edit(su, 2, n=-8)),
        "w NULL": (NULL, lambda su: _seg_edit(su, 1, w=None)),
        "w 4 bytes off": (ALIGN, lambda su: _seg_edit(su, 1, w=_off4(su, su.w[1]).ptr)),
        "ldw % 4": (ALIGN, lambda su: _seg_edit(su, 2, ldw=su.w[2].ld + 2)),
        "y NULL": (NULL, lambda su: _seg_edit(su, 2, y=None)),
        "x NULL": (NULL, lambda su: dict(x=None)),
        "M 0": (SHAPE, lambda su: dict(M=0)),
        "M negative": (SHAPE, lambda su: dict(M=-1)),
        "K % 8": (ALIGN, lambda su: dict(K=su.c.K - 4)),
        "ldx % 4": (ALIGN, lambda su: dict(ldx=su.x.ld + 2)),
        "K 0": (SHAPE, lambda su: dict(K=0)),
        "x 4 bytes off": (ALIGN, lambda su: dict(x=_off4(su, su.x).ptr)),
    },
    "bwd_x": {
        "n % 8": (ALIGN, lambda su: _seg_edit(su, 1, n=20)),
        "ldy % 4": (ALIGN, lambda su: _seg_edit(su, 1, ldy=su.y[1].ld + 2)),
        "g 4 bytes off": (ALIGN, lambda su: _seg_edit(su, 0, y=_off4(su, su.y[0]).ptr)),
        "K % 4": (ALIGN, lambda su: dict(K=su.c.K - 2)),
        "ldgx % 4": (ALIGN, lambda su: dict(ldgx=su.gx.ld + 2)),
        "gx NULL": (NULL, lambda su: dict(gx=None)),
        "workspace NULL": (NULL, lambda su: dict(ws=None)),
        "workspace one byte short": (SHAPE, lambda su: dict(ws_bytes=su.ws_bytes - 1)),
        "segs NULL": (NULL, lambda su: dict(segs=None)),
        "nseg 33": (SHAPE, lambda su: _seg_edit(su, 0, count=33)),
        "w NULL": (NULL, lambda su: _seg_edit(su, 1, w=None)),
        "ldw % 4": (ALIGN, lambda su: _seg_edit(su, 0, ldw=su.w[0].ld + 2)),
        "g NULL": (NULL, lambda su: _seg_edit(su, 1, y=None)),
        "M 0": (SHAPE, lambda su: dict(M=0)),
        "K 0": (SHAPE, lambda su: dict(K=0)),
        "gx 4 bytes off": (ALIGN, lambda su: dict(gx=_off4(su, su.gx).ptr)),
        "workspace 4 bytes off": (ALIGN, lambda su: dict(ws=su.ws.ptr + 4)),
    },
    "bwd_w": {
        "gw NULL": (NULL, lambda su: _seg_edit(su, 1, gw=None)),
        "ldgw % 4": (ALIGN, lambda su: _seg_edit(su, 0, ldgw=su.gw[0].ld + 2)),
        "gw 4 bytes off": (ALIGN, lambda su: _seg_edit(su, 1, gw=_off4(su, su.gw[1]).ptr)),
        "K % 4": (ALIGN, lambda su: dict(K=su.c.K - 2)),
        "x NULL": (NULL, lambda su: dict(x=None)),
        "nseg 0": (SHAPE, lambda su: dict(nseg=0)),
        "n 0": (SHAPE, lambda su: _seg_edit(su, 0, n=0)),
        "g NULL": (NULL, lambda su: _seg_edit(su, 0, y=None)),
        "M 0": (SHAPE, lambda su: dict(M=0)),
        "ldx % 4": (ALIGN, lambda su: dict(ldx=su.x.ld + 2)),
        "x 4 bytes off": (ALIGN, lambda su: dict(x=_off4(su, su.x).ptr)),
    },
}


@pytest.fixture(scope="module")
def refusal_setups(L):
    return {e: _Setup(L, R.make_case(e, n, "exact"), e) for e, n in REFUSE_CASE.items()}


@pytest.mark.parametrize("entry,fault", [(e, f) for e in ("fwd", "bwd_x", "bwd_w") for f in REFUSALS[e]])
def test_refusals_come_before_any_launch(L, refusal_setups, entry, fault):
    """One fault at a time in an otherwise valid call: the documented code, and every buffer bitwise as it was (outputs and the
    workspace still the sentinel) -- no kernel ran.  The faulty operand is only ever passed to a call that must be refused."""
    su = refusal_setups[entry]
    code, edit = REFUSALS[entry][fault]
    for m in su.everything():
        m.reset()
    for accumulate in ((0, 1) if entry == "bwd_w" else (0,)):
        assert su.call(accumulate, **edit(su)) == code, fault
    assert all(m.untouched() for m in su.everything()), fault
    assert all(bool((m.bits == SENT).all()) for m in su.outputs()), fault


@pytest.mark.parametrize("entry", ["fwd", "bwd_x", "bwd_w"])
def test_refusal_setup_is_valid_without_the_fault(L, refusal_setups, entry):
    """the same call with nothing wrong is accepted: each refusal above is due to its one fault"""
    su = refusal_setups[entry]
    for m in su.everything():
        m.reset()
    assert su.call(0) == 0
    assert all(m.pad_intact() for m in su.everything())
    assert not any(bool((m.t.view(torch.int32) == SENT).any()) for m in su.outputs() if m is not su.ws)


def test_workspace_size_refuses_and_table_layout(L):
    lib = L.load()
    assert lib.ideas_sizeof_linear_seg() == C.sizeof(L.LinearSeg) and L.LINEAR_MAX_SEGMENTS == 32
    for bad in ((0, 4, 8), (8, 0, 8), (8, 4, 0), (-8, 4, 8)):
        assert lib.ideas_linear_bwd_x_workspace(*bad) == 0
