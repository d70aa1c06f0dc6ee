"""GPU: the derived-weight forms of csrc/weight_prep.hip against a CPU restatement of their written contract (include/ideas_hip.h),
byte for byte, through every route that makes them: ideas_weight_prep, the single-tensor entry points, ideas_weight_prep_batched.

The restatements are torch on the CPU, one rounding per step as the contract says (round-to-nearest-even throughout):
  split planes    hi = bf16(w), mid = bf16(w - hi), lo = bf16((w - hi) - mid) in f32, at [pl][(ci//16)*taps + tap][n][ci%16]
  bf16 pack       bf16(w * scale[b, ci]) (one f32 multiply; bf16(w) without a scale) at [b][(ci//32)*taps + tap][n][32], the 8-element
                  chunk c of a row stored at c ^ ((n >> 2) & 3)
  Winograd planes U = (w0, ((w0 + w2) + w1) / 2, ((w0 + w2) - w1) / 2, w2) over kx in f64, then h = bf16(f32(U)), m = bf16(f32(U - h)),
                  l = bf16(f32((U - h) - m)) with the residuals in f64, at [v][pl][(c//16)*3 + ky][n][c%16]
Each reads the matrix from flat CPU memory through the same (dims, strides, offset) the kernel is given, so no torch view is trusted.
Inputs: magnitudes in [2^-60, 2^60) plus exact and signed zeros; no f32 subnormal arises anywhere (the device may flush those:
tests/test_ops_gpu.py::test_b3_weight_split_is_exact_and_step_major covers that exclusion).  The whole destination is compared, written
over a guard pattern inside guard bands."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

B3, WINO, PACK = 0, 1, 2            # IDEAS_PREP_*
GUARD = 64                          # bf16 elements on either side of a destination (a multiple of 8: the destination stays 16-byte aligned)
PATTERN = 0x7A5C                    # a bf16 near 2.9e35 (2^117): no value made from magnitudes below 2^61 has these bits


# ------------------------------------------------------------------------------------------------- inputs
def flat_input(numel, seed):
    """Seeded on the CPU: random sign, mantissa in [1, 2), exponent in [-60, 60): a base per 1024-element block (so that neighbouring
    taps are mostly of one magnitude and the Winograd sums are real sums) plus a jitter of +-2; one element in 64 an exact zero, half of
    them negative."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(-58, 58, ((numel + 1023) // 1024,), generator=g).repeat_interleave(1024)[:numel]
    e = (base + torch.randint(-2, 3, (numel,), generator=g)).clamp(-60, 59)
    w = torch.ldexp(1.0 + torch.rand(numel, generator=g), e)
    w = torch.where(torch.rand(numel, generator=g) < 0.5, -w, w)
    z = torch.rand(numel, generator=g) < 1.0 / 64
    w[z] = torch.where(torch.rand(int(z.sum()), generator=g) < 0.5, -0.0, 0.0)
    assert w.dtype == torch.float32 and float(w[~z].abs().min()) >= 2.0 ** -60 and float(w.abs().max()) < 2.0 ** 60
    return w


def gather(flat, dims, strides, offset):
    """[N][TY][TX][C] matrix whose element (n, ty, tx, c) is flat[offset + n*sn + ty*sty + tx*stx + c*sc]; every index inside `flat`."""
    idx = torch.tensor(offset)
    for d, s in zip(dims, strides):
        idx = idx.unsqueeze(-1) + torch.arange(d) * s
    assert int(idx.min()) >= 0 and int(idx.max()) < flat.numel(), (dims, strides, offset, flat.numel())
    return flat[idx]


# ------------------------------------------------------------------------------------------------- the contract, on the CPU
def bits(t):
    return t.contiguous().view(torch.int16).flatten()


def oracle_b3(m, scale=None):
    n, ty, tx, c = m.shape
    hi = m.bfloat16()
    r = m - hi.float()
    mid = r.bfloat16()
    lo = (r - mid.float()).bfloat16()
    p = torch.stack((hi, mid, lo)).view(3, n, ty * tx, c // 16, 16)
    return bits(p.permute(0, 3, 2, 1, 4))


def oracle_pack(m, scale=None):
    n, ty, tx, c = m.shape
    x = m[None] if scale is None else m[None] * scale[:, None, None, None, :]
    p = x.bfloat16().view(-1, n, ty * tx, c // 32, 4, 8)
    out = torch.empty(p.shape[0], c // 32, ty * tx, n, 4, 8, dtype=torch.bfloat16)
    rows = torch.arange(n)
    for chunk in range(4):
        out[:, :, :, rows, chunk ^ ((rows >> 2) & 3)] = p[:, :, :, :, chunk].permute(0, 3, 2, 1, 4)
    return bits(out)


def oracle_wino(m, scale=None):
    n, _, _, c = m.shape                              # [N][ky][kx][C]
    w0, w1, w2 = (m[:, :, k].double() for k in range(3))
    s = w0 + w2
    u = torch.stack((w0, (s + w1) / 2, (s - w1) / 2, w2))
    h = u.float().bfloat16()
    r = u - h.double()
    mid = r.float().bfloat16()
    lo = (r - mid.double()).float().bfloat16()
    p = torch.stack((h, mid, lo), 1).view(4, 3, n, 3, c // 16, 16)
    return bits(p.permute(0, 1, 4, 3, 2, 5))


ORACLE = {B3: oracle_b3, WINO: oracle_wino, PACK: oracle_pack}


# ------------------------------------------------------------------------------------------------- jobs and routes
class Job:
    """One matrix of one form: `dims` read through `strides` from element `offset` of the flat device buffer `dev` (`flat` on the
    CPU); the Winograd form's kernel size is implied and its fifth stride (the base offset) is 0: `offset` is in the pointer."""

    def __init__(self, op, name, flat, dev, dims, strides, offset=0, scale=None):
        self.op, self.name, self.dev, self.strides, self.offset = op, name, dev, tuple(strides), offset
        self.dims = tuple(dims)
        self.a = (dims[0], dims[3]) if op == WINO else self.dims
        self.scale = scale
        self.want = ORACLE[op](gather(flat, dims, strides, offset), None if scale is None else scale.cpu())
        self.w = dev.data_ptr() + 4 * offset
        # a dense [Cout][K] matrix on a 16-byte boundary: what ideas_b3_split_weights / ideas_bf16_pack_weights take
        k = dims[1] * dims[2] * dims[3]
        self.dense = op != WINO and self.strides == (k, dims[2] * dims[3], dims[3], 1) and self.w % 16 == 0

    def desc(self, lib, dst=0):
        from ideas_amd import _lib
        d = _lib.PrepDesc(dst=dst, w=self.w, s=self.strides, a=self.a)
        numel = C.c_int64()
        _lib.check(lib.ideas_weight_prep_plan(C.byref(d), self.op, C.byref(numel)), "ideas_weight_prep_plan")
        assert numel.value * (1 if self.scale is None else self.scale.shape[0]) == self.want.numel()
        return d


def guarded(numel):
    buf = torch.full((numel + 2 * GUARD,), PATTERN, device="cuda", dtype=torch.int16)
    assert (buf.data_ptr() + 2 * GUARD) % 16 == 0
    return buf


def check_bytes(buf, job, route):
    got = buf.cpu()
    assert bool((got[:GUARD] == PATTERN).all()) and bool((got[-GUARD:] == PATTERN).all()), (job.name, route, "guard band written")
    got = got[GUARD:-GUARD]
    if not torch.equal(got, job.want):
        bad = (got != job.want).nonzero().flatten()
        raise AssertionError((job.name, route, f"{bad.numel()} of {got.numel()} bf16 differ, first at {int(bad[0])}: "
                              f"{int(got[bad[0]]) & 0xffff:#06x} != {int(job.want[bad[0]]) & 0xffff:#06x}; "
                              f"{int((got == PATTERN).sum())} still hold the guard pattern"))


def run_routes(jobs):
    """Every job of one form through every route there is for it; all must give the oracle's bytes."""
    from ideas_amd import _lib
    lib, st = _lib.load(), _lib.stream_ptr()
    op = jobs[0].op
    units = set()
    for j in jobs:
        nb = 1 if j.scale is None else j.scale.shape[0]
        sp = _lib.ptr(j.scale)
        routes = {}
        d0 = j.desc(lib)
        units.add(d0.unit)

        def entry(dst, d0=d0):
            d0.dst = dst
            return lib.ideas_weight_prep(C.byref(d0), op, sp, nb, st)
        routes["ideas_weight_prep"] = entry
        if op == B3:
            routes["strided"] = lambda dst: lib.ideas_b3_split_weights_strided(dst, j.w, *j.dims, *j.strides, st)
            if j.dense:
                routes["dense"] = lambda dst: lib.ideas_b3_split_weights(dst, j.w, j.dims[0], j.strides[0], j.dims[3], st)
        elif op == PACK:
            routes["strided"] = lambda dst: lib.ideas_bf16_pack_weights_strided(dst, j.w, sp, nb, *j.dims, *j.strides, st)
            if j.dense:
                routes["dense"] = lambda dst: lib.ideas_bf16_pack_weights(dst, j.w, sp, nb, j.dims[0], j.strides[0], j.dims[3], st)
        else:
            routes["legacy"] = lambda dst: lib.ideas_b3_wino_split_weights(dst, j.w, *j.a, *j.strides, 0, st)
            # the same matrix with the offset passed as `base` instead of in the pointer
            routes["legacy, base"] = lambda dst: lib.ideas_b3_wino_split_weights(dst, j.dev.data_ptr(), *j.a, *j.strides, j.offset, st)
        for name, fn in routes.items():
            buf = guarded(j.want.numel())
            _lib.check(fn(buf.data_ptr() + 2 * GUARD), name)
            check_bytes(buf, j, name)
    plain = [j for j in jobs if j.scale is None]          # (the table takes no scale)
    if not plain:
        return units
    bufs = [guarded(j.want.numel()) for j in plain]
    table = (_lib.PrepDesc * len(plain))()
    block0 = 0
    for i, (j, buf) in enumerate(zip(plain, bufs)):
        d = j.desc(lib, buf.data_ptr() + 2 * GUARD)
        d.block0 = block0
        block0 += d.nblocks
        table[i] = d
    dev_table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    _lib.check(lib.ideas_weight_prep_batched(dev_table.data_ptr(), len(plain), op, block0, st), "ideas_weight_prep_batched")
    for j, buf in zip(plain, bufs):
        check_bytes(buf, j, "ideas_weight_prep_batched")
    return units


def matrix_views(op, shape, seed, scale=None):
    """The [Cout][TY][TX][Cin] matrix of one shape read through the stride sets the callers make (op/conv_plan.py) and the ones on
    either side of the 16-byte rule, each with values of its own."""
    co, ty, tx, ci = shape
    k = ty * tx * ci
    flat = flat_input(4 * co * k + 8 * co + 64, seed)
    dev = flat.cuda()
    mk = lambda name, strides, offset=0: Job(op, f"{shape} {name}", flat, dev, shape, strides, offset, scale)
    return [
        mk("OHWI parameter", (k, tx * ci, ci, 1)),                                                # unit
        mk("NCHW parameter", (k, tx, 1, ty * tx)),
        # plan_dgrad: w[:, :, cy::2, cx::2].permute(1, 2, 3, 0) of an OHWI-stored [O = Cin, I = Cout, 2 TY, 2 TX] parameter, cy = cx = 1
        mk("dgrad phase slice", (1, 4 * tx * co, 2 * co, 4 * k // ci * co), 2 * tx * co + co),
        mk("transposed parameter", (1, tx * co, co, k // ci * co)),                              # OHWI-stored [Cin, Cout, TY, TX] read as [O, I]
        mk("OHWI, one float behind a 16-byte boundary", (k, tx * ci, ci, 1), 1),
        mk("OHWI rows of K + 1 floats", (k + 1, tx * ci, ci, 1)),                                # sn no multiple of 4
    ]


def wino_views(o, i, seed):
    flat = flat_input(9 * o * i, seed)
    dev = flat.cuda()
    jobs = []
    if i % 16 == 0:       # forward matrix of the OHWI parameter, n = o, c = i; the same from NCHW memory
        jobs.append(Job(WINO, f"wino {o}x{i} forward", flat, dev, (o, 3, 3, i), (9 * i, 3 * i, i, 1)))
        jobs.append(Job(WINO, f"wino {o}x{i} forward, NCHW", flat, dev, (o, 3, 3, i), (9 * i, 3, 1, 9)))
    if o % 16 == 0:       # flipped, transposed matrix of the input gradient, n = i, c = o
        jobs.append(Job(WINO, f"wino {o}x{i} flipped + transposed", flat, dev, (i, 3, 3, o), (1, -3 * i, -i, 9 * i), 8 * i))
    return jobs


# ------------------------------------------------------------------------------------------------- cases
# non-square taps, two or more chunks, Cout no multiple of 4; the last of each form runs every thread's item loop twice
# (more than 2048 * 256 work items)
B3_SHAPES = [(5, 1, 1, 16), (24, 1, 3, 48), (7, 3, 3, 32)]
PACK_SHAPES = [(5, 1, 1, 32), (24, 1, 3, 96), (7, 3, 3, 32)]


@pytest.mark.parametrize("shape", B3_SHAPES)
def test_split_planes_are_the_contract_on_every_route(shape):
    assert run_routes(matrix_views(B3, shape, sum(shape))) == {0, 1}


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("shape", PACK_SHAPES)
def test_bf16_packs_are_the_contract_on_every_route(shape, scaled):
    scale = (torch.rand(3, shape[3], generator=torch.Generator().manual_seed(7)) + 0.5).cuda() if scaled else None
    assert run_routes(matrix_views(PACK, shape, sum(shape) + 1, scale)) == {0, 1}


@pytest.mark.parametrize("oi", [(5, 16), (16, 7), (48, 32)])
def test_winograd_planes_are_the_contract_on_every_route(oi):
    assert run_routes(wino_views(*oi, seed=sum(oi))) == {0}


@pytest.mark.parametrize("op, shape", [(B3, (512, 3, 3, 512)), (PACK, (1024, 3, 3, 512)), (WINO, (1024, 3, 3, 1024))])
def test_item_loops_that_run_twice(op, shape):
    co, ty, tx, ci = shape
    flat = flat_input(co * ty * tx * ci, 5)
    dev = flat.cuda()
    k = ty * tx * ci
    jobs = [Job(op, f"{shape} OHWI", flat, dev, shape, (k, tx * ci, ci, 1)),
            Job(op, f"{shape} NCHW", flat, dev, shape, (k, tx, 1, ty * tx))]
    from ideas_amd import _lib
    for j in jobs:
        assert j.desc(_lib.load()).nblocks == 2048 and j.want.numel() // {B3: 3, WINO: 12, PACK: 1}[op] // (4 if op != PACK else 8) > 2048 * 256
    run_routes(jobs)
