"""Memory footprint of the convolution launchers at ragged tiles: no store outside the output, no load outside the operands.

Every other conv test lets ``conv_*_raw`` allocate its output with ``torch.empty`` and compares only that tensor, so a ragged last
tile that stores a few rows past ``B * OH * OW``, a parity phase that touches a pixel of another parity, or a buffer-descriptor
range that is a tile too long would land in the caching allocator's slack and pass.  Here every operand of a launch lives inside
a larger buffer of the test's own (tests/conv_bounds.py): outputs between bands of a NaN bit pattern (plain stores) or of a small
finite pattern (atomics), inputs -- the derived weights the launchers fetch themselves included, through monkeypatched
``b3_planes`` / ``bf16_pack`` / ``b3_wino_planes`` -- between NaN bands.  After the launch

* the bands around every output are bit-identical to a copy taken before it, and so is every pixel no phase owns;
* every input buffer, bands and payload, is bit-identical to before;
* the output is finite, ``torch.equal`` to the same launch on ordinary tensors, and within the suite's bound of an f64
  reference made with torch.nn.functional on the CPU (f32: rel_err < TOL forward / GTOL gradients of test_ops_gpu.py; bf16:
  close_bf16 of test_bf16_gpu.py on bf16-exact operands).  Weight gradients are compared bitwise only where the split-K plan has
  a single split (otherwise the order of the f32 atomics differs from run to run).

The checker is shown to see what it claims to see, inside the tensors: the band comparison run as if the payload ended one
pixel-row early must report a violation (write side), and a NaN in the last pixel-row of x that the geometry reads / in the
last output-channel row of the weights (weight gradients: the last pixel-row of gy) must make the output non-finite (read side:
the family's load path propagates a NaN instead of masking it, the premise of the NaN input bands).  No family fails that by
design.  All operands are 16-byte aligned; misaligned pointers are only handed to the entry points that refuse them (-4, no launch).

Families, the kernel or tile each case asserts (predicates and environments of test_b3_pinned_gpu.py and
test_conv_epilogue_pinned_gpu.py, ideas_bf16_fwd_choice, ideas_b3_wino_n256_tiles, the *_supported queries) and the ragged
dimension it exercises:

  conv_igemm.hip     f32 MFMA forward, 128 x 32 / 128 x 64 / 128 x 128 tiles: M = 35 of 128, Cout 20 / 44 / 132 (second N tile 4
                     wide), Cin 4 (< BK) and 36; f32 weight gradient, OW >= BK and OW < BK, Cout 36 x Cin 20
  conv_direct.hip    VALU direct f32 (Cin 3, 6) and its weight gradient (Cin 3); bf16 pointwise smallk_vec 3 -> 40, rowdot 40 -> 3
  conv_b3.hip        split-bf16 generic, 16 -> 80 and the 64-channel N tile at Cout 132, M = 20 of 128; the multi kernel (Cout <= 64);
                     one parity phase alone; the phase of a 1x1 / stride-2 input gradient whose other pixels nobody owns
  conv_b3_pw.hip     flat 1x1 and its K-chunked form with the residual, M = 378 / 70 rows; the flat weight gradient, 529 pixels
  conv_b3_s2fir.hip  LDS-image kernel 17 x 33 -> 8 x 16 and 19 x 37 -> 9 x 18 (no multiple of the 8 x 16 patch), N tiles 64 / 128 / 256
                     at Cout 64 / 132 / 260; Blur + stride-2 at the same sizes with and without the side output, modulated too
  conv_b3_tphase.hip 16 -> 128 on 4 x 16 and 32 -> 192 on 5 x 18, 16-byte and 4-byte stores
  conv_b3_wino.hip   4-wave tile on 5 x 6 and 7 x 18, 8-wave tile on 7 x 18, row-sharing kernel on 8 x 16 at Cout 128, its 256-channel
                     tile at Cout 256; transposed; mirror padding; the generic tail
  conv_wino.hip      f32 Winograd 8 -> 12 on 5 x 6 (forward, transposed), its weight gradient with the fold into a strided target
  conv_b3_wgrad.hip  Cout 72, OW 4 (256 input channels: below, the dispatch keeps the f32 kernel)
  conv_b3_wgrad3.hip tap-fused stride 1 and 2, 64 -> 64 and 64 -> 128 at 16 x 16
  conv_bf16.hip      Cin 32, Cout 36 / 132 / 260 on 5 x 7 (128 x 64 and 128 x 128 tiles) and 16 x 16 (LDS-image kernel); the 8-wave
                     tile at 256 and 306 rows, 255 rows below it; the multi kernel; generic and tap-fused weight gradients
  conv_bf16_pw.hip   flat 1x1, 32 -> 64 on 3 x 9 x 14 with the residual"""
import contextlib
import ctypes as C
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from conv_bounds import BF, CL, Placer, is_pattern
from test_b3_pinned_gpu import _NO_S2IMG, _S2IMG
from test_bf16_gpu import TILE_8WAVE, close_bf16, fwd_choice
from test_conv_epilogue_pinned_gpu import (ACT_GAIN, ALPHA, RESID_GAIN, _TPHASE, _WINO_GENERIC, _Rng, _direct_kernel, _env, _is_b3_generic,
                                           _is_b3_pw, _is_b3_pwk, _is_bf16_generic, _is_bf16_img, _is_bf16_pw, _is_igemm_f32, _is_s2img,
                                           _math, _sup)
from test_ops_gpu import GTOL, TOL

pytestmark = pytest.mark.gpu
GAIN = 0.07
E_ALIGN = -4


def dcl(t, dtype=torch.float32):
    return t.to(dtype).cuda().contiguous(memory_format=CL)


def bfr(t):
    """Rounded to bf16 (kept as f32): operands the bf16 kernels see exactly."""
    return t.to(BF).float()


def ident(t):
    return t


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def sel(t, mask):
    """The pixels a launch owns ([B, C, n]); everything when it owns all."""
    return t if mask is None else t[:, :, mask.to(t.device)]


@contextlib.contextmanager
def derived_banded(P):
    """The derived weights the launchers fetch themselves, as banded copies (bf16 NaN bands) of what the original returns."""
    import ideas_amd.op.conv as CV
    mp = pytest.MonkeyPatch()
    for fn in ("b3_planes", "bf16_pack", "b3_wino_planes"):
        mp.setattr(CV, fn, lambda *a, _orig=getattr(CV, fn), _name=fn, **k: P.inp(_name, _orig(*a, **k)))
    try:
        yield
    finally:
        mp.undo()


def ref_conv(d, stride, pad, reflect, bf, epi, acc=False, transposed=False, resid_gain=RESID_GAIN):
    """f64 reference of one forward-family launch from the case's CPU operands (ideas_conv_igemm's epilogue, include/ideas_hip.h);
    bf16 with per-sample scales: the pack is bf16(w * in_scale[b]), one per sample."""
    x, w = d["x"].double(), d["w"].double()
    if reflect:
        x = F.pad(x, [pad] * 4, mode="reflect")
    if transposed:
        conv = lambda a, ww: F.conv_transpose2d(a, ww, stride=stride, padding=pad)
    else:
        conv = lambda a, ww: F.conv2d(a, ww, stride=stride, padding=0 if reflect else pad)
    if d["lin"] is None:
        y = conv(x, w)
    else:
        cax = 0 if transposed else 1          # the weight's input-channel axis
        ys = []
        for b in range(x.shape[0]):
            wb = w * d["lin"][b].double().view([-1 if i == cax else 1 for i in range(4)])
            ys.append(conv(x[b:b + 1], wb.float().to(BF).double() if bf else wb))
        y = torch.cat(ys)
    y = y * GAIN
    if d["lout"] is not None:
        y = y * d["lout"].double()[:, :, None, None]
    if epi:
        y = F.leaky_relu(y + d["bias"].double().view(1, -1, 1, 1), ALPHA) * ACT_GAIN
        y = (y + d["resid"].double()) * resid_gain
    if acc:
        y = y + d["prev"].double()
    return y


class Case:
    env, f32, bf16, poisons, roundings, grad = {}, False, False, ("x", "w"), 1, False

    def __init__(self, name, **kw):
        self.name = name
        self.__dict__.update(kw)

    def __repr__(self):
        return self.name

    def bitwise(self, name):
        return True


def _dev(P, d, name):
    return None if d[name] is None else P.inp(name, d[name].cuda())


# ------------------------------------------------------------------------------------------------ forward-family launches
class Fwd(Case):
    """One ``launch_fwd``: dtype "f32" (CV.MATH = F32) / "b3" / "bf16"; ``expect(p, with_resid)[0]``: the intended kernel runs;
    ``wmat``: the launch reads the dense f32 matrix (banded here; the other forms are banded by ``derived_banded``)."""
    k, stride, pad, mod, reflect, epi, acc, wmat, last, tile = 3, 1, 1, False, False, False, False, False, None, None

    def geom(self):
        from ideas_amd.op.conv_plan import ConvGeom
        return ConvGeom(self.k, self.k, self.stride, self.pad, self.reflect)

    def data(self):
        r = _Rng(self.seed)
        B, cin, H, W = self.shape
        q = bfr if self.bf16 else ident
        oh, ow = self.geom().out_size(H, W)
        d = dict(x=q(r.n(B, cin, H, W)), w=q(r.n(self.cout, cin, self.k, self.k)))
        d["lin"], d["lout"] = (r.u(B, cin), r.u(B, self.cout)) if self.mod else (None, None)
        d["bias"] = r.n(self.cout) * 0.3 if self.epi else None
        d["resid"] = q(r.n(B, self.cout, oh, ow)) if self.epi else None
        d["prev"] = q(r.n(B, self.cout, oh, ow))
        return d

    def launch(self, P, d):
        import ideas_amd.op.conv as CV
        from ideas_amd.op.conv_plan import plan_fwd
        adt = BF if self.bf16 else torch.float32
        x = P.act("x", dcl(d["x"], adt), self.last)
        w = P.weight(dcl(d["w"]))
        L = plan_fwd(x.shape, w, self.geom())
        p = CV._params(L, GAIN, self.acc, self.epi, ALPHA, ACT_GAIN, RESID_GAIN)
        assert self.expect(p, self.epi)[0], (self.name, "not the intended kernel")
        if self.tile is not None:
            assert fwd_choice(p, self.mod) == self.tile, (self.name, fwd_choice(p, self.mod))
        if self.wmat:
            L = dataclasses.replace(L, wview=P.inp("wmat", L.wmat.clone().reshape(self.cout, -1)), wsrc=None)
        resid = None if d["resid"] is None else P.inp("resid", dcl(d["resid"], adt))
        y = P.out("y", dcl(d["prev"], adt), keep=self.acc)
        CV.launch_fwd(y, x, L, GAIN, _dev(P, d, "lin"), _dev(P, d, "lout"), _dev(P, d, "bias"), resid, act=self.epi, alpha=ALPHA,
                      act_gain=ACT_GAIN, resid_gain=RESID_GAIN, accumulate=self.acc)
        return {"y": (y, None)}

    def ref(self, d):
        return {"y": ref_conv(d, self.stride, self.pad, self.reflect, self.bf16, self.epi, self.acc)}


def _is_direct(kernel):
    def expect(p, resid):
        import ideas_amd.op.conv as CV
        from ideas_amd import _lib
        return CV.MATH == _lib.F32 and p.Cin % 4 != 0 and _direct_kernel(p) == kernel, True
    return expect


def _is_direct_bf16(kernel):     # op/conv.py::launch_fwd, bf16: no MFMA kernel for the geometry, the VALU kernels are its declared path
    def expect(p, resid):
        return _sup("ideas_bf16_direct_supported", p) and not _sup("ideas_bf16_conv_supported", p, 0) and _direct_kernel(p) == kernel, True
    return expect


def _fwd_cases():
    out, seed = [], [1000]

    def add(name, **kw):
        seed[0] += 1
        kw.setdefault("roundings", 2 if kw.get("epi") else 1)      # bf16 with the residual: two roundings, as the suite counts them
        out.append(Fwd(name, seed=seed[0], **kw))
    # f32 MFMA: M = 1 x 5 x 7 = 35 rows of a 128-row tile; 128 x 32 / 128 x 64 / 128 x 128 (two N tiles, the second 4 wide); Cin 4 < BK
    for cout in (20, 44, 132):
        for cin in (4, 36):
            for mod in (False, True):
                add("igemm_f32-%d-%d%s" % (cin, cout, "-mod" if mod else ""), f32=True, wmat=True, shape=(1, cin, 5, 7), cout=cout,
                    mod=mod, expect=_is_igemm_f32)
        for var in ("reflect", "epi", "acc"):
            add("igemm_f32-36-%d-%s" % (cout, var), f32=True, wmat=True, shape=(1, 36, 5, 7), cout=cout, expect=_is_igemm_f32,
                **{var: True})
    # VALU direct
    for cin, cout in ((3, 8), (6, 10)):
        for var in ("plain", "mod", "epi"):
            add("direct_f32-%d-%s" % (cin, var), f32=True, wmat=True, shape=(2, cin, 5, 7), cout=cout, expect=_is_direct("direct"),
                **({} if var == "plain" else {var: True}))
    add("direct_bf16-3-40", bf16=True, wmat=True, shape=(2, 3, 5, 7), cout=40, k=1, pad=0, expect=_is_direct_bf16("smallk_vec"))
    add("direct_bf16-40-3", bf16=True, wmat=True, shape=(2, 40, 5, 7), cout=3, k=1, pad=0, expect=_is_direct_bf16("rowdot"))
    add("direct_bf16-40-3-epi", bf16=True, wmat=True, shape=(2, 40, 5, 7), cout=3, k=1, pad=0, epi=True, expect=_is_direct_bf16("rowdot"))
    # split-bf16 generic: 16 -> 80 on 9 x 11 / stride 2 (M = 20), and the 64-channel N tile small grids take above 64 channels
    for cout in (80, 132):
        for var in ("plain", "mod", "epi", "acc"):
            add("b3_generic-%d-%s" % (cout, var), env=_NO_S2IMG, shape=(1, 16, 9, 11), cout=cout, stride=2, pad=0, expect=_is_b3_generic,
                **({} if var == "plain" else {var: True}))
    # flat 1x1 and its K-chunked form
    pw = {"IDEAS_B3_PW": None}
    add("b3_pw-16-48", env=pw, shape=(2, 16, 7, 5), cout=48, k=1, pad=0, expect=_is_b3_pw)
    add("b3_pw-32-64-resid", env=pw, shape=(3, 32, 9, 14), cout=64, k=1, pad=0, epi=True, expect=_is_b3_pw)
    add("b3_pw-96-136-resid", env=pw, shape=(1, 96, 10, 13), cout=136, k=1, pad=0, epi=True, expect=_is_b3_pw)
    add("b3_pwk-256-64-resid", env=pw, shape=(3, 256, 9, 14), cout=64, k=1, pad=0, epi=True, expect=_is_b3_pwk)
    add("b3_pwk-512-320-resid", env=pw, shape=(1, 512, 3, 3), cout=320, k=1, pad=0, epi=True, expect=_is_b3_pwk)
    # LDS-image kernel: one whole 8 x 16 patch, and 9 x 18 outputs (a second, ragged patch in both directions); N tiles 64 / 128 / 256
    for hw in ((17, 33), (19, 37)):
        for cout in (64, 132, 260):
            for mod in (False, True):
                add("s2img-%dx%d-%d%s" % (hw + (cout, "-mod" if mod else "")), env=_S2IMG, shape=(1, 16) + hw, cout=cout, stride=2, pad=0,
                    mod=mod, expect=_is_s2img)
    add("s2img-19x37-132-epi", env=_S2IMG, shape=(1, 16, 19, 37), cout=132, stride=2, pad=0, epi=True, expect=_is_s2img)
    # bf16 MFMA: the generic tiles on 5 x 7 (M = 35), the LDS-image kernel on 16 x 16; the 8-wave tile and the 255 / 256 boundary
    t64, t128 = (128, 64, 4), (128, 128, 4)
    for cout, tile in ((36, t64), (132, t128), (260, t128)):
        for var in ("plain", "mod", "epi"):
            kw = {} if var == "plain" else {var: True}
            add("bf16_generic-%d-%s" % (cout, var), bf16=True, shape=(1, 32, 5, 7), cout=cout, expect=_is_bf16_generic, tile=(tile, 0), **kw)
            add("bf16_img-%d-%s" % (cout, var), bf16=True, env={"IDEAS_BF16_IMG": None}, shape=(1, 32, 16, 16), cout=cout,
                expect=_is_bf16_img, **kw)
    add("bf16_8wave-256rows", bf16=True, shape=(1, 32, 33, 33), cout=256, stride=2, pad=0, expect=_is_bf16_generic, tile=(TILE_8WAVE, 0))
    add("bf16_8wave-255rows", bf16=True, shape=(1, 32, 31, 35), cout=256, stride=2, pad=0, expect=_is_bf16_generic, tile=(t128, 0))
    add("bf16_8wave-306rows-260", bf16=True, shape=(1, 64, 35, 37), cout=260, stride=2, pad=0, expect=_is_bf16_generic, tile=(TILE_8WAVE, 0))
    add("bf16_8wave-512rows-epi", bf16=True, shape=(2, 32, 33, 33), cout=256, stride=2, pad=0, epi=True, expect=_is_bf16_generic,
        tile=(TILE_8WAVE, 0))
    add("bf16_8wave-per-sample", bf16=True, shape=(2, 32, 33, 33), cout=256, stride=2, pad=0, mod=True, expect=_is_bf16_generic,
        tile=(TILE_8WAVE, 0))
    add("bf16_pw-32-64-resid", bf16=True, env={"IDEAS_BF16_PW": None}, shape=(3, 32, 9, 14), cout=64, k=1, pad=0, epi=True, expect=_is_bf16_pw)
    add("bf16_pw-64-72", bf16=True, env={"IDEAS_BF16_PW": None}, shape=(2, 64, 5, 13), cout=72, k=1, pad=0, expect=_is_bf16_pw)
    return out


# ------------------------------------------------------------------------------------------------ Winograd forward
class Wino(Case):
    """``launch_wino``: dtype "f32" (conv3x3_wino_kernel) or "b3" with the tile ``kernel`` names -- "narrow" (4 waves), "wide" (8
    waves), "rows" (row-sharing), "n256" (its 256-channel tile).  ``transposed``: the input gradient's weights, w [x channels, out]."""
    mod, reflect, epi, transposed, kernel = False, False, False, False, None

    def data(self):
        r = _Rng(self.seed)
        B, cin, H, W = self.shape
        d = dict(x=r.n(B, cin, H, W), w=r.n(*((cin, self.cout) if self.transposed else (self.cout, cin)), 3, 3))
        d["lin"], d["lout"] = (r.u(B, cin), r.u(B, self.cout)) if self.mod else (None, None)
        d["bias"] = r.n(self.cout) * 0.3 if self.epi else None
        d["resid"] = r.n(B, self.cout, H, W) if self.epi else None
        return d

    def launch(self, P, d):
        import os
        import ideas_amd.op.conv as CV
        from ideas_amd import _lib
        from ideas_amd.op.conv_plan import ConvGeom
        B, cin, H, W = self.shape
        x = P.act("x", dcl(d["x"]))
        w = P.weight(dcl(d["w"]), 1 if self.transposed else 0)
        g = ConvGeom(3, 3, 1, 1, self.reflect)
        if self.f32:
            assert CV.MATH == _lib.F32 and CV._wino_ok(g, cin, W) and cin % 8 == 0 and cin % 16 != 0
            u = CV.wino_weights(w.flip(2, 3).permute(1, 2, 3, 0) if self.transposed else w.permute(0, 2, 3, 1))
            u, dt = P.inp("umat", u.reshape(4 * self.cout * 3, cin)), _lib.F32
        else:
            p0 = _lib.ConvParams(B, H, W, cin, H, W, self.cout, H, W, 3, 3, 1, 1, 1, 1, -1, -1, 1, 1, 0, 0, int(self.reflect), int(self.epi),
                                 ALPHA, ACT_GAIN, RESID_GAIN, 0, GAIN)
            assert CV._b3_wino_ok(g, cin, self.cout, W) and _sup("ideas_b3_wino_supported", p0)
            # csrc/conv_b3_wino.hip::wino_choose, as test_b3_pinned_gpu.py::_wino2d restates it
            wide, w2 = cin % 32 == 0 and self.cout > 64, W // 2
            tp = 32 if w2 % 32 == 0 else 16 if w2 % 16 == 0 else 8 if w2 % 8 == 0 else 0
            rows = wide and os.environ.get("IDEAS_B3_WINO2D") != "0" and tp and H % (64 // tp) == 0
            fn = _lib.load().ideas_b3_wino_n256_tiles
            fn.restype, fn.argtypes = C.c_int64, [C.c_int] * 5
            n256 = int(fn(B, H, W, cin, self.cout)) > 0
            assert ("n256" if n256 else "rows" if rows else "wide" if wide else "narrow") == self.kernel, (self.name, wide, tp, rows, n256)
            u, dt = CV.b3_wino_planes(w, self.transposed), _lib.F32_B3
        resid = None if d["resid"] is None else P.inp("resid", dcl(d["resid"]))
        y = P.out("y", torch.empty((B, self.cout, H, W), device="cuda").contiguous(memory_format=CL))
        CV.launch_wino(y, x, u, B, cin, H, W, self.cout, GAIN, self.reflect, _dev(P, d, "lin"), _dev(P, d, "lout"), _dev(P, d, "bias"), resid,
                       act=self.epi, alpha=ALPHA, act_gain=ACT_GAIN, resid_gain=RESID_GAIN, dtype=dt)
        return {"y": (y, None)}

    def ref(self, d):
        return {"y": ref_conv(d, 1, 1, self.reflect, False, self.epi, transposed=self.transposed)}


def _wino_cases():
    out, seed = [], [2000]

    def add(name, **kw):
        seed[0] += 1
        out.append(Wino(name, seed=seed[0], **kw))
    for var in ("plain", "mod", "reflect", "epi", "transposed"):
        kw = {} if var == "plain" else {var: True}
        # f32: Cin % 8 == 0 and not % 16; 15 column pairs of a 128-pair block, 12 of 64 channels
        add("wino_f32-5x6-%s" % var, f32=True, shape=(1, 8, 5, 6), cout=12, **kw)
        # split-bf16, 4-wave 64 x 64 tile: 5 x 6 (H no multiple of a row patch, 3 pair columns) and 7 x 18 (9 pair columns), Cout 36
        add("wino_b3-narrow-5x6-%s" % var, env=_B3_WINO, shape=(1, 16, 5, 6), cout=36, kernel="narrow", **kw)
        add("wino_b3-narrow-7x18-%s" % var, env=_B3_WINO, shape=(2, 16, 7, 18), cout=36, kernel="narrow", **kw)
        # 8-wave 64 x 128 tile where the row-sharing kernel does not apply (9 pair columns): Cout 72 and 132
        add("wino_b3-wide-7x18-%s" % var, env=_B3_WINO, shape=(1, 32, 7, 18), cout=132 if var == "mod" else 72, kernel="wide", **kw)
        # row-sharing kernel on 8 x 16 at Cout 128, and its 256-channel tile at Cout 256
        add("wino_b3-rows-8x16-%s" % var, env=dict(_B3_WINO, IDEAS_B3_WINO_N256="0"), shape=(1, 32, 8, 16), cout=128, kernel="rows", **kw)
        add("wino_b3-n256-8x16-%s" % var, env=dict(_B3_WINO, IDEAS_B3_WINO_N256="1"), shape=(1, 32, 8, 16), cout=256, kernel="n256", **kw)
    # the generic tail instead of the branch-free epilogues
    add("wino_b3-narrow-7x18-tail", env=_WINO_GENERIC, shape=(2, 16, 7, 18), cout=36, kernel="narrow", epi=True, mod=True)
    add("wino_b3-rows-8x16-tail", env=dict(_WINO_GENERIC, IDEAS_B3_WINO_N256="0"), shape=(1, 32, 8, 16), cout=128, kernel="rows", epi=True)
    return out


_B3_WINO = {"IDEAS_B3_WINO_EPI": None, "IDEAS_B3_WINO2D": None, "IDEAS_B3_WINO_N256": None}


# ------------------------------------------------------------------------------------------------ transposed / dgrad phases
class Trans(Case):
    """The parity phases of a k x k / stride-2 / pad-0 transposed conv of x [B, cin, h, w] with w [cin, cout, k, k].  mode "multi":
    all of them through ``launch_multi`` (conv_b3_multi_kernel, conv_b3_tphase_kernel where ``tphase``, conv_bf16_multi_kernel);
    "phases": the planned launches one by one through ``launch_fwd`` -- with k = 1 there is one, and the pixels of the other
    parities (``need_zero``) are nobody's; "phase0": launch (0, 0) alone.  Pixels no launch owns keep the fill pattern."""
    k, mod, mode, tphase, store16 = 3, False, "multi", False, None

    def data(self):
        r = _Rng(self.seed)
        B, cin, h, w_ = self.shape
        q = bfr if self.bf16 else ident
        d = dict(x=q(r.n(B, cin, h, w_)), w=q(r.n(cin, self.cout, self.k, self.k)))
        d["lin"], d["lout"] = (r.u(B, cin), r.u(B, self.cout)) if self.mod else (None, None)
        return d

    def launch(self, P, d):
        import ideas_amd.op.conv as CV
        from ideas_amd import _lib
        from ideas_amd.op.conv_plan import ConvGeom, convT_out_size, plan_dgrad
        adt = BF if self.bf16 else torch.float32
        B, cin, h, w_ = self.shape
        x = P.act("x", dcl(d["x"], adt))
        w = P.weight(dcl(d["w"]), 1)
        g = ConvGeom(self.k, self.k, 2, 0, False)
        out_hw = convT_out_size(h, w_, g)
        launches, need_zero = plan_dgrad(x.shape, w, g, out_hw)
        assert (len(launches), need_zero) == ((4, False) if self.k == 3 else (1, True))
        for L in launches:
            p = CV._params(L, GAIN)
            assert _sup("ideas_bf16_conv_supported", p, int(self.mod)) if self.bf16 else _sup("ideas_b3_conv_supported", p)
        y = P.out("y", torch.empty((B, self.cout) + out_hw, device="cuda", dtype=adt).contiguous(memory_format=CL))
        lin, lout = _dev(P, d, "lin"), _dev(P, d, "lout")
        if self.mode == "multi":
            if not self.bf16:     # csrc/conv_b3_tphase.hip::tphase_match (IDEAS_B3_TPHASE=1: plain launches too), else conv_b3_multi_kernel
                assert (cin % 16 == 0 and self.cout > 64 and out_hw == (2 * h + 1, 2 * w_ + 1)) == self.tphase
            if self.tphase:
                fn = _lib.load().ideas_b3_tphase_store16
                fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
                assert int(fn(y.data_ptr(), self.cout)) == int(self.store16)
            assert CV.B3_MULTI and CV.launch_multi(y, x, launches, GAIN, lin, lout)
            return {"y": (y, None)}
        mask = torch.zeros(out_hw, dtype=torch.bool)
        for L in (launches if self.mode == "phases" else launches[:1]):
            assert (L.osy, L.osx) == (2, 2) and (self.mode == "phases" or (L.ooy, L.oox) == (0, 0))
            CV.launch_fwd(y, x, L, GAIN, lin, lout)
            mask[L.ooy::2, L.oox::2] = True
        assert bool(mask[-1, -1]) and not bool(mask.all())        # the launch owns the last pixel-row (write-side check), not every pixel
        return {"y": (y, mask)}

    def ref(self, d):
        return {"y": ref_conv(d, 2, 0, False, self.bf16, False, transposed=True)}


def _trans_cases():
    out, seed = [], [3000]

    def add(name, **kw):
        seed[0] += 1
        out.append(Trans(name, seed=seed[0], **kw))
    tp = _TPHASE              # IDEAS_B3_TPHASE=1 (plain launches too), the store form left to the library
    for mod in (False, True):
        t = "-mod" if mod else ""
        add("b3_multi-16-32" + t, env=tp, shape=(1, 16, 4, 5), cout=32, mod=mod)                  # Cout <= 64: 128 x 32 tile, M = 6 .. 20
        add("b3_multi-16-44" + t, env=tp, shape=(1, 16, 4, 5), cout=44, mod=mod)                  # 128 x 64 tile
        for st in (True, False):
            env = tp if st else dict(tp, IDEAS_B3_TPHASE_STORE="0")
            s = "" if st else "-store4"
            add("b3_tphase-16-128" + t + s, env=env, shape=(2, 16, 4, 16), cout=128, mod=mod, tphase=True, store16=st)
            add("b3_tphase-32-192" + t + s, env=env, shape=(2, 32, 5, 18), cout=192, mod=mod, tphase=True, store16=st)
        add("b3_phase0-16-80" + t, env=_NO_S2IMG, shape=(1, 16, 4, 5), cout=80, mod=mod, mode="phase0")
        add("b3_need_zero-16-80" + t, env={"IDEAS_B3_PW": None}, shape=(1, 16, 4, 5), cout=80, k=1, mod=mod, mode="phases")
        add("bf16_multi-32-36" + t, bf16=True, shape=(2, 32, 5, 9), cout=36, mod=mod)
        add("bf16_multi-32-132" + t, bf16=True, shape=(2, 32, 4, 16), cout=132, mod=mod)
    add("bf16_phase0-32-36", bf16=True, shape=(2, 32, 5, 9), cout=36, mode="phase0")
    return out


# ------------------------------------------------------------------------------------------------ Blur + stride-2
class S2fir(Case):
    """ideas_b3_blur_conv_s2(_mod), called the way ``blur_conv_s2_raw`` calls them, on x [B, cin, h, w] with the (1, 3, 3, 1) FIR and
    pads (2, 2): y and, ``want_xb``, the blurred tensor as a banded side output of its own."""
    mod, want_xb, epi = False, False, False

    def data(self):
        r = _Rng(self.seed)
        B, cin, h, w_ = self.shape
        oh, ow = (h + 1 - 3) // 2 + 1, (w_ + 1 - 3) // 2 + 1
        d = dict(x=r.n(B, cin, h, w_), w=r.n(self.cout, cin, 3, 3))
        d["lin"], d["lout"] = (r.u(B, cin), r.u(B, self.cout)) if self.mod else (None, None)
        d["bias"] = r.n(self.cout) * 0.3 if self.epi else None
        d["resid"] = r.n(B, self.cout, oh, ow) if self.epi else None
        return d

    def launch(self, P, d):
        import ideas_amd.op.conv as CV
        from ideas_amd import _lib
        from ideas_amd.model import make_kernel
        B, cin, h, w_ = self.shape
        x = P.act("x", dcl(d["x"]))
        w = P.weight(dcl(d["w"]))
        fir = make_kernel((1, 3, 3, 1)).cuda()
        assert CV.blur_conv_s2_ok(x, w, fir, (2, 2), want_xb=self.want_xb)
        L, hb, wb = CV._blur_conv_plan(tuple(x.shape), w, fir, (2, 2))
        assert (hb, wb) == (h + 1, w_ + 1) and (L.OH % 8 != 0 or L.OW % 16 != 0) == self.ragged
        kh, kv = CV.fir_factors(fir)
        p = CV._params(L, GAIN, False, self.epi, ALPHA, ACT_GAIN, 1.0)
        y = P.out("y", torch.empty((B, self.cout, L.YH, L.YW), device="cuda").contiguous(memory_format=CL))
        xb = P.out("xb", torch.empty((B, cin, hb, wb), device="cuda").contiguous(memory_format=CL)) if self.want_xb else None
        planes = CV.b3_planes(L)
        resid = None if d["resid"] is None else P.inp("resid", dcl(d["resid"]))
        bias, lin, lout = _dev(P, d, "bias"), _dev(P, d, "lin"), _dev(P, d, "lout")
        lib, ptr = _lib.load(), _lib.ptr
        if self.mod:
            rc = lib.ideas_b3_blur_conv_s2_mod(ptr(y), ptr(xb), ptr(x), ptr(planes), kh, kv, ptr(lin), ptr(lout), ptr(bias), ptr(resid),
                                               C.byref(p), h, w_, 2, _lib.stream_ptr())
        else:
            rc = lib.ideas_b3_blur_conv_s2(ptr(y), ptr(xb), ptr(x), ptr(planes), kh, kv, ptr(bias), ptr(resid), C.byref(p), h, w_, 2,
                                           _lib.stream_ptr())
        _lib.check(rc, "ideas_b3_blur_conv_s2")
        return dict(y=(y, None), **({"xb": (xb, None)} if self.want_xb else {}))

    def ref(self, d):
        from ideas_amd.model import make_kernel
        cin = self.shape[1]
        fir = make_kernel((1, 3, 3, 1)).double().flip(0, 1)
        xb = F.conv2d(F.pad(d["x"].double(), [2, 2, 2, 2]), fir.expand(cin, 1, 4, 4).contiguous(), groups=cin)
        y = ref_conv(dict(d, x=xb), 2, 0, False, False, self.epi, resid_gain=1.0)
        return dict(y=y, **({"xb": xb} if self.want_xb else {}))


def _s2fir_cases():
    out, seed = [], [4000]
    for hw, ragged in (((16, 32), False), ((18, 36), True), ((19, 37), True)):        # -> 8 x 16, 9 x 18, 9 x 18 from an odd raw size
        for cout in (64, 132, 260):
            for mod in (False, True):
                for xb in ((False, True) if hw[0] % 2 == 0 else (False,)):             # the side output needs the blurred size 2 OH + 1
                    seed[0] += 1
                    out.append(S2fir("s2fir-%dx%d-%d%s%s" % (hw + (cout, "-mod" if mod else "", "-xb" if xb else "")),
                                     env={"IDEAS_S2FIR_CFG": None}, seed=seed[0], shape=(1, 16) + hw, cout=cout, mod=mod, want_xb=xb,
                                     ragged=ragged, epi=(cout == 132)))
    return out


# ------------------------------------------------------------------------------------------------ weight gradients
def _splits(site, p, scaled):
    """Splits of the launch's split-K plan (csrc/conv_igemm.hip::ideas_conv_splitk_plan, the diagnostic beside the ABI)."""
    from ideas_amd import _lib
    fn = C.CDLL(_lib.LIB_PATH).ideas_conv_splitk_plan
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.POINTER(_lib.ConvParams), C.c_int, C.c_int64, C.POINTER(C.c_int64)]
    out = (C.c_int64 * 4)()
    assert fn(site, C.byref(p), int(scaled), 0, out) == 0
    return int(out[0])


class Wgrad(Case):
    """``launch_wgrad`` (``via`` "raw": ``conv_wgrad_raw(out=)``) into a banded gw: zeroed, or (``prefill``) holding finite values the
    kernel must add to.  ``expect(p)``: the intended kernel; ``site``: its split-K plan, for the bitwise comparison.  The read-side
    operands are x and ("w") gy."""
    k, stride, pad, mod, reflect, prefill, via, site, grad = 3, 1, 1, False, False, False, "launch", None, True

    def geom(self):
        from ideas_amd.op.conv_plan import ConvGeom
        return ConvGeom(self.k, self.k, self.stride, self.pad, self.reflect)

    def data(self):
        r = _Rng(self.seed)
        B, cin, H, W = self.shape
        q = bfr if self.bf16 else ident
        oh, ow = self.geom().out_size(H, W)
        d = dict(x=q(r.n(B, cin, H, W)), gy=q(r.n(B, self.cout, oh, ow)), prev=r.n(self.cout, cin, self.k, self.k))
        d["lin"], d["lout"] = (r.u(B, cin), r.u(B, self.cout)) if self.mod else (None, None)
        return d

    def launch(self, P, d):
        import ideas_amd.op.conv as CV
        from ideas_amd.op.conv_plan import plan_wgrad
        adt = BF if self.bf16 else torch.float32
        x = P.act("x", dcl(d["x"], adt))
        gy = P.act("gy", dcl(d["gy"], adt), key="w")
        L = plan_wgrad(x.shape, gy.shape, self.geom())
        p = CV._params(L, GAIN)
        assert self.expect(p), (self.name, "not the intended kernel")
        self.single = self.site is not None and _splits(self.site, p, self.mod) == 1
        gw = P.out("gw", dcl(d["prev"]), keep=self.prefill, kind="atomic")
        lin, lout = _dev(P, d, "lin"), _dev(P, d, "lout")
        if self.via == "raw":
            got = CV.conv_wgrad_raw(gy, x, self.geom(), tuple(gw.shape), GAIN, lin, lout, out=gw)
            assert got.data_ptr() == gw.data_ptr()
        else:
            CV.launch_wgrad(gw, gy, x, L, GAIN, lin, lout)
        return {"gw": (gw, None)}

    def bitwise(self, name):
        return self.single

    def ref(self, d):
        x, gy = d["x"].double(), d["gy"].double()
        if self.mod:
            x, gy = x * d["lin"].double()[:, :, None, None], gy * d["lout"].double()[:, :, None, None]
        if self.reflect:
            x = F.pad(x, [self.pad] * 4, mode="reflect")
        w0 = torch.zeros(self.cout, self.shape[1], self.k, self.k, dtype=torch.float64, requires_grad=True)
        ref, = torch.autograd.grad(F.conv2d(x, w0, stride=self.stride, padding=0 if self.reflect else self.pad) * GAIN, w0, gy)
        return {"gw": ref + d["prev"].double() if self.prefill else ref}


class WinoWgrad(Wgrad):
    """ideas_conv3x3_wino_wgrad into a banded, zeroed dU, then ideas_wino_wgrad_fold into a banded target whose strides
    (so, sky, skx, si) are not the contiguous ones: gw is the lower half of the last axis of a [O, 3, 3, 2 I] buffer, and the upper
    half -- the gaps between its rows -- must keep its pattern as the bands do."""

    def launch(self, P, d):
        import ideas_amd.op.conv as CV
        from ideas_amd import _lib
        B, ci, h, w_ = self.shape
        co = self.cout
        x = P.act("x", dcl(d["x"]))
        gy = P.act("gy", dcl(d["gy"]), key="w")
        assert CV.MATH == _lib.F32 and CV._wino_ok(self.geom(), ci, w_, fwd=False) and co % 4 == 0
        p = _lib.ConvParams(B, h, w_, ci, h, w_, co, h, w_, 3, 3, 1, 1, 1, 1, -1, -1, 1, 1, 0, 0, int(self.reflect), 0, 0.2, 1.0, 1.0, 0, GAIN)
        self.single = _splits(1, p, self.mod) == 1
        gu = P.out("gu", torch.empty((4 * co * 3, ci), device="cuda"), kind="atomic")
        lin, lout = _dev(P, d, "lin"), _dev(P, d, "lout")
        rc = _lib.load().ideas_conv3x3_wino_wgrad(_lib.ptr(gu), _lib.ptr(gy), _lib.ptr(x), _lib.ptr(lin), _lib.ptr(lout), C.byref(p), _lib.F32,
                                                  _lib.stream_ptr())
        _lib.check(rc, "ideas_conv3x3_wino_wgrad")
        if P.banded:          # the fold re-zeroes dU behind its read: its write-side checks are made here, before the fold
            torch.cuda.synchronize()
            b = P.outs["gu"]
            assert not b.changed() and b.changed(shrink_rows=1), (self.name, "gu")
            b.sensitivity_done = True
        gap = torch.tensor([0x35A5A5A5], dtype=torch.int32).view(torch.float32).item()
        base = torch.full((co, 3, 3, 2 * ci), gap)
        base[..., :ci] = d["prev"].permute(0, 2, 3, 1) if self.prefill else 0.0
        base = P.out("gw", base.reshape(co * 9, 2 * ci).cuda(), keep=True, kind="atomic").view(co, 3, 3, 2 * ci)
        gw = base[..., :ci].permute(0, 3, 1, 2)
        assert gw.stride() == (18 * ci, 1, 6 * ci, 2 * ci) and not gw.is_contiguous(memory_format=CL)
        CV._wino_fold(gu, gw, co, ci, tuple(gw.shape), x.device, clear=True)
        torch.cuda.synchronize()
        assert bool((base[..., ci:].view(torch.int32) == 0x35A5A5A5).all()), (self.name, "the fold touched the gaps of its strided target")
        assert not bool(gu.any()), (self.name, "the fold did not re-zero dU")
        return {"gw": (gw, None)}


def _mfma_f32(p):
    import ideas_amd.op.conv as CV
    from ideas_amd import _lib
    return CV.MATH == _lib.F32 and p.Cin % 4 == 0 and p.Cout % 4 == 0


def _direct_wgrad(p):
    return p.Cin % 4 != 0


def _b3_generic_wgrad(p):
    return _sup("ideas_b3_wgrad_supported", p) and not _sup("ideas_b3_wgrad3_supported", p) and p.TY * p.TX == 9


def _b3_wgrad3(p):
    import os
    return _sup("ideas_b3_wgrad_supported", p) and _sup("ideas_b3_wgrad3_supported", p) and os.environ.get("IDEAS_B3_WGRAD3") != "0"


def _b3_pw_wgrad(p):       # csrc/conv_b3_pw.hip::ideas_b3_pw_wgrad_ok: 1x1 / stride 1, no scales, Cin % 64 == 0, Cout % 64 == 0, >= 512 pixels
    import os
    return ((p.TY, p.TX, p.sy, p.sx, p.offy, p.offx) == (1, 1, 1, 1, 0, 0) and (p.OH, p.OW) == (p.IH, p.IW) and p.Cin % 64 == 0 and p.Cout % 64 == 0
            and p.B * p.OH * p.OW >= 512 and os.environ.get("IDEAS_B3_PW_WGRAD") != "0")


def _bf16_generic_wgrad(p):
    return _sup("ideas_bf16_wgrad_supported", p, 0) and p.Cout > 8 and p.Cin > 8 and not _sup("ideas_bf16_wgrad3_supported", p)


def _bf16_wgrad3(p):
    return _sup("ideas_bf16_wgrad_supported", p, 0) and _sup("ideas_bf16_wgrad3_supported", p)


def _wgrad_cases():
    out, seed = [], [5000]

    def add(name, cls=Wgrad, **kw):
        for prefill in (False, True):          # once into zeros, once into finite values: the kernel must add, not overwrite
            seed[0] += 1
            out.append(cls(name + ("-prefill" if prefill else ""), seed=seed[0], prefill=prefill, **kw))
    for mod in (False, True):
        t = "-mod" if mod else ""
        # f32 MFMA: Cout 36 x Cin 20 -- both tile edges ragged; OW = 7 < BK = 16 and OW = 19 >= BK
        add("wgrad_f32-ow7" + t, f32=True, shape=(2, 20, 5, 7), cout=36, mod=mod, expect=_mfma_f32, site=0)
        add("wgrad_f32-ow19" + t, f32=True, shape=(1, 20, 3, 19), cout=36, mod=mod, expect=_mfma_f32, site=0)
        add("wgrad_direct-3" + t, f32=True, shape=(2, 3, 5, 7), cout=8, mod=mod, expect=_direct_wgrad)
        # split-bf16 generic: Cout 72 of a 128-channel tile, OW = 4 (four image rows a K-step)
        add("wgrad_b3-72-ow4" + t, env={"IDEAS_B3_WGRAD3": None}, shape=(1, 256, 4, 4), cout=72, mod=mod, expect=_b3_generic_wgrad, site=2)
        # tap-fused: the pinned 64 -> 64 at 16 x 16 and Cout 128, stride 1 and stride 2 (33 x 33 -> 16 x 16)
        for cout in (64, 128):
            add("wgrad3_b3-s1-%d" % cout + t, env={"IDEAS_B3_WGRAD3": None}, shape=(1, 64, 16, 16), cout=cout, mod=mod, expect=_b3_wgrad3, site=3)
            add("wgrad3_b3-s2-%d" % cout + t, env={"IDEAS_B3_WGRAD3": None, "IDEAS_B3_WGRAD3_S2": None}, shape=(1, 64, 33, 33), cout=cout,
                stride=2, pad=0, mod=mod, expect=_b3_wgrad3, site=3)
        # Winograd-domain gradient: 15 column pairs (< GBK = 8 per row: W / 2 = 3) and W / 2 = 9 >= GBK, 12 x 3 * 8 of a 64 x 128 tile
        add("wgrad_wino-5x6" + t, cls=WinoWgrad, f32=True, shape=(1, 8, 5, 6), cout=12, mod=mod)
        add("wgrad_wino-3x18-reflect" + t, cls=WinoWgrad, f32=True, shape=(2, 8, 3, 18), cout=12, mod=mod, reflect=True)
        # bf16 generic: OW = 4 (eight rows a K-step), Cin 24 x Cout 40; tap-fused at its smallest shape and with 2 x 2 channel tiles
        add("wgrad_bf16-24-40" + t, bf16=True, shape=(2, 24, 8, 4), cout=40, mod=mod, expect=_bf16_generic_wgrad, site=5)
        add("wgrad3_bf16-64-64" + t, bf16=True, env={"IDEAS_BF16_WGRAD3_MIN_WORK": "0", "IDEAS_BF16_WGRAD3": None}, shape=(1, 64, 8, 32), cout=64,
            mod=mod, expect=_bf16_wgrad3, site=6)
    add("wgrad3_bf16-128-128", bf16=True, env={"IDEAS_BF16_WGRAD3_MIN_WORK": "0", "IDEAS_BF16_WGRAD3": None}, shape=(2, 128, 9, 64), cout=128,
        expect=_bf16_wgrad3, site=6)
    # flat 1x1: 529 pixels, no multiple of its 32-pixel step; through conv_wgrad_raw(out=)
    add("wgrad_b3_pw-64-64", env={"IDEAS_B3_PW_WGRAD": None}, shape=(1, 64, 23, 23), cout=64, k=1, pad=0, via="raw", expect=_b3_pw_wgrad, site=4)
    add("wgrad_b3_pw-128-64", env={"IDEAS_B3_PW_WGRAD": None}, shape=(1, 128, 23, 23), cout=64, k=1, pad=0, via="raw", expect=_b3_pw_wgrad, site=4)
    return out


CASES = _fwd_cases() + _wino_cases() + _trans_cases() + _s2fir_cases() + _wgrad_cases()
assert len({c.name for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_conv_launch_stays_inside_its_operands(case):
    with _env(**case.env), _math(case.f32):
        d = case.data()
        plain = Placer(False)
        got0 = case.launch(plain, d)
        torch.cuda.synchronize()
        banded = Placer(True)
        with derived_banded(banded):
            got1 = case.launch(banded, d)
        torch.cuda.synchronize()
        # ---- write side: the bands around every output, and the checker's own sensitivity
        assert set(got1) <= set(banded.outs) and banded.ins
        for name, b in banded.outs.items():
            assert not b.changed(), (case.name, name, "a band around the output changed")
            assert getattr(b, "sensitivity_done", False) or b.changed(shrink_rows=1), (case.name, name, "the band check is blind")
        # ---- read side: operands untouched (bf16: the residual among them), output finite, placement changes nothing, f64 bound
        for name, b in banded.ins.items():
            assert b.intact(), (case.name, name, "an input buffer changed")
        ref = case.ref(d)
        for name, (y1, mask) in got1.items():
            y0 = got0[name][0]
            if mask is not None:
                assert bool(is_pattern(y1)[:, :, ~mask.cuda()].all()), (case.name, name, "a pixel of another parity was touched")
            assert bool(torch.isfinite(sel(y1, mask)).all()), (case.name, name, "non-finite: a load reached a NaN band")
            if case.bitwise(name):
                assert torch.equal(bits(y1), bits(y0)), (case.name, name, "banded placement changed the result")
            if y1.dtype == BF or (case.bf16 and case.grad):
                close_bf16(sel(y1, mask), sel(ref[name], mask), (case.name, name), roundings=case.roundings)
            else:
                err = rel_err(sel(y1, mask), sel(ref[name], mask))
                print(case.name, name, "rel err %.3e" % err)
                assert err < (GTOL if case.grad else TOL), (case.name, name, err)
        # ---- read side, sensitivity: a NaN in the last pixel-row of x / the last row of the weights (gradients: of gy) reaches the output
        for poison in case.poisons:
            got = case.launch(Placer(False, poison), d)
            torch.cuda.synchronize()
            y, mask = next(iter(got.values()))
            assert not bool(torch.isfinite(sel(y, mask)).all()), (case.name, poison, "a NaN operand left the output finite")


# ------------------------------------------------------------------------------------------------ refusals: no launch
def _refused(call, ptrs, names, P):
    """``call(ptrs)`` with each of ``names`` in turn 4 bytes off its 16-byte boundary: IDEAS_E_ALIGN, and every buffer untouched."""
    for b in list(P.ins.values()) + list(P.outs.values()):
        b.arm()
    assert call(ptrs) == 0                  # (the aligned call is a valid launch: what follows is refused for alignment alone)
    torch.cuda.synchronize()
    for b in list(P.ins.values()) + list(P.outs.values()):
        b.arm()
    for n in names:
        assert ptrs[n] % 16 == 0
        assert call(dict(ptrs, **{n: ptrs[n] + 4})) == E_ALIGN, n
    torch.cuda.synchronize()
    for k, b in list(P.ins.items()) + list(P.outs.items()):
        assert b.intact(), (k, "touched by a refused call")


def _fwd_operands(P, dtype, B, cin, H, W, cout, g):
    """Banded operands of one forward launch with every optional pointer: (pointers by name, params, Launch)."""
    import ideas_amd.op.conv as CV
    from ideas_amd import _lib
    from ideas_amd.op.conv_plan import plan_fwd
    r = _Rng(7)
    adt = BF if dtype == _lib.BF16 else torch.float32
    x, w = P.inp("x", dcl(r.n(B, cin, H, W), adt)), dcl(r.n(cout, cin, g.kh, g.kw))
    L = plan_fwd(x.shape, w, g)
    p = CV._params(L, GAIN)
    lin = P.inp("in_scale", r.u(B, cin).cuda())
    with derived_banded(P):
        wm = (P.inp("wmat", L.wmat.clone().reshape(cout, -1)) if dtype == _lib.F32 else CV.b3_planes(L) if dtype == _lib.F32_B3
              else CV.bf16_pack(L, lin))
    y = P.out("y", torch.empty((B, cout, L.YH, L.YW), device="cuda", dtype=adt).contiguous(memory_format=CL))
    resid = P.inp("resid", dcl(r.n(B, cout, L.YH, L.YW), adt))
    ptrs = dict(y=y.data_ptr(), x=x.data_ptr(), wmat=wm.data_ptr(), in_scale=lin.data_ptr(), out_scale=P.inp("out_scale", r.u(B, cout).cuda()).data_ptr(),
                bias=P.inp("bias", r.n(cout).cuda()).data_ptr(), resid=resid.data_ptr())
    return ptrs, p, L


@pytest.mark.parametrize("dtype", ["f32", "b3", "bf16"])
def test_conv_igemm_refuses_misaligned_operands(dtype):
    from ideas_amd import _lib
    from ideas_amd.op.conv_plan import ConvGeom
    dt = {"f32": _lib.F32, "b3": _lib.F32_B3, "bf16": _lib.BF16}[dtype]
    P = Placer(True)
    ptrs, p, _ = _fwd_operands(P, dt, 2, 32, 5, 7, 36, ConvGeom(3, 3, 1, 1, False))
    names = ["x", "wmat", "in_scale"] + (["y", "out_scale", "bias", "resid"] if dtype == "bf16" else [])
    lib = _lib.load()
    _refused(lambda q: lib.ideas_conv_igemm(q["y"], q["x"], q["wmat"], q["in_scale"], q["out_scale"], q["bias"], q["resid"], C.byref(p), dt,
                                            _lib.stream_ptr()), ptrs, names, P)


@pytest.mark.parametrize("dtype", ["b3", "bf16"])
def test_conv_igemm_multi_refuses_misaligned_operands(dtype):
    import ideas_amd.op.conv as CV
    from ideas_amd import _lib
    from ideas_amd.op.conv_plan import ConvGeom, convT_out_size, plan_dgrad
    bf = dtype == "bf16"
    r, P = _Rng(8), Placer(True)
    x, w = P.inp("x", dcl(r.n(1, 32, 4, 5), BF if bf else torch.float32)), dcl(r.n(32, 36, 3, 3))
    g = ConvGeom(3, 3, 2, 0, False)
    launches, _ = plan_dgrad(x.shape, w, g, convT_out_size(4, 5, g))
    lin, lout = P.inp("in_scale", r.u(1, 32).cuda()), P.inp("out_scale", r.u(1, 36).cuda())
    with derived_banded(P):
        ws = [CV.bf16_pack(L, lin) if bf else CV.b3_planes(L) for L in launches]
    y = P.out("y", torch.empty((1, 36, 9, 11), device="cuda", dtype=x.dtype).contiguous(memory_format=CL))
    ps = (_lib.ConvParams * 4)(*[CV._params(L, GAIN) for L in launches])
    ptrs = dict(x=x.data_ptr(), in_scale=lin.data_ptr(), **{"wmat%d" % i: t.data_ptr() for i, t in enumerate(ws)})
    lib = _lib.load()

    def call(q):
        arr = (C.c_void_p * 4)(*[q["wmat%d" % i] for i in range(4)])
        return lib.ideas_conv_igemm_multi(4, y.data_ptr(), q["x"], arr, q["in_scale"], lout.data_ptr(), ps, _lib.BF16 if bf else _lib.F32_B3,
                                          _lib.stream_ptr())
    _refused(call, ptrs, sorted(ptrs), P)


@pytest.mark.parametrize("dtype", ["f32", "b3", "bf16"])
def test_conv_wgrad_refuses_misaligned_operands(dtype):
    import ideas_amd.op.conv as CV
    from ideas_amd import _lib
    from ideas_amd.op.conv_plan import ConvGeom, plan_wgrad
    dt = {"f32": _lib.F32, "b3": _lib.F32_B3, "bf16": _lib.BF16}[dtype]
    adt = BF if dtype == "bf16" else torch.float32
    r, P = _Rng(9), Placer(True)
    x, gy = P.inp("x", dcl(r.n(1, 64, 16, 16), adt)), P.inp("gy", dcl(r.n(1, 64, 16, 16), adt))
    lin, lout = P.inp("in_scale", r.u(1, 64).cuda()), P.inp("out_scale", r.u(1, 64).cuda())
    gw = P.out("gw", dcl(torch.zeros(64, 64, 3, 3)), kind="atomic")
    p = CV._params(plan_wgrad(x.shape, gy.shape, ConvGeom(3, 3, 1, 1, False)), GAIN)
    ptrs = dict(x=x.data_ptr(), gy=gy.data_ptr(), in_scale=lin.data_ptr(), out_scale=lout.data_ptr())
    lib = _lib.load()
    _refused(lambda q: lib.ideas_conv_wgrad(gw.data_ptr(), q["gy"], q["x"], q["in_scale"], q["out_scale"], C.byref(p), dt, _lib.stream_ptr()),
             ptrs, ["x", "gy"] + ([] if dtype == "bf16" else ["in_scale", "out_scale"]), P)


@pytest.mark.parametrize("dtype", ["f32", "b3"])
def test_conv3x3_wino_refuses_misaligned_operands(dtype):
    import ideas_amd.op.conv as CV
    from ideas_amd import _lib
    r, P = _Rng(10), Placer(True)
    B, cin, H, W, cout = 1, 8 if dtype == "f32" else 16, 5, 6, 12
    x, w = P.inp("x", dcl(r.n(B, cin, H, W))), dcl(r.n(cout, cin, 3, 3))
    lin, lout = P.inp("in_scale", r.u(B, cin).cuda()), P.inp("out_scale", r.u(B, cout).cuda())
    with derived_banded(P):
        u = P.inp("umat", CV.wino_weights(w.permute(0, 2, 3, 1)).reshape(-1, cin)) if dtype == "f32" else CV.b3_wino_planes(w, False)
    y = P.out("y", torch.empty((B, cout, H, W), device="cuda").contiguous(memory_format=CL))
    p = _lib.ConvParams(B, H, W, cin, H, W, cout, H, W, 3, 3, 1, 1, 1, 1, -1, -1, 1, 1, 0, 0, 0, 0, ALPHA, 1.0, 1.0, 0, GAIN)
    ptrs = dict(x=x.data_ptr(), umat=u.data_ptr(), in_scale=lin.data_ptr())
    lib, dt = _lib.load(), _lib.F32 if dtype == "f32" else _lib.F32_B3
    _refused(lambda q: lib.ideas_conv3x3_wino(y.data_ptr(), q["x"], q["umat"], q["in_scale"], lout.data_ptr(), None, None, C.byref(p), dt,
                                              _lib.stream_ptr()), ptrs, sorted(ptrs), P)
    if dtype == "f32":      # the Winograd-domain weight gradient checks x, gy and both scales
        gy = P.inp("gy", dcl(r.n(B, cout, H, W)))
        gu = P.out("gu", torch.empty((4 * cout * 3, cin), device="cuda"), kind="atomic")
        ptrs = dict(x=x.data_ptr(), gy=gy.data_ptr(), in_scale=lin.data_ptr(), out_scale=lout.data_ptr())
        _refused(lambda q: lib.ideas_conv3x3_wino_wgrad(gu.data_ptr(), q["gy"], q["x"], q["in_scale"], q["out_scale"], C.byref(p), _lib.F32,
                                                        _lib.stream_ptr()), ptrs, sorted(ptrs), P)


@pytest.mark.parametrize("mod", [False, True])
def test_blur_conv_s2_refuses_misaligned_operands(mod):
    import ideas_amd.op.conv as CV
    from ideas_amd import _lib
    from ideas_amd.model import make_kernel
    r, P = _Rng(11), Placer(True)
    B, cin, h, w_, cout = 1, 16, 16, 32, 64
    x, w = P.inp("x", dcl(r.n(B, cin, h, w_))), dcl(r.n(cout, cin, 3, 3))
    fir = make_kernel((1, 3, 3, 1)).cuda()
    L, hb, wb = CV._blur_conv_plan(tuple(x.shape), w, fir, (2, 2))
    kh, kv = CV.fir_factors(fir)
    p = CV._params(L, GAIN)
    with derived_banded(P):
        planes = CV.b3_planes(L)
    lin, lout = P.inp("in_scale", r.u(B, cin).cuda()), P.inp("out_scale", r.u(B, cout).cuda())
    y = P.out("y", torch.empty((B, cout, L.YH, L.YW), device="cuda").contiguous(memory_format=CL))
    xb = P.out("xb", torch.empty((B, cin, hb, wb), device="cuda").contiguous(memory_format=CL))
    ptrs = dict(x=x.data_ptr(), wplanes=planes.data_ptr(), xb_out=xb.data_ptr(), in_scale=lin.data_ptr())
    lib = _lib.load()
    if mod:
        call = lambda q: lib.ideas_b3_blur_conv_s2_mod(y.data_ptr(), q["xb_out"], q["x"], q["wplanes"], kh, kv, q["in_scale"], lout.data_ptr(), None,
                                                       None, C.byref(p), h, w_, 2, _lib.stream_ptr())
    else:
        call = lambda q: lib.ideas_b3_blur_conv_s2(y.data_ptr(), q["xb_out"], q["x"], q["wplanes"], kh, kv, None, None, C.byref(p), h, w_, 2,
                                                   _lib.stream_ptr())
    _refused(call, ptrs, ["x", "wplanes", "xb_out"] + (["in_scale"] if mod else []), P)
