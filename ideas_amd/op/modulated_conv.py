"""Modulated / demodulated convolution without per-sample weights.

Mirror of ``ModulatedConv2d.forward`` (stylegan2/model.py:236-277; the same-resolution and upsample branches IDEAS
instantiates, models.py:143-152, and the downsample branch of the layer library).  The reference materialises a [B*Cout, Cin, 3, 3] weight
per call and runs a ``groups=batch`` conv (B small convs for cuDNN).  Here the arithmetic is re-associated:

    y[b,o] = (scale * d[b,o]) * sum_{i,k} W[o,i,k] * (s[b,i] * x[b,i, . + k])

so ONE implicit GEMM with the shared weight serves the whole batch: ``s`` scales the activation tile while it
is staged into LDS, ``d`` scales the accumulator in the epilogue (kernel: csrc/conv_igemm.hip).  The
demodulation factor d[b,o] = rsqrt(sum_i s[b,i]^2 * wsq[o,i] + 1e-8), wsq = scale^2 * sum_k W^2, is a
wavefront-shuffle reduction (csrc/modconv_aux.hip) instead of a pass over the per-sample weights; its derivative (to the style
and to W) is folded into the backward of the conv Function (ideas_demod_bwd, ideas_demod_wgrad).
Difference to the reference's association is f32-roundoff class (SURVEY.md §7 measured 1.8e-6 abs on |y|~4).

One autograd Function, ``_ModConv``, owns all three modes (same, up, down), each with or without the demodulation, same and
down also with bias + leaky-ReLU in the conv epilogue.  ``_mod_forward`` is the one place that picks the raw conv call of a mode
(the no-grad ``resid`` path of ``modulated_conv2d`` goes through it too), and the one ``backward`` is six steps: activation
prologue, the conv's input gradient with the two scales trading places (down: then the blur's adjoint), the two per-sample dots,
``_style_grads``, and the weight gradient + ``_demod_wgrad`` under ``weight_grad``.  The mode picks the raw calls and the operand
roles, nothing else.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib
from ..precision import to_act, to_f32
from . import conv as _conv
from .conv import conv2d, conv_dgrad_raw, conv_fwd_raw, conv_transpose2d, conv_wgrad_raw, _nhwc
from .conv_plan import ConvGeom, convT_out_size
from . import conv_plan
from . import scratch
from .upfirdn2d import _geometry, blur_bias_act, blur_pads, upfirdn2d, upfirdn2d_raw
from .fused_act import bias_sink, fused_leaky_relu
from .grad_sink import weight_grad


def pixel_dot(a: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """out[b,c] = sum over pixels of a[b,c,h,w]*g[b,c,h,w] (both NHWC in memory), a float64 [B,C] (double products and sums)."""
    a, g = _nhwc(a), _nhwc(g)
    b, c, h, w = a.shape
    out = scratch.zeros((b, c), a.device, torch.float64)          # consumed (divided into a new tensor) before the caller returns
    if a.dtype != g.dtype:
        a, g = a.float(), g.float()
    if a.dtype == torch.bfloat16 and c % 4:
        a, g = a.float(), g.float()
    rc = _lib.load().ideas_pixel_dot(_lib.ptr(out), _lib.ptr(a), _lib.ptr(g), b, h * w, c, _lib.act_dtype(a), _lib.stream_ptr())
    _lib.check(rc, "ideas_pixel_dot")
    return out


def _weight_sqsum(w: torch.Tensor, scale: float, dtype, entry: str, key: str) -> torch.Tensor:
    def make():
        cout, cin, kh, kw = w.shape
        wsq = torch.empty((cout, cin), device=w.device, dtype=dtype)
        _lib.check(getattr(_lib.load(), entry)(_lib.ptr(wsq), _lib.ptr(w), cout, cin, kh, kw, *w.stride(), float(scale * scale),
                                               _lib.stream_ptr()), entry)
        return wsq
    return conv_plan.cached(w, (key, float(scale)), make)


def weight_sqsum(w: torch.Tensor, scale: float) -> torch.Tensor:
    """wsq[o,i] = scale^2 * sum_k W[o,i,k]^2 (one kernel over the parameter in whatever strides it has; memoised per optimiser
    step like the other derived weights)."""
    return _weight_sqsum(w, scale, torch.float32, "ideas_weight_sqsum", "wsq")


def weight_sqsum_f64(w: torch.Tensor, scale: float) -> torch.Tensor:
    """The same table in double, for the backward's demodulation algebra (ideas_demod_bwd); memoised like the f32 one."""
    return _weight_sqsum(w, scale, torch.float64, "ideas_weight_sqsum_f64", "wsq64")


def demod_raw(s: torch.Tensor, wsq: torch.Tensor, eps: float) -> torch.Tensor:
    """d[b,o] = rsqrt((s*s) @ wsq^T + eps) on the shuffle-reduction kernel (no autograd: the modulated-conv Functions own the
    derivative, _style_grads / _demod_wgrad)."""
    return _demod_raw(s.detach(), wsq, eps)


def demod_of(w: torch.Tensor, s: torch.Tensor, gain: float, eps: float) -> torch.Tensor:
    """demod_raw(s, weight_sqsum(w, gain), eps), memoised on (weight, style tensor) while the derived-weight cache is on: the same
    styles reach a layer two or three times per iteration, and the bf16 packs of the input gradients are keyed on this tensor."""
    sd = s.detach()
    return conv_plan.cached_on(w, ("demod", float(gain), float(eps)), sd, lambda: _demod_raw(sd, weight_sqsum(w, gain), eps))


def _demod_raw(s: torch.Tensor, wsq: torch.Tensor, eps: float) -> torch.Tensor:
    b, cin = s.shape
    cout = wsq.shape[0]
    d = torch.empty((b, cout), device=s.device, dtype=torch.float32)
    rc = _lib.load().ideas_demod(_lib.ptr(d), _lib.ptr(s), _lib.ptr(wsq), b, cin, cout, float(eps), _lib.stream_ptr())
    _lib.check(rc, "ideas_demod")
    return d


def _style_grads(dot_s, dot_d, s, d, w, gain: float, eps: float = 1e-8):
    """(gs, gq) of one modulated conv from its two per-sample reductions (float64 [B,Cin] / [B,Cout]): the direct term
    <x, dL/d(s x)> = dot_s / s and the term through the demodulation d(s, W), by ideas_demod_bwd, which works in double -- the two
    terms cancel to a small remainder -- and OVERWRITES dot_d (with gq in double, its own intermediate).  gq[b,o] = dL/dq of d = rsqrt(q + eps) is what the weight gradient through the
    demodulation needs (_demod_wgrad).
    Where s == 0 exactly the direct quotient is undefined and 0 is used (the true value needs a second, unscaled
    input-gradient launch; s = affine(style) with bias 1 never hits an exact zero in training — DESIGN.md §5)."""
    b, cin = s.shape
    gs = torch.empty_like(s)
    gq = wsq = None
    cout = w.shape[0]
    if dot_s.dtype != torch.float64 or (dot_d is not None and dot_d.dtype != torch.float64):
        raise RuntimeError("_style_grads takes the float64 accumulators of pixel_dot / act_bwd_dot")
    if d is not None:
        gq, wsq = torch.empty_like(d), weight_sqsum_f64(w, gain)
    rc = _lib.load().ideas_demod_bwd(_lib.ptr(gs), _lib.ptr(gq), _lib.ptr(dot_s), _lib.ptr(dot_d), _lib.ptr(d), _lib.ptr(s),
                                     _lib.ptr(wsq), b, cin, cout, float(eps), _lib.stream_ptr())
    _lib.check(rc, "ideas_demod_bwd")
    return gs, gq


def _demod_wgrad(gw: torch.Tensor, w: torch.Tensor, gq: torch.Tensor, s: torch.Tensor, gain: float) -> None:
    """gw[o,i,k] += 2 gain^2 W[o,i,k] * sum_b gq[b,o] s[b,i]^2: the weight gradient through wsq, added in place."""
    cout, cin, kh, kw = w.shape
    rc = _lib.load().ideas_demod_wgrad(_lib.ptr(gw), _lib.ptr(w), _lib.ptr(gq), _lib.ptr(s), s.shape[0], cout, cin, kh, kw,
                                       *w.stride(), *gw.stride(), float(2.0 * gain * gain), _lib.stream_ptr())
    _lib.check(rc, "ideas_demod_wgrad")


def act_bwd_dot(gy: torch.Tensor, out: torch.Tensor, bias: torch.Tensor, alpha: float, act_gain: float, bias_grad_into=None):
    """(g_pre, bias_grad[C], dot[B,C] float64) from the incoming gradient and the saved post-activation output.  ``bias_grad_into``: add
    the bias gradient into that f32 [C] buffer (the parameter's .grad) instead of returning a fresh one (returns None for it)."""
    gy, out = _nhwc(gy), _nhwc(out)
    if gy.dtype != out.dtype:
        gy = gy.to(out.dtype)
    b, c, h, w = out.shape
    gpre = torch.empty_like(out)
    bg = bias_grad_into if bias_grad_into is not None else torch.zeros(c, device=out.device, dtype=torch.float32)
    dot = scratch.zeros((b, c), out.device, torch.float64)
    rc = _lib.load().ideas_act_bwd_dot(_lib.ptr(gpre), _lib.ptr(bg), _lib.ptr(dot), _lib.ptr(gy), _lib.ptr(out),
                                       _lib.ptr(bias), None, b, h * w, c, float(alpha), float(act_gain), _lib.act_dtype(out),
                                       _lib.stream_ptr())
    _lib.check(rc, "ideas_act_bwd_dot")
    return gpre, (None if bias_grad_into is not None else bg), dot


def _mod_geom(mode: str, k: int) -> ConvGeom:
    """The conv of each mode: same-resolution (pad k // 2); up: stride 2, run as the input gradient of that conv; down: stride 2
    behind the Blur -- a 1x1 kernel: unstrided behind the decimating FIR, as ConvLayer's skip branch."""
    if mode == "same":
        return ConvGeom(k, k, 1, k // 2, False)
    return ConvGeom(k, k, 1 if (mode == "down" and k == 1) else 2, 0, False)


def _down_blur(x, fir, k: int, pad2):
    """(down, pad4, blurred size, the adjoint's pads) of the down mode's Blur: ``upfirdn2d(x, fir, down=down, pad=pad2)``."""
    down = 2 if k == 1 else 1
    return (down,) + _geometry((x.shape[2], x.shape[3]), fir, 1, down, pad2)


def _mod_forward(x, w, s, d, mode: str, fir, pad2, gain: float, bias=None, slope: float = 0.2, act_gain: float = 1.0, resid=None,
                 want_xb: bool = False):
    """(y, xb) of one modulated conv from its scales ``s`` [B, Cin] / ``d`` [B, Cout] or None: the only place that picks the raw
    call.  ``bias``: bias + leaky-ReLU in the conv epilogue (same and down).  ``xb``: the down mode's blurred tensor (None where
    the fused launch was not asked for it), None in the other modes."""
    k = w.shape[2]
    g = _mod_geom(mode, k)
    epi = dict(lin=s, lout=d, bias=bias, act=bias is not None, act_gain=act_gain, alpha=slope)
    if mode == "same":                                              # stylegan2/model.py:271-275
        return conv_fwd_raw(x, w, g, gain, resid=resid, **epi), None
    if mode == "up":                                                # :250-260; w.transpose: read as conv weight [O'=Cin, I'=Cout]
        return conv_dgrad_raw(x, w.transpose(0, 1), g, convT_out_size(x.shape[2], x.shape[3], g), gain, lin=s, lout=d), None
    # down (:263-269): ONE kernel (ideas_b3_blur_conv_s2_mod) where ``mod_blur_conv_ok`` admits the shape (looked up through the
    # module at call time), else the blur kernel + the scaled stride-2 conv
    if k == 3 and _conv.mod_blur_conv_ok(x, w, fir, pad2, want_xb=want_xb):
        return _conv.blur_conv_s2_raw(x, w, fir, pad2, gain, want_xb=want_xb, **epi)
    down, pad4, bhw, _ = _down_blur(x, fir, k, pad2)
    xb = upfirdn2d_raw(x, fir, (1, 1), (down, down), pad4, bhw, flip=True)
    return conv_fwd_raw(xb, w, g, gain, **epi), xb


class _ModConv(Function):
    """y = gain * d[b,o] * conv(s[b,i] * x, W) in one of three modes -- ``same`` (pad k // 2), ``up`` (the stride-2 transposed
    variant; its Blur follows outside) and ``down`` (stylegan2/model.py:210-216, 263-269: Blur, then the stride-2 conv) -- with the
    demodulation d = rsqrt(sum_i s^2 wsq + eps) (``demod``) computed and differentiated inside: the backward returns the complete
    style gradient (direct + through d) and adds the through-d term to the weight gradient, 2 small kernels instead of ~20 tensor ops.

    ``b`` (same and down): bias + leaky-ReLU in the conv epilogue (StyledConv_without_noise, stylegan2/model.py:371-377).  Only the
    post-activation output is kept for the backward; the pre-activation needed by d(demod) is recovered inside the fused
    backward-prologue kernel (ideas_act_bwd_dot).

    Down is re-associated like the other modes -- the blur is linear and per channel, so the style scales the BLURRED activation:

        y[b,o] = gain * d[b,o] * sum_{i,k} W[o,i,k] * (s[b,i] * xb[b,i, 2. + k]),   xb = upfirdn2d(x, fir, pad2)

    The blurred tensor is kept only for the weight gradient (the fused kernel's side output); the style gradient's direct term is
    taken on the raw side, <x, B^T g> = <B x, g> per sample and channel."""

    @staticmethod
    def forward(ctx, x, w, s, b, mode: str, fir, pad2, gain: float, demod: bool, eps: float, slope: float, act_gain: float):
        x = _nhwc(x)
        s = s.contiguous()
        ctx.bias_ref = b                      # the parameter (gradient sink), not its contiguous copy
        if b is not None:
            b = b.contiguous()
        d = demod_of(w, s, gain, eps) if demod else None
        need_w = ctx.needs_input_grad[1]
        y, xb = _mod_forward(x, w, s, d, mode, fir, pad2, gain, b, slope, act_gain, want_xb=need_w)
        ctx.mode, ctx.pad2, ctx.gain, ctx.eps, ctx.slope, ctx.act_gain = mode, pad2, gain, eps, slope, act_gain
        keep = dict(x=x, w=w, s=s, fir=fir, d=d, b=b,
                    y=y if (b is not None or d is not None) else None,     # read by the activation backward / the demodulation term only
                    xb=xb if need_w else None)
        ctx.names = [n for n, t in keep.items() if t is not None]
        ctx.save_for_backward(*(keep[n] for n in ctx.names))
        return y

    @staticmethod
    @once_differentiable          # raw kernels below: a create_graph pass must use second_order() and raises otherwise
    def backward(ctx, gy):
        t = dict(zip(ctx.names, ctx.saved_tensors))
        x, w, s, d, b, y = t["x"], t["w"], t["s"], t.get("d"), t.get("b"), t.get("y")
        mode, gain = ctx.mode, ctx.gain
        g = _mod_geom(mode, w.shape[2])
        need_x, need_w, need_s, need_b = ctx.needs_input_grad[:4]
        gb = dot_d = None
        if b is not None:
            gpre, gb, dot_d = act_bwd_dot(gy, y, b, ctx.slope, ctx.act_gain, bias_grad_into=bias_sink(ctx.bias_ref) if need_b else None)
        else:
            gpre = gy = _nhwc(gy)
        gx = gw = gs = gq = None
        if need_x or need_s:                  # the conv's input gradient: the per-sample scales trade places
            if mode == "up":
                gx = conv_fwd_raw(gpre, w.transpose(0, 1), g, gain, lin=d, lout=s)
            elif mode == "same":
                gx = conv_dgrad_raw(gpre, w, g, (x.shape[2], x.shape[3]), gain, lin=d, lout=s)
            else:                             # ... and the blur's adjoint
                down, _, bhw, g_pad = _down_blur(x, t["fir"], w.shape[2], ctx.pad2)
                gx = conv_dgrad_raw(gpre, w, g, bhw, gain, lin=d, lout=s)
                gx = upfirdn2d_raw(gx, t["fir"], (down, down), (1, 1), g_pad, (x.shape[2], x.shape[3]), flip=False)
        if need_s or (need_w and d is not None):
            dot_s = pixel_dot(x, gx) if need_s else scratch.zeros(tuple(s.shape), s.device, torch.float64)
            if d is not None and dot_d is None:
                dot_d = pixel_dot(gy, y)
            gs, gq = _style_grads(dot_s, dot_d, s, d, w, gain, ctx.eps)
        if need_w:
            xin = t["xb"] if mode == "down" else x            # what the conv read

            def grad(out):
                if mode == "up":              # the transposed conv's weight [Cin, Cout]: operand roles and scales trade places
                    r = conv_wgrad_raw(xin, gpre, g, (w.shape[1], w.shape[0], w.shape[2], w.shape[3]), gain, lin=d, lout=s,
                                       out=None if out is None else out.transpose(0, 1)).transpose(0, 1)
                else:
                    r = conv_wgrad_raw(gpre, xin, g, tuple(w.shape), gain, lin=s, lout=d, out=out)
                if gq is not None:
                    _demod_wgrad(r, w, gq, s, gain)
                return r
            gw = weight_grad(w, grad, gpre, xin, s, d, gq)
        return ((gx if need_x else None), gw, (gs if need_s else None), (gb if need_b else None),
                None, None, None, None, None, None, None, None)


_SECOND_ORDER = [False]


class second_order:
    """Context manager: build the modulated conv from individually double-differentiable ops
    (x*s -> conv2d / conv_transpose2d -> *d, demodulation in plain torch) so that
    ``autograd.grad(..., create_graph=True)`` w.r.t. the style works — what the path-length regulariser
    (stylegan2/train.py:85-98) needs.  Two extra elementwise passes; used only on those regularisation steps."""

    def __enter__(self):
        self.prev = _SECOND_ORDER[0]
        _SECOND_ORDER[0] = True
        return self

    def __exit__(self, *exc):
        _SECOND_ORDER[0] = self.prev


def _modulated_conv2d_composite(x, w, style, demodulate, upsample, fir, eps, act_bias, negative_slope, act_scale, downsample=False):
    cout, cin, k, _ = w.shape
    scale = 1.0 / math.sqrt(cin * k * k)
    xs = x * style.view(style.shape[0], cin, 1, 1)
    if downsample:
        y = conv2d(upfirdn2d(xs, fir, pad=blur_pads(fir.shape[0], k, up=False)), w, None, stride=2, padding=0, gain=scale)
    elif upsample:
        y = conv_transpose2d(xs, w.transpose(0, 1), None, stride=2, gain=scale)
    else:
        y = conv2d(xs, w, None, stride=1, padding=k // 2, gain=scale)
    if demodulate:
        wsq = (w * w).sum(dim=(2, 3)) * (scale * scale)
        d = torch.rsqrt((style * style) @ wsq.t() + eps)
        y = y * d.view(d.shape[0], cout, 1, 1)
    if upsample:
        y = upfirdn2d(y, fir, pad=blur_pads(fir.shape[0], k, up=True))
    if act_bias is not None:
        y = fused_leaky_relu(y, act_bias, negative_slope, act_scale)
    return y


def modulated_conv2d(x: torch.Tensor, weight: torch.Tensor, style: torch.Tensor, demodulate: bool = True,
                     upsample: bool = False, fir: Optional[torch.Tensor] = None, eps: float = 1e-8,
                     act_bias: Optional[torch.Tensor] = None, negative_slope: float = 0.2,
                     act_scale: float = 2 ** 0.5, resid: Optional[torch.Tensor] = None, downsample: bool = False) -> torch.Tensor:
    """``x`` [B,Cin,H,W]; ``weight`` [1,Cout,Cin,k,k] (the reference's parameter); ``style`` [B,Cin] = the
    already-affine-transformed modulation (stylegan2/model.py:239).  ``fir`` = the 4x4 blur (
    here) used after the stride-2 transposed conv (stylegan2/model.py:202-208, 258-261); it already carries the x4
    upsample gain.  ``act_bias`` fuses the FusedLeakyReLU that always follows (stylegan2/model.py:374-375).
    ``downsample``: the Blur (``fir``, unit gain, pads of stylegan2/model.py:212-216) in front of a stride-2 conv (:263-269)."""
    if upsample and downsample:
        raise ValueError("modulated_conv2d: upsample and downsample are exclusive")
    _lib.require_cuda(x, weight, style)
    mode = "down" if downsample else "up" if upsample else "same"
    if mode != "same" and fir is None:
        raise RuntimeError(f"modulated_conv2d({mode}sample=True) needs the blur FIR")
    if downsample:
        if resid is not None:
            raise RuntimeError("modulated_conv2d(resid=...) is the no-grad fast path of the fused same-resolution conv")
        _lib.require_cuda(fir, act_bias)
    x, style = to_act(x), to_f32(style)
    if resid is not None:
        resid = to_act(resid)
    w = weight[0] if weight.dim() == 5 else weight
    cout, cin, k, _ = w.shape
    if _SECOND_ORDER[0] and torch.is_grad_enabled() and resid is None:
        return _modulated_conv2d_composite(x, w, style, demodulate, upsample, fir, eps, act_bias, negative_slope, act_scale, downsample)
    scale = 1.0 / math.sqrt(cin * k * k)
    pad2 = blur_pads(fir.shape[0], k, up=upsample) if mode != "same" else None
    # bias + leaky-ReLU ride in the conv epilogue of the same and down modes; elsewhere the activation follows as its own op
    fuse_act = act_bias is not None and not upsample and demodulate and cout % 4 == 0
    if resid is not None:
        if not fuse_act or torch.is_grad_enabled():
            raise RuntimeError("modulated_conv2d(resid=...) is the no-grad fast path of the fused same-resolution conv")
        style = style.contiguous()
        d = demod_raw(style, weight_sqsum(w, scale), eps)
        return _mod_forward(x, w, style, d, mode, None, None, scale, act_bias.contiguous(), float(negative_slope), float(act_scale),
                            resid=resid)[0]
    y = _ModConv.apply(x, w, style, act_bias if fuse_act else None, mode, *((fir, pad2) if downsample else (None, None)),
                       scale, bool(demodulate), float(eps), float(negative_slope), float(act_scale))
    if upsample:
        if act_bias is not None:          # blur + bias + leaky-ReLU in one pass over the upsampled tensor
            return blur_bias_act(y, fir, pad2, act_bias, negative_slope, act_scale)
        return upfirdn2d(y, fir, pad=pad2)
    if act_bias is not None and not fuse_act:
        y = fused_leaky_relu(y, act_bias, negative_slope, act_scale)
    return y
