"""Gradient sink.  Inside ``with grad_sink(params):`` the weight gradients of those parameters are produced on a side
stream and accumulated straight into their (pre-existing, e.g. flat-bucket) ``.grad`` — the Functions return None
for the weight, so autograd neither allocates, zero-fills nor adds.  The weight-gradient kernels (MFMA-bound) then
overlap the HBM-bound elementwise backward passes of the following layers on the main stream.  Leaving the context
joins the side stream.  Only plain backward passes qualify (no create_graph), and only parameters named by the caller:
a Function cannot see the ``inputs=`` filter of ``torch.autograd.backward``.
"""
from __future__ import annotations

import os

import torch

from .. import _lib

_SINK = {"ids": None, "stream": None}
# IDEAS_SINK_PRIORITY=low puts the side stream on the device's LOWEST priority (ideas_stream_create).  Measured round 5, same box,
# interleaved: f32 412.2 -> 413.6 ms, bf16 154.7 -> 154.2 ms (noise) -- and the same with the whole iteration on a highest-priority
# stream (414.2 ms).  A kernel trace shows 20-us torch adds of the main stream taking up to 1.9 ms next to a weight-gradient grid, but
# the chip is busy throughout: the queue priority changes who waits, not how much work the compute units retire.  Default: off.
SINK_LOW_PRIORITY = os.environ.get("IDEAS_SINK_PRIORITY", "default") == "low"
_SIDE_STREAM = os.environ.get("IDEAS_SIDE_STREAM", "1") != "0"


class grad_sink:
    """``defer=True``: leaving the context does NOT join the side stream; the caller does (``join()``) before it consumes the
    gradients.  The D phase's weight gradients are wanted only by the discriminators' optimiser step, which the step defers to the
    first discriminator call of the G phase (train_step._Deferred) -- until then they may keep running under the generator
    forwards of the G phase instead of holding the main stream at the end of the backward pass."""

    def __init__(self, params, defer: bool = False):
        self.ids = {id(p) for p in params if p.grad is not None and p.is_cuda}
        self.defer = defer
        self.pending = False

    def __enter__(self):
        if not self.ids:            # nothing to sink (no pre-existing device gradients): plain autograd
            return self
        if _SINK["stream"] is None:
            _SINK["stream"] = _lib.make_stream(-1) if SINK_LOW_PRIORITY else torch.cuda.Stream()
        _SINK["ids"] = self.ids
        return self

    def __exit__(self, *exc):
        if _SINK["ids"] is not None:
            _SINK["ids"] = None
            if self.defer and exc[0] is None:
                self.pending = True
            else:
                torch.cuda.current_stream().wait_stream(_SINK["stream"])

    def join(self):
        if self.pending:
            self.pending = False
            torch.cuda.current_stream().wait_stream(_SINK["stream"])


def _sink_target(w: torch.Tensor):
    ids = _SINK["ids"]
    if ids is None or torch.is_grad_enabled():
        return None
    base = w._base if w._base is not None else w
    if id(base) not in ids:
        return None
    gr = base.grad
    if gr is None or gr.shape != base.shape or gr.stride() != base.stride():
        return None
    if base is w:
        return gr
    if w.numel() != base.numel() or w.data_ptr() != base.data_ptr():
        return None
    return gr.as_strided(w.shape, w.stride())


def weight_grad(w: torch.Tensor, compute, *uses):
    """``compute(out)`` -> the gradient of ``w`` (added to ``out`` when that is not None).  Returns it, or None after
    sinking it into ``w.grad`` on the side stream (``uses``: the tensors the kernels read, for the allocator)."""
    tgt = _sink_target(w)
    if tgt is None:
        return compute(None)
    if not _SIDE_STREAM:                 # (A/B only: same in-place accumulation, on the current stream)
        compute(tgt)
        return None
    side, cur = _SINK["stream"], torch.cuda.current_stream()
    side.wait_stream(cur)
    for t in uses:
        if t is not None:
            t.record_stream(side)
    with torch.cuda.stream(side):
        compute(tgt)
    return None
