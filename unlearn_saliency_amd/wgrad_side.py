"""Backward-weight on a side stream, beside backward-data.

Backward-weight and backward-data of one convolution depend on the same dY and on nothing of each other.  The
backward-weight kernel runs ONE wave per SIMD (register budget) and leaves LDS for a second workgroup, so issuing it on a
side stream lets the two kernels share the CUs — the matrix pipes idle less than when either runs alone.  Every such
launch (resblock.py, conv.py, conv_bf16.py) goes through `beside()`, which

  1. makes the side stream wait for the main stream (dy and everything before it are complete for it);
  2. launches the kernel on the side stream: the stream is passed to the ops.py wrapper, no `torch.cuda.stream` context
     (~10 us of host time per use; an SD step has ~470 of them and is host-bound);
  3. `record_stream`s the tensors it reads on the side stream (they are freed when the backward node returns);
  4. keeps autograd from accumulating into dy in place meanwhile (`hold_until_join`);
  5. queues one join of the main stream behind the side stream at the end of the backward pass.

The policy around it — where the gradient goes, whether the launch runs beside backward-data, when the node must join the
streams itself — is `ConvWgrad` for the nodes that walk several fp32 convolutions by hand (resblock.py); the single-layer
nodes (conv._ConvFn, conv_bf16._weight_bias_grad) overlap only what lands in `.grad` and never join.

Under data parallel a gradient slice's all-reduce waits for the side stream itself (dist.BucketedGradReducer).
SALUN_WGRAD_OVERLAP=0 keeps everything on one stream.  `overlap_disabled()` rebinds `OVERLAP`: read it as
`wgrad_side.OVERLAP`, never through `from ... import`.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import gradsink, ops, streams

OVERLAP = os.environ.get("SALUN_WGRAD_OVERLAP", "1") != "0"


class overlap_disabled:
    """Context manager: keep backward-weight on the main stream.  Needed whenever something else than the
    convolution kernels writes a parameter's `.grad` during the same backward pass — e.g. the l1 penalty of FT_l1 /
    GA_l1 (`_steps.l1_regularization`), whose AccumulateGrad `w.grad.add_()` runs on the main stream and would race
    with a side-stream `salun_conv2d_backward_weight` accumulating into the same slice."""

    def __enter__(self):
        global OVERLAP
        self._prev = OVERLAP
        OVERLAP = False
        return self

    def __exit__(self, *exc):
        global OVERLAP
        OVERLAP = self._prev
        return False


_streams: dict = {}


def stream(device: torch.device) -> "torch.cuda.Stream":
    """The side stream of `device`, created at first use (with a hardware queue of its own, streams.py)."""
    s = _streams.get(device)
    if s is None:
        s = _streams[device] = streams.concurrent_stream(device)
    return s


def existing_stream(device: torch.device) -> Optional["torch.cuda.Stream"]:
    """The side stream of `device` if one was ever created, else None."""
    return _streams.get(device)


_join_queued: set = set()
# Gradient tensors a side-stream kernel is still reading.  autograd OWNS a gradient buffer once every node it was handed
# to has returned, and accumulates further contributions into it IN PLACE when nobody else holds it
# (InputBuffer::add: `old.add_(new)` if use_count == 1) — on the main stream, while the side stream may still be reading
# it: `record_stream` guards against reuse after free, not against that write.  A held reference makes the engine
# accumulate out of place.  Found in round 4 (the first AttnBlock's proj_out weight gradient changed from run to run
# once the attention's backward became short enough for the residual's accumulation to overtake the 1x1 backward-weight).
_held: dict = {}


def hold_until_join(t: torch.Tensor) -> None:
    """Keep `t` referenced until the side stream has passed the kernels enqueued on it so far, at the latest until the
    end-of-backward join.  One event per EIGHT tensors (an event per tensor was 11 us of host time on each of ~470
    backward-weight launches of an SD step): a batch is released when the event recorded behind its last member has
    completed.  Inside a stream capture events cannot be queried: the references simply live until the join."""
    st = _held.get(t.device)
    if st is None:
        st = _held[t.device] = {"open": [], "closed": []}
    st["open"].append(t)
    if len(st["open"]) < 8 or torch.cuda.is_current_stream_capturing():
        return
    ev = torch.cuda.Event()
    ev.record(stream(t.device))
    st["closed"].append((ev, st["open"]))
    st["open"] = []
    closed = st["closed"]
    while closed and closed[0][0].query():
        closed.pop(0)


def release_held(device) -> None:
    """After the main stream has been made to wait for the side stream: nothing is being read there any more."""
    _held.pop(device, None)


def _join_at_end_of_backward(device: torch.device) -> None:
    """Single process: the main stream waits for the side stream ONCE, when the whole backward pass has been issued
    (autograd's end-of-backward callback) — so after `loss.backward()` returns, gradients are ordered on the current
    stream as usual, and inside the pass the weight-gradient kernels of one block overlap the next block's work.
    Caveat: if a backward pass dies with an exception the engine drops its callbacks; call `reset_join_state()` (or
    set SALUN_WGRAD_OVERLAP=0) before reusing the process after such a failure."""
    if device in _join_queued:
        return
    _join_queued.add(device)

    def _join():
        _join_queued.discard(device)
        torch.cuda.current_stream(device).wait_stream(stream(device))
        _held.pop(device, None)

    torch.autograd.Variable._execution_engine.queue_callback(_join)


def reset_join_state() -> None:
    """Forget a pending end-of-backward join (only needed after a backward pass was aborted by an exception) and make
    the current streams wait for whatever the side streams still have in flight."""
    _join_queued.clear()
    _held.clear()
    for dev, side in _streams.items():
        torch.cuda.current_stream(dev).wait_stream(side)


def beside(device: torch.device, reads, launch, alloc: bool = False):
    """Steps 1 - 5 above around `launch(side)`, which issues the kernel on the side stream (the `stream=` argument of
    the ops.py wrappers); returns what `launch` returned.  `reads`: the tensors the kernel reads, dy last.  With
    `alloc` the result is a fresh tensor (no `.grad` sink), which must belong to the side stream: the stream context is
    entered, and the result is recorded on the main stream, which consumes it.  A launch that returns None launched
    nothing."""
    main, side = torch.cuda.current_stream(device), stream(device)
    side.wait_stream(main)
    if alloc:
        with torch.cuda.stream(side):
            out = launch(side)
        if out is not None:
            out.record_stream(main)
    else:
        out = launch(side)
    if out is not None:
        for t in reads:
            t.record_stream(side)
        hold_until_join(reads[-1])
        _join_at_end_of_backward(device)
    return out


class ConvWgrad:
    """The weight gradients of the fp32 convolutions of ONE backward node that walks several layers by hand
    (resblock.py): `wgrad(xin, dy, w, stride, pad)` per convolution, `wgrad.finish()` before the node returns.
    Each gradient goes where gradsink.dest(w) says; the launch runs beside backward-data whenever `OVERLAP` (read once
    per node), else on the main stream.  A gradient that goes back to autograd from the side stream is consumed by
    AccumulateGrad on the main stream as soon as the node returns, so `finish()` joins the streams then — and only then:
    gradients added into `.grad` wait for the end-of-backward join."""
    __slots__ = ("device", "overlap", "join")

    def __init__(self, device: torch.device):
        self.device, self.overlap, self.join = device, OVERLAP, False

    def __call__(self, xin, dy, w, stride: int, pad: int):
        d = gradsink.dest(w)
        if self.overlap:
            dw = beside(self.device, (xin, dy), lambda side: ops.conv2d_backward_weight(
                xin, dy, w.shape, stride, pad, out=d.out, accumulate=d.accumulate, shared=True, stream=side),
                alloc=not d.accumulate)
        else:
            dw = ops.conv2d_backward_weight(xin, dy, w.shape, stride, pad, out=d.out, accumulate=d.accumulate)
        dw = d.returned(dw)
        if dw is not None:
            self.join = self.overlap
        return dw

    def finish(self) -> None:
        if self.join:
            torch.cuda.current_stream(self.device).wait_stream(stream(self.device))
            release_held(self.device)
