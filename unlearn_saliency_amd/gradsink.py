"""Where a custom backward node puts a parameter's gradient: ONE rule, `dest(p)` / `pair(gamma, beta)`.

With the flat arena (flat.py) every parameter's `.grad` is a persistent view of one fp32 vector that is zeroed
once per step.  autograd's own route — return dW from backward, AccumulateGrad does `.grad += dW` — costs one extra
elementwise launch per parameter per step (62 for ResNet-18, 334 for the DDPM U-Net).  The kernels that produce
weight gradients here can accumulate into a destination themselves (`salun_conv2d_backward_weight(accumulate=1)`,
`salun_bn_backward(grad_*_acc)`), so a custom Function asks `dest(p)` for a `Dest`, hands the kernel `Dest.out` and
`Dest.accumulate`, and returns `Dest.returned(...)` to autograd: None when the kernel added into `.grad`, else the
tensor the kernel produced.

`sink(p)` is None — and the gradient goes back to autograd — whenever that shortcut is not provably equivalent: no
`.grad` yet, a non-contiguous / non-fp32 `.grad`, gradient hooks on the tensor, or a double-backward
(`torch.is_grad_enabled()` inside backward means create_graph=True).
"""
from __future__ import annotations

import torch

_enabled = True


def enable(flag: bool) -> None:
    global _enabled
    _enabled = bool(flag)


def sink(p):
    if not _enabled or p is None or not isinstance(p, torch.nn.Parameter) or torch.is_grad_enabled():
        return None
    g = p.grad
    if g is None or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape or not g.is_cuda:
        return None
    if p._backward_hooks:  # tensor hooks would see / rewrite the incoming gradient: keep autograd's route
        return None
    return g


class Dest:
    """Destination of one parameter's gradient.  `out`: the tensor the kernel writes — the parameter's `.grad` (then
    `accumulate` is True: the kernel adds), a fresh tensor, or None when the kernel allocates its result itself."""
    __slots__ = ("out", "accumulate")

    def __init__(self, out, accumulate: bool):
        self.out, self.accumulate = out, accumulate

    def returned(self, produced=None):
        """What the node returns to autograd for this parameter: None when the kernel added into `.grad`, else the
        gradient (`produced`: what the kernel returned, for a kernel that allocates; default `out`).
        Nothing else to do on arrival: autograd still runs the leaf's AccumulateGrad node when the Function returns None
        for it, and that node fires the post-accumulate-grad hooks (the bucketed all-reduce of dist.BucketedGradReducer)
        exactly once, after our kernels were enqueued, so stream order holds.  tests/test_gradsink.py pins this engine
        behaviour; if it ever changes, fire the hooks HERE."""
        if self.accumulate:
            return None
        return self.out if produced is None else produced

    def add(self, g):
        """A gradient some other launch produced (a sum shared by two parameters): added into `.grad`, or handed on."""
        if self.accumulate:
            self.out.add_(g)
            return None
        return g


def dest(p, fresh=None, when: bool = True) -> Dest:
    """The destination of `p`'s gradient: `sink(p)` if `when` (the site's own condition for the shortcut) and the sink
    exists; else `fresh(p.shape, ...)` (`torch.empty` / `torch.zeros`), or no tensor (the kernel allocates)."""
    g = sink(p) if when else None
    if g is not None:
        return Dest(g, True)
    return Dest(fresh(p.shape, dtype=torch.float32, device=p.device) if fresh is not None else None, False)


def pair(gamma, beta, fresh=None):
    """(Dest, Dest) of a norm layer's gamma / beta, whose kernels have ONE accumulate switch: both sunk, or neither."""
    gw, gb = sink(gamma), sink(beta)
    if gw is not None and gb is not None:
        return Dest(gw, True), Dest(gb, True)
    return dest(gamma, fresh, False), dest(beta, fresh, False)
