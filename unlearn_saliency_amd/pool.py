"""`nn.MaxPool2d(2, 2)` on K24 (csrc/salun_pool.hip).

`maxpool2x2(x)` is one autograd node: one forward and one backward launch.  It saves the byte map of selected
positions only — the input is not kept alive for the backward.  Inputs outside the kernel's domain (odd sizes,
non-fp32, CPU tensors, autocast regions) run `F.max_pool2d` — LOUDLY: every such call is counted in
`LIBRARY_POOL_CALLS`, as `conv.LIBRARY_CONV_CALLS` counts the convolutions that went to the library.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import ops
from .fastfn import FastFunction

# calls that went to the library pooling instead of K24, by reason
LIBRARY_POOL_CALLS = {"shape": 0, "dtype_or_autocast": 0}


def library_pool_calls() -> int:
    return sum(LIBRARY_POOL_CALLS.values())


def reset_library_pool_calls() -> None:
    for k in LIBRARY_POOL_CALLS:
        LIBRARY_POOL_CALLS[k] = 0


class _MaxPool2x2(FastFunction):
    @staticmethod
    def forward(ctx, x):
        y, idx = ops.maxpool2x2_forward(x)
        ctx.save_for_backward(idx)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        return ops.maxpool2x2_backward(dy.contiguous(), idx)


def maxpool2x2(x: torch.Tensor) -> torch.Tensor:
    """max_pool2d(x, kernel_size=2, stride=2) with the library's selection rule (first of equal maxima, NaN wins)."""
    if not (x.is_cuda and x.dtype == torch.float32) or torch.is_autocast_enabled():
        LIBRARY_POOL_CALLS["dtype_or_autocast"] += 1
        return F.max_pool2d(x, 2, 2)
    if x.dim() != 4 or x.shape[2] < 2 or x.shape[3] < 2 or x.shape[2] % 2 or x.shape[3] % 2 or x.shape[0] * x.shape[1] < 1:
        LIBRARY_POOL_CALLS["shape"] += 1
        return F.max_pool2d(x, 2, 2)
    return _MaxPool2x2.apply(x.contiguous())
