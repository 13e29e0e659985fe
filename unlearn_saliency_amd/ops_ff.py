"""Tensor-level wrappers of the Fisher-forgetting kernels (K18, csrc/salun_ff.hip; include/salun.h).

Same conventions as ops.py / ops_iu.py: device tensors only, raw pointers and the current stream handed to
libsalun.so, a failing call raises `SalunError`.  `F` of the grouped-square wrappers is an fp32 device tensor that is
ADDED into, so one flat vector in arena layout collects every layer of a network over every batch.  `dy` stacks the G
class groups along the batch axis, (G*B, ...); `x` is the layer input of ONE group, (B, ...), shared by all groups.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _lib, ops, weightimg
from ._lib import c_double, c_int64, c_uint64, check
from .ops import _dev, _stream


def _groups(dy: torch.Tensor, B: int, w: torch.Tensor) -> int:
    G = w.numel()
    if G < 1 or dy.shape[0] != G * B:
        raise ValueError(f"dy has {dy.shape[0]} rows; expected G * B = {G} * {B}")
    return G


def conv_sq(x: torch.Tensor, dy: torch.Tensor, w: torch.Tensor, F: torch.Tensor, stride: int, pad: int) -> None:
    """F (K, C, R, R) += sum_g w[g] conv2d_backward_weight(x, dy[g*B:(g+1)*B])^2.  x: (B, C, H, W)."""
    B, C, H, W = x.shape
    K, P, Q = dy.shape[1], dy.shape[2], dy.shape[3]
    G = _groups(dy, B, w)
    if F.dim() != 4 or F.shape[0] != K or F.shape[1] != C or F.shape[2] != F.shape[3]:
        raise ValueError(f"F {tuple(F.shape)} is not a (K={K}, C={C}, R, R) weight")
    R = F.shape[2]
    L = _lib.lib()
    nbytes = int(L.salun_ff_conv_sq_workspace_bytes(G, B, C, K, R, P, Q))
    if nbytes == 0:
        raise NotImplementedError(f"ff conv_sq: {tuple(x.shape)} -> {tuple(dy.shape[1:])} with a {R}x{R} filter is "
                                  "outside the backward-weight kernels' domain")
    ws = ops.workspace(nbytes, x.device)
    rc = L.salun_ff_conv_sq(_dev(x, torch.float32, "x"), _dev(dy, torch.float32, "dy"), _dev(w, torch.float32, "w"),
                            _dev(F, torch.float32, "F"), G, B, C, H, W, K, R, stride, pad, P, Q,
                            _dev(ws, torch.uint8, "ws"), nbytes, _stream())
    if rc == _lib.SALUN_EINVAL:  # the workspace query is by size alone; the launch itself refuses e.g. 2x2 maps
        raise NotImplementedError(f"ff conv_sq: {tuple(x.shape)} -> {tuple(dy.shape[1:])} with a {R}x{R} filter is "
                                  "outside the backward-weight kernels' domain")
    check(rc, "salun_ff_conv_sq")


def linear_sq(x: torch.Tensor, dy: torch.Tensor, w: torch.Tensor, F: torch.Tensor) -> None:
    """F (M, K) += sum_g w[g] (dy_g^T x)^2.  x: (B, K), dy: (G*B, M)."""
    if x.dim() != 2 or dy.dim() != 2:
        raise ValueError(f"x {tuple(x.shape)} / dy {tuple(dy.shape)} must be (B, K) / (G*B, M)")
    B, K = x.shape
    M = dy.shape[1]
    G = _groups(dy, B, w)
    if F.numel() != M * K:
        raise ValueError(f"F must have {M}x{K} elements")
    check(_lib.lib().salun_ff_linear_sq(_dev(x, torch.float32, "x"), _dev(dy, torch.float32, "dy"),
                                        _dev(w, torch.float32, "w"), _dev(F, torch.float32, "F"), G, B, M, K,
                                        _stream()), "salun_ff_linear_sq")


def vec_sq(dy: torch.Tensor, w: torch.Tensor, F_beta: Optional[torch.Tensor], B: int,
           x: Optional[torch.Tensor] = None, running_mean: Optional[torch.Tensor] = None,
           running_var: Optional[torch.Tensor] = None, eps: float = 0.0,
           F_gamma: Optional[torch.Tensor] = None) -> None:
    """Per-channel group sums squared.  dy: (G*B, C, ...).  F_beta[c] += sum_g w[g] (sum dy_g[:, c])^2 (a bias or BN
    beta); with x (B, C, ...) and the running statistics also F_gamma[c] += sum_g w[g] (sum dy_g[:, c] x^[:, c])^2."""
    G = _groups(dy, B, w)
    C = dy.shape[1]
    HW = dy.numel() // (dy.shape[0] * C) if dy.numel() else 0
    if F_gamma is not None and (x is None or x.numel() * G != dy.numel() or running_mean is None
                                or running_var is None):
        raise ValueError("F_gamma needs x (B, C, ...) of one group and the running statistics")
    for t in (F_beta, F_gamma, running_mean, running_var):
        if t is not None and t.numel() != C:
            raise ValueError(f"per-channel vectors must have {C} elements")
    L = _lib.lib()
    nbytes = int(L.salun_ff_vec_sq_workspace_bytes(G, C))
    ws = ops.workspace(nbytes, dy.device)
    f = lambda t, nm: _dev(t, torch.float32, nm, True)
    check(L.salun_ff_vec_sq(f(x if F_gamma is not None else None, "x"), _dev(dy, torch.float32, "dy"),
                            f(running_mean, "running_mean"), f(running_var, "running_var"), c_double(eps),
                            _dev(w, torch.float32, "w"), G, B, C, HW, f(F_gamma, "F_gamma"), f(F_beta, "F_beta"),
                            _dev(ws, torch.uint8, "ws"), nbytes, _stream()), "salun_ff_vec_sq")


def apply_table(shapes: Sequence[torch.Size], num_classes: int, override_row: Optional[int]) -> tuple:
    """(int64 table rows, number of tiles) of `salun_ff_apply` for parameters of these shapes in arena order.
    `override_row` is the reference's `class_to_replace` when its override applies (a Python index into dim 0 of every
    parameter with shape[0] == num_classes, negative allowed), else None."""
    rows, off, tiles = [], 0, 0
    for s in shapes:
        n = 1
        for d in s:
            n *= int(d)
        n0 = int(s[0]) if len(s) else 1
        multi = len(s) > 1
        d1 = int(s[1]) if multi else 1
        inner = n // (n0 * d1) if n0 * d1 else 1
        if inner > 256:
            raise NotImplementedError(f"fisher_new: parameter of shape {tuple(s)} has more than 256 elements per "
                                      "(row, dim-1) slice")
        classrow = n0 == num_classes
        row = -1
        if classrow and override_row is not None:
            if not -n0 <= override_row < n0:  # the reference's mu[class_to_replace] raises the same way
                raise IndexError(f"index {override_row} is out of bounds for dimension 0 with size {n0}")
            row = override_row % n0
        flags = (1 if classrow else 0) | (2 if multi else 0)
        rows.append([off, n0, d1, inner, flags, row, tiles])
        tiles += n0 if multi else (n0 + 255) // 256
        off += n
    return rows, tiles


def apply(p: torch.Tensor, F: torch.Tensor, shapes: Sequence[torch.Size], num_classes: int,
          override_row: Optional[int], nbatches: int, alpha: float, seed: int) -> None:
    """p <- mu + sqrt(var) z in place over the flat arena (the reference's get_mean_var and noise draw for every
    parameter); F: the raw sum of the batches' grad2 terms, divided by `nbatches` inside; z = fill_normal(seed)."""
    rows, tiles = apply_table(shapes, num_classes, override_row)
    n = sum(r[1] * r[2] * r[3] for r in rows)
    if p.numel() != n or F.numel() != n:
        raise ValueError(f"p and F must have {n} elements (the parameters' total)")
    if nbatches < 1:
        raise ValueError("fisher_new needs at least one batch")
    tab = torch.tensor(rows, dtype=torch.int64).reshape(-1).to(p.device)
    weightimg.params_written()  # a raw-pointer write of the parameters: derived weight images are stale
    check(_lib.lib().salun_ff_apply(_dev(p, torch.float32, "p"), _dev(F, torch.float32, "F"),
                                    _dev(tab, torch.int64, "table"), len(rows), c_int64(tiles), c_double(nbatches),
                                    c_double(alpha), c_uint64(seed), _stream()), "salun_ff_apply")
