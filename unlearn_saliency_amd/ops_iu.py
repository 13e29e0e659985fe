"""Tensor-level wrappers of the IU / WoodFisher kernels (K17, csrc/salun_iu.hip; include/salun.h).

Same conventions as ops.py: device tensors only, raw pointers and the current stream handed to libsalun.so, a
failing call raises `SalunError`.  `out` of the dot wrappers is a (B, 2) fp64 device tensor that is ADDED into
(column 0: tangent g_0, column 1: tangent v), so one buffer collects every layer of a network.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, ops, weightimg
from ._lib import c_double, c_int64, check
from .ops import _dev, _stream


def _out(out: torch.Tensor, B: int) -> None:
    if tuple(out.shape) != (B, 2):
        raise ValueError(f"out must be ({B}, 2), got {tuple(out.shape)}")


def _ws(B: int, n: int, device: torch.device):
    nbytes = int(_lib.lib().salun_iu_dot_workspace_bytes(B, c_int64(n)))
    return ops.workspace(nbytes, device), nbytes


def conv_dot(y2: torch.Tensor, dy: torch.Tensor, out: torch.Tensor) -> None:
    """out[i, j] += <y2[i, j*K:(j+1)*K], dy[i]>   y2: (B, 2K, P, Q) = conv(x, [U_0; U_1]), dy: (B, K, P, Q)."""
    B = dy.shape[0]
    n = dy.numel() // B if B else 0
    if y2.shape[0] != B or y2.numel() != 2 * dy.numel():
        raise ValueError(f"y2 {tuple(y2.shape)} is not the two-tangent stack of dy {tuple(dy.shape)}")
    _out(out, B)
    ws, nbytes = _ws(B, n, dy.device)
    check(_lib.lib().salun_iu_conv_dot(_dev(y2, torch.float32, "y2"), _dev(dy, torch.float32, "dy"), B, c_int64(n),
                                       _dev(out, torch.float64, "out"), _dev(ws, torch.uint8, "ws"), nbytes, _stream()),
          "salun_iu_conv_dot")


def bn_dot(x: torch.Tensor, dy: torch.Tensor, running_mean: torch.Tensor, running_var: torch.Tensor, eps: float,
           u0_gamma: torch.Tensor, u0_beta: torch.Tensor, u1_gamma: torch.Tensor, u1_beta: torch.Tensor,
           out: torch.Tensor) -> None:
    """Eval BatchNorm: out[i, j] += sum_c u_gamma_j[c] sum_pq dy x^ + u_beta_j[c] sum_pq dy, x^ from the running
    statistics.  x, dy: (B, C, H, W)."""
    if x.shape != dy.shape or x.dim() < 2:
        raise ValueError(f"x {tuple(x.shape)} and dy {tuple(dy.shape)} must be the same (B, C, ...) shape")
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C) if B * C else 0
    _out(out, B)
    for t in (running_mean, running_var, u0_gamma, u0_beta, u1_gamma, u1_beta):
        if t.numel() != C:
            raise ValueError(f"per-channel vectors must have {C} elements")
    ws, nbytes = _ws(B, C * HW, x.device)
    f = lambda t, nm: _dev(t, torch.float32, nm)
    check(_lib.lib().salun_iu_bn_dot(f(x, "x"), f(dy, "dy"), f(running_mean, "running_mean"),
                                     f(running_var, "running_var"), c_double(eps), f(u0_gamma, "u0_gamma"),
                                     f(u0_beta, "u0_beta"), f(u1_gamma, "u1_gamma"), f(u1_beta, "u1_beta"), B, C, HW,
                                     _dev(out, torch.float64, "out"), _dev(ws, torch.uint8, "ws"), nbytes, _stream()),
          "salun_iu_bn_dot")


def linear_dot(x: torch.Tensor, dy: torch.Tensor, u0_w: torch.Tensor, u0_b: Optional[torch.Tensor],
               u1_w: torch.Tensor, u1_b: Optional[torch.Tensor], out: torch.Tensor) -> None:
    """out[i, j] += sum_m dy[i, m] (U_j x_i + u_bj)[m]   x: (B, K), dy: (B, M), U_j: (M, K), u_bj: (M,) or None."""
    if x.dim() != 2 or dy.dim() != 2 or x.shape[0] != dy.shape[0]:
        raise ValueError(f"x {tuple(x.shape)} / dy {tuple(dy.shape)} must be (B, K) / (B, M)")
    B, K = x.shape
    M = dy.shape[1]
    if u0_w.numel() != M * K or u1_w.numel() != M * K:
        raise ValueError(f"tangent weights must have {M}x{K} elements")
    if (u0_b is None) != (u1_b is None) or (u0_b is not None and (u0_b.numel() != M or u1_b.numel() != M)):
        raise ValueError("tangent biases: both None or both of M elements")
    _out(out, B)
    check(_lib.lib().salun_iu_linear_dot(_dev(x, torch.float32, "x"), _dev(dy, torch.float32, "dy"),
                                         _dev(u0_w, torch.float32, "u0_w"), _dev(u0_b, torch.float32, "u0_b", True),
                                         _dev(u1_w, torch.float32, "u1_w"), _dev(u1_b, torch.float32, "u1_b", True),
                                         B, M, K, _dev(out, torch.float64, "out"), _stream()), "salun_iu_linear_dot")


def recurrence(ab: torch.Tensor, N: float = 1000.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The WoodFisher loop in scalar form over the (n, 2) fp64 pairs (a_i, b_i) -> device fp64 [beta, s]."""
    if ab.dim() != 2 or ab.shape[1] != 2:
        raise ValueError(f"ab must be (n, 2), got {tuple(ab.shape)}")
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=ab.device)
    check(_lib.lib().salun_iu_recurrence(_dev(ab, torch.float64, "ab"), c_int64(ab.shape[0]), c_double(N),
                                         _dev(out, torch.float64, "out"), _stream()), "salun_iu_recurrence")
    return out


def apply(p: torch.Tensor, v: torch.Tensor, g0: torch.Tensor, beta: torch.Tensor, mask: Optional[torch.Tensor],
          alpha: float) -> None:
    """p += alpha (v - beta g0) where mask != 0 (everywhere for mask None); beta: device fp64 (its first element)."""
    n = p.numel()
    if v.numel() != n or g0.numel() != n or (mask is not None and mask.numel() != n):
        raise ValueError("p, v, g0 and mask must have the same length")
    weightimg.params_written()  # a raw-pointer write of the parameters: derived weight images are stale
    check(_lib.lib().salun_iu_apply(_dev(p, torch.float32, "p"), _dev(v, torch.float32, "v"),
                                    _dev(g0, torch.float32, "g0"), _dev(beta, torch.float64, "beta"),
                                    _dev(mask, torch.uint8, "mask", True), c_double(alpha), c_int64(n), _stream()),
          "salun_iu_apply")
