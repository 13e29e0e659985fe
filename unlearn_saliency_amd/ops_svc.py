"""Tensor-level wrappers of K25 (csrc/salun_svc.hip; include/salun.h): the RBF C-SVC of the membership-inference
attack, fitted and evaluated on the device.

Same conventions as ops.py: device tensors only, raw pointers and the current stream handed to libsalun.so, a failing
call raises `SalunError`.  `fit` is gram -> fit, `decision` evaluates a fitted model; both are stream-ordered.  The
solver's loop is bounded by `max_iter`; a fit that ends there raises `SvcNotConverged` — reported, never silent.

`wide=True` selects the kernels that take up to SALUN_SVC_WIDE_MAX_D features (the probability vector of a 100- or
200-class model); the default keeps the register-resident pair and its limit of SALUN_SVC_MAX_D.  A model remembers
which pair fitted it.
"""
from __future__ import annotations

import time
from typing import Optional

import torch

from . import _lib
from ._lib import c_double, c_int64, c_size_t, c_void_p, check
from .ops import _dev, _stream


class SvcNotConverged(RuntimeError):
    """The SMO loop used all of `max_iter` updates without meeting m(alpha) - M(alpha) < eps."""

    def __init__(self, iterations: int, max_iter: int):
        super().__init__(f"RBF-SVC fit stopped by its iteration bound: {iterations} updates (max_iter {max_iter}) "
                         "without meeting the stopping tolerance")
        self.iterations = iterations
        self.max_iter = max_iter


def default_max_iter(n: int) -> int:
    return max(10_000_000 // n, 100) * n


class _Stage:
    """Device-synchronised seconds of one stage, added to `stages[name]` when a dict is given (tools/mia_bench.py)."""

    def __init__(self, stages, name):
        self.stages, self.name = stages, name

    def __enter__(self):
        if self.stages is not None:
            torch.cuda.synchronize()
            self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        if self.stages is not None:
            torch.cuda.synchronize()
            self.stages[self.name] = self.stages.get(self.name, 0.0) + time.perf_counter() - self.t0


class SvcModel:
    """A fitted model: X [n, d] fp32, coef [n] fp64 (alpha_t y_t; 0 off the support set), alpha [n] fp64, rho [1] fp64
    and status [2] int64 (updates made, converged), all on the device."""

    def __init__(self, X, coef, alpha, rho, status, gamma, C, eps, max_iter, wide=False):
        self.X, self.coef, self.alpha, self.rho, self.status = X, coef, alpha, rho, status
        self.gamma, self.C, self.eps, self.max_iter, self.wide = gamma, C, eps, max_iter, wide

    def raise_unless_converged(self) -> int:
        """One host read of the status; returns the number of updates."""
        iterations, converged = (int(v) for v in self.status.cpu())
        if not converged:
            raise SvcNotConverged(iterations, self.max_iter)
        return iterations


def workspace_bytes(n: int) -> int:
    return int(_lib.lib().salun_svc_rbf_workspace_bytes(c_int64(n)))


def max_features(wide: bool) -> int:
    return _lib.SALUN_SVC_WIDE_MAX_D if wide else _lib.SALUN_SVC_MAX_D


def rbf_gram(X: torch.Tensor, gamma: float, ws: Optional[torch.Tensor] = None, wide: bool = False) -> torch.Tensor:
    """The workspace with K [n, n] fp32 at its start (K = ws[:4 n^2].view(float32).view(n, n))."""
    n, d = X.shape
    nbytes = workspace_bytes(n)
    if nbytes == 0 or not 1 <= d <= max_features(wide):
        raise ValueError(f"RBF-SVC: n = {n}, d = {d} outside 2 <= n <= {_lib.SALUN_SVC_MAX_N}, "
                         f"1 <= d <= {max_features(wide)}")
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=X.device)
    name = "salun_svc_rbf_gram_wide" if wide else "salun_svc_rbf_gram"
    check(getattr(_lib.lib(), name)(_dev(X, torch.float32, "X"), c_int64(n), d, c_double(gamma),
                                    _dev(ws, torch.uint8, "ws"), c_size_t(ws.numel()), _stream()), name)
    return ws


def fit(X: torch.Tensor, y: torch.Tensor, C: float = 3.0, gamma: Optional[float] = None, eps: float = 1e-3,
        max_iter: Optional[int] = None, wait: bool = True, stages: Optional[dict] = None,
        wide: bool = False) -> SvcModel:
    """Fit on X [n, d] fp32 and y [n] uint8 (1 = member).  gamma defaults to 1 / d (sklearn's "auto").

    wait=True checks the inputs first (non-finite features and an empty class raise ValueError, as sklearn does) and the
    status afterwards (`SvcNotConverged`): two host reads.  wait=False launches only; the caller checks its inputs and
    calls `model.raise_unless_converged()` when it reads its results."""
    if X.dim() != 2 or y.dim() != 1 or y.shape[0] != X.shape[0]:
        raise ValueError(f"RBF-SVC: X {tuple(X.shape)} / y {tuple(y.shape)}: expected [n, d] and [n]")
    n, d = X.shape
    _dev(X, torch.float32, "X"), _dev(y, torch.uint8, "y")
    if wait:
        finite, members = (int(v) for v in torch.stack([torch.isfinite(X).all().long(), (y != 0).sum()]).cpu())
        if not finite:
            raise ValueError("RBF-SVC: non-finite features")
        if members == 0 or members == n:
            raise ValueError("RBF-SVC: the training set needs both classes")
    gamma = 1.0 / d if gamma is None else float(gamma)
    max_iter = default_max_iter(n) if max_iter is None else int(max_iter)
    with _Stage(stages, "gram"):
        ws = rbf_gram(X, gamma, wide=wide)
    alpha = torch.empty(n, dtype=torch.float64, device=X.device)
    rho = torch.empty(1, dtype=torch.float64, device=X.device)
    status = torch.empty(2, dtype=torch.int64, device=X.device)
    with _Stage(stages, "fit"):
        check(_lib.lib().salun_svc_rbf_fit(c_void_p(y.data_ptr()), c_int64(n), c_double(C), c_double(eps),
                                           c_int64(max_iter), c_void_p(alpha.data_ptr()), c_void_p(rho.data_ptr()),
                                           c_void_p(status.data_ptr()), c_void_p(ws.data_ptr()), c_size_t(ws.numel()),
                                           _stream()), "salun_svc_rbf_fit")
    coef = torch.where(y != 0, alpha, -alpha)
    model = SvcModel(X, coef, alpha, rho, status, gamma, float(C), float(eps), max_iter, wide)
    if wait:
        model.raise_unless_converged()
    return model


def decision_values(X: torch.Tensor, coef: torch.Tensor, rho: torch.Tensor, gamma: float, Z: torch.Tensor,
                    wide: bool = False):
    """(dec [m] fp64, pred [m] uint8) of Z [m, d] fp32: dec = sum_t coef_t K(x_t, z) - rho, pred = dec > 0."""
    n, d = X.shape
    m = Z.shape[0]
    if Z.dim() != 2 or Z.shape[1] != d or coef.shape != (n,) or rho.numel() != 1:
        raise ValueError(f"RBF-SVC decision: X {tuple(X.shape)}, coef {tuple(coef.shape)}, Z {tuple(Z.shape)}")
    dec = torch.empty(m, dtype=torch.float64, device=X.device)
    pred = torch.empty(m, dtype=torch.uint8, device=X.device)
    name = "salun_svc_rbf_decision_wide" if wide else "salun_svc_rbf_decision"
    check(getattr(_lib.lib(), name)(_dev(X, torch.float32, "X"), _dev(coef, torch.float64, "coef"),
                                    _dev(rho, torch.float64, "rho"), c_int64(n), d, c_double(gamma),
                                    _dev(Z, torch.float32, "Z"), c_int64(m), c_void_p(dec.data_ptr()),
                                    c_void_p(pred.data_ptr()), _stream()), name)
    return dec, pred


def decision(model: SvcModel, Z: torch.Tensor, stages: Optional[dict] = None):
    with _Stage(stages, "decision"):
        return decision_values(model.X, model.coef, model.rho, model.gamma, Z, wide=model.wide)
