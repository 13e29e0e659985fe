"""Float64 numpy model of K25 (csrc/salun_svc.hip): the RBF C-SVC dual solved by SMO with second-order working-set
selection (Fan, Chen, Lin 2005, WSS 2), no shrinking.

It restates the device algorithm operation for operation:
  * kernel entries: squared distance summed over the features in index order in float64, times -gamma, exp in
    float64, rounded ONCE to float32 (libsvm's Qfloat);
  * alpha, G and rho in float64; v_t = -y_t G_t;
  * i = the lowest index of max v over I_up, j = the lowest index of min -(m - v_t)^2 / a_it over {t in I_low, v_t < m}
    with a_it = 2 - 2 K_it, a <= 0 replaced by 1e-12;
  * libsvm's clipped two-variable update; G += Q_i dalpha_i, then += Q_j dalpha_j;
  * stop when m - M < eps or after max_iter updates;
  * rho: mean of y_t G_t over free variables, else the midpoint of the bounds.
"""
from __future__ import annotations

import numpy as np

TAU = 1e-12


def rbf_gram64(X, Z, gamma):
    """exp(-gamma * |x - z|^2) in float64, the squared distance summed over the features in index order."""
    X = np.asarray(X, np.float32).astype(np.float64)
    Z = np.asarray(Z, np.float32).astype(np.float64)
    d2 = np.zeros((X.shape[0], Z.shape[0]), np.float64)
    for k in range(X.shape[1]):
        diff = X[:, k][:, None] - Z[:, k][None, :]
        d2 = d2 + diff * diff
    return np.exp(-gamma * d2)


def rbf_gram(X, gamma):
    """The training kernel matrix as the solver reads it: float64 entries rounded once to float32."""
    return rbf_gram64(X, X, gamma).astype(np.float32)


def default_max_iter(n):
    return max(10_000_000 // n, 100) * n


def fit(K, y01, C=3.0, eps=1e-3, max_iter=None):
    """K [n, n] float32, y01 [n] in {0, 1} (1 = member = +1).  Returns alpha, rho, iterations, converged."""
    n = len(y01)
    if max_iter is None:
        max_iter = default_max_iter(n)
    y = np.where(np.asarray(y01) > 0, 1.0, -1.0)
    pos = y > 0
    alpha = np.zeros(n, np.float64)
    G = -np.ones(n, np.float64)
    it, converged = 0, False
    while True:
        v = -y * G
        up = np.where(pos, alpha < C, alpha > 0)
        low = np.where(pos, alpha > 0, alpha < C)
        m = v[up].max() if up.any() else -np.inf
        M = v[low].min() if low.any() else np.inf
        if not (m - M >= eps):
            converged = True
            break
        if it >= max_iter:
            break
        i = int(np.argmax(np.where(up, v, -np.inf)))
        Ki = K[i].astype(np.float64)
        cand = low & (v < m)
        if not cand.any():
            converged = True
            break
        a = 2.0 - 2.0 * Ki
        a = np.where(a > 0, a, TAU)
        b = m - v
        obj = np.where(cand, -(b * b) / a, np.inf)
        j = int(np.argmin(obj))
        Kj = K[j].astype(np.float64)
        ai, aj = alpha[i], alpha[j]
        if y[i] != y[j]:
            quad = 2.0 + 2.0 * Ki[j]
            if quad <= 0:
                quad = TAU
            delta = (-G[i] - G[j]) / quad
            diff = ai - aj
            ni, nj = ai + delta, aj + delta
            if diff > 0:
                if nj < 0:
                    nj, ni = 0.0, diff
            else:
                if ni < 0:
                    ni, nj = 0.0, -diff
            if diff > 0:
                if ni > C:
                    ni, nj = C, C - diff
            else:
                if nj > C:
                    nj, ni = C, C + diff
        else:
            quad = 2.0 - 2.0 * Ki[j]
            if quad <= 0:
                quad = TAU
            delta = (G[i] - G[j]) / quad
            s = ai + aj
            ni, nj = ai - delta, aj + delta
            if s > C:
                if ni > C:
                    ni, nj = C, s - C
            else:
                if nj < 0:
                    nj, ni = 0.0, s
            if s > C:
                if nj > C:
                    nj, ni = C, s - C
            else:
                if ni < 0:
                    ni, nj = 0.0, s
        dai, daj = ni - ai, nj - aj
        alpha[i], alpha[j] = ni, nj
        G = G + (y[i] * y * Ki) * dai
        G = G + (y[j] * y * Kj) * daj
        it += 1
    yG = y * G
    upper, lower = alpha >= C, alpha <= 0
    free = ~upper & ~lower
    if free.any():
        rho = float(np.sum(yG[free]) / free.sum())
    else:
        ub_set = (upper & ~pos) | (lower & pos)
        lb_set = (upper & pos) | (lower & ~pos)
        ub = yG[ub_set].min() if ub_set.any() else np.inf
        lb = yG[lb_set].max() if lb_set.any() else -np.inf
        rho = float((ub + lb) / 2)
    return alpha, rho, it, converged


def decision(X, coef, rho, Q, gamma):
    """f(z) = sum_t coef_t K(x_t, z) - rho in float64 (coef_t = alpha_t y_t)."""
    return rbf_gram64(Q, X, gamma) @ np.asarray(coef, np.float64) - rho


def certificate(X, y01, alpha, C, gamma):
    """m(alpha) - M(alpha) in float64 from the UNROUNDED kernel."""
    y = np.where(np.asarray(y01) > 0, 1.0, -1.0)
    pos = y > 0
    G = (rbf_gram64(X, X, gamma) * np.outer(y, y)) @ alpha - 1.0
    v = -y * G
    up = np.where(pos, alpha < C, alpha > 0)
    low = np.where(pos, alpha > 0, alpha < C)
    return float(v[up].max() - v[low].min())
