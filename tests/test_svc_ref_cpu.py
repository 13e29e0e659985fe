"""The float64 model of K25 (tests/svc_ref_cpu.py: WSS 2, no shrinking, float32 kernel entries, lowest-index ties)
against sklearn's recorded answers (tests/golden/svc_rbf.npz), with exactly the bounds the device tests use
(tests/test_svc_gpu.py).  This shows without a GPU that a non-shrinking solver meets them."""
import os

import numpy as np
import pytest

import svc_ref_cpu as R

C, EPS = 3.0, 1e-3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svc_rbf.npz")
_g = np.load(GOLDEN)
CASES = [str(c) for c in _g["cases"]]
_fits: dict = {}


def case(name):
    return {k: _g[f"{name}/{k}"] for k in ("X", "y", "Q", "dual_coef", "support", "intercept", "dec_ref", "gap", "b",
                                            "frac", "pred_ref")}


def model_fit(name):
    """One fit per case, shared by the tests below and left unchanged."""
    if name not in _fits:
        c = case(name)
        gamma = 1.0 / c["X"].shape[1]
        alpha, rho, it, conv = R.fit(R.rbf_gram(c["X"], gamma), c["y"], C, EPS)
        ysign = np.where(c["y"] > 0, 1.0, -1.0)
        _fits[name] = dict(alpha=alpha, rho=rho, it=it, conv=conv, gamma=gamma,
                           dec=R.decision(c["X"], alpha * ysign, rho, c["Q"], gamma))
    return _fits[name]


def test_fixture_states_its_own_rule():
    assert len(CASES) == 13
    for name in CASES:
        c = case(name)
        assert float(c["b"]) == 4.0 * max(float(c["gap"]), 1e-3)
        assert float(c["frac"]) == float((np.abs(c["dec_ref"]) <= c["b"]).mean()) <= 0.03
        assert c["X"].dtype == np.float32 and c["Q"].shape[0] == 600


@pytest.mark.parametrize("name", CASES)
def test_model_is_feasible_and_optimal(name):
    c, f = case(name), model_fit(name)
    a, n = f["alpha"], len(c["y"])
    assert f["conv"] and f["it"] < 1e5
    assert (a >= 0).all() and (a <= C).all()
    assert abs(np.sum(np.where(c["y"] > 0, a, -a))) <= 1e-9
    assert R.certificate(c["X"], c["y"], a, C, f["gamma"]) <= EPS + 2 * n * C * 2.0 ** -24


@pytest.mark.parametrize("name", CASES)
def test_model_decisions_and_predictions_match_sklearn(name):
    c, f = case(name), model_fit(name)
    b = float(c["b"])
    err = float(np.abs(f["dec"] - c["dec_ref"]).max())
    print(f"{name}: iterations {f['it']} max|dec - dec_ref| {err:.3e} (b {b:.3e})")
    assert err <= b
    pred = f["dec"] > 0
    clear = np.abs(c["dec_ref"]) > b
    assert np.array_equal(pred[clear], c["pred_ref"][clear].astype(bool))
    acc = lambda p: 0.5 * (p[:300].mean() + 1 - p[300:].mean())
    assert abs(acc(pred) - acc(c["pred_ref"].astype(bool))) <= float(c["frac"]) + 1e-12


def test_sklearn_decision_is_the_stated_formula():
    """dec_ref = sum_t dual_coef_t K(x_support_t, z) + intercept: the sign convention the device kernel implements
    (coef = alpha_t y_t with y = +1 for members, rho = -intercept)."""
    for name in CASES:
        c = case(name)
        gamma = 1.0 / c["X"].shape[1]
        dec = R.decision(c["X"][c["support"]], c["dual_coef"], -float(c["intercept"]), c["Q"], gamma)
        assert np.abs(dec - c["dec_ref"]).max() <= 2.0 ** -40 * np.abs(c["dual_coef"]).sum()


def test_closed_form_two_points():
    X = np.array([[0.25], [0.75]], np.float32)
    K = R.rbf_gram(X, 1.0)
    alpha, rho, it, conv = R.fit(K, np.array([1, 0], np.uint8), C, EPS)
    want = min(C, 1.0 / (1.0 - float(K[0, 1])))
    assert conv and abs(alpha[0] - want) <= 2.0 ** -23 * want and alpha[0] == alpha[1] and abs(rho) <= 2.0 ** -23


def test_iteration_bound_is_reported():
    c = case("conf1d_64_64")
    alpha, rho, it, conv = R.fit(R.rbf_gram(c["X"], 1.0), c["y"], C, EPS, max_iter=1)
    assert it == 1 and not conv and (alpha >= 0).all() and (alpha <= C).all()
    assert np.count_nonzero(alpha) == 2 and np.sum(np.where(c["y"] > 0, alpha, -alpha)) == 0
