"""The wide pair of K25 (k_svc_gram_wide / k_svc_decision_wide, csrc/salun_svc.hip): up to 1024 features, for the
membership-inference attack's probability-vector feature at 100 / 200 classes.  Held to the float64 model of
tests/svc_ref_cpu.py with the bounds tests/test_svc_gpu.py holds the narrow pair to, and to the narrow pair itself, bit
for bit, wherever both take the shape (d <= 16)."""
from ctypes import c_double, c_int64, c_size_t, c_void_p

import numpy as np
import pytest
import torch

import svc_ref_cpu as R

pytestmark = pytest.mark.gpu

C, EPS = 3.0, 1e-3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gram(X, gamma, wide):
    from unlearn_saliency_amd import ops_svc
    n = X.shape[0]
    ws = ops_svc.rbf_gram(dev(X), gamma, wide=wide)
    return ws[:4 * n * n].view(torch.float32).view(n, n).cpu().numpy()


# d: 1 and 16 (both pairs), 17 (first past the narrow limit), 31 / 32 / 33 (around one LDS tile), 100 and 200 (the class
# counts), 1024 (the limit).  n: 2, one ragged block, several blocks with a ragged last one.
@pytest.mark.parametrize("d", [1, 16, 17, 31, 32, 33, 100, 200, 1024])
def test_gram_wide_entries(d):
    for n in (2, 255, 600):
        X = np.random.default_rng(100 * d + n).random((n, d)).astype(np.float32)
        gamma = 1.0 / d
        got = _gram(X, gamma, True)
        want = R.rbf_gram(X, gamma)
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, (n, d, int(ulps.max()))
        assert (ulps != 0).mean() <= 0.01, (n, d, float((ulps != 0).mean()))
        assert (np.diag(got) == 1.0).all()
        if d <= 16:
            assert np.array_equal(got.view(np.uint32), _gram(X, gamma, False).view(np.uint32)), (n, d)


def _probability_sets(n_in, n_out, m, d, seed):
    """Softmax rows, what the attack's "prob" feature holds: members peaked, non-members flatter, and query points from
    both."""
    rng = np.random.default_rng(seed)

    def rows(k, temperature):
        z = rng.normal(size=(k, d)) * temperature
        e = np.exp(z - z.max(1, keepdims=True))
        return (e / e.sum(1, keepdims=True)).astype(np.float32)

    X = np.concatenate([rows(n_in, 3.0), rows(n_out, 2.0)])
    y = np.concatenate([np.ones(n_in, np.uint8), np.zeros(n_out, np.uint8)])
    Q = np.concatenate([rows(m // 2, 3.0), rows(m - m // 2, 2.0)])
    return X, y, Q


def _gaussian_sets(n_in, n_out, m, d, seed, mu=0.05):
    """Two overlapping Gaussian clusters, unit variance per feature: |x - z|^2 is of order d, so with gamma = 1 / d the
    kernel is far from constant and the solution has free, bounded and zero multipliers."""
    rng = np.random.default_rng(seed)
    rows = lambda k, centre: rng.normal(centre, 1.0, (k, d)).astype(np.float32)
    X = np.concatenate([rows(n_in, mu), rows(n_out, -mu)])
    y = np.concatenate([np.ones(n_in, np.uint8), np.zeros(n_out, np.uint8)])
    return X, y, np.concatenate([rows(m // 2, mu), rows(m - m // 2, -mu)])


@pytest.mark.parametrize("d", [16, 100, 200])
def test_decision_wide(d):
    from unlearn_saliency_amd import ops_svc
    X, _, Q = _probability_sets(400, 400, 257, d, seed=d)
    rng = np.random.default_rng(d + 1)
    coef = rng.normal(size=800) * (rng.random(800) < 0.6)       # zeros are skipped, as off-support entries are
    rho, gamma = 0.125, 1.0 / d
    for nsv, m in ((1, 1), (255, 64), (800, 257)):
        args = (dev(X[:nsv]), dev(coef[:nsv]), dev(np.array([rho])), gamma, dev(Q[:m]))
        dec, pred = ops_svc.decision_values(*args, wide=True)
        want = R.decision(X[:nsv], coef[:nsv], rho, Q[:m], gamma)
        assert np.abs(dec.cpu().numpy() - want).max() <= 2.0 ** -40 * max(np.abs(coef[:nsv]).sum(), 1.0), (nsv, m)
        assert np.array_equal(pred.cpu().numpy().astype(bool), dec.cpu().numpy() > 0)
        if d <= 16:
            narrow, _ = ops_svc.decision_values(*args)
            assert torch.equal(narrow.view(torch.int64), dec.view(torch.int64)), (nsv, m)


@pytest.mark.parametrize("d", [100, 200])
@pytest.mark.parametrize("sets", [_probability_sets, _gaussian_sets], ids=["probabilities", "gaussians"])
def test_fit_wide_is_feasible_and_optimal(sets, d):
    """gram_wide -> fit -> decision_wide: the bounds of test_svc_gpu.py (feasibility exact, the optimality certificate
    from the unrounded float64 kernel, decisions against the float64 model at the device's own alpha and rho).  On
    probability vectors, which is what the attack feeds it, gamma = 1 / d leaves the kernel nearly constant and all
    multipliers but one end at C (the float64 model agrees); the Gaussian clusters give a mixed support set."""
    from unlearn_saliency_amd import ops_svc
    X, y, Q = sets(300, 300, 200, d, seed=7 + d)
    n = len(y)
    model = ops_svc.fit(dev(X), dev(y), C=C, eps=EPS, wide=True)
    assert model.wide and model.gamma == 1.0 / d
    a, rho = model.alpha.cpu().numpy(), float(model.rho.cpu())
    assert (a >= 0).all() and (a <= C).all() and (a > 0).any()
    if sets is _gaussian_sets:
        assert (a == C).any() and ((a > 0) & (a < C)).sum() > 100 and (a == 0).any()
    assert abs(np.sum(np.where(y > 0, a, -a))) <= 1e-9
    cert = R.certificate(X, y, a, C, model.gamma)
    print(f"d {d}: iterations {int(model.status[0])} certificate {cert:.3e}")
    assert cert <= EPS + 2 * n * C * 2.0 ** -24
    dec, pred = ops_svc.decision(model, dev(Q))
    coef = np.where(y > 0, a, -a)
    want = R.decision(X, coef, rho, Q, model.gamma)
    assert np.abs(dec.cpu().numpy() - want).max() <= 2.0 ** -40 * np.abs(coef).sum()
    assert np.array_equal(pred.cpu().numpy().astype(bool), dec.cpu().numpy() > 0)
    again = ops_svc.fit(dev(X), dev(y), C=C, eps=EPS, wide=True)
    assert torch.equal(again.alpha.view(torch.int64), model.alpha.view(torch.int64))


def test_limits_of_both_pairs():
    from unlearn_saliency_amd import _lib, ops_svc
    L = _lib.lib()
    E = -22
    n, d = 8, 4
    X = torch.rand(n, d, device="cuda")
    ws = torch.zeros(ops_svc.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    coef = torch.ones(n, dtype=torch.float64, device="cuda")
    rho = torch.zeros(1, dtype=torch.float64, device="cuda")
    dec = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    p = lambda t: c_void_p(t.data_ptr())
    gram = lambda d_: L.salun_svc_rbf_gram_wide(p(X), c_int64(n), d_, c_double(0.5), p(ws), c_size_t(ws.numel()), None)
    decide = lambda d_: L.salun_svc_rbf_decision_wide(p(X), p(coef), p(rho), c_int64(n), d_, c_double(0.5), p(X),
                                                      c_int64(n), p(dec), None, None)
    assert gram(0) == E and gram(1025) == E and decide(0) == E and decide(1025) == E
    assert L.salun_svc_rbf_gram_wide(p(X), c_int64(n), d, c_double(0.5), p(ws), c_size_t(ws.numel() - 1), None) == -28
    torch.cuda.synchronize()
    assert not bool(ws.any()) and bool((dec == 7.0).all())  # nothing was launched
    y = (torch.arange(n, device="cuda") % 2).to(torch.uint8)
    with pytest.raises(ValueError, match="1 <= d <= 1024"):
        ops_svc.fit(torch.rand(n, 1025, device="cuda"), y, wide=True)
    with pytest.raises(ValueError, match="1 <= d <= 16"):
        ops_svc.fit(torch.rand(n, 17, device="cuda"), y)
    assert ops_svc.fit(torch.rand(n, 17, device="cuda"), y, wide=True).wide
