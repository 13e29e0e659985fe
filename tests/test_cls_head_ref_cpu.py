"""The CPU side of K23's tests: the float64 model of cls_head_ref_cpu.py against torch's float64 autograd through
adaptive_avg_pool2d -> linear -> cross_entropy, the premises of the exact-answer families, the fp32 restatement inside
the bounds, and the bounds' size.  No GPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cls_head_ref_cpu as R

GAUSS = [(s, amp) for s in R.SHAPES for amp in (1.0, 4.0)]


def _torch64(x, w, bias, labels, g):
    B, C, HW = x.shape
    xt = torch.tensor(x, dtype=torch.float64).view(B, C, HW, 1).requires_grad_()
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(bias, dtype=torch.float64, requires_grad=True)
    y = torch.from_numpy(labels)
    pooled = F.adaptive_avg_pool2d(xt, 1).flatten(1)
    logits = F.linear(pooled, wt, bt)
    loss = F.cross_entropy(logits, y)
    (loss * g).backward()
    per = F.cross_entropy(logits, y, reduction="none")
    return pooled, logits, loss, per, xt.grad.view(B, C, HW), wt.grad, bt.grad


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("g", [1.0, -1.0, 0.37])
def test_model_equals_torch_float64_autograd(shape, g):
    x, w, bias, labels = R.gaussian(shape)
    ex = R.model(x, w, bias, labels, g)
    pooled, logits, loss, per, dx, dw, db = _torch64(x, w, bias, labels, g)
    close = lambda a, b: np.allclose(a, b.detach().numpy(), rtol=1e-12, atol=1e-14)
    assert close(ex.pooled, pooled) and close(ex.logits, logits) and close(ex.loss, per)
    assert close(ex.loss_mean, loss) and close(ex.dx, dx) and close(ex.dw, dw) and close(ex.db, db)
    assert close(ex.p, torch.softmax(logits, -1))
    assert ex.hits == int((logits.argmax(-1) == torch.from_numpy(labels)).sum()) and ex.count == shape[0]


def test_tie_and_bad_label_rules():
    x = np.zeros((4, 3, 4), np.float32)
    w = np.zeros((5, 3), np.float32)
    bias = np.array([1.0, 2.0, 2.0, 0.0, 2.0], np.float32)       # the maximum at 1, 2 and 4: index 1 wins
    ex = R.model(x, w, bias, np.array([1, 2, -1, 5]))
    assert ex.hit.tolist() == [True, False, False, False] and ex.hits == 1 and ex.count == 4
    assert np.isnan(ex.loss[2:]).all() and np.isfinite(ex.loss[:2]).all()
    assert np.isnan(ex.dlogits[2:]).all() and np.isnan(ex.dx[2:]).all()
    assert np.isfinite(ex.dlogits[:2]).all() and np.isfinite(ex.dx[:2]).all()
    assert np.isnan(ex.loss_sum) and np.isnan(ex.dw).all() and np.isnan(ex.db).all()
    em = R.emulate32(x, w, bias, np.array([1, 2, -1, 5]))
    assert em.hit.tolist() == ex.hit.tolist() and np.isnan(em.loss[2:]).all() and np.isnan(em.dx[2:]).all()


@pytest.mark.parametrize("shape", [(1, 24, 16, 2), (64, 512, 16, 2), (64, 24, 64, 16), (4, 512, 1, 128)])
def test_uniform_family_premises(shape):
    """K and B powers of two: p = 1 / K, dlogits = (1 / K - onehot) / B and the loss log K are what fp32 must give."""
    B, C, HW, K = shape
    assert B & (B - 1) == 0 and K & (K - 1) == 0
    x, w, bias, labels = R.uniform_logits(shape)
    ex = R.model(x, w, bias, labels)
    assert (ex.p == 1.0 / K).all() and (ex.logits == 3.0).all()
    d = (1.0 / K - ex.onehot) / B
    assert (ex.dlogits == d).all() and (d.astype(np.float32).astype(np.float64) == d).all()
    assert np.allclose(ex.loss, math.log(K), rtol=1e-15) and (ex.dx == 0).all()
    em = R.emulate32(x, w, bias, labels)
    assert (em.p.astype(np.float64) == ex.p).all() and (em.dlogits.astype(np.float64) == ex.dlogits).all()


@pytest.mark.parametrize("shape", [(1, 24, 1, 2), (64, 512, 16, 10), (64, 512, 64, 100), (8, 24, 64, 10)])
def test_dyadic_family_premises(shape):
    """HW a power of two, B * HW <= 8192: every partial sum of pooled, logits, dW, db and dx is an fp32 number, so the
    float64 model's values ARE the fp32 answers in any summation order (the restatement reproduces them bit for bit),
    and a shift of 96 on the bias moves the logits by exactly 96."""
    B, C, HW, K = shape
    assert HW & (HW - 1) == 0 and B & (B - 1) == 0 and B * HW <= 8192
    x, w, bias, labels = R.dyadic(shape)
    ex = R.model(x, w, bias, labels)
    em = R.emulate32(x, w, bias, labels)
    f32 = lambda a: (a.astype(np.float32).astype(np.float64) == a).all()
    assert f32(ex.pooled) and f32(ex.logits)
    assert (em.pooled.astype(np.float64) == ex.pooled).all() and (em.logits.astype(np.float64) == ex.logits).all()
    xs, ws, bs, ls = R.dyadic(shape, shift=96.0)
    assert (xs == x).all() and (ws == w).all() and (ls == labels).all() and (bs == bias + np.float32(96.0)).all()
    es = R.model(xs, ws, bs, ls)
    assert (es.logits == ex.logits + 96.0).all() and f32(es.logits)
    assert (R.emulate32(xs, ws, bs, ls).p == em.p).all()
    # the backward on a dyadic p
    p = R.dyadic_p(shape)
    d = (p.astype(np.float64) - ex.onehot) / B
    dw, db, dx = d.T @ ex.pooled, d.sum(0), (d @ w.astype(np.float64)) / HW
    assert f32(d) and f32(dw) and f32(db) and f32(dx)


@pytest.mark.parametrize("shape,amp", GAUSS)
def test_fp32_restatement_lies_inside_the_bounds(shape, amp):
    """A correct fp32 implementation in the kernel's order stays inside every per-element bound."""
    for g in (1.0, -1.0, 0.37):
        x, w, bias, labels = R.gaussian(shape, amp=amp)
        ex = R.model(x, w, bias, labels, g)
        bd = R.bounds(ex, x, w, bias, g)
        em = R.emulate32(x, w, bias, labels, g)
        for n in ("pooled", "logits", "p", "loss", "dlogits", "dx", "dw", "db", "loss_sum", "loss_mean"):
            err = np.abs(np.asarray(getattr(em, n), np.float64) - getattr(ex, n))
            assert (err <= getattr(bd, n)).all(), (n, float((err / np.maximum(getattr(bd, n), 1e-300)).max()))
        assert em.hits == ex.hits or _near_tie(ex, bd)


def _near_tie(ex, bd):
    """A hit may differ from the model's only where two logits are closer than their bounds."""
    top2 = np.sort(ex.logits, -1)[:, -2:]
    return bool(((top2[:, 1] - top2[:, 0]) <= 2 * bd.logits.max(-1)).any()) if ex.logits.shape[1] > 1 else False


def test_bounds_are_not_vacuous():
    """The median of bound / |value| over all elements of all outputs of the Gaussian cases stays below
    MEDIAN_REL_LIMIT = 2 * 65 * sqrt(64 * 512) * u = 1.4e-3 (derived next to the constant).  (Single outputs are not
    held to it: db and dW are sums over the batch that cancel, which the derivation of the number does not cover.)"""
    every = []
    for shape, amp in GAUSS:
        x, w, bias, labels = R.gaussian(shape, amp=amp)
        ex = R.model(x, w, bias, labels)
        bd = R.bounds(ex, x, w, bias)
        for n in ("pooled", "logits", "p", "loss", "dlogits", "dx", "dw", "db"):
            rel = R.rel_size(getattr(bd, n), getattr(ex, n))
            assert np.isfinite(rel).all() and (rel > 0).all(), n
            every.append(rel if n != "dx" else rel[::shape[2]])        # dx repeats each value HW times
    assert np.median(np.concatenate(every)) < R.MEDIAN_REL_LIMIT
