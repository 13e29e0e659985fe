"""K23 (csrc/salun_cls_head.hip) on the GPU against the float64 model and bounds of cls_head_ref_cpu.py: exact-answer
families bit for bit, Gaussian families inside the per-element bounds, accumulate mode, the incoming gradient, ties,
bad labels, run-to-run identity, error codes and the running meters.  Every C-ABI call runs inside the guarded arena
(guarded_arena.py): nothing outside the outputs may change."""
from ctypes import c_int64, c_size_t, c_void_p

import numpy as np
import pytest
import torch

import cls_head_ref_cpu as R
from guarded_arena import SENTINEL, Arena

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
FWD_OUT = ("pooled", "logits", "p", "loss", "loss_mean")


def _lib():
    from unlearn_saliency_amd import _lib
    return _lib.lib()


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).view(torch.int32)


def _meters(loss_sum=0.0, hits=0, count=0):
    return dict(loss_sum=torch.tensor([loss_sum], dtype=torch.float64).view(torch.int32), hits=_i64([hits]),
                count=_i64([count]))


def forward(x, w, bias, labels, meters=None, skew=0, mean=True):
    """-> (code, dict of host arrays).  meters: dict of int32 bit patterns (see _meters) or None."""
    B, C, HW = x.shape
    K = w.shape[0]
    t = torch.from_numpy
    a = Arena().put("x", t(x), skew=skew).put("w", t(w)).put("bias", t(bias)).put("labels", _i64(labels))
    a.put("pooled", shape=(B, C), out=True).put("logits", shape=(B, K), out=True).put("p", shape=(B, K), out=True)
    a.put("loss", shape=(B,), out=True)
    if mean:
        a.put("loss_mean", shape=(1,), out=True)
    if meters is not None:
        for n in ("loss_sum", "hits", "count"):
            a.put(n, meters[n], out=True)
    a.put("ws", torch.zeros(4, dtype=torch.int32), out=True).upload()
    L = _lib()
    code = L.salun_cls_head_forward(a.ptr("x"), a.ptr("w"), a.ptr("bias"), a.ptr("labels"), a.ptr("pooled"),
                                    a.ptr("logits"), a.ptr("p"), a.ptr("loss"), a.ptr("loss_mean"), a.ptr("loss_sum"),
                                    a.ptr("hits"), a.ptr("count"), c_int64(B), C, HW, K, a.ptr("ws"), c_size_t(16),
                                    c_void_p(None))
    after = a.download()
    out = {n: a.part(after, n).numpy().copy() for n in FWD_OUT if n in a.parts}
    if meters is not None:
        raw = lambda n: after[a.parts[n][0]:a.parts[n][0] + 2].clone()
        out["loss_sum"] = float(raw("loss_sum").view(torch.float64)[0])
        out["hits"] = int(raw("hits").view(torch.int64)[0])
        out["count"] = int(raw("count").view(torch.int64)[0])
    return code, out


def backward(p, pooled, w, labels, g, HW, dw0=None, db0=None, want_dx=True, skew=0):
    """-> (code, dict).  dw0 / db0: contents to accumulate into (accumulate mode) or None."""
    B, K = p.shape
    C = pooled.shape[1]
    t = torch.from_numpy
    a = Arena().put("p", t(p)).put("pooled", t(pooled)).put("w", t(w)).put("labels", _i64(labels))
    if g is not None:
        a.put("g", t(np.array([g], F32)))
    a.put("dlogits", shape=(B, K), out=True)
    if want_dx:
        a.put("dx", shape=(B, C, HW), out=True, skew=skew)
    a.put("dw", None if dw0 is None else t(dw0), shape=(K, C), out=True)
    a.put("db", None if db0 is None else t(db0), shape=(K,), out=True)
    a.upload()
    code = _lib().salun_cls_head_backward(a.ptr("p"), a.ptr("pooled"), a.ptr("w"), a.ptr("labels"), a.ptr("g"),
                                          a.ptr("dlogits"), a.ptr("dx"), a.ptr("dw"), a.ptr("db"),
                                          int(dw0 is not None), int(db0 is not None), c_int64(B), C, HW, K, c_void_p(None))
    after = a.download()
    return code, {n: a.part(after, n).numpy().copy() for n in ("dlogits", "dx", "dw", "db") if n in a.parts}


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same_bits(got, want64):
    """The fp32 result equals the float64 answer exactly (and the answer is an fp32 number)."""
    return np.array_equal(np.asarray(got, F64), want64)


def inside(got, want, bound):
    err = np.abs(np.asarray(got, F64) - want)
    return bool((err <= bound).all()), float((err / np.maximum(bound, 1e-300)).max())


# ------------------------------------------------------------------------------------------- Gaussian families
@pytest.mark.parametrize("shape", R.ALL_SHAPES)
def test_gaussian_within_per_element_bounds(shape):
    """Every B x C x HW x K of the grid with grad_output 1; the twelve shapes of R.SHAPES also with grad_output -1 (at
    four times the logit spread) and 0.37."""
    combos = [(1.0, 1.0), (-1.0, 4.0), (0.37, 1.0)] if shape in R.SHAPES else [(1.0, 4.0 if sum(shape) % 2 else 1.0)]
    for g, amp in combos:
        _gaussian_case(shape, g, amp)


def _gaussian_case(shape, g, amp):
    B, C, HW, K = shape
    x, w, bias, labels = R.gaussian(shape, amp=amp)
    ex = R.model(x, w, bias, labels, g)
    bd = R.bounds(ex, x, w, bias, g)
    code, f = forward(x, w, bias, labels, _meters())
    assert code == 0
    for n in FWD_OUT:
        ok, worst = inside(f[n].reshape(getattr(ex, n).shape) if n != "loss_mean" else f[n][0], getattr(ex, n),
                           getattr(bd, n))
        assert ok, (n, worst)
    assert f["count"] == B and abs(f["loss_sum"] - ex.loss_sum) <= bd.loss_sum
    if f["hits"] != ex.hits:  # only where two logits are closer than their bounds
        top2 = np.sort(ex.logits, -1)[:, -2:]
        assert K > 1 and ((top2[:, 1] - top2[:, 0]) <= 2 * bd.logits.max(-1)).any()
    code, r = backward(f["p"], f["pooled"], w, labels, g, HW)
    assert code == 0
    for n in ("dlogits", "dx", "dw", "db"):
        ok, worst = inside(r[n], getattr(ex, n), getattr(bd, n))
        assert ok, (n, worst)


@pytest.mark.parametrize("shape", [(5, 24, 16, 10), (257, 512, 16, 10), (64, 24, 1, 100)])
def test_two_runs_are_bit_identical(shape):
    x, w, bias, labels = R.gaussian(shape, seed=3)
    runs = []
    for _ in range(2):
        _, f = forward(x, w, bias, labels, _meters(1.5, 2, 3))
        _, r = backward(f["p"], f["pooled"], w, labels, 0.37, shape[2])
        runs.append({**f, **r})
    for n, v in runs[0].items():
        other = runs[1][n]
        assert np.array_equal(bits(v), bits(other)) if isinstance(v, np.ndarray) else v == other, n


@pytest.mark.parametrize("shape", [(5, 24, 16, 10), (64, 512, 64, 2)])
def test_unaligned_x_takes_the_scalar_route_with_the_same_bounds(shape):
    B, C, HW, K = shape
    x, w, bias, labels = R.gaussian(shape, seed=5)
    ex = R.model(x, w, bias, labels)
    bd = R.bounds(ex, x, w, bias)
    code, f = forward(x, w, bias, labels, skew=1)
    assert code == 0
    for n in FWD_OUT[:4]:
        assert inside(f[n], getattr(ex, n), getattr(bd, n))[0], n
    code, r = backward(f["p"], f["pooled"], w, labels, 1.0, HW, skew=1)
    assert code == 0 and inside(r["dx"], ex.dx, bd.dx)[0]


# --------------------------------------------------------------------------------------- exact-answer families
@pytest.mark.parametrize("shape", [(1, 24, 16, 2), (64, 512, 16, 2), (64, 24, 64, 16), (4, 512, 1, 128)])
@pytest.mark.parametrize("g", [1.0, -1.0, 0.25])
def test_uniform_logits_are_exact(shape, g):
    B, C, HW, K = shape
    x, w, bias, labels = R.uniform_logits(shape)
    ex = R.model(x, w, bias, labels, g)
    code, f = forward(x, w, bias, labels)
    assert code == 0
    assert same_bits(f["p"], ex.p) and same_bits(f["logits"], ex.logits)
    code, r = backward(f["p"], f["pooled"], w, labels, g, HW)
    assert code == 0
    assert same_bits(r["dlogits"], ex.dlogits) and (r["dx"] == 0).all()


@pytest.mark.parametrize("shape", [(1, 24, 1, 2), (64, 512, 16, 10), (64, 512, 64, 100), (8, 24, 64, 10)])
def test_dyadic_inputs_are_exact_and_a_shift_changes_no_bit_of_p(shape):
    B, C, HW, K = shape
    x, w, bias, labels = R.dyadic(shape)
    ex = R.model(x, w, bias, labels)
    code, f = forward(x, w, bias, labels)
    assert code == 0
    assert same_bits(f["pooled"], ex.pooled) and same_bits(f["logits"], ex.logits)
    xs, ws, bs, ls = R.dyadic(shape, shift=96.0)
    code, fs = forward(xs, ws, bs, ls)
    assert code == 0
    assert same_bits(fs["logits"], ex.logits + 96.0)
    assert np.isfinite(fs["p"]).all() and np.array_equal(bits(fs["p"]), bits(f["p"]))
    assert np.array_equal(bits(fs["loss"]), bits(f["loss"]))
    # the backward on a dyadic p: dlogits, dW, db and dx bit for bit, also when added to dyadic contents
    p = R.dyadic_p(shape)
    d = (p.astype(F64) - ex.onehot) / B
    dw, db, dx = d.T @ ex.pooled, d.sum(0), (d @ w.astype(F64)) / HW
    code, r = backward(p, f["pooled"], w, labels, 1.0, HW)
    assert code == 0
    assert same_bits(r["dlogits"], d) and same_bits(r["dw"], dw) and same_bits(r["db"], db)
    assert same_bits(r["dx"], np.repeat(dx[:, :, None], HW, -1))
    rng = np.random.default_rng(5)
    dw0 = (rng.integers(-64, 65, (K, C)) / 8.0).astype(F32)
    db0 = (rng.integers(-64, 65, K) / 8.0).astype(F32)
    code, r = backward(p, f["pooled"], w, labels, 1.0, HW, dw0=dw0, db0=db0)
    assert code == 0 and same_bits(r["dw"], dw0.astype(F64) + dw) and same_bits(r["db"], db0.astype(F64) + db)


# ------------------------------------------------------------------------------------------------ accumulate
@pytest.mark.parametrize("shape", [(5, 24, 16, 10), (257, 512, 16, 10)])
def test_accumulate_lands_old_plus_new(shape):
    B, C, HW, K = shape
    x, w, bias, labels = R.gaussian(shape, seed=9)
    ex = R.model(x, w, bias, labels)
    bd = R.bounds(ex, x, w, bias)
    _, f = forward(x, w, bias, labels)
    rng = np.random.default_rng(1)
    dw0, db0 = rng.standard_normal((K, C)).astype(F32), rng.standard_normal(K).astype(F32)
    code, r = backward(f["p"], f["pooled"], w, labels, 1.0, HW, dw0=dw0, db0=db0)
    assert code == 0
    for got, old, new, e in ((r["dw"], dw0, ex.dw, bd.dw), (r["db"], db0, ex.db, bd.db)):
        bound = e + R.U * (np.abs(old) + np.abs(new) + e)          # one more rounding: fl(old + new^)
        assert inside(got, old.astype(F64) + new, bound)[0]
    # and overwrite mode ignores what was there
    code, r2 = backward(f["p"], f["pooled"], w, labels, 1.0, HW)
    assert inside(r2["dw"], ex.dw, bd.dw)[0] and inside(r2["db"], ex.db, bd.db)[0]


# ----------------------------------------------------------------------------------- ties, labels, error codes
def test_argmax_ties_go_to_the_lowest_index():
    K, C = 300, 24                                                  # K > 256: a thread holds two candidates
    x = np.zeros((6, C, 4), F32)
    w = np.zeros((K, C), F32)
    bias = np.zeros(K, F32)
    bias[[7, 70, 200, 290]] = 2.0                                   # the maximum in waves 0, 1, 3 and on a second trip
    labels = np.array([7, 70, 200, 290, 0, 7])
    _, f = forward(x, w, bias, labels, _meters())
    assert f["hits"] == 2 and f["count"] == 6                       # rows 0 and 5
    bias2 = np.zeros(K, F32)
    bias2[[290, 299]] = 1.0
    _, f = forward(x, w, bias2, np.array([290, 299, 290, 0, 1, 299]), _meters())
    assert f["hits"] == 2


@pytest.mark.parametrize("shape", [(5, 24, 16, 10), (64, 512, 16, 10)])
def test_bad_labels_poison_their_own_rows_only(shape):
    B, C, HW, K = shape
    x, w, bias, labels = R.gaussian(shape, seed=2)
    bad = labels.copy()
    bad[0], bad[B - 2] = -1, K
    rows = np.array([0, B - 2])
    good = np.setdiff1d(np.arange(B), rows)
    _, ref = forward(x, w, bias, labels, _meters())
    code, f = forward(x, w, bias, bad, _meters())
    assert code == 0 and f["count"] == B
    assert np.isnan(f["loss"][rows]).all() and np.array_equal(bits(f["loss"][good]), bits(ref["loss"][good]))
    for n in ("pooled", "logits", "p"):                             # the forward's other outputs do not see the label
        assert np.array_equal(bits(f[n]), bits(ref[n])), n
    assert np.isnan(f["loss_sum"]) and np.isnan(f["loss_mean"][0])
    assert f["hits"] == int((f["logits"].argmax(-1) == bad).sum())   # the bad rows hit nothing
    _, r0 = backward(ref["p"], ref["pooled"], w, labels, 1.0, HW)
    code, r = backward(f["p"], f["pooled"], w, bad, 1.0, HW)
    assert code == 0
    for n in ("dlogits", "dx"):
        assert np.isnan(r[n][rows]).all() and np.array_equal(bits(r[n][good]), bits(r0[n][good])), n


def test_error_codes_come_back_without_a_launch():
    from unlearn_saliency_amd import _lib
    L = _lib.lib()
    EINVAL = _lib.SALUN_EINVAL
    x, w, bias, labels = R.gaussian((5, 24, 16, 10))
    t = torch.from_numpy
    a = Arena().put("x", t(x)).put("w", t(w)).put("bias", t(bias)).put("labels", _i64(labels))
    for n, shp in (("pooled", (5, 24)), ("logits", (5, 10)), ("p", (5, 10)), ("loss", (5,)), ("dx", (5, 24, 16)),
                   ("dw", (10, 24)), ("db", (10,)), ("ws", (4,))):
        a.put(n, shape=shp, out=True)
    a.upload()
    P = a.ptr

    def fwd(B=5, C=24, HW=16, K=10, ws_bytes=16, **ptr):
        q = {n: ptr.get(n, P(n)) for n in ("x", "w", "bias", "labels", "pooled", "logits", "p", "loss", "ws")}
        return L.salun_cls_head_forward(q["x"], q["w"], q["bias"], q["labels"], q["pooled"], q["logits"], q["p"],
                                        q["loss"], ptr.get("loss_mean", c_void_p(None)), c_void_p(None), c_void_p(None),
                                        ptr.get("count", c_void_p(None)), c_int64(B), C, HW, K, q["ws"],
                                        c_size_t(ws_bytes), c_void_p(None))

    def bwd(B=5, C=24, HW=16, K=10, **ptr):
        q = {n: ptr.get(n, P(n)) for n in ("p", "pooled", "w", "labels", "logits", "dx", "dw", "db")}
        return L.salun_cls_head_backward(q["p"], q["pooled"], q["w"], q["labels"], c_void_p(None), q["logits"], q["dx"],
                                         q["dw"], q["db"], 0, 0, c_int64(B), C, HW, K, c_void_p(None))

    off = lambda n, k: c_void_p(P(n).value + k)
    for code in (fwd(B=0), fwd(B=-3), fwd(K=0), fwd(K=_lib.SALUN_CLS_HEAD_MAX_K + 1), fwd(C=0),
                 fwd(C=_lib.SALUN_CLS_HEAD_MAX_C + 1), fwd(HW=0), fwd(x=c_void_p(None)), fwd(labels=c_void_p(None)),
                 fwd(loss=c_void_p(None)), fwd(x=off("x", 2)), fwd(labels=off("labels", 4)), fwd(p=off("p", 1)),
                 fwd(count=off("ws", 4), loss_mean=P("loss")), fwd(loss_mean=P("loss"), ws=c_void_p(None)),
                 bwd(B=0), bwd(K=0), bwd(K=_lib.SALUN_CLS_HEAD_MAX_K + 1), bwd(p=c_void_p(None)), bwd(dx=off("dx", 2)),
                 bwd(labels=off("labels", 4)), bwd(logits=c_void_p(None))):
        assert code == EINVAL
    assert fwd(loss_mean=P("loss"), ws_bytes=3) == _lib.SALUN_ENOSPC
    assert L.salun_cls_head_workspace_bytes(c_int64(0), 24, 10) == 0
    assert L.salun_cls_head_workspace_bytes(c_int64(5), 24, _lib.SALUN_CLS_HEAD_MAX_K + 1) == 0
    assert L.salun_cls_head_workspace_bytes(c_int64(5), 24, 10) >= 4
    after = a.download()                                             # guards and inputs intact ...
    for n in ("pooled", "logits", "p", "loss", "dx", "dw", "db", "ws"):   # ... and no output was touched
        s, k = a.parts[n][0], a.parts[n][1]
        assert (after[s:s + k] == SENTINEL).all(), n


def test_meters_after_three_calls_equal_the_models_sums():
    shape = (64, 24, 16, 10)
    m = _meters()
    want_sum, want_hits, want_count, slack, near = 0.0, 0, 0, 0.0, False
    for seed in range(3):
        x, w, bias, labels = R.gaussian(shape, seed=seed)
        ex = R.model(x, w, bias, labels)
        bd = R.bounds(ex, x, w, bias)
        top2 = np.sort(ex.logits, -1)[:, -2:]
        near = near or bool(((top2[:, 1] - top2[:, 0]) <= 2 * bd.logits.max(-1)).any())
        want_sum, want_hits, want_count = want_sum + ex.loss_sum, want_hits + ex.hits, want_count + ex.count
        slack += bd.loss_sum
        code, f = forward(x, w, bias, labels, m)
        assert code == 0
        m = _meters(f["loss_sum"], f["hits"], f["count"])
    assert f["count"] == want_count == 192
    assert abs(f["loss_sum"] - want_sum) <= slack + 3 * 2.0 ** -53 * abs(want_sum)   # three float64 additions
    assert f["hits"] == want_hits or near


# ------------------------------------------------------------------------------------------ the autograd node
@pytest.mark.parametrize("g", [1.0, -1.0, 0.37])
def test_fused_cls_head_autograd_and_gradient_sink(g):
    """fused_cls_head returns (mean loss, logits), scales its backward by the incoming gradient, and adds the fc
    gradients into a pre-filled contiguous `.grad` (the flat arena's case) as old + new."""
    from unlearn_saliency_amd.cls_head import HeadMeters, fused_cls_head
    shape = (64, 24, 16, 10)
    B, C, HW, K = shape
    x, w, bias, labels = R.gaussian(shape, seed=4)
    ex = R.model(x, w, bias, labels, g)
    bd = R.bounds(ex, x, w, bias, g)
    fc = torch.nn.Linear(C, K).cuda()
    with torch.no_grad():
        fc.weight.copy_(torch.from_numpy(w))
        fc.bias.copy_(torch.from_numpy(bias))
    rng = np.random.default_rng(3)
    old_w, old_b = rng.standard_normal((K, C)).astype(F32), rng.standard_normal(K).astype(F32)
    fc.weight.grad, fc.bias.grad = torch.from_numpy(old_w).cuda(), torch.from_numpy(old_b).cuda()
    gw_ptr = fc.weight.grad.data_ptr()
    xt = torch.from_numpy(x).cuda().view(B, C, 4, HW // 4).requires_grad_()
    meters = HeadMeters(xt.device)
    loss, logits = fused_cls_head(xt, fc, torch.from_numpy(labels).cuda(), meters)
    assert loss.shape == () and not logits.requires_grad and logits.shape == (B, K)
    (loss * g).backward()
    g0 = R.model(x, w, bias, labels)
    assert abs(float(loss.detach()) - g0.loss_mean) <= R.bounds(g0, x, w, bias).loss_mean
    assert inside(xt.grad.cpu().numpy().reshape(B, C, HW), ex.dx, bd.dx)[0]
    assert fc.weight.grad.data_ptr() == gw_ptr                       # written in place by the kernel
    for got, old, new, e in ((fc.weight.grad, old_w, ex.dw, bd.dw), (fc.bias.grad, old_b, ex.db, bd.db)):
        assert inside(got.cpu().numpy(), old.astype(F64) + new, e + R.U * (np.abs(old) + np.abs(new) + e))[0]
    avg, top1, n = meters.read()
    assert n == B and abs(avg - g0.loss_mean) <= R.bounds(g0, x, w, bias).loss_sum / B + 2.0 ** -52 * abs(avg)
    # without a usable sink (no .grad yet) the gradients come back through autograd
    fc.weight.grad = fc.bias.grad = None
    loss, _ = fused_cls_head(xt, fc, torch.from_numpy(labels).cuda())
    (loss * g).backward()
    assert inside(fc.weight.grad.cpu().numpy(), ex.dw, bd.dw)[0] and inside(fc.bias.grad.cpu().numpy(), ex.db, bd.db)[0]
    with pytest.raises(TypeError, match="no CPU fallback"):
        fused_cls_head(xt.detach().cpu(), fc, torch.from_numpy(labels))
