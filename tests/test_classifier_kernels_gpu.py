"""The three small kernels of the classifier evaluation on the GPU: the 3 x 3 / stride-2 max-pool (csrc/salun_pool.hip),
uint8 HWC -> normalised fp32 CHW (csrc/salun_imgnorm.hip) and the evaluation head (csrc/salun_cls_head.hip), each
against torch on the CPU or the float64 restatement of cls_head_ref_cpu.py / conv_infer_ref_cpu.py.

Bounds of the head.  p: the per-element bound E_p of cls_head_ref_cpu.bounds — the head shares K23's statements up to p.
prob_sum: the sum of E_p[b, label] over the batch.  entropy_sum: E_p carried through f(p) = p log p, summed over the
batch: |f(p^) - f(p)| <= E_p (1 + |log(p - E_p)|) (the mean-value theorem; |f'| = |1 + log| grows towards 0), plus the
roundings of logf (LOG_U u), the product and the sum of K terms (gamma_(ceil(K / 256) + 8 + 3) of sum |p log p|).  The
float64 folds of B values add B 2^-53 relative, which the factor (1 + 2^-40) covers."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cls_head_ref_cpu as H
import conv_infer_ref_cpu as R

pytestmark = pytest.mark.gpu


def ops():
    from unlearn_saliency_amd import ops_infer
    return ops_infer


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------ pool
@pytest.mark.parametrize("shape", [(3, 7, 7), (2, 5, 9), (1, 1, 1), (2, 112, 112)], ids=str)
def test_pool_is_bit_equal_to_max_pool2d(shape):
    x = R.pool_data(shape)
    want = F.max_pool2d(x[None], 3, 2, 1)
    got = ops().maxpool3x3s2(x[None].cuda()).cpu()
    assert got.shape == want.shape and torch.equal(bits(got), bits(want))
    if shape[-1] > 1:
        assert bool(torch.isnan(want).any())


def test_pool_refuses_nonsense():
    from unlearn_saliency_amd import _lib
    x = torch.zeros(16, device="cuda")
    p = ctypes.c_void_p(x.data_ptr())
    f = _lib.lib().salun_maxpool3x3s2_forward
    assert f(p, p, 1, 2, 2, None) == -22 and f(None, p, 1, 2, 2, None) == -22 and f(p, None, 0, 2, 2, None) == -22
    assert f(p, ctypes.c_void_p(x.data_ptr() + 32), 1, 0, 2, None) == -22


# ------------------------------------------------------------------------------------------ normalise
@pytest.mark.parametrize("mean,std", [((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)), ((0.4914, 0.4822, 0.4465), (0.247, 0.243, 0.261))],
                         ids=["half", "uneven"])
def test_normalise_is_bit_equal_to_totensor_normalize(mean, std):
    """All 256 byte values in all 3 channels, each channel in another order, on a 2 x 16 x 24 x 3 batch."""
    g = torch.Generator().manual_seed(5)
    u = torch.stack([torch.stack([torch.arange(256)[torch.randperm(256, generator=g)] for _ in range(3)], -1)
                     for _ in range(3)]).view(2, 16, 24, 3).to(torch.uint8)
    assert all(len(set(u[..., c].reshape(-1).tolist())) == 256 for c in range(3))
    want = R.normalize_u8(u, mean, std)
    table = ops().u8_norm_table(mean, std)
    ref_table = R.normalize_u8(torch.arange(256, dtype=torch.uint8).view(1, 256, 1, 1).repeat(1, 1, 1, 3), mean, std)
    assert torch.equal(bits(table), bits(ref_table[0, :, :, 0]))
    got = ops().u8_to_chw_norm(u.cuda(), table.cuda()).cpu()
    assert got.shape == want.shape and torch.equal(bits(got), bits(want))


# ------------------------------------------------------------------------------------------ the evaluation head
C, HW, K = 512, 49, 10


def head_inputs(B, min_gap=1e-3):
    """Gaussian inputs whose float64 logits have a top-two gap above `min_gap` in every row (seed searched on the CPU)."""
    for seed in range(200):
        x, w, bias, _ = H.gaussian((B, C, HW, K), seed=seed)
        ex = H.model(x, w, bias, np.zeros(B, np.int64))
        if float(R.top_two_gap(torch.from_numpy(ex.logits)).min()) > min_gap:
            return x, w, bias, ex
    raise AssertionError("no seed gives the gap")


def entropy_bound(ex, e_p, skip=None):
    p = ex.p
    inner = np.maximum(p - e_p, 1e-300)
    t = e_p * (1 + np.abs(np.log(inner))) + H.gamma(math.ceil(K / 256) + 11) * np.abs(p * np.log(p)) * (1 + H.LOG_U)
    if skip is not None:
        t[:, skip] = 0
    return t.sum(-1)


def run_head(x, w, bias, label, meters, zero_safe=False):
    o = ops()
    logits, p = o.cls_head_eval(torch.from_numpy(x).cuda().view(x.shape[0], C, 7, 7), torch.from_numpy(w).cuda(),
                                torch.from_numpy(bias).cuda(), label, meters, zero_safe)
    return logits.cpu().numpy().astype(np.float64), p.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("B", [1, 5, 64])
def test_head_against_the_float64_restatement(B):
    x, w, bias, ex = head_inputs(B)
    label = 3
    bd = H.bounds(ex, x, w, bias)
    f = R.eval_figures(torch.from_numpy(ex.logits), label)
    m = ops().EvalMeters("cuda")
    logits, p = run_head(x, w, bias, label, m)
    got = m.read()
    print(f"head B = {B}: worst |p - p64| / E_p = {float((np.abs(p - ex.p) / bd.p).max()):.4f}")
    assert bool((np.abs(logits - ex.logits) <= bd.logits).all())
    assert bool((np.abs(p - ex.p) <= bd.p).all())
    assert got["hits"] == f.hits and got["count"] == B
    slack = 1 + 2.0 ** -40
    e_prob = float(bd.p[:, label].sum()) * slack
    e_ent = float(entropy_bound(ex, bd.p).sum()) * slack
    print(f"head B = {B}: |prob_sum - f64| = {abs(got['prob_sum'] - f.prob_sum):.3e} (bound {e_prob:.3e}), "
          f"|entropy_sum - f64| = {abs(got['entropy_sum'] - f.entropy_sum):.3e} (bound {e_ent:.3e})")
    assert abs(got["prob_sum"] - f.prob_sum) <= e_prob
    assert abs(got["entropy_sum"] - f.entropy_sum) <= e_ent
    assert e_prob <= B * float(bd.p.max()) * slack                 # "that bound times B"
    # a second call gives the same bits and accumulates into the same meters
    logits2, p2 = run_head(x, w, bias, label, m)
    again = m.read()
    assert np.array_equal(logits, logits2) and np.array_equal(p, p2)
    assert again["hits"] == 2 * f.hits and again["count"] == 2 * B
    assert abs(again["prob_sum"] - 2 * f.prob_sum) <= 2 * e_prob and abs(again["entropy_sum"] - 2 * f.entropy_sum) <= 2 * e_ent


def test_head_two_batches_accumulate_into_the_same_meters():
    xa, w, bias, ea = head_inputs(5)
    for seed in range(200):                                  # a second batch under the SAME weights, gap checked again
        xb = H.gaussian((64, C, HW, K), seed=1000 + seed)[0]
        eb = H.model(xb, w, bias, np.zeros(64, np.int64))
        if float(R.top_two_gap(torch.from_numpy(eb.logits)).min()) > 1e-3:
            break
    else:
        raise AssertionError("no seed gives the gap")
    label = 0
    m = ops().EvalMeters("cuda")
    run_head(xa, w, bias, label, m)
    run_head(xb, w, bias, label, m)
    got = m.read()
    fa, fb = R.eval_figures(torch.from_numpy(ea.logits), label), R.eval_figures(torch.from_numpy(eb.logits), label)
    ba, bb = H.bounds(ea, xa, w, bias), H.bounds(eb, xb, w, bias)
    assert got["count"] == 69 and got["hits"] == fa.hits + fb.hits
    assert abs(got["prob_sum"] - fa.prob_sum - fb.prob_sum) <= (ba.p[:, label].sum() + bb.p[:, label].sum()) * (1 + 2.0 ** -40)
    assert abs(got["entropy_sum"] - fa.entropy_sum - fb.entropy_sum) <= \
        (entropy_bound(ea, ba.p).sum() + entropy_bound(eb, bb.p).sum()) * (1 + 2.0 ** -40)


def test_head_entropy_of_an_underflowed_probability():
    """A class 200 below the maximum: exp underflows to 0 in fp32.  zero_safe = 0 gives the reference's NaN; zero_safe = 1
    a finite entropy equal to the float64 value with the 0 * log 0 term dropped."""
    x, w, bias, _ = head_inputs(5)
    w, bias = w.copy(), bias.copy()
    w[7], bias[7] = 0.0, -200.0
    ex = H.model(x, w, bias, np.zeros(5, np.int64))
    assert float((ex.m - ex.logits[:, 7]).min()) > 195
    m0, m1 = ops().EvalMeters("cuda"), ops().EvalMeters("cuda")
    _, p0 = run_head(x, w, bias, 1, m0, zero_safe=False)
    _, p1 = run_head(x, w, bias, 1, m1, zero_safe=True)
    assert bool((p0[:, 7] == 0).all()) and np.array_equal(p0, p1)
    assert math.isnan(m0.read()["entropy_sum"]) and m0.read()["count"] == 5
    f = R.eval_figures(torch.from_numpy(ex.logits), 1, drop_zero_below=1e-60)
    bd = H.bounds(ex, x, w, bias)
    got = m1.read()
    assert math.isfinite(got["entropy_sum"])
    assert abs(got["entropy_sum"] - f.entropy_sum) <= float(entropy_bound(ex, bd.p, skip=7).sum()) * (1 + 2.0 ** -40)
    assert abs(got["prob_sum"] - f.prob_sum) <= float(bd.p[:, 1].sum()) * (1 + 2.0 ** -40)


def test_head_refusals():
    from unlearn_saliency_amd import _lib
    L = _lib.lib()
    t = torch.zeros(4096, device="cuda")
    p = ctypes.c_void_p(t.data_ptr())
    args = lambda label, ws_bytes: (p, p, p, label, p, p, None, None, None, None, 1, 8, 4, 10, 0, p, ws_bytes, None)
    assert L.salun_cls_head_eval(*args(10, 4096)) == -22 and L.salun_cls_head_eval(*args(-1, 4096)) == -22
    assert L.salun_cls_head_eval(*args(0, 8)) == -28
    assert L.salun_cls_head_eval_workspace_bytes(5, 512, 10) == 16 + 40 and L.salun_cls_head_eval_workspace_bytes(0, 512, 10) == 0
