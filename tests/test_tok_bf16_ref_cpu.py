"""The float64 model of K14 in tok_bf16_ref_cpu.py against torch's float64 layer_norm / a * gelu(b) and autograd; the
premises of the exact tier (inputs and answers are bf16 / fp32 numbers, every partial sum below 2^24 units, no exact y a
cancellation); the mirror of the host logic against the numbers the cases are there for and against the library's
query; the coverage of the labels; and the bound itself: an fp32 emulation of each kernel's formulas stays inside it on
every Gaussian case, and two deliberately wrong emulations do not.  No GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

import tok_bf16_ref_cpu as R

_id = R._cid
F64 = torch.float64


def close(got, want, tol=1e-12):
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= tol * max(float(want.abs().max()), 1e-300)


def unit_of(t):
    """The largest power of two that every element of t is a whole multiple of."""
    k = 0
    while not torch.equal(t * 2.0 ** k, (t * 2.0 ** k).round()):
        k += 1
        assert k < 80
    return 2.0 ** -k


def capped(terms, dim):
    """Every partial sum of `terms` over `dim`, in any order, is exact in fp32."""
    return float(terms.abs().sum(dim).max()) / unit_of(terms) < 2 ** 24


def fp32_all(*ts):
    return all(R.is_f32(t) for t in ts)


def is_bf16(*ts):
    return all(torch.equal(R.bf16_round(t), t) and torch.equal(t.bfloat16().double(), t) for t in ts)


# ------------------------------------------------------------------------------------------ model against torch
@pytest.mark.parametrize("c", R.LN_CASES, ids=_id)
def test_ln_model_agrees_with_torch_float64(c):
    t = R.ln_gauss_inputs(c, offset=16.0)
    assert is_bf16(t.x, t.dy) and fp32_all(t.gamma, t.beta)
    x, g, b = (v.clone().requires_grad_(True) for v in (t.x, t.gamma, t.beta))
    y = F.layer_norm(x, (c.C,), g, b, t.eps)
    y.backward(t.dy)
    o = R.ln16_forward(t.x, t.gamma, t.beta, t.eps)
    close(o.y64, y.detach())
    assert torch.equal(o.y, R.bf16_round(o.y64)) and torch.equal(o.stats, torch.stack((o.mean, o.rstd), 1))
    close(o.mean, t.x.mean(1))
    close(o.rstd, 1 / torch.sqrt(t.x.var(1, unbiased=False) + t.eps))
    k = R.ln16_backward(t.dy, t.x, t.gamma, o.mean, o.rstd, t.gacc, t.bacc)
    close(k.dx64, x.grad)
    close(k.dgamma, g.grad + t.gacc)
    close(k.dbeta, b.grad + t.bacc)
    a = R.ln16_backward(t.dy, t.x, t.gamma, o.mean, o.rstd, absolute=True)
    assert (a.dx64 >= k.dx64.abs() * (1 - 1e-12)).all() and (a.dgamma >= (k.dgamma - t.gacc).abs() * (1 - 1e-9)).all()
    assert (R.ln16_forward(t.x, t.gamma, t.beta, t.eps, absolute=True).y >= o.y64.abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize("shift", R.GEGLU_SHIFTS)
@pytest.mark.parametrize("c", R.GEGLU_CASES, ids=_id)
def test_geglu_model_agrees_with_torch_float64(c, shift):
    t = R.geglu_gauss_inputs(c, shift)
    assert is_bf16(t.h, t.dy)
    h = t.h.clone().requires_grad_(True)
    a, b = h.chunk(2, dim=-1)
    out = a * F.gelu(b)
    out.backward(t.dy)
    o, k = R.geglu16_forward(t.h), R.geglu16_backward(t.h, t.dy)
    close(o.out64, out.detach())
    close(k.dh64[:, c.F:], h.grad[:, c.F:])
    if (c.rows, c.F, shift) == (1, 8, -4.0):
        # torch forms 1 + erf in float64: an absolute error of a few 2^-53 there, which the model's erfc form does not
        # have.  Eight gates around -4 leave dy gelu(b) with nothing large to hide it behind: this one comparison is
        # allowed torch's own loss, 2^-51 of what multiplies 1 + erf, beyond 1e-12 of the largest entry
        got, want = k.dh64[:, :c.F], h.grad[:, :c.F]
        assert bool(((got - want).abs() <= 1e-12 * want.abs().max() + 2.0 ** -51 * (t.dy * t.h[:, c.F:]).abs()).all())
    else:
        close(k.dh64[:, :c.F], h.grad[:, :c.F])
    assert (R.geglu16_backward(t.h, t.dy, absolute=True).dh64 >= k.dh64.abs() * (1 - 1e-12)).all()


def test_gelu_of_the_model_keeps_its_digits_in_the_negative_tail():
    """Against the C library's erfc at b = -5, -8, -16: where 1 + erf has lost its digits or is 0."""
    b = torch.tensor([-5.0, -8.0, -16.0], dtype=F64)
    want = torch.tensor([0.5 * v * math.erfc(-v / math.sqrt(2.0)) for v in b.tolist()], dtype=F64)
    assert -5e-15 < float(want[1]) < -4.9e-15
    got = R.gelu(b)
    assert float(((got - want) / want).abs().max()) < 1e-12
    naive = 0.5 * b * (1 + torch.erf(b * R.SQRT1_2))
    assert float(naive[2]) == 0.0 and abs(float(naive[0] / want[0]) - 1) > 1e-12
    assert float(R.bf16_round(want[1:2])) == float(want[1:2].float().bfloat16()) != 0.0      # gelu(-8) is a bf16 number
    assert -8.0 not in R.GATES and 8.0 not in R.GATES


# ------------------------------------------------------------------------------------------ the premises of the exact tier
@pytest.mark.parametrize("family", R.ln_families())
@pytest.mark.parametrize("c", R.LN_CASES, ids=_id)
def test_ln_exact_cases_are_exact_in_every_summation_order(c, family):
    rows, C = c[:2]
    t = R.ln_exact_inputs(c, family)
    assert is_bf16(t.x, t.dy) and fp32_all(t.gamma, t.beta, t.gacc, t.bacc)
    assert capped(t.x, 1) and capped((t.x - t.m[:, None]) ** 2, 1)
    o = R.ln16_forward(t.x, t.gamma, t.beta, t.eps)
    assert torch.equal(o.mean, t.m) and torch.equal(o.var, 4 * t.s * t.s) and torch.equal(o.rstd, t.rstd)
    assert fp32_all(o.var + t.eps, o.stats) and (rows == 1 or len(set(zip(o.mean.tolist(), o.rstd.tolist()))) > 1)
    assert bool((o.stats[1:] != o.stats[:-1]).any(1).all())          # a neighbouring row's statistic is another number
    assert set((2 * o.xh).abs().unique().tolist()) <= {0.0, 1.0, 2.0, 4.0}
    assert fp32_all(t.x - o.mean[:, None], o.xh, o.xh * t.gamma, o.y64) and is_bf16(o.y64) and torch.equal(o.y, o.y64)
    # no exact y is a cancellation
    terms = (o.xh * t.gamma).abs() + t.beta.abs()
    assert bool(torch.where(o.xh == 0, o.y64 == t.beta, o.y64.abs() >= 2.0 ** -6 * terms).all())
    gv = t.gamma[None, :]
    for dy in (t.dy, R.ln_vanishing_dy(t.x, t.gamma, o.mean, o.rstd)):
        vanishing = dy is not t.dy
        assert is_bf16(dy) and float(dy.abs().max()) > 0
        k = R.ln16_backward(dy, t.x, t.gamma, o.mean, o.rstd, t.gacc, t.bacc)
        assert fp32_all(k.g, k.g * k.xh, dy * k.xh) and capped(k.g, 1) and capped(k.g * k.xh, 1)
        assert capped(dy, 0) and capped(dy * k.xh, 0) and fp32_all(k.dgamma, k.dbeta, k.dgamma - t.gacc, k.dbeta - t.bacc)
        if vanishing:
            assert not k.m1.any() and not k.m2.any() and torch.equal(k.dx64, o.rstd[:, None] * gv * dy) and is_bf16(k.dx64)
            assert float((dy != 0).double().mean()) > 0.4
        if R.ln_exact_dx(c, vanishing):
            m1, m2 = k.m1[:, None], k.m2[:, None]
            assert fp32_all(k.m1, k.m2, k.g - m1, k.xh * m2, k.g - m1 - k.xh * m2, k.dx64)
            assert torch.equal(k.dx, R.bf16_round(k.dx64))


@pytest.mark.parametrize("c", R.GEGLU_CASES, ids=_id)
def test_geglu_exact_cases_have_bf16_answers(c):
    t = R.geglu_exact_inputs(c)
    a, b = t.h[:, :c.F], t.h[:, c.F:]
    assert is_bf16(t.h, t.dy) and set(b.unique().tolist()) <= set(R.GATES)
    o, k = R.geglu16_forward(t.h), R.geglu16_backward(t.h, t.dy)
    pos = b.clamp_min(0)
    assert torch.equal(o.out, a * pos) and torch.equal(k.dh[:, :c.F], t.dy * pos)
    assert torch.equal(k.dh[:, c.F:], t.dy * a * torch.where(b > 0, 1.0, torch.where(b == 0, 0.5, 0.0)).double())
    assert is_bf16(a * pos, t.dy * pos, t.dy * a, t.dy * a / 2)
    # the rounded float64 answer is a bf16 number at a distance from its neighbours that fp32 cannot bridge
    assert float((o.out64 - o.out).abs().max()) <= 1e-30 and float((k.dh64 - k.dh).abs().max()) <= 1e-30
    if c.rows * c.F >= 16:
        assert len(b.unique()) == len(R.GATES)


# ------------------------------------------------------------------------------------------ the mirror, the labels
def test_the_mirror_gives_the_numbers_the_cases_are_there_for():
    assert R.ln_parts(65541) == 1024 and R.rows_per_wg(65541) == 65
    per = R.wg_rows(65541)
    assert per[1008] == 21 and R.empty_wgs(65541) == list(range(1009, 1024)) and len(R.empty_wgs(65541)) == 15
    assert sum(per) == 65541 and set(per[:1008]) == {65}
    assert [R.ln_parts(r) for r in (1, 64, 65, 67, 130, 193, 4097, 65536, 65537)] == [1, 1, 2, 2, 3, 4, 65, 1024, 1024]
    assert [R.rows_per_wg(r) for r in (67, 130, 193, 4097)] == [34, 44, 49, 64] and R.wg_rows(130) == [44, 44, 42]
    assert R.rows_per_wg(65536) == 64 and not R.empty_wgs(65536)
    assert set(R.octets_per_lane(512)) == {1} and R.octets_per_lane(520) == [2] + [1] * 63
    assert R.octets_per_lane(1032) == [3] + [2] * 63 and set(R.octets_per_lane(2048)) == {4}
    assert R.octets_per_lane(8) == [1] + [0] * 63 and R.octets_per_lane(320) == [1] * 40 + [0] * 24
    assert R.ln_lds_bytes(2048) == 48 * 1024 and R.ln_c1(512) == 14 and R.ln_c1(520) == 22 and R.ln_c1(2048) == 38
    assert R.geglu_trips(2049, 2048) == (2, 256) and R.geglu_grid(2049, 2048) == 2048
    assert R.geglu_trips(2048, 2048) == (1, 0) and R.geglu_trips(1, 8) == (1, 0) and R.geglu_grid(7, 1280) == 5
    assert all(R.ln_ok(c.rows, c.C) for c in R.LN_CASES) and all(R.geglu_ok(c.rows, c.F) for c in R.GEGLU_CASES)
    assert not any(R.ln_ok(4, C) for C in R.LN_OUTSIDE_C) and not R.ln_ok(0, 8)
    assert not any(R.geglu_ok(4, Fh) for Fh in R.GEGLU_OUTSIDE_F)
    assert all(c.rows * c.C <= 2049 * 2048 for c in R.LN_CASES) and all(c.rows * c.F <= 2049 * 2048 for c in R.GEGLU_CASES)


def test_mirror_agrees_with_the_library_query():
    from unlearn_saliency_amd import _lib
    _lib.build()
    L = _lib.lib()
    n = 0
    for rows in (0, 1, 3, 63, 64, 65, 193, 4097, 65535, 65536, 65537, 65541, 1 << 20):
        for C in (0, 4, 8, 12, 16, 24, 320, 512, 520, 2040, 2048, 2056, -8):
            assert L.salun_ln_bf16_workspace_bytes(rows, C) == R.ln_ws_bytes(rows, C), (rows, C)
            n += 1
    assert n > 100 and R.ln_ws_bytes(65541, 8) == 1024 * 8 * 8


def test_cases_meet_every_required_label():
    seen = set().union(*(R.ln_routes(c.rows, c.C) for c in R.LN_CASES))
    assert not [r for r in R.LN_REQUIRED if r not in seen]
    seen = set().union(*(R.geglu_routes(c.rows, c.F) for c in R.GEGLU_CASES))
    assert not [r for r in R.GEGLU_REQUIRED if r not in seen]
    arena = set().union(*(R.ln_routes(c.rows, c.C) for c in R.LN_ARENA))
    assert {"parts capped", "empty workgroups", "four full slots", "C npo2", "one lane, one row", "C/8=64", "third slot partial",
            "C/8=65: lane 0 alone owns a second octet"} <= arena
    assert R.LN_BIG in R.LN_ARENA and R.GEGLU_BIG in R.GEGLU_ARENA


# ------------------------------------------------------------------------------------------ the reference alone, inside the bound
def worst(got, exact, bound):
    err = (got - exact).abs()
    assert bool(torch.isfinite(bound).all()) and bool((bound > 0).all() or (err[bound == 0] == 0).all())
    return float((err / bound.clamp_min(1e-300)).max())


def ln_ratios(c, offset, wrong=None):
    t = R.ln_gauss_inputs(c, offset)
    e = R.emulate_ln(t, wrong)
    o, bf = R.ln16_forward(t.x, t.gamma, t.beta, t.eps), R.ln16_forward_bound(t.x, t.gamma, t.beta, t.eps)
    k = R.ln16_backward(t.dy, t.x, t.gamma, e.mean, e.rstd)           # the backward model on the stats it is handed
    bb = R.ln16_backward_bound(t.dy, t.x, t.gamma, e.mean, e.rstd)
    return {"y": worst(e.y, o.y64, bf.y), "mean": worst(e.mean, o.mean, bf.mean), "rstd": worst(e.rstd, o.rstd, bf.rstd),
            "dx": worst(e.dx, k.dx64, bb.dx), "dgamma": worst(e.dgamma, k.dgamma, bb.dgamma),
            "dbeta": worst(e.dbeta, k.dbeta, bb.dbeta)}


def geglu_ratios(c, shift, wrong=None):
    t = R.geglu_gauss_inputs(c, shift)
    assert float(t.h[:, c.F:].abs().max()) < 12
    e = R.emulate_geglu(t, wrong)
    o, k = R.geglu16_forward(t.h), R.geglu16_backward(t.h, t.dy)
    bf, bb = R.geglu16_forward_bound(t.h), R.geglu16_backward_bound(t.h, t.dy)
    r = {"out": worst(e.out, o.out64, bf.out), "dh_a": worst(e.dh[:, :c.F], k.dh64[:, :c.F], bb.dh[:, :c.F]),
         "dh_b": worst(e.dh[:, c.F:], k.dh64[:, c.F:], bb.dh[:, c.F:])}
    tail = R.in_tail(t.h)
    if bool(tail.any()):
        r["out, tail"] = worst(e.out[tail], o.out64[tail], bf.out[tail])
        r["dh_b, tail"] = worst(e.dh[:, c.F:][tail], k.dh64[:, c.F:][tail], bb.dh[:, c.F:][tail])
    return r


@pytest.mark.parametrize("offset", R.LN_OFFSETS)
@pytest.mark.parametrize("c", R.LN_CASES, ids=_id)
def test_an_fp32_emulation_of_layer_norm_is_inside_the_bound(c, offset):
    r = ln_ratios(c, offset)
    print(f"ln {_id(c)} mu/sigma={offset:g}: worst |emulation - exact| / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("shift", R.GEGLU_SHIFTS)
@pytest.mark.parametrize("c", R.GEGLU_CASES, ids=_id)
def test_an_fp32_emulation_of_geglu_is_inside_the_bound(c, shift):
    r = geglu_ratios(c, shift)
    print(f"geglu {_id(c)} shift={shift:g}: worst |emulation - exact| / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r
    if c.rows * c.F >= 1 << 13 and shift:
        assert "out, tail" in r                                     # the interval [-6, -3] is populated


@pytest.mark.parametrize("c", [c for c in R.LN_CASES if c.C > 8], ids=_id)
def test_gamma_of_the_neighbouring_channel_is_outside_the_bound(c):
    r = ln_ratios(c, 0.0, wrong="gamma shifted")
    assert r["y"] > 1.0 and r["dx"] > 1.0, r
    assert max(r["mean"], r["rstd"], r["dgamma"], r["dbeta"]) <= 1.0, r      # what gamma does not enter stays inside


@pytest.mark.parametrize("c", [c for c in R.GEGLU_CASES if c.rows * c.F >= 1 << 13], ids=_id)
def test_the_tanh_form_of_gelu_is_outside_the_bound(c):
    r = geglu_ratios(c, 0.0, wrong="tanh")
    assert r["out"] > 1.0 and r["dh_a"] > 1.0 and r["dh_b"] > 1.0, r
