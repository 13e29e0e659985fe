"""gemm_bf16_ref_cpu.py on the CPU: the float64 model against torch.matmul, the exactness conditions of the integer tier, the
labels and splits the case tables claim against the library's host-only route query, the edges the tables must reach
(read from nt_facts / tn_facts), and that the exact tier's checker can tell a subtly wrong kernel from a right one.
No GPU."""
import ctypes
from functools import lru_cache

import pytest
import torch

import bf16_routes as M
import gemm_bf16_ref_cpu as R

F64 = torch.float64
NT, TN = 0, 1                         # SALUN_GEMM_BF16_NT / _TN
EINVAL, ENOSPC = -22, -28
_id = lambda c: c.id


@pytest.fixture(scope="module")
def L():
    from unlearn_saliency_amd import _lib
    _lib.build()
    return _lib.lib()


def gemm_route(L, op, m, n, k, variant=0, ws_bytes=0):
    buf, ns = ctypes.create_string_buffer(64), ctypes.c_int(-1)
    rc = L.salun_gemm_bf16_route(op, m, n, k, variant, ws_bytes, buf, 64, ctypes.byref(ns))
    return None if rc == EINVAL else M.ENOSPC if rc == ENOSPC else (buf.value.decode(), ns.value)


def _nt_exact(c):
    t = R.nt_inputs(c, "int")
    return t, R.nt_model(t.x, t.w, t.bias, t.addend)


_cached = lru_cache(maxsize=None)(_nt_exact)


def nt_exact(c):
    """-> (integer inputs, the exact answer with bias and addend); kept for the tests that share it, the two large cases apart"""
    return _nt_exact(c) if c.big else _cached(c)


def is_bf16(t64):
    return torch.equal(t64.float().bfloat16().to(F64), t64)


def is_f32(t64):
    return torch.equal(t64.float().to(F64), t64)


# ------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("c", R.NT_CASES, ids=_id)
def test_nt_model_is_the_float64_matmul_and_the_integer_tier_is_exact(c):
    t, y = nt_exact(c)
    assert is_bf16(t.x) and is_bf16(t.w) and is_f32(t.bias) and is_bf16(t.addend)
    for v in (t.x * 2.0 ** -R.scales(c)[0], t.w * 2.0 ** -R.scales(c)[1], t.bias / t.unit, t.addend / t.unit):
        assert torch.equal(v, v.round())                                   # whole multiples of the unit
    assert float((t.bias / t.unit).abs().min()) >= R.BIAS_LO               # y in the thousands of units
    want = torch.matmul(t.x, t.w.t()) + t.bias + t.addend
    assert torch.equal(y, want)                                            # integers: float64 is exact in any order
    for terms in R.NT_EPILOGUES:
        worst = R.nt_model(t.x, t.w, *R.pick(t, terms), absolute=True).max() / t.unit
        assert float(worst) <= R.nt_worst_units(c, terms) < 2 ** 24, terms
        assert is_bf16(R.to_bf16_rne(R.nt_model(t.x, t.w, *R.pick(t, terms)))), terms
    if not c.big:
        g = R.nt_inputs(c, "gauss")
        assert is_bf16(g.x) and is_bf16(g.w) and is_f32(g.bias) and is_bf16(g.addend)
        got, ref = R.nt_model(g.x, g.w, g.bias, g.addend), torch.matmul(g.x, g.w.t()) + g.bias + g.addend
        mag = R.nt_model(g.x, g.w, g.bias, g.addend, absolute=True)
        assert bool(((got - ref).abs() <= 1e-13 * mag).all())
        assert bool((mag >= got.abs()).all())


@pytest.mark.parametrize("c", R.TN_CASES, ids=_id)
def test_tn_model_is_the_float64_matmul_and_the_integer_tier_is_exact(c):
    t = R.tn_inputs(c, "int")
    assert is_bf16(t.dy) and is_bf16(t.x) and is_f32(t.dw0)
    for v in (t.dy * 2.0 ** -R.scales(c)[0], t.x * 2.0 ** -R.scales(c)[1], t.dw0 / t.unit):
        assert torch.equal(v, v.round())
    dw = R.tn_model(t.dy, t.x, t.dw0)
    assert torch.equal(dw, torch.matmul(t.dy.t(), t.x) + t.dw0)
    for acc in (False, True):
        worst = R.tn_model(t.dy, t.x, t.dw0 if acc else None, absolute=True).max() / t.unit
        assert float(worst) <= R.tn_worst_units(c, acc) < 2 ** 24
        assert is_f32(R.tn_model(t.dy, t.x, t.dw0 if acc else None))
    if c.Na == c.Nb:                                                       # the transposed answer is another matrix
        assert not torch.equal(R.tn_model(t.dy, t.x), R.tn_model(t.dy, t.x).t())
        assert not torch.equal(R.tn_model(t.dy, t.x), R.tn_model(t.x, t.dy))
    g = R.tn_inputs(c, "gauss")
    assert is_bf16(g.dy) and is_bf16(g.x) and is_f32(g.dw0)
    got, ref = R.tn_model(g.dy, g.x, g.dw0), torch.matmul(g.dy.t(), g.x) + g.dw0
    assert bool(((got - ref).abs() <= 1e-13 * R.tn_model(g.dy, g.x, g.dw0, absolute=True)).all())


def test_pack_model_and_its_special_values():
    v, want = R.pack_specials()
    assert is_f32(v) and is_bf16(want)
    assert torch.equal(R.pack_model(v), want)
    assert torch.equal(v.float().bfloat16().to(F64), want)                  # torch's own cast rounds to nearest even too
    assert torch.equal(torch.signbit(R.pack_model(v)), torch.signbit(want))
    ties = R.is_bf16_tie(v) & (v != 0)
    up = (want.abs() > v.abs()) & ties
    assert int(ties.sum()) >= 8 and 0 < int(up.sum()) < int(ties.sum())    # both parities: ties go up and down
    assert bool((torch.frexp(want)[1] > torch.frexp(v)[1]).any())          # one rounds up into the next binade
    w = R.pack_inputs(37, 53, 1)
    assert torch.equal(R.pack_model(w, True), w.float().t().contiguous().bfloat16().to(F64))
    for N, K in R.PACK_PLAIN:
        assert is_f32(R.pack_inputs(N, K, 2))
    assert {N * K % 4 for N, K in R.PACK_PLAIN} == {0, 1, 2, 3}


def test_impulse_codes_are_distinct_bf16_numbers():
    v = R.codes(128, 320)
    assert is_bf16(v) and len(torch.unique(v)) == v.numel() and float(v.abs().min()) > 2.0 ** -120
    with pytest.raises(AssertionError):
        R.codes(1, R.MAX_CODES + 1)
    assert len(R.NT_IMPULSE) >= 13 and {c.variant for c in R.NT_IMPULSE} == set(range(1, 14))
    assert {R.tn_facts(c).variant for c in R.TN_IMPULSE} == {1, 2, 3} and any(c.splits > 1 for c in R.TN_IMPULSE)
    for c in R.NT_IMPULSE:
        pts = R.nt_impulse_points(c)
        bk = R.nt_facts(c).bk
        assert {(0, 0), (c.M - 1, c.K - 1)} <= set(pts) and {k for _, k in pts} >= {bk - 1, bk}
        x, w, want = R.nt_impulse(c, *pts[-1])
        assert torch.equal(R.nt_model(x, w), want) and is_bf16(want)
    for c in R.TN_IMPULSE:
        pts = R.tn_impulse_points(c)
        rst = R.tn_facts(c).rst
        assert {(0, 0), (c.M - 1, c.Na - 1)} <= set(pts) and {m for m, _ in pts} >= {rst - 1, rst}
        dy, x, want = R.tn_impulse(c, *pts[-1])
        assert torch.equal(R.tn_model(dy, x), want) and is_f32(want)


# ------------------------------------------------------------------------------------------ labels and splits
def test_the_route_query_gives_the_label_and_split_every_case_claims(L):
    for c in R.NT_CASES:
        assert gemm_route(L, NT, c.M, c.N, c.K, c.variant) == (c.label, 1) == M.gemm_nt(c.M, c.N, c.K, c.variant), c.id
        assert R.nt_label(R.nt_facts(c).variant) == c.label
    for c in R.TN_CASES:
        f = R.tn_facts(c)
        ws = L.salun_gemm_bf16_tn_workspace_bytes(c.M, c.Na, c.Nb, c.variant)
        assert ws == f.ws_bytes == M.tn_workspace_bytes(c.M, c.Na, c.Nb, c.variant), c.id
        assert gemm_route(L, TN, c.M, c.Na, c.Nb, c.variant, ws) == (c.label, c.splits) == (f.label, f.splits), c.id
        assert M.gemm_tn(c.M, c.Na, c.Nb, c.variant, ws) == (c.label, c.splits)
    for m, n, k, v in R.NT_REFUSED:
        assert gemm_route(L, NT, m, n, k, v) is None and M.gemm_nt(m, n, k, v) is None, (m, n, k, v)
    for m, na, nb, v in R.TN_REFUSED:
        assert gemm_route(L, TN, m, na, nb, v, 1 << 30) is None and M.gemm_tn(m, na, nb, v, 1 << 30) is None, (m, na, nb, v)
    m, na, nb, v = R.TN_SHORT_WS
    ws = L.salun_gemm_bf16_tn_workspace_bytes(m, na, nb, v)
    assert ws > 0 and gemm_route(L, TN, m, na, nb, v, ws - 1) == M.ENOSPC == M.gemm_tn(m, na, nb, v, ws - 1)
    for m, n, k in R.AGREE:
        assert sum(M.gemm_nt(m, n, k, v) is not None for v in range(1, 14)) >= 5


def test_the_nt_cases_reach_every_form_and_every_edge():
    facts = {c: R.nt_facts(c) for c in R.NT_CASES}
    assert {c.label for c in R.NT_CASES if c.variant} == {M.NT_ARMS[v][0] for v in M.NT_ARMS}
    assert {c.variant for c in R.NT_CASES} == set(range(14))
    assert {facts[c].variant for c in R.NT_CASES if c.variant == 0} == {10, 11, 13}
    for v, (fam, wgm, wgn, nst, bk) in R.NT_FORMS.items():
        mine = [c for c in R.NT_CASES if c.variant == v]
        assert {c.K for c in mine} >= set(R.K_STEPS), v
        assert {c.M for c in mine} >= {1, 33, 64 * wgm - 1, 64 * wgm + 1, 77}, v
        assert {c.N for c in mine} >= ({64} if wgn == 1 else {128, 384}), v
        assert {facts[c].tile_class for c in mine} == {"ntile < 8", "ntile = 8q", "ntile = 8q + r"}, v
        assert any(facts[c].rows_past_m for c in mine) and any(facts[c].mfma_tile_partial for c in mine), v
        if fam == "nt_r":
            # every class of k-steps against the ring's depth that a K % 64 == 0 can give (the 32-deep forms never see
            # fewer than 2 steps, nor 3), and with them every arm of the wait selection the form has
            reachable = R.ring_classes_reachable(nst, bk)
            assert {facts[c].nk_class for c in mine} == reachable, v
            assert len(reachable) == (4 if bk == 64 else nst - 1), v   # 32-deep: {= NST-1, > NST} / {< NST-1, = NST, > NST}
            assert set().union(*[facts[c].arms for c in mine]) == ({R.KEEP, R.ONE, R.DRAIN} if nst == 4 else {R.KEEP, R.DRAIN}), v
            assert all(facts[c].ep == (2 if bk == 32 else 1) for c in mine), v
            if bk == 32:
                assert any(facts[c].ep2_second_pass_partial for c in mine), v
        if fam == "nt_p":
            big = [c for c in mine if c.big]
            assert len(big) == 1
            f = facts[big[0]]
            assert f.tiles == 513 and f.tiles_per_wg == 2 and f.one_tile_wg and f.early_return and f.crosses_tile
            assert f.empty_xcds == [1, 2, 3, 4, 5, 6, 7]
            assert any(facts[c].early_return and facts[c].tiles_per_wg == 1 for c in mine if not c.big)
    assert [(c.M, c.N, c.K, c.variant) for c in R.NT_CASES if c.big] == [(128 * 513 - 5, 128, 128, 5), (256 * 513 - 5, 64, 64, 6)]
    # both NST = 4 rings enter the middle arm
    assert all(any(R.ONE in facts[c].arms for c in R.NT_CASES if c.variant == v) for v in (7, 12))


def test_the_tn_cases_reach_every_form_and_every_edge():
    facts = {c: R.tn_facts(c) for c in R.TN_CASES}
    assert {c.variant for c in R.TN_CASES} == {0, 1, 2, 3}
    for v, (wga, wgb, rst, nst) in R.TN_FORMS.items():
        mine = [c for c in R.TN_CASES if c.variant == v]
        assert any(c.label == "tn<v%d>/S1" % v for c in mine) and any(c.splits > 1 for c in mine), v
        assert {c.M for c in mine} >= {1, rst - 1, rst + 1, 513, 16384}, v
        assert any(c.splits == 64 for c in mine), v
        one = {facts[c].stages_per_split[0] for c in mine if c.splits == 1}
        assert one >= {1, nst - 1, nst}, v
        assert set().union(*[facts[c].nk_classes for c in mine]) == {"< NST-1", "= NST-1", "= NST", "> NST"}, v
        assert set().union(*[facts[c].arms for c in mine]) == ({R.KEEP, R.ONE, R.DRAIN} if nst == 4 else {R.KEEP, R.DRAIN}), v
        assert any(facts[c].last_split_shorter for c in mine) and any(facts[c].last_stage_partial and c.splits > 1 for c in mine), v
        assert {c.Na for c in mine} >= {32, 96, 160, 288} and {c.Nb for c in mine} >= {32, 96, 160, 288}, v
        assert any(facts[c].zero_blocks for c in mine), v
        assert {facts[c].work_class for c in mine} >= {"work < 8", "work = 8q + r"}, v
    assert any(c.variant == 3 and c.Na == 32 for c in R.TN_CASES)
    assert any(R.ONE in facts[c].arms for c in R.TN_CASES)                  # the TN ring's NST = 4 arm (variant 2)
    assert {facts[c].variant for c in R.TN_CASES if c.variant == 0} == {2}


# ------------------------------------------------------------------------------------------ the checker can tell
def _round_with(t64, how):
    m, e = torch.frexp(t64)
    s = m * 256.0
    s = torch.trunc(s) if how == "truncate" else torch.sign(s) * torch.floor(s.abs() + 0.5)
    return torch.ldexp(s, e - 8)


SENSITIVE = [c for c in R.NT_CASES if c.M * c.N >= 4096]


@pytest.mark.parametrize("c", SENSITIVE, ids=_id)
def test_a_subtly_wrong_kernel_would_not_pass_the_exact_tier(c):
    t, exact = nt_exact(c)
    want = R.to_bf16_rne(exact)
    assert bool(R.is_bf16_tie(exact).any())                                 # the rounding of a tie is pinned
    assert not torch.equal(_round_with(exact, "truncate"), want)
    assert not torch.equal(_round_with(exact, "half away"), want)
    assert bool((want != exact).any())
    product = R.nt_model(t.x, t.w)
    assert not torch.equal(R.to_bf16_rne(R.to_bf16_rne(product) + t.bias + t.addend), want)       # epilogue after the rounding
    assert not torch.equal(R.to_bf16_rne(R.to_bf16_rne(product + t.bias) + t.addend), want)       # two roundings
    bk = R.nt_facts(c).bk
    stale = R.nt_model(t.x[:, :c.K - bk], t.w[:, :c.K - bk], t.bias, t.addend) if c.K > bk else t.bias + t.addend + 0 * exact
    assert bool((R.to_bf16_rne(stale) != want).any(dim=1).all())            # without the last k-step every row is wrong
    if c.M == c.N:
        assert not torch.equal(want, want.t())


def test_the_sensitive_cases_cover_every_form():
    assert {c.variant for c in SENSITIVE} == set(range(14)) and all(c in SENSITIVE for c in R.NT_CASES if c.big)


def test_the_bound_check_fails_on_a_nan_and_on_an_element_that_was_never_written(monkeypatch):
    """within_bound of the GPU tier, on the host: a NaN (the arena's sentinel is one, in fp32 and in every second bf16
    half) is outside every bound."""
    import test_gemm_bf16_exact_gpu as G
    from guarded_arena import SENTINEL
    monkeypatch.delenv("SALUN_MEASURED_DIR", raising=False)
    monkeypatch.setattr(G, "WORST", {})
    exact = torch.arange(1, 17, dtype=F64).view(4, 4)
    for bf16 in (False, True):
        G.within_bound("self-check", "none", exact.clone(), exact, exact, 64, 2, bf16)
        halves = torch.tensor([SENTINEL], dtype=torch.int32).view(torch.int16)
        unwritten = [float("nan"), float(torch.tensor([SENTINEL], dtype=torch.int32).view(torch.float32)[0])] + \
            [float(v) for v in G.values(halves)]
        assert sum(v != v for v in unwritten) == 3                           # the low bf16 half is a finite number
        for v in unwritten:
            got = exact.clone()
            got[2, 1] = v
            with pytest.raises(AssertionError):
                G.within_bound("self-check", "none", got, exact, exact, 64, 2, bf16)
    assert G.first_wrong(exact, exact[:2]).startswith("shape")
