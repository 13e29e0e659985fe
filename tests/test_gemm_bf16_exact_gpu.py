"""K16, the bf16 GEMMs of csrc/salun_gemm.hip (k_gemm_bf16_nt, _nt_p, _nt_r, k_gemm_bf16_tn + k_tn_reduce, k_pack_bf16,
k_pack_bf16_t), against the float64 model of gemm_bf16_ref_cpu.py (validated by test_gemm_bf16_ref_cpu.py), through the
C-ABI on a guarded arena (guarded_arena.py).  Before each call the test asks salun_gemm_bf16_route and asserts the label
the case claims; after each call everything but the outputs must hold the bits it was given.

(a) exact tier: small integers times one power of two per tensor.  Every fp32 partial sum is exact in every order and
    under every split (the cap asserted in test_gemm_bf16_ref_cpu.py), so y must EQUAL the model rounded once to bf16,
    nearest even - the sums are in the thousands of units and many are ties: the tier pins the rounding, and a stale ring
    stage is a wrong integer - and dw the model itself: NT without epilogue, with bias and with bias + addend; TN writing and
    accumulating, with the queried workspace and with NULL where none is needed.  A second call gives the same bits; all
    variants that accept a shape give the same bits.  A failure names the count and the first wrong (row, column).
(b) impulses: a single 1 in x (TN: dy), distinct bf16 codes in the other operand: that column where it belongs, 0 or the
    epilogue term elsewhere; first and last row, first and last k, both sides of a stage boundary, the last token.
(c) bound tier: Gaussian inputs.  With n the reduction length, e the epilogue additions (TN: the splits, + 1 when
    accumulating), u = 2^-24 and u16 = 2^-8 (derived, not measured):
        bf16 output  |got - exact| <= u16 |exact| + (1 + u16) gamma_(2n+e) abs_sum
        fp32 output  |got - exact| <= gamma_(2n+e) abs_sum
    no absolute slack, nothing scaled by a tensor's maximum.  The worst fraction of the bound per case and per label is
    printed and logged (profiles/gemm_bf16_bounds_measured.txt), not asserted.
(d) refusals: SALUN_EINVAL / SALUN_ENOSPC exactly where bf16_routes.py puts the call outside the domain (and for pointers
    4 bytes off a 16-byte boundary), every output sentinel in place.
(e) salun_pack_bf16: ties to even, signed zeros, the largest finite value, a round-up into the next binade; the scalar tail
    of the plain form and ragged 32 x 32 tiles of the transposed one, inside guards.
(f) conv_bf16.SalunLinearBF16 on the model, both tiers: y, dx, and dW / db in the flat arena's gradient sink over two
    backward passes, on the TN route (1040 tokens) and on the tap route (77)."""
import ctypes
import os
from ctypes import c_int64, c_size_t
from functools import lru_cache
from types import SimpleNamespace

import pytest
import torch

import bf16_routes as M
import gemm_bf16_ref_cpu as R
from guarded_arena import SENTINEL, Arena

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC = -22, -28
NT, TN = 0, 1                         # SALUN_GEMM_BF16_NT / _TN
F64 = torch.float64
_id = lambda c: c.id


def L():
    from unlearn_saliency_amd import _lib
    return _lib.lib()


def stream():
    from unlearn_saliency_amd.streams import _stream
    return _stream()


WORST = {}


def log(line):
    print(line)
    d = os.environ.get("SALUN_MEASURED_DIR")      # where a recording run keeps its figures (profiles/ has the last ones)
    if d and os.path.isdir(d):
        with open(os.path.join(d, "gemm_bf16_bounds_measured.txt"), "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module", autouse=True)
def _worst_ratio_per_label():
    yield
    for label in sorted(WORST):
        log(f"worst fraction of the bound on {label}: {WORST[label]:.4f}")


def route(op, m, n, k, variant=0, ws_bytes=0):
    """salun_gemm_bf16_route -> (label, splits), None (SALUN_EINVAL) or M.ENOSPC"""
    buf, ns = ctypes.create_string_buffer(64), ctypes.c_int(-1)
    rc = L().salun_gemm_bf16_route(op, m, n, k, variant, ws_bytes, buf, 64, ctypes.byref(ns))
    assert rc in (0, EINVAL, ENOSPC), rc
    return None if rc == EINVAL else M.ENOSPC if rc == ENOSPC else (buf.value.decode(), ns.value)


def values(bits):
    """bf16 bits -> their values in float64"""
    return bits.view(torch.bfloat16).double()


def first_wrong(got64, want64, origin=""):
    if got64.shape != want64.shape:
        return f"shape {tuple(got64.shape)}, want {tuple(want64.shape)}"
    bad = (got64 != want64).nonzero()
    if len(bad) == 0:
        return "no element differs"
    i = tuple(int(v) for v in bad[0])
    return f"{len(bad)} wrong, first at {i}: got {float(got64[i])!r}, want {float(want64[i])!r}{origin}"


def same16(got_bits, want64):
    """Bit for bit the float64 answer rounded ONCE to bf16, nearest even (+0 and -0 alike) -> (ok, what is wrong)"""
    want = R.to_bf16_rne(want64)
    assert torch.equal(want.float().bfloat16().double(), want), "the expected answer is not a bf16 number"
    got = values(got_bits)
    ok = got.shape == want.shape and torch.equal(got, want)
    return ok, (None if ok else first_wrong(got, want))


def same32(got, want64):
    """Bit for bit a float64 answer that fp32 holds exactly (+0 and -0 alike)"""
    assert torch.equal(want64.float().double(), want64), "the expected answer is not an fp32 number"
    ok = got.shape == want64.shape and torch.equal(got.double(), want64)
    return ok, (None if ok else first_wrong(got.double(), want64))


def untouched(a, after, *names):
    return all(bool((after[a.parts[n][0]:a.parts[n][0] + a.parts[n][1]] == SENTINEL).all()) for n in names if n in a.parts)


# ------------------------------------------------------------------------------------------ the calls
def call_nt(M_, N, K, variant, x, w, bias=None, addend=None, skew=()):
    """-> (rc, arena).  skew: names of the parts that lie 4 bytes off a 16-byte boundary"""
    sk = lambda name: int(name in skew)
    a = Arena().put("x", x, dtype="bf16", skew=sk("x")).put("w", w, dtype="bf16", skew=sk("w"))
    if bias is not None:
        a.put("bias", bias, skew=sk("bias"))
    if addend is not None:
        a.put("addend", addend, dtype="bf16", skew=sk("addend"))
    a.put("y", shape=(max(M_, 1), N), out=True, dtype="bf16", skew=sk("y")).upload()

    def run():
        return L().salun_gemm_bf16_nt(a.ptr("x"), a.ptr("w"), a.ptr("bias"), a.ptr("addend"), a.ptr("y"), c_int64(M_), N, K,
                                      variant, stream())
    a.run = run
    return run(), a


def call_tn(M_, Na, Nb, variant, dy, x, dw0=None, ws="queried", skew=()):
    """dw0: accumulate into it.  ws: "queried", "null" (NULL, 0 bytes), "null_sized" (NULL, the queried size), "short" (one
    byte short), "skew" (4 bytes off a 16-byte boundary) or "spare" (64 bytes where none are needed)"""
    need = L().salun_gemm_bf16_tn_workspace_bytes(c_int64(M_), Na, Nb, variant) if 0 <= variant <= 3 else 0
    a = Arena().put("dy", dy, dtype="bf16").put("x", x, dtype="bf16")
    a.put("dw", data=dw0, shape=(Na, Nb), out=True, skew=int("dw" in skew))
    if ws not in ("null", "null_sized") and (need or ws == "spare"):
        a.put("ws", shape=(max(need, 64) // 4,), out=True, skew=int(ws == "skew"))
    a.upload()
    stated = {"null": 0, "short": need - 1, "spare": 64}.get(ws, need)

    def run():
        return L().salun_gemm_bf16_tn(a.ptr("dy"), a.ptr("x"), a.ptr("dw"), c_int64(M_), Na, Nb, int(dw0 is not None), variant,
                                      a.ptr("ws"), c_size_t(stated), stream())
    a.run, a.need = run, need
    return run(), a


def nt_label(c):
    got = route(NT, c.M, c.N, c.K, c.variant)
    assert got == (c.label, 1) == M.gemm_nt(c.M, c.N, c.K, c.variant), (c.id, got)
    return got[0]


def tn_label(c):
    need = M.tn_workspace_bytes(c.M, c.Na, c.Nb, c.variant)
    got = route(TN, c.M, c.Na, c.Nb, c.variant, need)
    assert got == (c.label, c.splits) == M.gemm_tn(c.M, c.Na, c.Nb, c.variant, need), (c.id, got)
    return got[0]


@lru_cache(maxsize=4)
def nt_model(c, kind):
    """-> (inputs, the product without epilogue terms, the same over absolute values for the Gaussian kind): once per case"""
    t = R.nt_inputs(c, kind)
    return t, R.nt_model(t.x, t.w), (R.nt_model(t.x, t.w, absolute=True) if kind == "gauss" else None)


@lru_cache(maxsize=4)
def tn_model(c, kind):
    t = R.tn_inputs(c, kind)
    return t, R.tn_model(t.dy, t.x), (R.tn_model(t.dy, t.x, absolute=True) if kind == "gauss" else None)


def epilogue(y, t, terms, absolute=False):
    """(y + bias) + addend, the terms named"""
    f = (lambda v: v.abs()) if absolute else (lambda v: v)
    if "bias" in terms:
        y = y + f(t.bias)
    if "addend" in terms:
        y = y + f(t.addend)
    return y


# ------------------------------------------------------------------------------------------ (a) exact tier
@pytest.mark.parametrize("c", R.NT_CASES, ids=_id)
def test_nt_equals_the_exact_answer_rounded_once(c):
    t, product, _ = nt_model(c, "int")
    for terms in ((R.BIG_EPILOGUE,) if c.big else R.NT_EPILOGUES):
        label = nt_label(c)
        rc, a = call_nt(c.M, c.N, c.K, c.variant, t.x, t.w, *R.pick(t, terms))
        assert rc == 0, (terms, label)
        y = a.result("y")
        ok, wrong = same16(y, epilogue(product, t, terms))
        assert ok, (c.id, c.why, label, terms, wrong)
        a.restore(y=None)
        assert a.run() == 0 and torch.equal(a.result("y"), y), (c.id, label, terms, "a second call")


def _accepting(m, n, k):
    return [v for v in range(1, 14) if M.gemm_nt(m, n, k, v) is not None]


@pytest.mark.parametrize("shape", R.AGREE, ids=lambda s: "x".join(map(str, s)))
def test_all_variants_that_accept_a_shape_give_the_same_bits(shape):
    m, n, k = shape
    c = R.Nt(m, n, k, 0, None, "agree")
    vs = _accepting(m, n, k)
    assert len(vs) >= 5
    for kind in ("int", "gauss"):
        t = R.nt_inputs(c, kind)
        exact = R.nt_model(t.x, t.w, t.bias, t.addend)
        first = None
        for v in vs:
            assert route(NT, m, n, k, v) == (M.NT_ARMS[v][0], 1)
            rc, a = call_nt(m, n, k, v, t.x, t.w, t.bias, t.addend)
            assert rc == 0, v
            y = a.result("y")
            if kind == "int":
                ok, wrong = same16(y, exact)
                assert ok, (v, wrong)
            first = y if first is None else first
            assert torch.equal(y, first), (kind, v, first_wrong(values(y), values(first)))


@pytest.mark.parametrize("c", R.TN_CASES, ids=_id)
def test_tn_equals_the_exact_answer(c):
    t, dw, _ = tn_model(c, "int")
    for accumulate in (False, True):
        want = dw + t.dw0 if accumulate else dw
        bits = []
        for ws in (("queried",) if c.splits > 1 else ("null", "spare")):
            label = tn_label(c)
            rc, a = call_tn(c.M, c.Na, c.Nb, c.variant, t.dy, t.x, t.dw0 if accumulate else None, ws)
            assert (a.need > 0) == (c.splits > 1)
            assert rc == 0, (accumulate, ws, label)
            after = a.download()
            got = a.part(after, "dw")
            ok, wrong = same32(got, want)
            assert ok, (c.id, c.why, label, accumulate, ws, wrong)
            if ws == "spare":
                assert untouched(a, after, "ws")
            a.restore(dw=t.dw0 if accumulate else None)
            assert a.run() == 0 and torch.equal(a.result("dw").view(torch.int32), got.view(torch.int32)), "a second call"
            bits.append(got)
        assert all(torch.equal(b, bits[0]) for b in bits)


# ------------------------------------------------------------------------------------------ (b) impulses
@pytest.mark.parametrize("c", R.NT_IMPULSE, ids=_id)
def test_nt_impulses_give_the_weight_column_where_it_belongs(c):
    addend = R.nt_inputs(c, "int").addend
    label = nt_label(c)
    for row, k in R.nt_impulse_points(c):
        x, w, want = R.nt_impulse(c, row, k)
        origin = f" (impulse at row {row}, k {k}; {label})"
        rc, a = call_nt(c.M, c.N, c.K, c.variant, x, w)
        got = a.result("y")
        assert rc == 0 and torch.equal(values(got), want), first_wrong(values(got), want, origin)
        assert int((values(got) != 0).sum()) == c.N                      # exact zeros everywhere else
        rc, a = call_nt(c.M, c.N, c.K, c.variant, x, w, None, addend)
        ok, wrong = same16(a.result("y"), want + addend)
        assert rc == 0 and ok, (wrong, origin)


@pytest.mark.parametrize("c", R.TN_IMPULSE, ids=_id)
def test_tn_impulses_give_the_token_row_where_it_belongs(c):
    dw0 = R.tn_inputs(c, "int").dw0
    label = tn_label(c)
    for m, col in R.tn_impulse_points(c):
        dy, x, want = R.tn_impulse(c, m, col)
        origin = f" (impulse at token {m}, feature {col}; {label})"
        rc, a = call_tn(c.M, c.Na, c.Nb, c.variant, dy, x)
        got = a.result("dw").double()
        assert rc == 0 and torch.equal(got, want), first_wrong(got, want, origin)
        rc, a = call_tn(c.M, c.Na, c.Nb, c.variant, dy, x, dw0)        # one nonzero term joins dw0: one fp32 rounding
        got, acc = a.result("dw").double(), (want + dw0).float().double()
        assert rc == 0 and torch.equal(got, acc), first_wrong(got, acc, origin)


# ------------------------------------------------------------------------------------------ (c) bound tier
def within_bound(tag, label, got, exact, abs_sum, n, e, bf16):
    """Every element inside the bound of the module docstring; the worst fraction of it is logged first."""
    err = (got - exact).abs()
    bound = R.bound_gamma(2 * n + e) * abs_sum
    if bf16:
        bound = R.U16 * exact.abs() + (1 + R.U16) * bound
    frac = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    worst = float(frac.max()) if frac.numel() else 0.0
    worst = float("inf") if worst != worst else worst
    WORST[label] = max(WORST.get(label, 0.0), worst)
    log(f"{tag} {label}: n = {n}, e = {e}, worst |got - exact| = {worst:.4f} of the bound")
    inside = err <= bound                      # False for a NaN: an element never written (the sentinel) is outside too
    bad = (~inside).nonzero()
    assert got.shape == exact.shape and bool(inside.all()), \
        (tag, label, f"{len(bad)} outside the bound, first at {tuple(int(v) for v in bad[0])}: got {float(got[tuple(bad[0])])!r}")


@pytest.mark.parametrize("c", R.NT_SMALL, ids=_id)
def test_nt_within_the_per_element_bound(c):
    t, product, product_abs = nt_model(c, "gauss")
    label = nt_label(c)
    for terms in ((), ("bias", "addend")):
        rc, a = call_nt(c.M, c.N, c.K, c.variant, t.x, t.w, *R.pick(t, terms))
        assert rc == 0, (label, terms)
        y = a.result("y")
        within_bound(f"nt {c.id}{' + terms' if terms else ''}", label, values(y), epilogue(product, t, terms),
                     epilogue(product_abs, t, terms, absolute=True), c.K, len(terms), True)
        a.restore(y=None)
        assert a.run() == 0 and torch.equal(a.result("y"), y), (label, terms, "a second call")


@pytest.mark.parametrize("c", R.TN_CASES, ids=_id)
def test_tn_within_the_per_element_bound(c):
    t, dw, dw_abs = tn_model(c, "gauss")
    label = tn_label(c)
    for accumulate in (False, True):
        rc, a = call_tn(c.M, c.Na, c.Nb, c.variant, t.dy, t.x, t.dw0 if accumulate else None)
        assert rc == 0, (label, accumulate)
        got = a.result("dw")
        within_bound(f"tn {c.id}{' accumulate' if accumulate else ''}", label, got.double(), dw + t.dw0 if accumulate else dw,
                     dw_abs + t.dw0.abs() if accumulate else dw_abs, c.M, c.splits + int(accumulate), False)
        a.restore(dw=t.dw0 if accumulate else None)
        assert a.run() == 0 and torch.equal(a.result("dw").view(torch.int32), got.view(torch.int32)), (label, accumulate, "a second call")


# ------------------------------------------------------------------------------------------ (d) refusals
def _ones(*shape):
    return torch.ones(shape, dtype=F64)


@pytest.mark.parametrize("shape", R.NT_REFUSED, ids=lambda s: "x".join(map(str, s)))
def test_nt_shapes_outside_the_domain_are_refused_and_nothing_is_written(shape):
    m, n, k, v = shape
    assert M.gemm_nt(m, n, k, v) is None and route(NT, m, n, k, v) is None
    rc, a = call_nt(m, n, k, v, _ones(max(m, 1), k), _ones(n, k), _ones(n), _ones(max(m, 1), n))
    assert rc == EINVAL and untouched(a, a.download(), "y")


@pytest.mark.parametrize("name", ["x", "w", "y", "bias", "addend"])
def test_an_nt_pointer_off_the_16_byte_grid_is_refused_and_nothing_is_written(name):
    c = R.Nt(77, 128, 64, 0, None, "unaligned")
    t = R.nt_inputs(c, "int")
    assert route(NT, c.M, c.N, c.K, 0) == ("nt_r<2,2,3,64>", 1)          # the shape itself is inside the domain
    rc, a = call_nt(c.M, c.N, c.K, 0, t.x, t.w, t.bias, t.addend, skew=(name,))
    assert a.ptr(name).value % 16 == 4
    assert rc == EINVAL and untouched(a, a.download(), "y")
    rc, a = call_nt(c.M, c.N, c.K, 0, t.x, t.w, t.bias, t.addend)        # and is served with aligned pointers
    assert rc == 0 and same16(a.result("y"), R.nt_model(t.x, t.w, t.bias, t.addend))[0]


@pytest.mark.parametrize("shape", R.TN_REFUSED, ids=lambda s: "x".join(map(str, s)))
def test_tn_shapes_outside_the_domain_are_refused_and_nothing_is_written(shape):
    m, na, nb, v = shape
    assert M.gemm_tn(m, na, nb, v, 1 << 30) is None and route(TN, m, na, nb, v, 1 << 30) is None
    rc, a = call_tn(m, na, nb, v, _ones(max(m, 1), na), _ones(max(m, 1), nb), None, "spare")
    assert rc == EINVAL and untouched(a, a.download(), "dw", "ws")


@pytest.mark.parametrize("ws", ["short", "null", "null_sized", "skew"])
def test_a_tn_workspace_that_is_short_missing_or_unaligned_is_enospc_and_nothing_is_written(ws):
    m, na, nb, v = R.TN_SHORT_WS
    c = next(c for c in R.TN_CASES if (c.M, c.Na, c.Nb, c.variant) == R.TN_SHORT_WS)
    need = M.tn_workspace_bytes(m, na, nb, v)
    assert need > 0 and route(TN, m, na, nb, v, need - 1) == M.ENOSPC == M.gemm_tn(m, na, nb, v, need - 1)
    assert route(TN, m, na, nb, v, 0) == M.ENOSPC == M.gemm_tn(m, na, nb, v, 0)
    t = tn_model(c, "int")[0]
    rc, a = call_tn(m, na, nb, v, t.dy, t.x, None, ws)
    assert ws != "skew" or a.ptr("ws").value % 16 == 4
    assert rc == ENOSPC and untouched(a, a.download(), "dw", "ws")


def test_a_tn_gradient_off_the_16_byte_grid_is_refused_and_nothing_is_written():
    c = next(c for c in R.TN_CASES if (c.M, c.Na, c.Nb, c.variant) == R.TN_SHORT_WS)
    t = tn_model(c, "int")[0]
    rc, a = call_tn(c.M, c.Na, c.Nb, c.variant, t.dy, t.x, None, skew=("dw",))
    assert rc == EINVAL and untouched(a, a.download(), "dw", "ws")


# ------------------------------------------------------------------------------------------ (e) salun_pack_bf16
def call_pack(w, transposed):
    N, K = w.shape
    a = Arena().put("w", w).put("wp", shape=(K, N) if transposed else (N, K), out=True, dtype="bf16").upload()
    return L().salun_pack_bf16(a.ptr("w"), a.ptr("wp"), N, K, int(transposed), stream()), a


def bits16(t64):
    return t64.float().bfloat16().view(torch.int16)


@pytest.mark.parametrize("shape", R.PACK_PLAIN, ids=lambda s: "x".join(map(str, s)))
def test_pack_rounds_to_nearest_even_and_writes_only_its_output(shape):
    w = R.pack_inputs(*shape, seed=shape[0] * 1000 + shape[1])
    rc, a = call_pack(w, False)
    got = a.result("wp")
    assert rc == 0 and torch.equal(got, bits16(R.pack_model(w))), first_wrong(values(got), R.pack_model(w))   # bits: -0 is not +0


@pytest.mark.parametrize("shape", R.PACK_T, ids=lambda s: "x".join(map(str, s)))
def test_pack_transposed_rounds_to_nearest_even_and_writes_only_its_output(shape):
    w = R.pack_inputs(*shape, seed=shape[0] * 1000 + shape[1] + 1)
    rc, a = call_pack(w, True)
    got = a.result("wp")
    assert rc == 0 and torch.equal(got, bits16(R.pack_model(w, True))), first_wrong(values(got), R.pack_model(w, True))


def test_pack_special_values_one_by_one():
    v, want = R.pack_specials()
    n = (len(v) + 3) // 4 * 4 + 1                                        # the last special value sits in the scalar tail
    w = torch.zeros(n, dtype=F64)
    w[-len(v):] = v
    rc, a = call_pack(w.view(1, n), False)
    got = a.result("wp").view(-1)[-len(v):]
    assert rc == 0
    for i in range(len(v)):
        assert int(got[i]) == int(bits16(want)[i]), (float(v[i]), float(values(got)[i]), float(want[i]))


# ------------------------------------------------------------------------------------------ (f) SalunLinearBF16
LINEAR = [((2, 520), "wgrad_tn<v2>"), ((1, 77), "wgrad_tap<1,1>")]


def _conv_route(direction, shape, ws):
    buf, ns = ctypes.create_string_buffer(64), ctypes.c_int(-1)
    assert L().salun_conv2d_bf16_route(direction, *shape, 0, ws, buf, 64, ctypes.byref(ns)) == 0
    return buf.value.decode(), ns.value


@pytest.mark.parametrize("tier", ["exact", "bound"])
@pytest.mark.parametrize("lead,wgrad", LINEAR, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_linear_bf16_on_the_model(lead, wgrad, tier):
    from unlearn_saliency_amd import conv_bf16
    from unlearn_saliency_amd.flat import arena_of
    C, K = 64, 128
    tokens = lead[0] * lead[1]
    ex = tier == "exact"
    # the routes the layer takes: forward and input gradient on K16, the weight gradient as a 1x1 convolution over the tokens
    assert route(NT, tokens, K, C, 0) == ("nt_r<2,2,3,64>", 1) and route(NT, tokens, C, K, 0) == ("nt_r<4,1,3,32>", 1)
    shape = (1, tokens // 8, 8, C, K, 1, 1, 0) if tokens % 8 == 0 else (1, tokens, 1, C, K, 1, 1, 0)
    wlabel, splits = _conv_route(2, shape, L().salun_conv2d_bf16_wgrad_workspace_bytes(*shape))
    assert wlabel.startswith(wgrad), wlabel
    g = torch.Generator().manual_seed(tokens + 7 * ex)
    if ex:
        mk = lambda *s: torch.randint(-8, 9, s, generator=g).to(F64)
    else:
        mk = lambda *s: torch.randn(s, generator=g).bfloat16().to(F64)
    x, w, dy = mk(*lead, C) * 0.5, mk(K, C) * 2.0, mk(*lead, K)      # one power of two per tensor
    b = (torch.randint(1024, 4097, (K,), generator=g).to(F64) if ex else torch.randn((K,), generator=g).to(F64))
    res = (torch.randint(-255, 256, (*lead, K), generator=g).to(F64) * 4 if ex else mk(*lead, K))
    lin = torch.nn.Linear(C, K).cuda()
    with torch.no_grad():
        lin.weight.copy_(w.float().cuda()), lin.bias.copy_(b.float().cuda())
    lin.__class__ = conv_bf16.SalunLinearBF16
    arena = arena_of(lin)
    assert lin.bias.data_ptr() % 16 == 0 and conv_bf16._USE_K16[0]
    xd = x.float().cuda().bfloat16().requires_grad_(True)
    for _ in range(2):
        y = lin(xd, addend=res.float().cuda().bfloat16())
        y.backward(dy.float().cuda().bfloat16())
    torch.cuda.synchronize()
    assert lin.weight.grad.data_ptr() == arena.grads.data_ptr()
    x2, dy2 = x.view(tokens, C), dy.view(tokens, K)
    m = SimpleNamespace(y=R.nt_model(x2, w, b, res.view(tokens, K)), dx=R.nt_model(dy2, w.t().contiguous()), dw=R.tn_model(dy2, x2),
                        db=dy2.sum(0))
    got_y, got_dx = y.detach().cpu().double().view(tokens, K), xd.grad.cpu().double().view(tokens, C)
    got_dw, got_db = lin.weight.grad.cpu().double(), lin.bias.grad.cpu().double()
    tag = f"linear {tokens} tokens"
    if ex:
        for name, got, want in (("y", got_y, R.to_bf16_rne(m.y)), ("dx", got_dx, 2 * R.to_bf16_rne(m.dx)),
                                ("dW", got_dw, 2 * m.dw), ("db", got_db, 2 * m.db)):
            assert torch.equal(got, want), (tag, name, first_wrong(got, want))
        assert bool(R.is_bf16_tie(m.y).any()) and bool((R.to_bf16_rne(m.dx) != m.dx).any())
        return
    ya = R.nt_model(x2, w, b, res.view(tokens, K), absolute=True)
    within_bound(f"{tag} y", "linear y", got_y, m.y, ya, C, 2, True)
    # autograd adds the two passes' dx in bf16: the same bits twice, an exact doubling
    within_bound(f"{tag} dx", "linear dx", got_dx / 2, m.dx, R.nt_model(dy2, w.t().contiguous(), absolute=True), K, 0, True)
    # the sink accumulates: the second pass adds its product to the first one's, which carries the first one's error
    for name, got, exact, mag, e in (("dW", got_dw, m.dw, R.tn_model(dy2, x2, absolute=True), splits + 1),
                                     ("db", got_db, m.db, dy2.abs().sum(0), 1)):
        gam = R.bound_gamma(2 * tokens + e)
        b1 = gam * mag
        b2 = gam * (mag + exact.abs() + b1) + b1
        err = (got - 2 * exact).abs()
        worst = float((err / b2.clamp_min(1e-300)).max())
        WORST["linear " + name] = max(WORST.get("linear " + name, 0.0), worst)
        log(f"{tag} {name} {wlabel}: n = {tokens}, e = {e}, two passes, worst |got - exact| = {worst:.4f} of the bound")
        assert bool((err <= b2).all()), (tag, name)
