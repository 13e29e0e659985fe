"""K14 (csrc/salun_tok_bf16.hip: LayerNorm and GEGLU on bf16 tokens, forward and backward) against the float64 model of
tok_bf16_ref_cpu.py (validated by test_tok_bf16_ref_cpu.py), through the C-ABI, on every case of LN_CASES / GEGLU_CASES:

(a) exact tier: inputs whose statistics, outputs and backward sums are exact in fp32 in every summation order (the
    premise is asserted in test_tok_bf16_ref_cpu.py), so y, mean, dx, dgamma, dbeta, out and both halves of dh must EQUAL
    the float64 answer (rounded once to bf16 where the kernel rounds); rstd within the rsqrtf constant, its deviation in
    ulps logged.  stats = NULL gives the same y.  The backward is handed the MODEL's statistics, not the forward's.
    accumulate = 1 adds onto integer pre-fills exactly, in dgamma AND dbeta; accumulate = 0 overwrites NaN.  One case per
    label group runs in a guarded arena (guarded_arena.py): nothing outside the outputs changes and no element of an
    output or of the workspace keeps the sentinel, the partial rows of the empty workgroups of (65541, 8) included.
(b) bound tier: Gaussian inputs; every element of every output within the bound derived in tok_bf16_ref_cpu's docstring.
    The worst |got - exact| / bound is printed and logged (SALUN_MEASURED_DIR; profiles/tok_bf16_bounds_measured.txt has
    the last recording): recorded, the bound is what is asserted.  The backward runs twice: on the model's statistics
    (rounded to fp32) and on those the forward wrote; the model is evaluated on what the kernel was handed.
(c) the GELU tail: the elements with b in [-6, -3] as a line of their own, against the same per-element bound.
(d) invariances, bit for bit: a permutation of the rows; a row alone and inside (193, 1280).
(e) degenerate rows: a constant row, a row of zeros, a row holding inf or NaN beside untouched neighbours.
(f) the edges of the domain: every refusal is a host-side return code before any launch (outputs stay sentinels); through
    ops a transposed view, the two dispatch conditions of SD/unet.py, and gradients preset in weight.grad and bias.grad."""
import os
from ctypes import c_double, c_int64, c_size_t, c_void_p
from unittest import mock

import pytest
import torch

import tok_bf16_ref_cpu as R
from guarded_arena import SENTINEL, Arena

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC = -22, -28
BF = torch.bfloat16
F64 = torch.float64
_id = R._cid


def L():
    from unlearn_saliency_amd import _lib
    return _lib.lib()


def stream():
    from unlearn_saliency_amd.streams import _stream
    return _stream()


def ops():
    from unlearn_saliency_amd import ops as o
    return o


def log(line):
    print(line)
    d = os.environ.get("SALUN_MEASURED_DIR")      # where a recording run keeps its figures (profiles/ has the last ones)
    if d and os.path.isdir(d):
        with open(os.path.join(d, "tok_bf16_bounds_measured.txt"), "a") as f:
            f.write(line + "\n")


WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _worst_ratio_per_output():
    yield
    for label in sorted(WORST):
        log(f"worst over all cases, {label}: {WORST[label]:.4f}")
    log(f"assumed, not taken from the HIP math API reference: erff within {R.ERF_ULP / 2:g} ulp (ERF_ULP = {R.ERF_ULP:g} u), "
        f"rsqrtf within {R.RSQRT_ULP / 2:g} ulp (RSQRT_ULP = {R.RSQRT_ULP:g} u)")


def d16(t):
    """A float64 tensor of bf16 numbers on the device, as bf16."""
    assert torch.equal(R.bf16_round(t), t), "not a bf16 number"
    return t.to(BF).cuda().contiguous()


def d32(t):
    assert R.is_f32(t[torch.isfinite(t)]), "not an fp32 number"
    return t.float().cuda().contiguous()


def host(t):
    return t.detach().cpu().double()


def p(t):
    return c_void_p(None if t is None else t.data_ptr())


def same(got, want64, what=""):
    """Bit for bit the float64 answer, which the output's format holds exactly (+0 and -0 alike); nothing non-finite."""
    g = host(got).reshape(want64.shape)
    fmt = (lambda t: t.to(got.dtype).double())
    assert torch.equal(fmt(want64), want64), what + ": the expected answer is not a number of the output's format"
    bad = (g != want64) | ~torch.isfinite(g)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.numel()} wrong, first at {i}: got {float(g[i])!r}, want {float(want64[i])!r}")


def ulps_off(got, want64):
    """The largest |got - want| in fp32 ulps of want."""
    ulp = 2.0 ** (torch.floor(torch.log2(want64.abs().clamp_min(2.0 ** -126))) - 23)
    return float(((host(got).reshape(want64.shape) - want64).abs() / ulp).max())


def within(tag, got, exact, bound, label=None, mask=None):
    """Every element within its bound; the measured ratio is logged first."""
    g = host(got).reshape(exact.shape)
    if mask is not None:
        g, exact, bound = g[mask], exact[mask], bound[mask]
    err = (g - exact).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    worst = float(ratio.max()) if ratio.numel() else 0.0
    log(f"{tag}: worst |got - exact| / bound = {worst:.4f} over {ratio.numel()} elements")
    if label:
        WORST[label] = max(WORST.get(label, 0.0), worst)
    assert bool(torch.isfinite(g).all()), tag + ": non-finite"
    assert bool((err <= bound).all()), f"{tag}: {int((err > bound).sum())} elements outside the bound, worst ratio {worst:.4f}"
    return worst


# ------------------------------------------------------------------------------------------ the calls
def ln_forward(x, gamma, beta, eps, stats=True):
    rows, C = x.shape
    y = torch.full_like(x, float("nan"))
    st = torch.full((rows, 2), float("nan"), device="cuda") if stats else None
    rc = L().salun_ln_bf16_forward(p(x), p(gamma), p(beta), p(y), p(st), c_int64(rows), C, c_double(eps), stream())
    assert rc == 0, rc
    return y, st


def ln_backward(dy, x, gamma, stats, acc=None):
    """acc: (dgamma0, dbeta0) on the device, added onto (accumulate = 1); None: NaN pre-fills, overwritten."""
    rows, C = x.shape
    need = L().salun_ln_bf16_workspace_bytes(c_int64(rows), C)
    assert need == R.ln_ws_bytes(rows, C)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dx = torch.full_like(x, float("nan"))
    dg, db = acc if acc is not None else (torch.full((C,), float("nan"), device="cuda") for _ in range(2))
    rc = L().salun_ln_bf16_backward(p(dy), p(x), p(gamma), p(stats), p(dx), p(dg), p(db), c_int64(rows), C,
                                    int(acc is not None), p(ws), c_size_t(need), stream())
    assert rc == 0, rc
    return dx, dg, db


def geglu_forward(h):
    rows, F2 = h.shape
    out = torch.full((rows, F2 // 2), float("nan"), dtype=BF, device="cuda")
    assert L().salun_geglu_bf16_forward(p(h), p(out), c_int64(rows), F2 // 2, stream()) == 0
    return out


def geglu_backward(h, dy):
    rows, F2 = h.shape
    dh = torch.full_like(h, float("nan"))
    assert L().salun_geglu_bf16_backward(p(h), p(dy), p(dh), c_int64(rows), F2 // 2, stream()) == 0
    return dh


# ------------------------------------------------------------------------------------------ (a) exact tier
@pytest.mark.parametrize("family", R.ln_families())
@pytest.mark.parametrize("c", R.LN_CASES, ids=_id)
def test_layer_norm_equals_the_exact_answer(c, family):
    t = R.ln_exact_inputs(c, family)
    m = R.ln16_forward(t.x, t.gamma, t.beta, t.eps)
    x, g, b = d16(t.x), d32(t.gamma), d32(t.beta)
    tag = f"ln {_id(c)} {family}"
    y, st = ln_forward(x, g, b, t.eps)
    same(y, m.y, tag + " y")
    same(st[:, 0], m.mean, tag + " mean")
    off = ulps_off(st[:, 1], m.rstd)
    log(f"{tag}: rstd off the exact answer by {off:g} ulp at most (expected 0, the constant allows {R.RSQRT_ULP / 2:g})")
    WORST["exact tier, rstd deviation in ulp"] = max(WORST.get("exact tier, rstd deviation in ulp", 0.0), off)
    assert off <= R.RSQRT_ULP / 2 and bool(torch.isfinite(st).all()), tag
    y0, _ = ln_forward(x, g, b, t.eps, stats=False)
    assert torch.equal(y0.view(torch.int16), y.view(torch.int16)), tag + ": stats = NULL changes y"
    stats = d32(m.stats)                       # the model's statistics, not the forward's
    for name, dy in (("general", t.dy), ("vanishing", R.ln_vanishing_dy(t.x, t.gamma, m.mean, m.rstd))):
        for accumulate in (False, True):
            k = R.ln16_backward(dy, t.x, t.gamma, m.mean, m.rstd, *((t.gacc, t.bacc) if accumulate else (None, None)))
            dx, dg, db = ln_backward(d16(dy), x, g, stats, (d32(t.gacc), d32(t.bacc)) if accumulate else None)
            what = f"{tag} {name} accumulate={int(accumulate)}"
            same(dg, k.dgamma, what + " dgamma")
            same(db, k.dbeta, what + " dbeta")
            if R.ln_exact_dx(c, name == "vanishing"):
                same(dx, k.dx, what + " dx")
            elif not accumulate:
                bd = R.ln16_backward_bound(dy, t.x, t.gamma, m.mean, m.rstd)
                within(what + " dx (exact inputs, C no power of two)", dx, k.dx64, bd.dx)


@pytest.mark.parametrize("c", R.GEGLU_CASES, ids=_id)
def test_geglu_equals_the_exact_answer(c):
    t = R.geglu_exact_inputs(c)
    m, k = R.geglu16_forward(t.h), R.geglu16_backward(t.h, t.dy)
    h = d16(t.h)
    same(geglu_forward(h), m.out, f"geglu {_id(c)} out")
    dh = geglu_backward(h, d16(t.dy))
    same(dh[:, :c.F], k.dh[:, :c.F], f"geglu {_id(c)} dh[:, :F]")
    same(dh[:, c.F:], k.dh[:, c.F:], f"geglu {_id(c)} dh[:, F:]")


def no_sentinel(bits):
    """No 32-bit word, and no 16-bit half of one, still holds the sentinel pattern."""
    if bits.dtype == torch.int16:
        lo, hi = SENTINEL & 0xFFFF, SENTINEL >> 16
        return not bool(((bits == lo - 65536) | (bits == hi)).any())
    return not bool((bits.view(torch.int32) == SENTINEL).any())


@pytest.mark.parametrize("c", R.LN_ARENA, ids=_id)
def test_layer_norm_in_a_guarded_arena_writes_its_outputs_and_nothing_else(c):
    rows, C = c[:2]
    t = R.ln_exact_inputs(c, "eps0")
    m = R.ln16_forward(t.x, t.gamma, t.beta, t.eps)
    dy = R.ln_vanishing_dy(t.x, t.gamma, m.mean, m.rstd)
    k = R.ln16_backward(dy, t.x, t.gamma, m.mean, m.rstd)
    parts, need = R.ln_parts(rows), R.ln_ws_bytes(rows, C)
    assert L().salun_ln_bf16_workspace_bytes(c_int64(rows), C) == need
    a = Arena().put("x", t.x, dtype="bf16").put("dy", dy, dtype="bf16").put("gamma", t.gamma).put("beta", t.beta)
    a.put("stats_in", m.stats)
    a.put("y", shape=(rows, C), out=True, dtype="bf16").put("stats", shape=(rows, 2), out=True)
    a.put("dx", shape=(rows, C), out=True, dtype="bf16").put("dgamma", shape=(C,), out=True).put("dbeta", shape=(C,), out=True)
    a.put("ws", shape=(parts, C, 2), out=True).upload()
    q = a.ptr
    assert L().salun_ln_bf16_forward(q("x"), q("gamma"), q("beta"), q("y"), q("stats"), c_int64(rows), C, c_double(t.eps),
                                     stream()) == 0
    assert L().salun_ln_bf16_backward(q("dy"), q("x"), q("gamma"), q("stats_in"), q("dx"), q("dgamma"), q("dbeta"),
                                      c_int64(rows), C, 0, q("ws"), c_size_t(need), stream()) == 0
    after = a.download()                       # asserts that no guard and no input changed
    for name in ("y", "stats", "dx", "dgamma", "dbeta", "ws"):
        assert no_sentinel(a.part(after, name)), name + " keeps a sentinel"
    same(a.part(after, "y").view(BF), m.y, "y")
    same(a.part(after, "dx").view(BF), k.dx, "dx")
    same(a.part(after, "stats")[:, 0], m.mean, "mean")
    assert ulps_off(a.part(after, "stats")[:, 1], m.rstd) <= R.RSQRT_ULP / 2
    same(a.part(after, "dgamma"), k.dgamma, "dgamma")
    same(a.part(after, "dbeta"), k.dbeta, "dbeta")
    ws = a.part(after, "ws").double()
    empty = R.empty_wgs(rows)
    assert not bool(ws[empty].any()), "an empty workgroup's partial row is not zero"
    same(ws[:, :, 0].sum(0).float(), k.dgamma, "the partials' sum")   # sums of exact fp32 partials, exact in float64
    same(ws[:, :, 1].sum(0).float(), k.dbeta, "the partials' sum")
    if c is R.LN_BIG:
        assert len(empty) == 15 and parts == 1024


@pytest.mark.parametrize("c", R.GEGLU_ARENA, ids=_id)
def test_geglu_in_a_guarded_arena_writes_its_outputs_and_nothing_else(c):
    rows, F = c[:2]
    t = R.geglu_exact_inputs(c)
    m, k = R.geglu16_forward(t.h), R.geglu16_backward(t.h, t.dy)
    a = Arena().put("h", t.h, dtype="bf16").put("dy", t.dy, dtype="bf16")
    a.put("out", shape=(rows, F), out=True, dtype="bf16").put("dh", shape=(rows, 2 * F), out=True, dtype="bf16").upload()
    q = a.ptr
    assert L().salun_geglu_bf16_forward(q("h"), q("out"), c_int64(rows), F, stream()) == 0
    assert L().salun_geglu_bf16_backward(q("h"), q("dy"), q("dh"), c_int64(rows), F, stream()) == 0
    after = a.download()
    assert no_sentinel(a.part(after, "out")) and no_sentinel(a.part(after, "dh"))
    same(a.part(after, "out").view(BF), m.out, "out")
    same(a.part(after, "dh").view(BF), k.dh, "dh")


# ------------------------------------------------------------------------------------------ (b) bound tier
def ln_bound_backward(tag, t, x, g, stats64):
    """The backward on the fp32 statistics `stats64` (float64 holding fp32 numbers): plain, then accumulating."""
    mean, rstd = stats64[:, 0], stats64[:, 1]
    st = d32(stats64)
    for acc in (None, (t.gacc, t.bacc)):
        k = R.ln16_backward(t.dy, t.x, t.gamma, mean, rstd, *(acc or (None, None)))
        bd = R.ln16_backward_bound(t.dy, t.x, t.gamma, mean, rstd, *(acc or (None, None)))
        dx, dg, db = ln_backward(d16(t.dy), x, g, st, None if acc is None else (d32(acc[0]), d32(acc[1])))
        s = tag + (" +=" if acc else "")
        if acc is None:
            within(s + " dx", dx, k.dx64, bd.dx, "ln dx")
        within(s + " dgamma", dg, k.dgamma, bd.dgamma, "ln dgamma" + (" +=" if acc else ""))
        within(s + " dbeta", db, k.dbeta, bd.dbeta, "ln dbeta" + (" +=" if acc else ""))


@pytest.mark.parametrize("offset", R.LN_OFFSETS)
@pytest.mark.parametrize("c", R.LN_CASES, ids=_id)
def test_layer_norm_within_the_per_element_bound(c, offset):
    t = R.ln_gauss_inputs(c, offset)
    tag = f"ln {_id(c)} mu/sigma={offset:g}"
    m = R.ln16_forward(t.x, t.gamma, t.beta, t.eps)
    bf = R.ln16_forward_bound(t.x, t.gamma, t.beta, t.eps)
    x, g = d16(t.x), d32(t.gamma)
    y, st = ln_forward(x, g, d32(t.beta), t.eps)
    within(tag + " y", y, m.y64, bf.y, "ln y")
    within(tag + " mean", st[:, 0], m.mean, bf.mean, "ln mean")
    within(tag + " rstd", st[:, 1], m.rstd, bf.rstd, "ln rstd")
    ln_bound_backward(tag + " on the model's stats", t, x, g, R.f32(m.stats))
    ln_bound_backward(tag + " on the forward's stats", t, x, g, host(st))


@pytest.mark.parametrize("shift", R.GEGLU_SHIFTS)
@pytest.mark.parametrize("c", R.GEGLU_CASES, ids=_id)
def test_geglu_within_the_per_element_bound_and_in_the_tail(c, shift):
    t = R.geglu_gauss_inputs(c, shift)
    tag = f"geglu {_id(c)} shift={shift:g}"
    F = c.F
    m, k = R.geglu16_forward(t.h), R.geglu16_backward(t.h, t.dy)
    bf, bb = R.geglu16_forward_bound(t.h), R.geglu16_backward_bound(t.h, t.dy)
    h = d16(t.h)
    out, dh = geglu_forward(h), geglu_backward(h, d16(t.dy))
    within(tag + " out", out, m.out64, bf.out, "geglu out")
    within(tag + " dh[:, :F]", dh[:, :F], k.dh64[:, :F], bb.dh[:, :F], "geglu dh[:, :F]")
    within(tag + " dh[:, F:]", dh[:, F:], k.dh64[:, F:], bb.dh[:, F:], "geglu dh[:, F:]")
    # (c) the tail b in [-6, -3], where 1 + erff cancels: a line of its own, the same per-element bound
    tail = R.in_tail(t.h)
    if c.rows * F >= 1 << 13 and shift:
        assert float(tail.double().mean()) > 0.5
    if bool(tail.any()):
        within(tag + " tail out", out, m.out64, bf.out, "geglu tail out", mask=tail)
        within(tag + " tail dh[:, :F]", dh[:, :F], k.dh64[:, :F], bb.dh[:, :F], "geglu tail dh[:, :F]", mask=tail)
        within(tag + " tail dh[:, F:]", dh[:, F:], k.dh64[:, F:], bb.dh[:, F:], "geglu tail dh[:, F:]", mask=tail)


# ------------------------------------------------------------------------------------------ (d) invariances, bit for bit
def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def test_permuting_the_rows_permutes_the_results():
    c = R.LnCase(67, 320, "")
    t = R.ln_gauss_inputs(c, 16.0)
    perm = torch.randperm(c.rows, generator=torch.Generator().manual_seed(3))
    x, dy, g, b = d16(t.x), d16(t.dy), d32(t.gamma), d32(t.beta)
    y, st = ln_forward(x, g, b, t.eps)
    dx, _, _ = ln_backward(dy, x, g, st)
    pc = perm.cuda()
    xp, dyp = x[pc].contiguous(), dy[pc].contiguous()
    yp, stp = ln_forward(xp, g, b, t.eps)
    dxp, _, _ = ln_backward(dyp, xp, g, stp)
    assert torch.equal(bits(yp), bits(y[pc])) and torch.equal(bits(stp), bits(st[pc])) and torch.equal(bits(dxp), bits(dx[pc]))
    assert not torch.equal(bits(yp), bits(y))
    c = R.GegluCase(7, 1280, "")
    t = R.geglu_gauss_inputs(c, -4.0)
    perm = torch.randperm(c.rows, generator=torch.Generator().manual_seed(4)).cuda()
    h, dy = d16(t.h), d16(t.dy)
    out, dh = geglu_forward(h), geglu_backward(h, dy)
    hp, dyp = h[perm].contiguous(), dy[perm].contiguous()
    assert torch.equal(bits(geglu_forward(hp)), bits(out[perm])) and torch.equal(bits(geglu_backward(hp, dyp)), bits(dh[perm]))


def test_a_row_alone_and_inside_193x1280_gives_the_same_bits():
    c = R.LnCase(193, 1280, "")
    assert c[:2] in [k[:2] for k in R.LN_CASES]
    t = R.ln_gauss_inputs(c)
    x, dy, g, b = d16(t.x), d16(t.dy), d32(t.gamma), d32(t.beta)
    y, st = ln_forward(x, g, b, t.eps)
    dx, _, _ = ln_backward(dy, x, g, st)
    for r in (0, 97, 146, 192):                 # 146: the last row of workgroup 2 (rows_per_wg = 49); 192: the last of all
        x1, dy1 = x[r:r + 1].clone(), dy[r:r + 1].clone()
        y1, st1 = ln_forward(x1, g, b, t.eps)
        dx1, _, _ = ln_backward(dy1, x1, g, st1)
        assert torch.equal(bits(y1), bits(y[r:r + 1])) and torch.equal(bits(st1), bits(st[r:r + 1])), r
        assert torch.equal(bits(dx1), bits(dx[r:r + 1])), r
    t = R.geglu_gauss_inputs(R.GegluCase(7, 1280, ""))
    h, dy = d16(t.h), d16(t.dy)
    out, dh = geglu_forward(h), geglu_backward(h, dy)
    for r in (0, 6):
        h1, dy1 = h[r:r + 1].clone(), dy[r:r + 1].clone()
        assert torch.equal(bits(geglu_forward(h1)), bits(out[r:r + 1])) and torch.equal(bits(geglu_backward(h1, dy1)), bits(dh[r:r + 1]))


# ------------------------------------------------------------------------------------------ (e) degenerate rows
def test_a_constant_row_and_a_row_of_zeros():
    c = R.LnCase(6, 512, "")                                          # C a power of two: the row's sum is exact
    t = R.ln_gauss_inputs(c)
    t.eps = 2.0 ** -16
    t.beta = R.bf16_round(t.beta)                                     # so that y = beta is a bf16 number
    t.x[0], t.x[1] = 3.0, 0.0
    m = R.ln16_forward(t.x, t.gamma, t.beta, t.eps)
    bf = R.ln16_forward_bound(t.x, t.gamma, t.beta, t.eps)
    assert float(m.rstd[0]) == float(m.rstd[1]) == 256.0 and torch.equal(m.y64[:2], t.beta.expand(2, -1))
    x, g = d16(t.x), d32(t.gamma)
    y, st = ln_forward(x, g, d32(t.beta), t.eps)
    same(y[:2], t.beta.expand(2, -1).contiguous(), "y = beta on the constant row and on the row of zeros")
    assert host(st)[:2, 0].tolist() == [3.0, 0.0] and ulps_off(st[:2, 1], m.rstd[:2]) <= R.RSQRT_ULP / 2
    within("ln degenerate y", y, m.y64, bf.y)
    within("ln degenerate rstd", st[:, 1], m.rstd, bf.rstd)
    sk = host(st)
    k = R.ln16_backward(t.dy, t.x, t.gamma, sk[:, 0], sk[:, 1])
    bd = R.ln16_backward_bound(t.dy, t.x, t.gamma, sk[:, 0], sk[:, 1])
    dx, dg, db = ln_backward(d16(t.dy), x, g, st)
    within("ln degenerate dx", dx, k.dx64, bd.dx)
    within("ln degenerate dgamma", dg, k.dgamma, bd.dgamma)
    within("ln degenerate dbeta", db, k.dbeta, bd.dbeta)


def test_a_row_holding_inf_or_nan_leaves_the_other_rows_alone():
    c = R.LnCase(6, 520, "")
    t = R.ln_gauss_inputs(c)
    g, b, dy = d32(t.gamma), d32(t.beta), d16(t.dy)
    x = d16(t.x)
    y, st = ln_forward(x, g, b, t.eps)
    dx, _, _ = ln_backward(dy, x, g, st)
    x2 = x.clone()
    x2[2, 519], x2[4, 0] = float("inf"), float("nan")
    y2, st2 = ln_forward(x2, g, b, t.eps)
    dx2, _, _ = ln_backward(dy, x2, g, st2)
    keep = [0, 1, 3, 5]
    assert torch.equal(bits(y2[keep]), bits(y[keep])) and torch.equal(bits(st2[keep]), bits(st[keep]))
    assert torch.equal(bits(dx2[keep]), bits(dx[keep]))
    assert not bool(torch.isfinite(y2[2].float()).any()) and not bool(torch.isfinite(y2[4].float()).any())
    t = R.geglu_gauss_inputs(R.GegluCase(5, 24, ""))
    h, dy = d16(t.h), d16(t.dy)
    out, dh = geglu_forward(h), geglu_backward(h, dy)
    h2 = h.clone()
    h2[1, 3], h2[3, 24 + 7] = float("inf"), float("nan")
    out2, dh2 = geglu_forward(h2), geglu_backward(h2, dy)
    keep = [0, 2, 4]
    assert torch.equal(bits(out2[keep]), bits(out[keep])) and torch.equal(bits(dh2[keep]), bits(dh[keep]))
    assert not bool(torch.isfinite(out2[1, 3].float())) and not bool(torch.isfinite(out2[3, 7].float()))


# ------------------------------------------------------------------------------------------ (f) the edges of the domain
def refusal_arena():
    """Buffers of (4, 2056): large enough for every shape the refusals name, every output a sentinel."""
    rows, C = 4, 2056
    z = torch.zeros(rows, C, dtype=F64)
    a = Arena().put("x", z + 1, dtype="bf16").put("dy", z + 1, dtype="bf16").put("gamma", z[0] + 1).put("beta", z[0])
    a.put("stats_in", torch.tensor([[0.0, 1.0]] * rows, dtype=F64)).put("h", z + 1, dtype="bf16")
    a.put("y", shape=(rows, C), out=True, dtype="bf16").put("stats", shape=(rows, 2), out=True)
    a.put("dx", shape=(rows, C), out=True, dtype="bf16").put("dgamma", shape=(C,), out=True).put("dbeta", shape=(C,), out=True)
    a.put("ws", shape=(C * 2,), out=True)
    return a.put("out", shape=(rows, C), out=True, dtype="bf16").put("dh", shape=(rows, C), out=True, dtype="bf16").upload()


OUTS = ("y", "stats", "dx", "dgamma", "dbeta", "ws", "out", "dh")


def untouched(a):
    after = a.download()
    return all(bool((after[a.parts[n][0]:a.parts[n][0] + a.parts[n][1]] == SENTINEL).all()) for n in OUTS)


def off2(ptr):
    return c_void_p(ptr.value + 2)


def test_layer_norm_refusals_are_return_codes_and_write_nothing():
    a = refusal_arena()
    q = a.ptr

    def fwd(rows=4, C=8, **over):
        v = {n: q(n) for n in ("x", "gamma", "beta", "y", "stats")}
        v.update(over)
        return L().salun_ln_bf16_forward(v["x"], v["gamma"], v["beta"], v["y"], v["stats"], c_int64(rows), C, c_double(1e-5), stream())

    def bwd(rows=4, C=8, ws_bytes=None, **over):
        v = {n: q(n) for n in ("dy", "x", "gamma", "stats_in", "dx", "dgamma", "dbeta", "ws")}
        v.update(over)
        need = R.ln_ws_bytes(rows, C) if ws_bytes is None else ws_bytes
        return L().salun_ln_bf16_backward(v["dy"], v["x"], v["gamma"], v["stats_in"], v["dx"], v["dgamma"], v["dbeta"],
                                          c_int64(rows), C, 0, v["ws"], c_size_t(need), stream())

    for C in R.LN_OUTSIDE_C:
        assert not R.ln_ok(4, C) and fwd(C=C) == EINVAL and bwd(C=C, ws_bytes=1 << 16) == EINVAL, C
        assert L().salun_ln_bf16_workspace_bytes(c_int64(4), C) == 0, C
    assert fwd(rows=0) == EINVAL and bwd(rows=0, ws_bytes=1 << 16) == EINVAL
    assert L().salun_ln_bf16_workspace_bytes(c_int64(0), 8) == 0 and L().salun_ln_bf16_workspace_bytes(c_int64(-1), 8) == 0
    for name in ("x", "y"):                                           # two bytes off the 16-byte grid
        assert fwd(**{name: off2(q(name))}) == EINVAL, name
    for name in ("x", "dy", "dx"):
        assert bwd(**{name: off2(q(name))}) == EINVAL, name
    for name in ("x", "gamma", "beta", "y"):                          # each required pointer null
        assert fwd(**{name: c_void_p(None)}) == EINVAL, name
    for name in ("dy", "x", "gamma", "stats_in", "dx", "dgamma", "dbeta", "ws"):
        assert bwd(**{name: c_void_p(None)}) == EINVAL, name
    need = R.ln_ws_bytes(4, 8)
    assert need == 64 and bwd(ws_bytes=need - 1) == ENOSPC and bwd(ws_bytes=0) == ENOSPC
    assert untouched(a)
    assert fwd() == 0 and bwd() == 0                                  # the same arena and pointers, inside the domain
    after = a.download()
    assert all(no_sentinel(a.part(after, n).reshape(-1)[:32 if n in ("y", "dx") else 8]) for n in ("y", "dx", "dgamma", "dbeta"))


def test_geglu_refusals_are_return_codes_and_write_nothing():
    a = refusal_arena()
    q = a.ptr

    def fwd(rows=4, F=8, **over):
        v = {"h": q("h"), "out": q("out")}
        v.update(over)
        return L().salun_geglu_bf16_forward(v["h"], v["out"], c_int64(rows), F, stream())

    def bwd(rows=4, F=8, **over):
        v = {"h": q("h"), "dy": q("dy"), "dh": q("dh")}
        v.update(over)
        return L().salun_geglu_bf16_backward(v["h"], v["dy"], v["dh"], c_int64(rows), F, stream())

    for F in R.GEGLU_OUTSIDE_F:
        assert not R.geglu_ok(4, F) and fwd(F=F) == EINVAL and bwd(F=F) == EINVAL, F
    assert fwd(rows=0) == EINVAL and bwd(rows=0) == EINVAL
    for name in ("h", "out"):
        assert fwd(**{name: off2(q(name))}) == EINVAL and fwd(**{name: c_void_p(None)}) == EINVAL, name
    for name in ("h", "dy", "dh"):
        assert bwd(**{name: off2(q(name))}) == EINVAL and bwd(**{name: c_void_p(None)}) == EINVAL, name
    assert untouched(a)
    assert fwd() == 0 and bwd() == 0
    after = a.download()
    assert no_sentinel(a.part(after, "out").reshape(-1)[:32]) and no_sentinel(a.part(after, "dh").reshape(-1)[:64])


def test_a_transposed_view_through_ops_gives_the_bits_of_its_contiguous_copy():
    t = R.ln_gauss_inputs(R.LnCase(24, 320, ""))
    ln = torch.nn.LayerNorm(320, eps=t.eps).cuda()
    with torch.no_grad():
        ln.weight.copy_(d32(t.gamma))
        ln.bias.copy_(d32(t.beta))
    base = d16(t.x.t().contiguous())                                  # [320, 24]: its transpose is x, not contiguous
    dy = d16(t.dy)
    res = []
    for x in (base.t(), base.t().contiguous()):
        assert x.shape == (24, 320)
        x = x.detach().requires_grad_(True)
        ln.weight.grad = ln.bias.grad = None
        y = ops().layer_norm_bf16(x, ln)
        y.backward(dy)
        res.append((y.detach(), x.grad, ln.weight.grad.clone(), ln.bias.grad.clone()))
    assert not base.t().is_contiguous() and all(torch.equal(bits(u), bits(v)) for u, v in zip(*res))
    m = R.ln16_forward(t.x, t.gamma, t.beta, t.eps)
    within("ln through ops, transposed view, y", res[0][0], m.y64, R.ln16_forward_bound(t.x, t.gamma, t.beta, t.eps).y)
    t = R.geglu_gauss_inputs(R.GegluCase(24, 40, ""))
    base, dy, res = d16(t.h.t().contiguous()), d16(t.dy), []
    for h in (base.t(), base.t().contiguous()):
        h = h.detach().requires_grad_(True)
        out = ops().geglu_bf16(h)
        out.backward(dy)
        res.append((out.detach(), h.grad))
    assert all(torch.equal(bits(u), bits(v)) for u, v in zip(*res))
    within("geglu through ops, transposed view, out", res[0][0], R.geglu16_forward(t.h).out64, R.geglu16_forward_bound(t.h).out)


def _spy(name):
    return mock.patch.object(ops(), name, wraps=getattr(ops(), name))


@pytest.mark.parametrize("C,k14", [(320, True), (2056, False), (12, False)])
def test_the_layer_norm_dispatch_of_the_transformer_block(C, k14):
    from unlearn_saliency_amd.SD.unet import BasicTransformerBlock
    t = R.ln_gauss_inputs(R.LnCase(10, C, ""))
    ln = torch.nn.LayerNorm(C, eps=t.eps).cuda()
    with torch.no_grad():
        ln.weight.copy_(d32(t.gamma))
        ln.bias.copy_(d32(t.beta))
    x = d16(t.x).view(2, 5, C)
    with _spy("layer_norm_bf16") as spy, torch.no_grad(), torch.autocast("cuda", dtype=BF):
        y = BasicTransformerBlock._ln(ln, x)
    assert spy.call_count == int(k14) and y.shape == x.shape
    m = R.ln16_forward(t.x, t.gamma, t.beta, t.eps)
    bd = R.ln16_forward_bound(t.x, t.gamma, t.beta, t.eps).y
    if k14:
        assert y.dtype == BF
    else:                                      # the library's path: the same bound plus one fp32 -> bf16 rounding
        bd = bd + R.U16 * (m.y64.abs() + bd)
    within(f"ln dispatch C={C} {'K14' if k14 else 'library'} y", y.reshape(10, C), m.y64, bd)


@pytest.mark.parametrize("F2,k14", [(640, True), (32, True), (24, False)])
def test_the_geglu_dispatch_of_the_feed_forward(F2, k14):
    from unlearn_saliency_amd.SD.unet import GEGLU
    Fh = F2 // 2
    t = R.geglu_gauss_inputs(R.GegluCase(10, Fh, ""), -4.0 if F2 == 640 else 0.0)
    mod = GEGLU(F2, Fh).cuda().to(BF)                                 # proj: the identity, so that h is the test's tensor
    with torch.no_grad():
        mod.proj.weight.copy_(torch.eye(F2))
        mod.proj.bias.zero_()
    h = d16(t.h).view(2, 5, F2)
    with _spy("geglu_bf16") as spy, torch.no_grad():
        assert torch.equal(mod.proj(h), h)
        out = mod(h)
    assert spy.call_count == int(k14) and out.shape == (2, 5, Fh) and out.dtype == BF
    m, bd = R.geglu16_forward(t.h), R.geglu16_forward_bound(t.h).out
    if not k14:
        bd = bd + R.U16 * (m.out64.abs() + bd)
    within(f"geglu dispatch 2F={F2} {'K14' if k14 else 'library'} out", out.reshape(10, Fh), m.out64, bd)


@pytest.mark.parametrize("family", R.ln_families())
def test_gradients_preset_in_weight_grad_and_bias_grad_accumulate_exactly(family):
    c = R.LnCase(67, 320, "")
    t = R.ln_exact_inputs(c, family)
    m = R.ln16_forward(t.x, t.gamma, t.beta, t.eps)
    dy = R.ln_vanishing_dy(t.x, t.gamma, m.mean, m.rstd)
    k = R.ln16_backward(dy, t.x, t.gamma, m.mean, m.rstd, t.gacc, t.bacc)
    ln = torch.nn.LayerNorm(c.C, eps=t.eps).cuda()
    with torch.no_grad():
        ln.weight.copy_(d32(t.gamma))
        ln.bias.copy_(d32(t.beta))
    ln.weight.grad, ln.bias.grad = d32(t.gacc), d32(t.bacc)
    x = d16(t.x).view(1, c.rows, c.C).requires_grad_(True)
    y = ops().layer_norm_bf16(x, ln)
    same(y, m.y.view(1, c.rows, c.C), "y")
    y.backward(d16(dy).view(1, c.rows, c.C))
    same(x.grad, k.dx.view(1, c.rows, c.C), "dx")
    same(ln.weight.grad, k.dgamma, "weight.grad")
    same(ln.bias.grad, k.dbeta, "bias.grad")
    assert float((k.dbeta - t.bacc).abs().max()) > 0 and float((k.dgamma - t.gacc).abs().max()) > 0
