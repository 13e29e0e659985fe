"""K11 (csrc/salun_conv_bf16.hip, and the ring / TN kernels of csrc/salun_gemm.hip it routes to) against the float64 model
of conv_bf16_ref_cpu.py (validated by test_conv_bf16_ref_cpu.py), on every route the plan can pick (bf16_routes.py;
conv_bf16_ref_cpu.CASES).  Before each call the test asks salun_conv2d_bf16_route and asserts the label the case claims.

(a) exact tier: small integers times powers of two.  Every fp32 partial sum is exact in every order (the cap asserted in
    test_conv_bf16_ref_cpu.py), so y and dx must EQUAL the model rounded once to bf16, nearest even (some sums are ties:
    the tier pins the rounding), and dw, db, dnb the model itself: forward with and without each epilogue term, with the
    queried workspace, NULL and one byte short; backward-data without, with and in place on its addend; backward-weight
    writing and accumulating, with and without db and dnb, and with dw one float off a 16-byte boundary.
(b) impulses: a single 1 at a corner, an edge and an interior pixel, first and last channel - the weight patch where it
    belongs and zero (or the addend) elsewhere; backward-weight gives the shifted dy.
(c) bound tier: Gaussian inputs with the same scales.  With n the element's reduction length, e its epilogue additions,
    u = 2^-24 and u16 = 2^-8 (8 significand bits; derived, not measured):
        bf16 outputs  |got - exact| <= u16 |exact| + (1 + u16) gamma_(2n+e) abs_sum
        fp32 outputs  |got - exact| <= gamma_(2n+e) abs_sum
    (2n: product and add rounded separately, so it holds fused or not, for every tree and split; no absolute slack, nothing
    scaled by a tensor's maximum).  The worst fraction of the bound seen per route is printed and logged
    (profiles/conv_bf16_bounds_measured.txt), not asserted.
(d) invariances, bit for bit: an image alone and inside a batch; a second call; with and without the split (exact tier).
(e) nothing else is written: every tensor of a call lies in ONE guarded allocation (guarded_arena.py) and everything but
    the outputs must hold the bits it was given, after every call here; a refused call leaves the outputs' sentinels too.
    A refusal is asserted only where the mirror puts the shape outside the domain, and never accepted otherwise.
(f) the ring forms on 3x3 shapes, in a child process started with SALUN_CONV_RING=3."""
import ctypes
import os
import subprocess
import sys
from ctypes import c_size_t
from functools import lru_cache
from types import SimpleNamespace

import pytest
import torch

import bf16_routes as M
import conv_bf16_ref_cpu as R
from guarded_arena import SENTINEL, Arena

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC = -22, -28
FWD, DGRAD, WGRAD = 0, 1, 2           # SALUN_ROUTE_FORWARD / _BACKWARD_DATA / _BACKWARD_WEIGHT
UNALIGNED = 8                         # SALUN_ROUTE_OUT_UNALIGNED
RING = int(os.environ.get("SALUN_CONV_RING", "1"))   # the switch this process was started with (the child of (f): 3)
_id = lambda c: c.id
IN_FWD = [c for c in R.CASES if c.fwd]
IN_DGRAD = [c for c in R.CASES if c.dgrad]
IN_WGRAD = [c for c in R.CASES if c.wgrad]
XSHAPE = lambda c: (c.N, c.H, c.W, c.C)
YSHAPE = lambda c: (c.N, c.OH, c.OW, c.K)


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
        with open(os.path.join(d, "conv_bf16_bounds_measured.txt"), "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module", autouse=True)
def _worst_ratio_per_route():
    yield
    for route in sorted(WORST):
        log(f"worst fraction of the bound on {route}: {WORST[route]:.4f}")


def route(direction, shape, flags=0, ws_bytes=0):
    """salun_conv2d_bf16_route -> (label, splits), None (SALUN_EINVAL) or M.ENOSPC"""
    buf, ns = ctypes.create_string_buffer(64), ctypes.c_int(-1)
    rc = L().salun_conv2d_bf16_route(direction, *shape, flags, ws_bytes, buf, 64, ctypes.byref(ns))
    assert rc in (0, EINVAL, ENOSPC), rc
    return None if rc == EINVAL else M.ENOSPC if rc == ENOSPC else (buf.value.decode(), ns.value)


def values(bits):
    """bf16 bits -> their values in float64"""
    return bits.view(torch.bfloat16).double()


def same16(got_bits, want64):
    """Bit for bit the float64 answer rounded ONCE to bf16, nearest even (+0 and -0 alike)."""
    want = R.to_bf16_rne(want64)
    assert torch.equal(want.float().bfloat16().double(), want), "the expected answer is not a bf16 number"
    return got_bits.shape == want.shape and torch.equal(values(got_bits), want)


def same32(got, want64):
    """Bit for bit a float64 answer that fp32 holds exactly (+0 and -0 alike)."""
    want = want64.float()
    assert torch.equal(want.double(), want64), "the expected answer is not an fp32 number"
    return got.shape == want.shape and torch.equal(got, want)


def untouched(a, after, *names):
    return all(bool((after[a.parts[n][0]:a.parts[n][0] + a.parts[n][1]] == SENTINEL).all()) for n in names if n in a.parts)


# ------------------------------------------------------------------------------------------ the calls
def call_forward(shape, t, terms=(), ws=("queried", None)):
    """-> (rc, arena).  terms: subset of bias / nbias / addend; ws: ("queried", _), ("null", _) or ("short", bytes stated)."""
    N, H, W, C, K, Rr, stride, pad = shape
    a = Arena().put("x", t.x, dtype="bf16").put("w", R.packed(t.w), dtype="bf16")
    for name in terms:
        a.put(name, getattr(t, name), dtype="bf16" if name == "addend" else "f32")
    a.put("y", shape=(max(N, 1), max(R.out_extent(H, Rr, stride, pad), 1), max(R.out_extent(W, Rr, stride, pad), 1), K),
          out=True, dtype="bf16")
    dws = L().salun_conv2d_bf16_data_workspace_bytes(*shape)
    if ws[0] != "null" and dws:
        a.put("ws", shape=(dws // 4,), out=True)
    a.upload()
    stated = ws[1] if ws[0] == "short" else dws          # a NULL workspace whatever size is stated
    rc = L().salun_conv2d_bf16_forward(a.ptr("x"), a.ptr("w"), a.ptr("bias"), a.ptr("nbias"), a.ptr("addend"), a.ptr("y"),
                                       *shape, a.ptr("ws"), c_size_t(stated), stream())
    return rc, a


def call_backward_data(shape, t, addend=None, ws=("queried", None)):
    """addend: None, "apart" or "inplace" (addend == dx)."""
    N, H, W, C, K, Rr, stride, pad = shape
    a = Arena().put("dy", t.dy, dtype="bf16").put("w", R.packed(t.w), dtype="bf16")
    if addend == "apart":
        a.put("addend", t.addend, dtype="bf16")
    a.put("dx", data=t.addend if addend == "inplace" else None, shape=(max(N, 1), max(H, 1), max(W, 1), C), out=True, dtype="bf16")
    dws = L().salun_conv2d_bf16_data_workspace_bytes(*shape)
    if ws[0] != "null" and dws:
        a.put("ws", shape=(dws // 4,), out=True)
    a.upload()
    stated = ws[1] if ws[0] == "short" else dws
    rc = L().salun_conv2d_bf16_backward_data(a.ptr("dy"), a.ptr("w"), a.ptr("dx" if addend == "inplace" else "addend"),
                                             a.ptr("dx"), *shape, a.ptr("ws"), c_size_t(stated), stream())
    return rc, a


def call_backward_weight(shape, t, accumulate=False, db=False, dnb=False, skew=0, short=0):
    """short: bytes the stated workspace size falls short of the queried one."""
    N, H, W, C, K, Rr, stride, pad = shape
    wsb = L().salun_conv2d_bf16_wgrad_workspace_bytes(*shape)
    a = Arena().put("x", t.x, dtype="bf16").put("dy", t.dy, dtype="bf16")
    a.put("dw", data=t.dw0 if accumulate else None, shape=(K, C, Rr, Rr), out=True, skew=skew)
    if db:
        a.put("db", data=t.db0 if accumulate else None, shape=(K,), out=True)
    if dnb:
        a.put("dnb", shape=(max(N, 1), K), out=True)
    a.put("ws", shape=(max(wsb, 16) // 4,), out=True).upload()
    rc = L().salun_conv2d_bf16_backward_weight_ex(a.ptr("x"), a.ptr("dy"), a.ptr("dw"), a.ptr("db"), a.ptr("dnb"), *shape,
                                                  int(accumulate), a.ptr("ws"), c_size_t(wsb - short), stream())
    return rc, a


def asked_route(c, direction, ws=("queried", None), aligned=True):
    """The route query's answer for the call about to be made, held to the mirror's and, for the queried workspace and
    aligned pointers, to the label the case claims."""
    if direction == "wgrad":
        wsb = M.wgrad_workspace_bytes(c.shape)
        got = route(WGRAD, c.shape, 0 if aligned else UNALIGNED, wsb)
        assert got == M.backward_weight(c.shape, wsb, aligned), (c.id, got)
        claim = c.wgrad
    else:
        asked = dict(R.data_ws_modes(c.shape, direction))[ws[0]]
        got = route(FWD if direction == "fwd" else DGRAD, c.shape, 0, asked)
        want = M.forward(c.shape, asked, True, RING) if direction == "fwd" else M.backward_data(c.shape, asked)
        assert got == want, (c.id, direction, ws, got)
        claim = c.fwd if direction == "fwd" else c.dgrad
        if ws[0] != "queried" and got[0].startswith("igemm"):
            assert got[0].endswith("/S1") and got[1] == 1, (c.id, direction, ws, got)   # only the split is gone
            assert got[0].split("/")[0] == claim.split("/")[0]
    if aligned and ws[0] == "queried":
        assert got[0] == claim, (c.id, direction, got)
    return got[0]


def epilogue(y, t, terms, absolute=False):
    """((y + bias[k]) + nbias[n][k]) + addend, the terms named"""
    f = (lambda v: v.abs()) if absolute else (lambda v: v)
    if "bias" in terms:
        y = y + f(t.bias)
    if "nbias" in terms:
        y = y + f(t.nbias)[:, None, None, :]
    if "addend" in terms:
        y = y + f(t.addend)
    return y


@lru_cache(maxsize=None)
def model(c, direction, kind):
    """-> (inputs, exact answer without epilogue terms, the same over absolute values for the Gaussian kind): once per case"""
    t = R.inputs(c, direction, kind)
    both = (False, True) if kind == "gauss" else (False,)
    if direction == "fwd":
        out = [R.forward(t.x, t.w, c.stride, c.pad, absolute=ab) for ab in both]
    elif direction == "dgrad":
        out = [R.backward_data(t.dy, t.w, XSHAPE(c), c.stride, c.pad, absolute=ab) for ab in both]
    else:
        out = [R.backward_weight(t.x, t.dy, c.R, c.stride, c.pad, absolute=ab) for ab in both]
    return (t, out[0], out[1] if kind == "gauss" else None)


# ------------------------------------------------------------------------------------------ (a) exact tier
def check_forward_exact(c):
    t, conv, _ = model(c, "fwd", "int")
    for terms in R.FWD_TERMS:
        bits = []
        for ws in R.data_ws_modes(c.shape, "fwd"):
            label = asked_route(c, "fwd", ws)
            rc, a = call_forward(c.shape, t, terms, ws)
            assert rc == 0, (terms, ws, label)
            y = a.result("y")
            assert same16(y, epilogue(conv, t, terms)), (terms, ws, label)
            bits.append(y)
        assert all(torch.equal(b, bits[0]) for b in bits), terms      # split or not: the same bits


@pytest.mark.parametrize("c", IN_FWD, ids=_id)
def test_forward_equals_the_exact_answer_rounded_once(c):
    check_forward_exact(c)


@pytest.mark.parametrize("c", IN_DGRAD, ids=_id)
def test_backward_data_equals_the_exact_answer_rounded_once(c):
    t, dx, _ = model(c, "dgrad", "int")
    for addend in R.DGRAD_ADDEND:
        bits = []
        for ws in R.data_ws_modes(c.shape, "dgrad"):
            label = asked_route(c, "dgrad", ws)
            rc, a = call_backward_data(c.shape, t, addend, ws)
            assert rc == 0, (addend, ws, label)
            got = a.result("dx")
            assert same16(got, dx + t.addend if addend else dx), (addend, ws, label)
            bits.append(got)
        assert all(torch.equal(b, bits[0]) for b in bits), addend


@pytest.mark.parametrize("c", IN_WGRAD, ids=_id)
def test_backward_weight_equals_the_exact_answer(c):
    t, (dw, db, dnb), _ = model(c, "wgrad", "int")
    for accumulate, with_db, with_dnb, unaligned in R.WGRAD_VARIANTS:
        if unaligned and c.K * c.C > 512 * 512:
            continue
        label = asked_route(c, "wgrad", aligned=not unaligned)
        assert not unaligned or label.startswith("wgrad_tap")
        rc, a = call_backward_weight(c.shape, t, accumulate, with_db, with_dnb, skew=int(unaligned))
        what = (accumulate, with_db, with_dnb, unaligned, label)
        assert rc == 0, what
        after = a.download()
        assert same32(a.part(after, "dw"), dw + t.dw0 if accumulate else dw), what
        if with_db:
            assert same32(a.part(after, "db"), db + t.db0 if accumulate else db), what
        if with_dnb:
            assert same32(a.part(after, "dnb"), dnb), what          # always overwritten


# ------------------------------------------------------------------------------------------ (b) impulses
# pad 1 with a ragged split, the 128 x 256 tile, pad 0 and 2, stride 2 at pad 1 / 0 / 2, 1x1 stride 2, the 1x1-pixel image,
# extents below the filter, the TN route
IMPULSE = [R.CASES[i] for i in (1, 3, 7, 8, 9, 10, 11, 12, 13, 14, 20)]


def _impulses(shape):
    """[(n, h, w, channel)] in the last image: a corner, an edge, an interior pixel x the first and the last channel"""
    N, H, W, C = shape
    return [(N - 1, h, w, ch) for h, w in R.impulse_points(H, W) for ch in (0, C - 1)]


def _one(shape, at):
    t = torch.zeros(shape, dtype=torch.float64)
    t[at] = 1.0
    return t


@pytest.mark.parametrize("c", IMPULSE, ids=_id)
def test_impulses_give_the_weight_patch_where_it_belongs(c):
    s, p, taps = c.stride, c.pad, [(r, q) for r in range(c.R) for q in range(c.R)]
    f = R.inputs(c, "fwd", "int")
    for n, h, w, ch in _impulses(XSHAPE(c)):
        want = torch.zeros(YSHAPE(c), dtype=torch.float64)
        for r, q in taps:                                   # output (oh, ow) reads x[oh s - p + r][ow s - p + q]
            a_, b_ = h + p - r, w + p - q
            if a_ % s == 0 and b_ % s == 0 and 0 <= a_ // s < c.OH and 0 <= b_ // s < c.OW:
                want[n, a_ // s, b_ // s, :] = f.w[:, ch, r, q]
        label = asked_route(c, "fwd")
        rc, a = call_forward(c.shape, SimpleNamespace(x=_one(XSHAPE(c), (n, h, w, ch)), w=f.w))
        assert rc == 0 and same16(a.result("y"), want), (label, h, w, ch)
    d = R.inputs(c, "dgrad", "int")
    for n, oh, ow, k in _impulses(YSHAPE(c)):
        want = d.addend.clone()                             # pixels no output reads: exactly the addend
        for r, q in taps:
            h, w = oh * s - p + r, ow * s - p + q
            if 0 <= h < c.H and 0 <= w < c.W:
                want[n, h, w, :] += d.w[k, :, r, q]
        t = SimpleNamespace(dy=_one(YSHAPE(c), (n, oh, ow, k)), w=d.w, addend=d.addend)
        label = asked_route(c, "dgrad")
        rc, a = call_backward_data(c.shape, t, "apart")
        assert rc == 0 and same16(a.result("dx"), want), (label, oh, ow, k)
        rc, a = call_backward_data(c.shape, t, None)
        got = a.result("dx")
        assert rc == 0 and same16(got, want - d.addend), (label, oh, ow, k)
        assert int((values(got) != 0).sum()) <= c.C * c.R * c.R     # exact zeros everywhere else
    g = R.inputs(c, "wgrad", "int")
    for n, h, w, ch in _impulses(XSHAPE(c)):
        want = torch.zeros((c.K, c.C, c.R, c.R), dtype=torch.float64)
        for r, q in taps:                                   # the shifted dy
            a_, b_ = h + p - r, w + p - q
            if a_ % s == 0 and b_ % s == 0 and 0 <= a_ // s < c.OH and 0 <= b_ // s < c.OW:
                want[:, ch, r, q] = g.dy[n, a_ // s, b_ // s, :]
        t = SimpleNamespace(x=_one(XSHAPE(c), (n, h, w, ch)), dy=g.dy, dw0=g.dw0, db0=g.db0)
        label = asked_route(c, "wgrad")
        rc, a = call_backward_weight(c.shape, t)
        assert rc == 0 and same32(a.result("dw"), want), (label, h, w, ch)


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
    assert bool((err <= bound).all()), (tag, label)


@pytest.mark.parametrize("c", IN_FWD, ids=_id)
def test_forward_within_the_per_element_bound(c):
    t, conv, conv_abs = model(c, "fwd", "gauss")
    full = ("bias", "nbias", "addend")
    for ws in R.data_ws_modes(c.shape, "fwd")[:2]:          # queried and NULL: split and not
        label = asked_route(c, "fwd", ws)
        for terms in ((), full):
            rc, a = call_forward(c.shape, t, terms, ws)
            assert rc == 0, (label, terms)
            y = a.result("y")
            within_bound(f"fwd {c.id}{' + terms' if terms else ''}", label, values(y), epilogue(conv, t, terms),
                         epilogue(conv_abs, t, terms, absolute=True), c.C * c.R * c.R, len(terms), True)
        rc, a = call_forward(c.shape, t, full, ws)          # a second call: the same bits
        assert rc == 0 and torch.equal(a.result("y"), y), label


@pytest.mark.parametrize("c", IN_DGRAD, ids=_id)
def test_backward_data_within_the_per_element_bound(c):
    t, dx, dx_abs = model(c, "dgrad", "gauss")
    for ws in R.data_ws_modes(c.shape, "dgrad")[:2]:
        label = asked_route(c, "dgrad", ws)
        for addend in (None, "apart"):
            rc, a = call_backward_data(c.shape, t, addend, ws)
            assert rc == 0, (label, addend)
            got = a.result("dx")
            within_bound(f"dgrad {c.id}{' + addend' if addend else ''}", label, values(got), dx + t.addend if addend else dx,
                         dx_abs + t.addend.abs() if addend else dx_abs, c.K * c.R * c.R, 1 if addend else 0, True)
        rc, a = call_backward_data(c.shape, t, "apart", ws)
        assert rc == 0 and torch.equal(a.result("dx"), got), label
        rc, a = call_backward_data(c.shape, t, "inplace", ws)
        assert rc == 0 and torch.equal(a.result("dx"), got), label       # in place on the addend: the same bits


@pytest.mark.parametrize("c", IN_WGRAD, ids=_id)
def test_backward_weight_within_the_per_element_bound(c):
    t, (dw, db, dnb), (dw_abs, db_abs, dnb_abs) = model(c, "wgrad", "gauss")
    n = c.N * c.OH * c.OW
    for unaligned in ((False, True) if c.K * c.C <= 512 * 512 else (False,)):
        label = asked_route(c, "wgrad", aligned=not unaligned)
        seen = {}
        for accumulate in (False, True):
            rc, a = call_backward_weight(c.shape, t, accumulate, True, True, skew=int(unaligned))
            assert rc == 0, (label, accumulate)
            after = a.download()
            seen[accumulate] = a.part(after, "dw")
            tag = f"{c.id}{' accumulate' if accumulate else ''}"
            within_bound("wgrad dw " + tag, label, a.part(after, "dw").double(), dw + t.dw0 if accumulate else dw,
                         dw_abs + t.dw0.abs() if accumulate else dw_abs, n, int(accumulate), False)
            within_bound("wgrad db " + tag, "colsum", a.part(after, "db").double(), db + t.db0 if accumulate else db,
                         db_abs + t.db0.abs() if accumulate else db_abs, n, int(accumulate), False)
            within_bound("wgrad dnb " + tag, "colsum", a.part(after, "dnb").double(), dnb, dnb_abs, c.OH * c.OW, 0, False)
            # without db and dnb: the dw bits are unchanged; and a second call gives them again
            for with_sums in (False, True):
                rc, a = call_backward_weight(c.shape, t, accumulate, with_sums, with_sums, skew=int(unaligned))
                assert rc == 0 and torch.equal(a.result("dw").view(torch.int32), seen[accumulate].view(torch.int32)), (label, accumulate)


# ------------------------------------------------------------------------------------------ (d) invariances
# three images inside one pixel tile on a split route (forward 4 ragged splits, backward-data 3), the 1x1-pixel image,
# 1x1 stride 2; each plans the same kernel and split for one image as for three
ALONE = [R.CASES[i] for i in (1, 13, 12)]


@pytest.mark.parametrize("c", ALONE, ids=_id)
def test_an_image_alone_equals_the_same_image_inside_a_batch(c):
    c1 = c._replace(N=1)
    ws, ws1 = ("queried", None), ("queried", None)
    assert route(FWD, c1.shape, 0, M.data_workspace_bytes(c1.shape))[0] == asked_route(c, "fwd") == c.fwd
    assert route(DGRAD, c1.shape, 0, M.data_workspace_bytes(c1.shape))[0] == asked_route(c, "dgrad") == c.dgrad
    full = ("bias", "nbias", "addend")
    t = model(c, "fwd", "gauss")[0]
    rc, a = call_forward(c.shape, t, full, ws)
    y = a.result("y")
    assert rc == 0
    d = model(c, "dgrad", "gauss")[0]
    rc, a = call_backward_data(c.shape, d, "apart", ws)
    dx = a.result("dx")
    assert rc == 0
    for n in range(c.N):
        t1 = SimpleNamespace(x=t.x[n:n + 1], w=t.w, bias=t.bias, nbias=t.nbias[n:n + 1], addend=t.addend[n:n + 1])
        rc, a = call_forward(c1.shape, t1, full, ws1)
        assert rc == 0 and torch.equal(a.result("y")[0], y[n]), ("fwd", n)
        d1 = SimpleNamespace(dy=d.dy[n:n + 1], w=d.w, addend=d.addend[n:n + 1])
        rc, a = call_backward_data(c1.shape, d1, "apart", ws1)
        assert rc == 0 and torch.equal(a.result("dx")[0], dx[n]), ("dgrad", n)


# ------------------------------------------------------------------------------------------ (e) refusals
def _dummy(shape):
    """Tensors of ones for a shape outside the domain (extents that are not positive stand in as 1)."""
    N, H, W, C, K, Rr, stride, pad = shape
    N, OH, OW = max(N, 1), max(R.out_extent(H, Rr, stride, pad), 1), max(R.out_extent(W, Rr, stride, pad), 1)
    one = lambda *s: torch.ones(s, dtype=torch.float64)
    return SimpleNamespace(x=one(N, H, W, C), w=one(K, C, Rr, Rr), dy=one(N, OH, OW, K), bias=one(K), nbias=one(N, K),
                           addend=one(N, OH, OW, K), dw0=one(K, C, Rr, Rr), db0=one(K))


@pytest.mark.parametrize("shape", R.REFUSED, ids=lambda s: "x".join(map(str, s)))
def test_shapes_outside_the_domain_are_refused_and_nothing_is_written(shape):
    t = _dummy(shape)
    assert M.forward(shape, 1 << 30) is None and route(FWD, shape, 0, 1 << 30) is None
    rc, a = call_forward(shape, t, ("bias", "nbias", "addend"))
    assert rc == EINVAL and untouched(a, a.download(), "y", "ws")
    assert M.backward_data(shape, 1 << 30) is None and route(DGRAD, shape, 0, 1 << 30) is None
    t.addend = torch.ones((max(shape[0], 1), shape[1], shape[2], shape[3]), dtype=torch.float64)
    rc, a = call_backward_data(shape, t, "apart")
    assert rc == EINVAL and untouched(a, a.download(), "dx", "ws")
    assert M.backward_weight(shape, 1 << 30) is None and route(WGRAD, shape, 0, 1 << 30) is None
    rc, a = call_backward_weight(shape, t, False, True, True)
    assert rc == EINVAL and untouched(a, a.download(), "dw", "db", "dnb", "ws")


@pytest.mark.parametrize("shape", R.SHORT_WS, ids=lambda s: "x".join(map(str, s)))
def test_a_backward_weight_workspace_one_byte_short_is_enospc_and_nothing_is_written(shape):
    c = next(c for c in R.CASES if c.shape == shape)
    wsb = L().salun_conv2d_bf16_wgrad_workspace_bytes(*shape)
    assert route(WGRAD, shape, 0, wsb - 1) == M.ENOSPC == M.backward_weight(shape, wsb - 1)
    rc, a = call_backward_weight(shape, model(c, "wgrad", "int")[0], False, True, True, short=1)
    assert rc == ENOSPC and untouched(a, a.download(), "dw", "db", "dnb", "ws")


# ------------------------------------------------------------------------------------------ (f) the 3x3 ring forms
def ring3_child():
    """In a process started with SALUN_CONV_RING=3: the route query, asked WITHOUT an override, plans ring<...> for every
    RING3 shape (the query and the launch read the same switch); then the exact tier's forward variants."""
    assert RING == 3
    for c in R.RING3_CASES:
        got = route(FWD, c.shape, 0, M.data_workspace_bytes(c.shape))
        assert got == (c.fwd, 1), (c.id, got)
    for c in R.RING3_CASES:
        check_forward_exact(c)
    print("ring3 ok")


def test_ring_forms_on_3x3_shapes_in_a_child_process():
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); import test_conv_bf16_exact_gpu as t; t.ring3_child()" % here
    env = dict(os.environ, SALUN_CONV_RING="3", PYTHONPATH=os.path.dirname(here))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ring3 ok"), out.stderr[-3000:]
