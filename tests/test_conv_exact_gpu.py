"""K8 / K8r (csrc/salun_conv.hip, csrc/salun_conv_ring.hip) against the float64 model of conv_ref_cpu.py (validated by
test_conv_ref_cpu.py), on every route the host-side dispatch can take (conv_routes.py; conv_ref_cpu.CASES):

(a) exact tier: small integers times powers of two.  Every fp32 partial sum is exact in every order (the cap asserted
    in test_conv_ref_cpu.py), so y, dx and dw must EQUAL the float64 answer: forward with and without each epilogue
    term, with and without the split workspace; backward-data with, without and in place on its addend; backward-weight
    writing and accumulating.  Impulse inputs say where a wrong kernel is wrong.
(b) bound tier: Gaussian inputs with the same scales; every element within gamma_(2n+e) * abs_sum of the exact answer
    (n = length of the element's reduction, e = epilogue additions; 2n: product and add rounded separately, so the bound
    holds fused or not, for every summation tree and split; no absolute slack, nothing scaled by the tensor's maximum).
    The largest error seen, in units of u * abs_sum, is printed and logged (profiles/conv_bounds_measured.txt) but not
    asserted: nothing here is taken from what the kernels do today.
(c) invariances, bit for bit: an image with its neighbours zeroed / alone, a second call, the ring tiles.
(d) a weight view one float off a 16-byte boundary (slow staging; the split and the merged stride-2 kernel step aside).

The kernels are called through the C-ABI on views the test owns: every tensor of a call lies 16-byte aligned in ONE flat
allocation with 4096 floats of NaN before and after every input and of a sentinel pattern around every output (and in
the output itself before the call); after the call everything but the outputs must hold the bits it was given.  Where
the mirror says a call is outside the library's domain the test asserts SALUN_EINVAL; it never accepts a refusal
otherwise."""
import ctypes
import os
from ctypes import c_size_t, c_void_p

import pytest
import torch

import conv_ref_cpu as R
import conv_routes as M
from guarded_arena import GUARD, NAN_BITS, SENTINEL, Arena

pytestmark = pytest.mark.gpu

EINVAL = -22
CASES = R.CASES
_id = lambda c: c.id
XSHAPE = lambda c: (c.N, c.C, c.H, c.W)


def L():
    from unlearn_saliency_amd import _lib
    return _lib.lib()


def stream():
    from unlearn_saliency_amd.streams import _stream
    return _stream()


def log(line):
    print(line)
    d = os.environ.get("SALUN_MEASURED_DIR")      # where a recording run keeps its figures (profiles/ has the last ones)
    if d and os.path.isdir(d):
        with open(os.path.join(d, "conv_bounds_measured.txt"), "a") as f:
            f.write(line + "\n")


def same(got, want64):
    """Bit-for-bit equality with a float64 answer that fp32 holds exactly (+0 and -0 alike)."""
    want = want64.float()
    assert torch.equal(want.double(), want64), "the expected answer is not an fp32 number"
    return got.shape == want.shape and torch.equal(got, want)


# ------------------------------------------------------------------------------------------ the calls
def call_forward(c, t, terms=(), ws=False, skew=0):
    """-> (rc, arena, route the mirror expects).  terms: subset of bias / nbias / addend."""
    a = Arena().put("x", t.x).put("w", t.w, skew=skew)
    for name in terms:
        a.put(name, getattr(t, name))
    a.put("y", shape=(c.N, c.K, c.P, c.Q), out=True)
    wsb = M.data_ws_bytes(c.N, c.K, c.P, c.Q, c.R, c.stride) if ws else 0
    if wsb:
        a.put("ws", shape=(wsb // 4,), out=True)
    a.upload()
    rc = L().salun_conv2d_forward_fused(a.ptr("x"), a.ptr("w"), a.ptr("bias"), a.ptr("nbias"), a.ptr("addend"), a.ptr("y"),
                                        c.N, c.C, c.H, c.W, c.K, c.R, c.stride, c.pad, c.P, c.Q, a.ptr("ws"),
                                        c_size_t(wsb), stream())
    return rc, a, M.forward(c, epi=("nbias" in terms or "addend" in terms), ws=wsb > 0, w_al=skew == 0)


def call_backward_data(c, t, addend=None, ws=False, skew=0):
    """addend: None, "apart" or "inplace" (addend == dx)."""
    a = Arena().put("dy", t.dy).put("w", t.w, skew=skew)
    if addend == "apart":
        a.put("addend", t.addend)
    a.put("dx", data=t.addend if addend == "inplace" else None, shape=XSHAPE(c), out=True)
    wsb = M.data_ws_bytes(c.N, c.C, c.H, c.W, c.R, 1) if (ws and c.stride == 1) else 0
    if wsb:
        a.put("ws", shape=(wsb // 4,), out=True)
    a.upload()
    rc = L().salun_conv2d_backward_data_ws(a.ptr("dy"), a.ptr("w"), a.ptr("dx" if addend == "inplace" else "addend"),
                                           a.ptr("dx"), c.N, c.C, c.H, c.W, c.K, c.R, c.stride, c.pad, c.P, c.Q,
                                           a.ptr("ws"), c_size_t(wsb), stream())
    return rc, a, M.backward_data(c, ws=wsb > 0, w_al=skew == 0)


def call_backward_weight(c, t, accumulate=False, shared=False):
    wsb = L().salun_conv2d_wgrad_workspace_bytes(c.N, c.C, c.K, c.R, c.P, c.Q)
    a = Arena().put("x", t.x).put("dy", t.dy)
    a.put("dw", data=t.dw0 if accumulate else None, shape=(c.K, c.C, c.R, c.R), out=True)
    a.put("ws", shape=(max(wsb, 16) // 4,), out=True).upload()
    rc = L().salun_conv2d_backward_weight_ex(a.ptr("x"), a.ptr("dy"), a.ptr("dw"), c.N, c.C, c.H, c.W, c.K, c.R, c.stride,
                                             c.pad, c.P, c.Q, int(accumulate), 1 if shared else 0, a.ptr("ws"),
                                             c_size_t(wsb), stream())
    return rc, a, M.backward_weight(c, shared)[0]


def forward_variants(c):
    for ws in ((False, True) if M.data_ws_bytes(c.N, c.K, c.P, c.Q, c.R, c.stride) else (False,)):
        for terms in ((), ("bias",), ("nbias",), ("addend",), ("bias", "nbias", "addend")):
            yield terms, ws


def backward_data_variants(c):
    for ws in ((False, True) if (c.stride == 1 and M.data_ws_bytes(c.N, c.C, c.H, c.W, c.R, 1)) else (False,)):
        for addend in (None, "apart", "inplace"):
            yield addend, ws


def backward_weight_variants(c):
    for shared in ((False, True) if M.backward_weight(c, True) != M.backward_weight(c, False) else (False,)):
        for accumulate in (False, True):
            yield accumulate, shared


IN_FWD = [c for c in CASES if M.forward(c)]
IN_DGRAD = [c for c in CASES if M.backward_data(c)]
IN_WGRAD = [c for c in CASES if M.backward_weight(c)[0]]


def exact_forward(c, t, terms, conv=None):
    conv = R.forward(t.x, t.w, c.stride, c.pad, c.P, c.Q) if conv is None else conv
    return R.epilogue(conv, *(getattr(t, n) if n in terms else None for n in ("bias", "nbias", "addend")))


# ------------------------------------------------------------------------------------------ (a) exact tier
@pytest.mark.parametrize("c", IN_FWD, ids=_id)
def test_forward_equals_the_exact_answer(c):
    t = R.inputs(c, "fwd", "int")
    conv = R.forward(t.x, t.w, c.stride, c.pad, c.P, c.Q)
    for terms, ws in forward_variants(c):
        rc, a, route = call_forward(c, t, terms, ws)
        if route is None:                      # epilogue terms outside the stride-1 fast kernels
            assert rc == EINVAL, (terms, ws)
            continue
        assert rc == 0, (terms, ws, route)
        assert same(a.result("y"), exact_forward(c, t, terms, conv)), (terms, ws, route)


@pytest.mark.parametrize("c", IN_DGRAD, ids=_id)
def test_backward_data_equals_the_exact_answer(c):
    t = R.inputs(c, "dgrad", "int")
    dx = R.backward_data(t.dy, t.w, XSHAPE(c), c.stride, c.pad)
    for addend, ws in backward_data_variants(c):
        rc, a, route = call_backward_data(c, t, addend, ws)
        assert rc == 0, (addend, ws, route)
        assert same(a.result("dx"), dx + t.addend if addend else dx), (addend, ws, route)


@pytest.mark.parametrize("c", IN_WGRAD, ids=_id)
def test_backward_weight_equals_the_exact_answer(c):
    t = R.inputs(c, "wgrad", "int")
    dw = R.backward_weight(t.x, t.dy, c.R, c.stride, c.pad)
    for accumulate, shared in backward_weight_variants(c):
        rc, a, route = call_backward_weight(c, t, accumulate, shared)
        assert rc == 0, (accumulate, shared, route)
        assert same(a.result("dw"), dw + t.dw0 if accumulate else dw), (accumulate, shared, route)


def test_shapes_outside_the_domain_are_refused_and_nothing_is_written():
    """Every (case, direction) the mirror puts outside the library's domain returns SALUN_EINVAL."""
    n = 0
    for c in CASES:
        if not M.forward(c):
            rc, a, _ = call_forward(c, R.inputs(c, "fwd", "int"))
            assert rc == EINVAL and bool((a.result("y").view(torch.int32) == SENTINEL).all()), c
            n += 1
        if not M.backward_data(c):
            rc, a, _ = call_backward_data(c, R.inputs(c, "dgrad", "int"))
            assert rc == EINVAL and bool((a.result("dx").view(torch.int32) == SENTINEL).all()), c
            n += 1
        if not M.backward_weight(c)[0]:
            rc, a, _ = call_backward_weight(c, R.inputs(c, "wgrad", "int"))
            assert rc == EINVAL and bool((a.result("dw").view(torch.int32) == SENTINEL).all()), c
            n += 1
    assert n >= 4


# one case per route family (conv_routes.py names them): 64- and 128-pixel tiles, several images per tile and
# the split, slow staging, 1x1, stride 2 at pad 1 / 0, the merged and the per-class stride-2 backward-data with its
# PSZ > 256 form and its empty classes, and every backward-weight kernel
IMPULSE = [R.Case(*s) for s in [
    (3, 8, 8, 16, 16, 3, 1, 1), (5, 64, 4, 4, 64, 3, 1, 1), (2, 40, 16, 16, 72, 3, 1, 1), (48, 8, 32, 32, 24, 3, 1, 1),
    (12, 8, 32, 32, 130, 3, 1, 1), (3, 32, 8, 16, 40, 1, 1, 0), (3, 8, 16, 32, 24, 3, 2, 1), (3, 8, 16, 16, 24, 3, 2, 0),
    (4, 64, 16, 32, 16, 3, 2, 1), (4, 64, 16, 32, 16, 3, 2, 0), (4, 64, 16, 16, 16, 1, 2, 0), (3, 24, 8, 16, 12, 3, 2, 1),
    (3, 24, 8, 16, 12, 1, 2, 0), (1, 8, 2, 256, 8, 3, 2, 1), (3, 3, 8, 16, 40, 3, 1, 1), (3, 64, 8, 8, 32, 3, 1, 1),
    (3, 64, 8, 16, 40, 3, 1, 1), (4, 64, 16, 16, 40, 3, 2, 1), (2, 64, 2, 64, 16, 3, 1, 1), (3, 32, 16, 16, 40, 1, 2, 0)]]
assert all(c in CASES for c in IMPULSE)


@pytest.mark.parametrize("c", IMPULSE, ids=_id)
def test_impulses_give_the_weight_patch_where_it_belongs(c):
    """x (dy) a single 1 at each corner and at one interior point of the last image's last channel: the output is the
    (flipped) weight patch around that point, clipped at the border, and zero everywhere else."""
    YSHAPE = (c.N, c.K, c.P, c.Q)
    if M.forward(c):
        t = R.inputs(c, "fwd", "int")
        for x in R.impulses(XSHAPE(c)):
            t.x = x
            rc, a, route = call_forward(c, t, ws=True)
            want = R.forward(x, t.w, c.stride, c.pad, c.P, c.Q)
            assert rc == 0 and same(a.result("y"), want), route
            assert int((want != 0).sum()) <= c.K * c.R * c.R
    if M.backward_data(c):
        t = R.inputs(c, "dgrad", "int")
        for dy in R.impulses(YSHAPE):
            t.dy = dy
            rc, a, route = call_backward_data(c, t, ws=True)
            assert rc == 0 and same(a.result("dx"), R.backward_data(dy, t.w, XSHAPE(c), c.stride, c.pad)), route
    if M.backward_weight(c)[0]:
        t = R.inputs(c, "wgrad", "int")
        for dy in R.impulses(YSHAPE):
            t.dy = dy
            for accumulate, shared in backward_weight_variants(c):
                if not accumulate:
                    rc, a, route = call_backward_weight(c, t, False, shared)
                    assert rc == 0 and same(a.result("dw"), R.backward_weight(t.x, dy, c.R, c.stride, c.pad)), route


# ------------------------------------------------------------------------------------------ (b) bound tier
def within_bound(tag, got, exact, abs_sum, n, e):
    """|got - exact| <= gamma_(2n+e) * abs_sum for every element; the measured ratio to u * abs_sum is logged first."""
    err = (got.double() - exact).abs()
    ratio = torch.where(abs_sum > 0, err / (R.U * abs_sum.clamp_min(1e-300)),
                        torch.where(err > 0, float("inf"), 0.0).double())
    log(f"{tag}: n = {n}, e = {e}, worst |got - exact| = {float(ratio.max()):.3f} u * abs_sum "
        f"(bound {R.bound_gamma(2 * n + e) / R.U:.1f})")
    assert bool((err <= R.bound_gamma(2 * n + e) * abs_sum).all()), tag


@pytest.mark.parametrize("c", IN_FWD, ids=_id)
def test_forward_within_the_per_element_bound(c):
    t = R.inputs(c, "fwd", "gauss")
    conv = R.forward(t.x, t.w, c.stride, c.pad, c.P, c.Q)
    conv_abs = R.forward(t.x, t.w, c.stride, c.pad, c.P, c.Q, absolute=True)
    full = ("bias", "nbias", "addend")
    for terms, ws in forward_variants(c):
        if terms not in ((), full if M.forward(c, epi=True, ws=ws) else ("bias",)):
            continue
        rc, a, route = call_forward(c, t, terms, ws)
        assert rc == 0, route
        absolute = R.epilogue(conv_abs, *(getattr(t, n).abs() if n in terms else None for n in full))
        within_bound(f"fwd {c.id} {route}", a.result("y"), exact_forward(c, t, terms, conv), absolute,
                     c.C * c.R * c.R, len(terms))


@pytest.mark.parametrize("c", IN_DGRAD, ids=_id)
def test_backward_data_within_the_per_element_bound(c):
    t = R.inputs(c, "dgrad", "gauss")
    dx = R.backward_data(t.dy, t.w, XSHAPE(c), c.stride, c.pad)
    dx_abs = R.backward_data(t.dy, t.w, XSHAPE(c), c.stride, c.pad, absolute=True)
    for addend, ws in backward_data_variants(c):
        if addend == "inplace":
            continue
        rc, a, route = call_backward_data(c, t, addend, ws)
        assert rc == 0, route
        within_bound(f"dgrad {c.id} {route}{' + addend' if addend else ''}", a.result("dx"),
                     dx + t.addend if addend else dx, dx_abs + t.addend.abs() if addend else dx_abs,
                     c.K * c.R * c.R, 1 if addend else 0)


@pytest.mark.parametrize("c", IN_WGRAD, ids=_id)
def test_backward_weight_within_the_per_element_bound(c):
    t = R.inputs(c, "wgrad", "gauss")
    dw = R.backward_weight(t.x, t.dy, c.R, c.stride, c.pad)
    dw_abs = R.backward_weight(t.x, t.dy, c.R, c.stride, c.pad, absolute=True)
    for accumulate, shared in backward_weight_variants(c):
        rc, a, route = call_backward_weight(c, t, accumulate, shared)
        assert rc == 0, route
        within_bound(f"wgrad {c.id} {route}{' accumulate' if accumulate else ''}", a.result("dw"),
                     dw + t.dw0 if accumulate else dw, dw_abs + t.dw0.abs() if accumulate else dw_abs,
                     c.N * c.P * c.Q, int(accumulate))


# ------------------------------------------------------------------------------------------ (c) invariances
def _only_image(x, n):
    z = torch.zeros_like(x)
    z[n] = x[n]
    return z


@pytest.mark.parametrize("c", IN_FWD, ids=_id)
def test_forward_of_an_image_does_not_depend_on_its_neighbours(c):
    """Gaussian inputs.  The first and the last image with every other image zeroed (same N: same kernel, split or not)
    give the bits of the batched call; so does the image alone where N = 1 takes the same route; so does a second call."""
    t = R.inputs(c, "fwd", "gauss")
    for ws in ((False, True) if M.data_ws_bytes(c.N, c.K, c.P, c.Q, c.R, c.stride) else (False,)):
        rc, a, route = call_forward(c, t, ("bias",), ws)
        y = a.result("y")
        rc2, a2, _ = call_forward(c, t, ("bias",), ws)
        assert rc == 0 and rc2 == 0 and torch.equal(a2.result("y").view(torch.int32), y.view(torch.int32)), route
        for n in {0, c.N - 1}:
            t1 = R.inputs(c, "fwd", "gauss")
            t1.x = _only_image(t.x, n)
            rc, a1, _ = call_forward(c, t1, ("bias",), ws)
            assert rc == 0 and torch.equal(a1.result("y")[n], y[n]), (route, n)
            c1 = c._replace(N=1)
            if M.forward(c1, ws=ws) == route:
                t1.x = t.x[n:n + 1]
                rc, a1, _ = call_forward(c1, t1, ("bias",), ws)
                assert rc == 0 and torch.equal(a1.result("y")[0], y[n]), (route, n, "alone")


@pytest.mark.parametrize("c", IN_DGRAD, ids=_id)
def test_backward_data_of_an_image_does_not_depend_on_its_neighbours(c):
    t = R.inputs(c, "dgrad", "gauss")
    for ws in ((False, True) if (c.stride == 1 and M.data_ws_bytes(c.N, c.C, c.H, c.W, c.R, 1)) else (False,)):
        rc, a, route = call_backward_data(c, t, None, ws)
        dx = a.result("dx")
        rc2, a2, _ = call_backward_data(c, t, None, ws)
        assert rc == 0 and rc2 == 0 and torch.equal(a2.result("dx").view(torch.int32), dx.view(torch.int32)), route
        for n in {0, c.N - 1}:
            t1 = R.inputs(c, "dgrad", "gauss")
            t1.dy = _only_image(t.dy, n)
            rc, a1, _ = call_backward_data(c, t1, None, ws)
            assert rc == 0 and torch.equal(a1.result("dx")[n], dx[n]), (route, n)
            c1 = c._replace(N=1)
            if M.backward_data(c1, ws=ws) == route:
                t1.dy = t.dy[n:n + 1]
                rc, a1, _ = call_backward_data(c1, t1, None, ws)
                assert rc == 0 and torch.equal(a1.result("dx")[0], dx[n]), (route, n, "alone")


@pytest.mark.parametrize("c", IN_WGRAD, ids=_id)
def test_backward_weight_is_the_same_on_a_second_call(c):
    t = R.inputs(c, "wgrad", "gauss")
    for accumulate, shared in backward_weight_variants(c):
        if not accumulate:
            (rc, a, route), (rc2, a2, _) = call_backward_weight(c, t, False, shared), call_backward_weight(c, t, False, shared)
            assert rc == 0 and rc2 == 0 and torch.equal(a.result("dw").view(torch.int32), a2.result("dw").view(torch.int32)), route


# ------------------------------------------------------------------------------------------ the ring kernels
def call_ring(N, Cred, H, W, Kout, cfg, x, img, terms, t, inplace=None):
    a = Arena().put("x", x).put("img", img)
    for name in terms:
        a.put(name, getattr(t, name))
    a.put("y", data=inplace, shape=(N, Kout, H, W), out=True).upload()
    rc = L().salun_conv3x3_packed(a.ptr("x"), a.ptr("img"), a.ptr("bias"), a.ptr("nbias"),
                                  a.ptr("y" if inplace is not None else "addend"), a.ptr("y"), N, Cred, H, W, Kout, cfg,
                                  stream())
    return rc, a


def pack(w, dgrad):
    """The packed image of the OIHW weight `w` (float64 on the host) as a host tensor, or None if not packable."""
    from unlearn_saliency_amd import _lib
    K, C = w.shape[:2]
    nbytes = L().salun_conv3x3_pack_bytes(K, C, dgrad)
    assert nbytes == M.ring_pack_bytes(K, C, dgrad)
    if nbytes == 0:
        return None
    a = Arena().put("w", w).put("img", shape=(nbytes // 4,), out=True).upload()
    job = _lib.PackJob(a.ptr("w").value, None if dgrad else a.ptr("img").value, a.ptr("img").value if dgrad else None, K, C)
    assert L().salun_conv3x3_pack_weights(ctypes.cast(ctypes.pointer(job), c_void_p), 1, stream()) == 0
    return a.result("img")


@pytest.mark.parametrize("cfg", sorted(M.RING_TILES))
@pytest.mark.parametrize("shape", R.RING_CASES, ids=lambda s: "x".join(map(str, s)))
def test_ring_tiles_equal_the_exact_answer(shape, cfg):
    """Every ring tile on integer inputs, H != W included: plain, with bias + nbias + addend, on impulses; backward-data
    plain and with the addend in place.  Outside the tile's domain: SALUN_EINVAL."""
    N, C, H, W, K = shape
    c = R.Case(N, C, H, W, K, 3, 1, 1)
    t = R.inputs(c, "fwd", "int")
    img = pack(t.w, 0)
    route = M.ring(N, C, H, W, K, cfg)
    rc, a = call_ring(N, C, H, W, K, cfg, t.x, img, (), t)
    if route is None:
        assert rc == EINVAL and bool((a.result("y").view(torch.int32) == SENTINEL).all())
    else:
        conv = R.forward(t.x, t.w, 1, 1, H, W)
        assert rc == 0 and same(a.result("y"), conv), route
        full = ("bias", "nbias", "addend")
        rc, a = call_ring(N, C, H, W, K, cfg, t.x, img, full, t)
        assert rc == 0 and same(a.result("y"), exact_forward(c, t, full, conv)), route
        for x in R.impulses(XSHAPE(c))[1:4]:
            rc, a = call_ring(N, C, H, W, K, cfg, x, img, (), t)
            assert rc == 0 and same(a.result("y"), R.forward(x, t.w, 1, 1, H, W)), route
    d = R.inputs(c, "dgrad", "int")
    imd = pack(d.w, 1)
    assert (imd is None) == (K % 8 != 0)
    if imd is not None:
        route = M.ring(N, K, H, W, C, cfg)
        rc, a = call_ring(N, K, H, W, C, cfg, d.dy, imd, (), d)
        if route is None:
            assert rc == EINVAL
            return
        dx = R.backward_data(d.dy, d.w, XSHAPE(c), 1, 1)
        assert rc == 0 and same(a.result("y"), dx), route
        rc, a = call_ring(N, K, H, W, C, cfg, d.dy, imd, (), d, inplace=d.addend)
        assert rc == 0 and same(a.result("y"), dx + d.addend), route


# ------------------------------------------------------------------------------------------ (d) misaligned weight
@pytest.mark.parametrize("c", [R.Case(2, 64, 8, 8, 64, 3, 1, 1), R.Case(3, 32, 8, 16, 40, 1, 1, 0),
                               R.Case(4, 64, 16, 32, 16, 3, 2, 1)], ids=_id)
def test_weight_one_float_off_a_16_byte_boundary(c):
    """Slow staging; no split although a workspace is offered; the stride-2 backward-data leaves the merged kernel for
    the per-class ones.  Exact tier: the answers do not change."""
    assert c in CASES
    t = R.inputs(c, "fwd", "int")
    rc, a, route = call_forward(c, t, ("bias",), ws=True, skew=1)
    assert "/slow/S1" in route and M.forward(c, ws=True) != route
    assert rc == 0 and same(a.result("y"), exact_forward(c, t, ("bias",))), route
    rc, a, route = call_forward(c, t, ("bias", "nbias"), ws=True, skew=1)
    assert route is None and rc == EINVAL          # the epilogue terms live in the fast kernels only
    t = R.inputs(c, "dgrad", "int")
    for addend in (None, "apart", "inplace"):
        rc, a, route = call_backward_data(c, t, addend, ws=True, skew=1)
        assert "/slow/S1" in route if c.stride == 1 else (route.startswith("dgrad_tap") and
                                                          M.backward_data(c).startswith("dgrad_s2"))
        dx = R.backward_data(t.dy, t.w, XSHAPE(c), c.stride, c.pad)
        assert rc == 0 and same(a.result("dx"), dx + t.addend if addend else dx), route
