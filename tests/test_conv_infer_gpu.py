"""K27 (csrc/salun_conv_infer.hip) against the float64 model of conv_infer_ref_cpu.py (validated by
test_conv_infer_ref_cpu.py), with the conventions of test_conv_exact_gpu.py: the kernel is called through the C-ABI on
views inside guarded_arena.Arena (NaN guards around inputs, sentinels around and inside outputs; everything but the
output must be unchanged after the call).

(a) exact tier: small integers times powers of two; every summation order is exact, so y must EQUAL the float64 answer
    — every subset of the epilogue, with and without ReLU, every tile, and on impulse inputs.
(b) bound tier: Gaussian inputs; every element within gamma_(2n+e) * abs_sum of the float64 answer (n = C R R products,
    e = epilogue operations; no absolute slack).  The largest error seen, in units of u * abs_sum, is logged
    (profiles/conv_infer_bounds_measured.txt) and not asserted.
(c) bit for bit: a second call; an image alone against the image in its batch; every tile against every other.
(d) refusals: SALUN_EINVAL with the output sentinels intact.
(e) the route query agrees with the mirror of the plan for what was launched."""
import ctypes
import os

import pytest
import torch

import conv_infer_ref_cpu as R
from guarded_arena import SENTINEL, Arena

pytestmark = pytest.mark.gpu

EINVAL = -22
_id = lambda c: c.id
_cache = {}


def L():
    from unlearn_saliency_amd import _lib
    return _lib.lib()


def stream():
    from unlearn_saliency_amd.streams import _stream
    return _stream()


def log(line):
    print(line)
    d = os.environ.get("SALUN_MEASURED_DIR")
    if d and os.path.isdir(d):
        with open(os.path.join(d, "conv_infer_bounds_measured.txt"), "a") as f:
            f.write(line + "\n")


def same(got, want64):
    want = want64.float()
    assert torch.equal(want.double(), want64), "the expected answer is not an fp32 number"
    return got.shape == want.shape and torch.equal(got, want)


def data(c, kind):
    """The inputs of a case and its float64 convolution (and |.| convolution), computed once and left unchanged."""
    key = (c, kind)
    if key not in _cache:
        t = R.inputs(c, kind)
        t.conv = R.forward(t.x, t.w, c)
        t.conv_abs = R.forward(t.x, t.w, c, absolute=True) if kind == "gauss" else None
        _cache[key] = t
    return _cache[key]


def call(c, t, names=(), relu=False, tile=0, x=None, alias=None, null=()):
    a = Arena().put("x", t.x if x is None else x).put("w", t.w)
    for n in names:
        a.put(n, getattr(t, n))
    a.put("y", shape=(x.shape[0] if x is not None else c.N, c.K, c.P, c.Q), out=True).upload()
    N = x.shape[0] if x is not None else c.N
    ptr = lambda n: ctypes.c_void_p(None) if n in null else a.ptr(n)
    rc = L().salun_conv2d_infer(ptr("x"), ptr("w"), ptr("scale"), ptr("shift"), a.ptr("y") if alias else ptr("addend"),
                                a.ptr("y"), N, c.C, c.H, c.W, c.K, c.R, c.stride, c.pad, c.P, c.Q, int(relu), tile,
                                stream())
    return rc, a


def exact(c, t, names, relu, conv=None):
    return R.epilogue(t.conv if conv is None else conv, **R.terms_of(t, names), relu=relu)


def tiles_for(c):
    """Every forced tile at the small shapes; the large ones (the 224 x 224 stem, the 512-channel layer) run the plan's
    own choice and one forced tile, which keeps a case within a few seconds."""
    return (0,) + R.TILES if c.N * c.C * c.H * c.W * c.K <= 1 << 24 else (0, 3)


# ------------------------------------------------------------------------------------------ (a) exact tier
@pytest.mark.parametrize("c", R.CASES, ids=_id)
def test_equals_the_exact_answer(c):
    t = data(c, "int")
    for tile in tiles_for(c):
        for names in (R.EPILOGUES if tile else [(), ("scale", "shift", "addend")]):
            for relu in (False, True):
                rc, a = call(c, t, names, relu, tile)
                assert rc == 0, (names, relu, tile)
                assert same(a.result("y"), exact(c, t, names, relu)), (names, relu, R.route(c, tile))


@pytest.mark.parametrize("c", [c for c in R.CASES if c.H <= 56], ids=_id)
def test_impulses_give_the_weight_patch_where_it_belongs(c):
    t = data(c, "int")
    for x in R.impulses((c.N, c.C, c.H, c.W)):
        want = R.forward(x, t.w, c)
        assert int((want != 0).sum()) <= c.K * c.R * c.R
        for tile in (0, 3):
            rc, a = call(c, t, x=x, tile=tile)
            assert rc == 0 and same(a.result("y"), want), R.route(c, tile)


# ------------------------------------------------------------------------------------------ (b) bound tier
@pytest.mark.parametrize("c", R.CASES, ids=_id)
def test_within_the_per_element_bound(c):
    t = data(c, "gauss")
    n = c.C * c.R * c.R
    for names in ((), ("scale", "shift", "addend")):
        abs_sum = R.epilogue(t.conv_abs, **R.terms_of(t, names), absolute=True)
        want = exact(c, t, names, False)
        for tile in (0, 3):
            rc, a = call(c, t, names, False, tile)
            assert rc == 0
            err = (a.result("y").double() - want).abs()
            e = len(names)
            log(f"infer {c.id} {R.route(c, tile)} {'+'.join(names) or 'plain'}: n = {n}, e = {e}, worst |got - exact| = "
                f"{float((err / (R.U * abs_sum)).max()):.3f} u * abs_sum (bound {R.bound_gamma(2 * n + e) / R.U:.1f})")
            assert bool((err <= R.bound_gamma(2 * n + e) * abs_sum).all()), (c.id, names, tile)
            # ReLU rounds nothing: the same call with it gives act() of the same bits
            rc, b = call(c, t, names, True, tile)
            y = a.result("y")
            assert rc == 0 and torch.equal(b.result("y"), torch.where(y < 0, torch.zeros_like(y), y))


# ------------------------------------------------------------------------------------------ (c) bit for bit
@pytest.mark.parametrize("c", R.CASES, ids=_id)
def test_same_bits_again_alone_and_on_every_tile(c):
    t = data(c, "gauss")
    names = ("scale", "shift")
    rc, a = call(c, t, names, True)
    y = a.result("y")
    rc2, a2 = call(c, t, names, True)
    assert rc == 0 and rc2 == 0 and torch.equal(a2.result("y").view(torch.int32), y.view(torch.int32))
    for tile in tiles_for(c)[1:]:
        rc, b = call(c, t, names, True, tile)
        assert rc == 0 and torch.equal(b.result("y").view(torch.int32), y.view(torch.int32)), R.route(c, tile)
    for n in {0, c.N - 1}:
        rc, b = call(c, t, names, True, x=t.x[n:n + 1])
        assert rc == 0 and torch.equal(b.result("y")[0].view(torch.int32), y[n].view(torch.int32)), n


# ------------------------------------------------------------------------------------------ (d) refusals
def test_refusals_return_einval_and_write_nothing():
    base = R.CASES[0]
    untouched = lambda a: bool((a.result("y").view(torch.int32) == SENTINEL).all())
    for name, change in R.REFUSED.items():
        c = base._replace(**change)
        assert R.route(c) is None
        rc, a = call(c, R.inputs(c, "int"))
        assert rc == EINVAL and untouched(a), name
    t = data(base, "int")
    rc, a = call(base, t, null=("x",))
    assert rc == EINVAL and untouched(a), "NULL x"
    rc, a = call(base, t, alias=True)
    assert rc == EINVAL and untouched(a), "addend == y"
    rc, a = call(base, t, tile=7)
    assert rc == EINVAL and untouched(a), "unknown tile"
    rc, a = call(base, t)                                   # and the same arena layout is served when nothing is wrong
    assert rc == 0 and same(a.result("y"), t.conv)


# ------------------------------------------------------------------------------------------ (e) route query
@pytest.mark.parametrize("c", R.CASES, ids=_id)
def test_route_query_agrees_with_the_mirror(c):
    for tile in (0,) + R.TILES:
        buf = ctypes.create_string_buffer(96)
        rc = L().salun_conv2d_infer_route(c.N, c.C, c.H, c.W, c.K, c.R, c.stride, c.pad, c.P, c.Q, tile, buf, 96)
        assert rc == 0 and buf.value.decode() == R.route(c, tile)
        assert L().salun_conv2d_infer_route(c.N, c.C, c.H, c.W, c.K, c.R, c.stride, c.pad, c.P, c.Q, tile, buf, 8) == -28
    for change in R.REFUSED.values():
        r = c._replace(**change)
        buf = ctypes.create_string_buffer(96)
        assert L().salun_conv2d_infer_route(r.N, r.C, r.H, r.W, r.K, r.R, r.stride, r.pad, r.P, r.Q, 0, buf, 96) == EINVAL
