"""K30 (csrc/salun_conv1x1_infer.hip) against the float64 model of conv1x1_ref_cpu.py (validated by
test_conv1x1_ref_cpu.py), with the conventions of test_conv_infer_gpu.py: the kernel is called through the C-ABI on views
inside guarded_arena.Arena (NaN guards around inputs, sentinels around and inside the output; everything but the output
must be unchanged after the call).

(a) exact tier: integer inputs; y must EQUAL the float64 answer - every subset of the epilogue, with and without ReLU,
    every forced tile.
(b) bound tier: Gaussian inputs; every element within gamma_(2n+e) * abs_sum of the float64 answer (n = C products,
    e = epilogue operations), the bound of the K27 tests.
(c) bit for bit: K27 with R = 1 on the same inputs (no tolerance: the same FMA chain); a second call; an image alone
    against the image in its batch; every tile; x and y one float off the 16-byte boundary (the 4-byte path).
(d) refusals: SALUN_EINVAL with the output sentinels intact.
(e) the route query agrees with the mirror of the plan."""
import ctypes

import pytest
import torch

import conv1x1_ref_cpu as P
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


def same(got, want64):
    want = want64.float()
    assert torch.equal(want.double(), want64), "the expected answer is not an fp32 number"
    return got.shape == want.shape and torch.equal(got, want)


def data(c, kind):
    """The inputs of a case and its float64 convolution (and |.| convolution), computed once and left unchanged."""
    key = (c, kind)
    if key not in _cache:
        t = P.inputs(c, kind)
        t.conv = P.forward(t.x, t.w, c)
        t.conv_abs = P.forward(t.x, t.w, c, absolute=True) if kind == "gauss" else None
        _cache[key] = t
    return _cache[key]


def call(c, t, names=(), relu=False, tile=0, x=None, alias=None, null=(), skew=0):
    a = Arena().put("x", t.x if x is None else x, skew=skew).put("w", t.w)
    for n in names:
        a.put(n, getattr(t, n))
    N = x.shape[0] if x is not None else c.N
    a.put("y", shape=(N, c.K, c.H, c.W), out=True, skew=skew).upload()
    ptr = lambda n: ctypes.c_void_p(None) if n in null else a.ptr(n)
    rc = L().salun_conv1x1_infer(ptr("x"), ptr("w"), ptr("scale"), ptr("shift"), a.ptr("y") if alias else ptr("addend"),
                                 a.ptr("y"), N, c.C, ctypes.c_int64(c.H * c.W), c.K, int(relu), tile, stream())
    return rc, a


def exact(t, names, relu):
    return P.epilogue(t.conv, **P.terms_of(t, names), relu=relu)


# ------------------------------------------------------------------------------------------ (a) exact tier
@pytest.mark.parametrize("c", P.CASES, ids=_id)
def test_equals_the_exact_answer(c):
    t = data(c, "int")
    for tile in (0,) + P.TILES:
        for names in (P.EPILOGUES if tile else [(), ("scale", "shift", "addend")]):
            for relu in (False, True):
                rc, a = call(c, t, names, relu, tile)
                assert rc == 0, (names, relu, tile)
                assert same(a.result("y"), exact(t, names, relu)), (names, relu, P.route(c, tile))


# ------------------------------------------------------------------------------------------ (b) bound tier
@pytest.mark.parametrize("c", P.CASES, ids=_id)
def test_within_the_per_element_bound(c):
    t = data(c, "gauss")
    n = c.C
    for names in ((), ("scale", "shift", "addend")):
        abs_sum = P.epilogue(t.conv_abs, **P.terms_of(t, names), absolute=True)
        want = exact(t, names, False)
        e = len(names)
        for tile in (0,) + P.TILES:
            rc, a = call(c, t, names, False, tile)
            assert rc == 0
            err = (a.result("y").double() - want).abs()
            print(f"pw {c.id} {P.route(c, tile)} {'+'.join(names) or 'plain'}: n = {n}, e = {e}, worst |got - exact| = "
                  f"{float((err / (P.U * abs_sum)).max()):.3f} u * abs_sum (bound {P.bound_gamma(2 * n + e) / P.U:.1f})")
            assert bool((err <= P.bound_gamma(2 * n + e) * abs_sum).all()), (c.id, names, tile)


# ------------------------------------------------------------------------------------------ (c) bit for bit
@pytest.mark.parametrize("c", P.CASES, ids=_id)
def test_k27_bits_again_alone_and_on_every_tile(c):
    from unlearn_saliency_amd import ops_infer
    t = data(c, "gauss")
    bits = lambda v: v.contiguous().view(torch.int32)
    for names, relu in (((), False), (("scale", "shift", "addend"), True)):
        dev = {n: getattr(t, n).float().cuda() for n in ("x", "w") + names}
        k27 = ops_infer.conv2d_infer(dev["x"], dev["w"], dev.get("scale"), dev.get("shift"), dev.get("addend"), relu, 1, 0)
        k30 = ops_infer.conv1x1_infer(dev["x"], dev["w"], dev.get("scale"), dev.get("shift"), dev.get("addend"), relu)
        assert torch.equal(bits(k30), bits(k27)), (names, P.route(c))
        rc, a = call(c, t, names, relu)
        y = a.result("y")
        assert rc == 0 and torch.equal(bits(y), bits(k27.cpu()))
    names, relu = ("scale", "shift", "addend"), True          # y: the last loop's, with the whole epilogue and ReLU
    rc2, a2 = call(c, t, names, relu)
    assert rc2 == 0 and torch.equal(bits(a2.result("y")), bits(y))
    for tile in P.TILES:
        rc, b = call(c, t, names, relu, tile)
        assert rc == 0 and torch.equal(bits(b.result("y")), bits(y)), P.route(c, tile)
    rc, a = call(c, t, ("scale", "shift"), True)
    y = a.result("y")
    for n in {0, c.N - 1}:
        rc, b = call(c, t, ("scale", "shift"), True, x=t.x[n:n + 1])
        assert rc == 0 and torch.equal(bits(b.result("y")[0]), bits(y[n])), n


def test_one_float_off_the_16_byte_boundary_takes_the_4_byte_path_and_gives_the_same_bits():
    c = P.SKEWED
    assert "/vec16/" in P.route(c) and "/vec4/" in P.route(c, aligned16=False)
    for kind in ("int", "gauss"):
        t = data(c, kind)
        for tile in (0,) + P.TILES:
            rc, a = call(c, t, ("scale", "shift", "addend"), True, tile)
            rc2, b = call(c, t, ("scale", "shift", "addend"), True, tile, skew=1)
            assert b.ptr("x").value % 16 == 4 and b.ptr("y").value % 16 == 4 and a.ptr("x").value % 16 == 0
            assert rc == 0 and rc2 == 0
            assert torch.equal(b.result("y").view(torch.int32), a.result("y").view(torch.int32)), tile
            if kind == "int":
                assert same(b.result("y"), exact(t, ("scale", "shift", "addend"), True))


# ------------------------------------------------------------------------------------------ (d) refusals
def test_refusals_return_einval_and_write_nothing():
    base = P.CASES[0]
    untouched = lambda a: bool((a.result("y").view(torch.int32) == SENTINEL).all())
    for name, change in P.REFUSED.items():
        c = base._replace(**change)
        assert P.route(c) is None
        rc, a = call(c, P.inputs(c, "int"))
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
@pytest.mark.parametrize("c", P.CASES, ids=_id)
def test_route_query_agrees_with_the_mirror(c):
    for tile in (0,) + P.TILES:
        for a16 in (1, 0):
            buf = ctypes.create_string_buffer(96)
            rc = L().salun_conv1x1_infer_route(c.N, c.C, ctypes.c_int64(c.H * c.W), c.K, tile, a16, 1, buf, 96)
            assert rc == 0 and buf.value.decode() == P.route(c, tile, bool(a16))


def test_thin_caller_runs_k30_inside_the_domain_and_k27_outside_it_and_counts_nothing():
    from unlearn_saliency_amd import conv_infer, ops_infer
    conv_infer.reset_library_infer_calls()
    g = torch.Generator().manual_seed(5)
    for C, K in ((16, 32), (8, 64)):
        x = torch.randn((2, C, 5, 5), generator=g).cuda()
        w = torch.randn((K, C, 1, 1), generator=g).cuda()
        s, h = torch.randn(K, generator=g).cuda(), torch.randn(K, generator=g).cuda()
        got = conv_infer.conv1x1_bn_act(x, w, s, h, None, True)
        assert torch.equal(got, ops_infer.conv2d_infer(x, w, s, h, None, True, 1, 0))
    assert conv_infer.library_infer_calls() == 0
    x = torch.randn((1, 12, 5, 5), generator=g).cuda()       # C = 12: neither kernel serves it; conv_bn_act counts it
    w = torch.randn((32, 12, 1, 1), generator=g).cuda()
    got = conv_infer.conv1x1_bn_act(x, w)
    assert torch.allclose(got, torch.nn.functional.conv2d(x, w), rtol=1e-4, atol=1e-4)
    assert conv_infer.LIBRARY_INFER_CALLS["conv_shape"] == 1 and conv_infer.library_infer_calls() == 1
    conv_infer.reset_library_infer_calls()
