"""K27 with a nearest-neighbour 2x input (salun_conv2d_infer_up2, csrc/salun_conv_infer.hip): the decoder's Upsample in
one launch.  Called through the C-ABI on views inside guarded_arena.Arena, as test_conv_infer_gpu.py does.

The reference is F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1) in float64 on the CPU.
(a) exact tier: integers small enough that every partial sum is exact (|x| <= 3, |w| <= 2, at most 288 products), so y
    must EQUAL the reference on every tile.  A gather that takes virtual row -1 for stored row 0, or virtual row 2H for
    stored row H - 1, fails here: the border rows of the reference see zeros there.
(b) bound tier: Gaussian inputs, every element within gamma_(2n+1) * abs_sum, n = 9 C.
(c) bit for bit: equal to salun_conv2d_infer on the materialised up-sampled tensor with the same tile; a second call; an
    image alone against the image in its batch.
(d) refusals: SALUN_EINVAL with the output sentinels intact.
(e) the route label; the plain labels of conv_infer_ref_cpu.CASES are what they were."""
import ctypes
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

import conv_infer_ref_cpu as R
from guarded_arena import SENTINEL, Arena

pytestmark = pytest.mark.gpu

EINVAL = -22
Up = namedtuple("Up", "N C H W K epilogue")
CASES = [Up(2, 8, 3, 3, 32, False),      # generic; 72 pixels: a masked tile that spans two images
         Up(2, 16, 5, 7, 64, False),     # fast; 280 pixels: three tiles of 128, odd sizes
         Up(1, 32, 4, 4, 32, True)]      # scale + shift + addend + relu
TILES = (0, 1, 2, 3)
_id = lambda c: "x".join(str(int(v)) for v in c)
_cache = {}


def L():
    from unlearn_saliency_amd import _lib
    return _lib.lib()


def stream():
    from unlearn_saliency_amd.streams import _stream
    return _stream()


def up2(x):
    return F.interpolate(x, scale_factor=2, mode="nearest")


def reference(x, w, t=None, absolute=False):
    """float64: conv2d(up2(x), w, padding=1) and, with `t`, K27's epilogue with ReLU."""
    if absolute:
        x, w = x.abs(), w.abs()
    y = F.conv2d(up2(x.double()), w.double(), padding=1)
    if t is not None:
        y = R.epilogue(y, t.scale, t.shift, t.addend, relu=True)
    return y


def data(c, kind):
    key = (c, kind)
    if key not in _cache:
        g = torch.Generator().manual_seed(11 + len(_cache))
        t = type("T", (), {})()
        if kind == "int":
            t.x = torch.randint(-3, 4, (c.N, c.C, c.H, c.W), generator=g).double()
            t.w = torch.randint(-2, 3, (c.K, c.C, 3, 3), generator=g).double()
            t.scale = (torch.randint(1, 3, (c.K,), generator=g) * (1 - 2 * (torch.arange(c.K) % 2))).double()
            t.shift = torch.randint(-2, 3, (c.K,), generator=g).double()
            t.addend = torch.randint(-2, 3, (c.N, c.K, 2 * c.H, 2 * c.W), generator=g).double()
        else:
            t.x = torch.randn((c.N, c.C, c.H, c.W), generator=g).double()
            t.w = torch.randn((c.K, c.C, 3, 3), generator=g).double()
            t.scale, t.shift = torch.randn(c.K, generator=g).double(), torch.randn(c.K, generator=g).double()
            t.addend = torch.randn((c.N, c.K, 2 * c.H, 2 * c.W), generator=g).double()
        t.x, t.w, t.scale, t.shift, t.addend = (v.float().double() for v in (t.x, t.w, t.scale, t.shift, t.addend))
        t.want = reference(t.x, t.w, t if c.epilogue else None)
        t.abs_sum = reference(t.x, t.w, absolute=True)
        _cache[key] = t
    return _cache[key]


def call(c, t, tile=0, x=None, materialised=False, R_=3, stride=1, pad=1, H=None, W=None):
    """The up2 entry point on x, or (materialised) the plain entry point on up2(x); the epilogue where the case has one."""
    x = t.x if x is None else x
    N = x.shape[0]
    H, W = (c.H if H is None else H), (c.W if W is None else W)
    a = Arena().put("x", up2(x) if materialised else x).put("w", t.w)
    if c.epilogue:
        a.put("scale", t.scale).put("shift", t.shift).put("addend", t.addend[:N])
    a.put("y", shape=(N, c.K, 2 * H, 2 * W), out=True).upload()
    fn = L().salun_conv2d_infer if materialised else L().salun_conv2d_infer_up2
    h, w_ = (2 * H, 2 * W) if materialised else (H, W)
    rc = fn(a.ptr("x"), a.ptr("w"), a.ptr("scale"), a.ptr("shift"), a.ptr("addend"), a.ptr("y"), N, c.C, h, w_, c.K, R_,
            stride, pad, 2 * H, 2 * W, int(c.epilogue), tile, stream())
    return rc, a


def bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_equals_the_exact_answer_on_every_tile(c):
    t = data(c, "int")
    want = t.want.float()
    assert torch.equal(want.double(), t.want) and float(t.abs_sum.max()) < 2 ** 24
    for tile in TILES:
        rc, a = call(c, t, tile)
        assert rc == 0, tile
        assert torch.equal(a.result("y"), want), tile


def test_border_taps_read_zero_not_the_edge_row():
    """x = 1 everywhere, w = 1 on one tap: the output is 0 exactly where that tap falls on virtual row / column -1 or 2H."""
    c = CASES[0]
    t = type("T", (), {})()
    t.x = torch.ones((c.N, c.C, c.H, c.W), dtype=torch.float64)
    for r in range(3):
        for s in range(3):
            t.w = torch.zeros((c.K, c.C, 3, 3), dtype=torch.float64)
            t.w[:, 0, r, s] = 1.0
            want = reference(t.x, t.w).float()
            zeros = int((want == 0).sum())              # per plane: a row and / or a column of 2H, 2W minus their corner
            rows, cols = (r != 1) * 2 * c.W, (s != 1) * 2 * c.H
            assert zeros == c.N * c.K * (rows + cols - (1 if rows and cols else 0))
            rc, a = call(c, t)
            assert rc == 0 and torch.equal(a.result("y"), want), (r, s)


@pytest.mark.parametrize("c", CASES[:2], ids=_id)
def test_within_the_per_element_bound(c):
    t = data(c, "gauss")
    n = 9 * c.C
    for tile in (0, 3):
        rc, a = call(c, t, tile)
        assert rc == 0
        err = (a.result("y").double() - t.want).abs()
        print(f"up2 {_id(c)} tile {tile}: worst |got - exact| = {float((err / (R.U * t.abs_sum)).max()):.3f} u * abs_sum "
              f"(bound {R.bound_gamma(2 * n + 1) / R.U:.1f})")
        assert bool((err <= R.bound_gamma(2 * n + 1) * t.abs_sum).all()), tile


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_same_bits_as_the_materialised_map_again_and_alone(c):
    t = data(c, "gauss")
    first = None
    for tile in TILES:
        rc, a = call(c, t, tile)
        rc2, b = call(c, t, tile, materialised=True)
        assert rc == 0 and rc2 == 0
        y = a.result("y")
        assert torch.equal(bits(y), bits(b.result("y"))), tile
        first = y if first is None else first
        assert torch.equal(bits(y), bits(first)), tile                 # every tile gives the same bits
    rc, a = call(c, t)
    assert rc == 0 and torch.equal(bits(a.result("y")), bits(first))     # a second call
    for n in {0, c.N - 1}:
        rc, b = call(c, t, x=t.x[n:n + 1])
        assert rc == 0 and torch.equal(bits(b.result("y")[0]), bits(first[n])), n


def test_refusals_return_einval_and_write_nothing():
    base = CASES[0]
    t = data(base, "int")
    untouched = lambda a: bool((bits(a.result("y")) == SENTINEL).all())
    w_of = lambda r, C=base.C: torch.ones((base.K, C, r, r), dtype=torch.float64)
    rc, a = call(base, t, stride=2)
    assert rc == EINVAL and untouched(a), "stride 2"
    for r, pad in ((1, 0), (7, 3)):
        tt = type("T", (), dict(x=t.x, w=w_of(r)))()
        rc, a = call(base, tt, R_=r, pad=pad)
        assert rc == EINVAL and untouched(a), f"R = {r}"
    tall = type("T", (), dict(x=torch.ones((1, 8, 513, 1), dtype=torch.float64), w=w_of(3)))()
    rc, a = call(base._replace(N=1, H=513, W=1), tall)
    assert rc == EINVAL and untouched(a), "H = 513"
    c12 = base._replace(C=12)
    t12 = type("T", (), dict(x=torch.ones((2, 12, 3, 3), dtype=torch.float64), w=w_of(3, 12)))()
    rc, a = call(c12, t12)
    assert rc == EINVAL and untouched(a), "C = 12"
    rc, a = call(base, t)                                   # and the same arena layout is served when nothing is wrong
    assert rc == 0 and torch.equal(a.result("y"), t.want.float())


def test_route_labels():
    from unlearn_saliency_amd import ops_infer
    for c in CASES:
        plain = R.Case(c.N, c.C, 2 * c.H, 2 * c.W, c.K, 3, 1, 1)
        for tile in TILES:
            want = R.route(plain, tile).replace("infer<3,1>", "infer<3,1>^2")
            assert ops_infer.conv2d_infer_up2_route(c.N, c.C, c.H, c.W, c.K, tile=tile) == want
    assert ops_infer.conv2d_infer_up2_route(2, 16, 5, 7, 64) == "infer<3,1>^2/64x64/fast/B5"
    assert ops_infer.conv2d_infer_up2_route(1, 256, 256, 256, 256, tile=3) == "infer<3,1>^2/128x128/fast/B4096"
    for kw in (dict(stride=2), dict(R=1, pad=0), dict(R=7, pad=3)):
        assert ops_infer.conv2d_infer_up2_route(2, 8, 3, 3, 32, **kw) is None
    assert ops_infer.conv2d_infer_up2_route(1, 8, 513, 1, 32) is None and ops_infer.conv2d_infer_up2_route(2, 12, 3, 3, 32) is None
    assert ops_infer.conv2d_infer_up2_route(1, 8, 512, 1, 32) is not None
    # the plain entry point's plan and labels are what they were
    for c in R.CASES:
        for tile in TILES:
            buf = ctypes.create_string_buffer(96)
            rc = L().salun_conv2d_infer_route(c.N, c.C, c.H, c.W, c.K, c.R, c.stride, c.pad, c.P, c.Q, tile, buf, 96)
            assert rc == 0 and buf.value.decode() == R.route(c, tile)


def test_conv_up2_bn_act_takes_the_kernel_and_counts_the_library():
    from unlearn_saliency_amd import conv_infer
    c = CASES[2]
    t = data(c, "int")
    conv_infer.reset_library_infer_calls()
    dev = lambda v: v.float().cuda()
    y = conv_infer.conv_up2_bn_act(dev(t.x), dev(t.w), dev(t.scale), dev(t.shift), dev(t.addend), relu=True)
    assert conv_infer.library_infer_calls() == 0 and torch.equal(y.cpu(), t.want.float())
    y = conv_infer.conv_up2_bn_act(dev(t.x)[:, :4].contiguous(), dev(t.w)[:, :4].contiguous())     # C = 4: outside the domain
    assert conv_infer.LIBRARY_INFER_CALLS["conv_up2"] == 1
    assert torch.equal(y.cpu(), reference(t.x[:, :4], t.w[:, :4]).float())
    conv_infer.reset_library_infer_calls()
