"""The float64 model of conv_bf16_ref_cpu.py against torch's float64 convolution and its autograd, the rounding
to_bf16_rne against torch's own, the premise of the exact tier (every partial sum of every integer case below 2^24 units,
and a bf16 tie somewhere), and the route every case of test_conv_bf16_exact_gpu.py claims: against the mirror
bf16_routes.py for every (workspace, alignment, switch) variant the GPU tests call, and against the library's host-only
queries.  No GPU."""
import ctypes

import pytest
import torch

import bf16_routes as M
import conv_bf16_ref_cpu as R

ALL = R.CASES + R.RING3_CASES
DIRECTIONS = ("fwd", "dgrad", "wgrad")
EINVAL, ENOSPC = -22, -28
FWD, DGRAD, WGRAD = 0, 1, 2           # SALUN_ROUTE_FORWARD / _BACKWARD_DATA / _BACKWARD_WEIGHT
UNALIGNED = 8                         # SALUN_ROUTE_OUT_UNALIGNED
ring_bits = lambda v: (v + 1) << 8    # SALUN_ROUTE_RING(v)
_id = lambda c: c.id


def _close(got, want, exact):
    assert got.shape == want.shape
    if exact:
        assert torch.equal(got, want)
    else:
        assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-300)


def _kinds(c):
    return ("int", "gauss") if c.N * c.OH * c.OW * c.C * c.K * c.R * c.R <= 10 ** 8 else ("int",)


@pytest.mark.parametrize("c", ALL, ids=_id)
def test_model_agrees_with_torch_float64_and_its_autograd(c):
    for kind in _kinds(c):
        exact = kind == "int"
        t = R.inputs(c, "fwd", kind)
        x = R.nchw(t.x).requires_grad_(True)
        w = t.w.clone().requires_grad_(True)
        conv = torch.nn.functional.conv2d(x, w, None, c.stride, c.pad)
        assert conv.shape == (c.N, c.K, c.OH, c.OW)
        _close(R.forward(t.x, t.w, c.stride, c.pad), R.nhwc(conv.detach()), exact)
        want = ((conv.detach() + t.bias[None, :, None, None]) + t.nbias[:, :, None, None]) + R.nchw(t.addend)
        _close(R.forward(t.x, t.w, c.stride, c.pad, t.bias, t.nbias, t.addend), R.nhwc(want), exact)
        # backward-data: the gradient of the same convolution with respect to x, for the dgrad inputs' dy and w
        d = R.inputs(c, "dgrad", kind)
        dx, = torch.autograd.grad(torch.nn.functional.conv2d(x, d.w, None, c.stride, c.pad), x, R.nchw(d.dy))
        _close(R.backward_data(d.dy, d.w, (c.N, c.H, c.W, c.C), c.stride, c.pad), R.nhwc(dx), exact)
        _close(R.backward_data(d.dy, d.w, (c.N, c.H, c.W, c.C), c.stride, c.pad, d.addend), R.nhwc(dx) + d.addend, exact)
        # backward-weight: ... with respect to w, for the wgrad inputs' x and dy
        g = R.inputs(c, "wgrad", kind)
        dw, = torch.autograd.grad(torch.nn.functional.conv2d(R.nchw(g.x), w, None, c.stride, c.pad), w, R.nchw(g.dy))
        got_dw, got_db, got_dnb = R.backward_weight(g.x, g.dy, c.R, c.stride, c.pad)
        _close(got_dw, dw, exact)
        _close(got_dnb, g.dy.sum(dim=(1, 2)), exact)
        _close(got_db, g.dy.reshape(-1, c.K).sum(dim=0), exact)
        got_dw, got_db, _ = R.backward_weight(g.x, g.dy, c.R, c.stride, c.pad, g.dw0, g.db0)
        _close(got_dw, dw + g.dw0, exact)
        _close(got_db, g.dy.reshape(-1, c.K).sum(dim=0) + g.db0, exact)


def test_abs_sum_is_the_sum_of_absolute_terms():
    c = R.CASES[10]
    t = R.inputs(c, "fwd", "gauss")
    a = R.forward(t.x, t.w, c.stride, c.pad, t.bias, t.nbias, t.addend, absolute=True)
    want = R.forward(t.x.abs(), t.w.abs(), c.stride, c.pad) + t.bias.abs() + t.nbias.abs()[:, None, None, :] + t.addend.abs()
    _close(a, want, False)
    assert (a >= R.forward(t.x, t.w, c.stride, c.pad, t.bias, t.nbias, t.addend).abs()).all()
    g = R.inputs(c, "wgrad", "gauss")
    dw, db, dnb = R.backward_weight(g.x, g.dy, c.R, c.stride, c.pad, g.dw0, g.db0, absolute=True)
    assert (dw >= R.backward_weight(g.x, g.dy, c.R, c.stride, c.pad, g.dw0, g.db0)[0].abs()).all()
    _close(db, g.dy.abs().sum(dim=(0, 1, 2)) + g.db0.abs(), False)
    _close(dnb, g.dy.abs().sum(dim=(1, 2)), False)


def test_to_bf16_rne_is_torchs_rounding():
    g = torch.Generator().manual_seed(0)
    v = torch.randn(200000, generator=g) * torch.exp2(torch.randint(-20, 20, (200000,), generator=g).float())
    ties = torch.arange(257, 512, 2).float().repeat(2) * torch.tensor([1.0, -8.0]).repeat_interleave(128)  # 9-bit odd numbers
    whole = torch.arange(-70000, 70000, 7).float()
    for t in (v, ties, whole):
        assert torch.equal(R.to_bf16_rne(t.double()), t.bfloat16().double())
    assert bool(R.is_bf16_tie(ties.double()).all()) and not bool(R.is_bf16_tie(whole.double()[::2] * 2).all())
    assert torch.equal(R.to_bf16_rne(torch.tensor([257.0, 259.0, -261.0]).double()), torch.tensor([256.0, 260.0, -260.0]).double())
    assert R.U16 == 2.0 ** -8 and float((R.to_bf16_rne(v.double()) - v.double()).abs().div(v.double().abs()).max()) <= R.U16


def test_inputs_are_bf16_numbers_where_the_kernels_read_bf16():
    for c in ALL[:8] + ALL[-3:]:
        for kind in ("int", "gauss"):
            f, d, g = (R.inputs(c, direction, kind) for direction in DIRECTIONS)
            for t in (f.x, f.w, f.addend, d.dy, d.w, d.addend, g.x, g.dy):
                assert torch.equal(t.float().bfloat16().double(), t)
            for t in (f.bias, f.nbias, g.dw0, g.db0):
                assert torch.equal(t.float().double(), t)


def abs_sums(c, direction):
    """-> [(sum of the magnitudes of every term of every element, the element's unit)] with every epilogue term on"""
    t = R.inputs(c, direction, "int")
    if direction == "fwd":
        return [(R.forward(t.x, t.w, c.stride, c.pad, t.bias, t.nbias, t.addend, absolute=True), t.unit)]
    if direction == "dgrad":
        return [(R.backward_data(t.dy, t.w, (c.N, c.H, c.W, c.C), c.stride, c.pad, t.addend, absolute=True), t.unit)]
    dw, db, dnb = R.backward_weight(t.x, t.dy, c.R, c.stride, c.pad, t.dw0, t.db0, absolute=True)
    return [(dw, t.unit), (db, t.unit_k), (dnb, t.unit_k.view(1, -1))]


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("c", ALL, ids=_id)
def test_exact_tier_premise_every_partial_sum_below_2_to_24_units(c, direction):
    """A condition, not a measurement: every term a whole multiple of its element's unit and the sum of their magnitudes
    below 2^24 units, so every fp32 partial sum - any order, any split, epilogue terms included - is exact."""
    for a, unit in abs_sums(c, direction):
        lg = torch.log2(unit)
        assert torch.equal(lg, lg.round()) and float(lg.abs().max()) <= 24
        units = a / unit
        assert torch.equal(units, units.round()), "a term is not a whole multiple of its element's unit"
        assert float(units.max()) < 2 ** 24


def test_the_exact_tier_pins_nearest_even():
    """Some exact sums lie half way between two bf16 numbers, in both directions of the tie: the bit-for-bit comparison
    then fails for any rounding but nearest-even (truncation, round-half-up, round-half-away)."""
    up = down = 0
    for c in R.CASES[:5]:
        t = R.inputs(c, "fwd", "int")
        y = R.forward(t.x, t.w, c.stride, c.pad)
        tie = R.is_bf16_tie(y)
        up += int((tie & (R.to_bf16_rne(y).abs() > y.abs())).sum())
        down += int((tie & (R.to_bf16_rne(y).abs() < y.abs())).sum())
        d = R.inputs(c, "dgrad", "int")
        dx = R.backward_data(d.dy, d.w, (c.N, c.H, c.W, c.C), c.stride, c.pad)
        assert torch.equal(R.to_bf16_rne(dx), dx.float().bfloat16().double())
    assert up >= 10 and down >= 10, (up, down)


# ------------------------------------------------------------------------------------------ the routes
def mirror_routes(c, ring=1):
    """{direction: [route of every variant the GPU tests call]}; the first of each list is the case's claim"""
    out = {"fwd": [M.forward(c.shape, ws, True, ring) for _, ws in R.data_ws_modes(c.shape, "fwd")],
           "dgrad": [M.backward_data(c.shape, ws) for _, ws in R.data_ws_modes(c.shape, "dgrad")]}
    wws = M.wgrad_workspace_bytes(c.shape)
    out["wgrad"] = [M.backward_weight(c.shape, wws, True), M.backward_weight(c.shape, wws, False)]
    return out


@pytest.mark.parametrize("c", ALL, ids=_id)
def test_every_case_takes_the_route_it_claims(c):
    ring3 = c in R.RING3_CASES
    got = mirror_routes(c, 3 if ring3 else 1)
    for direction, claim in (("fwd", c.fwd), ("dgrad", c.dgrad), ("wgrad", c.wgrad)):
        if claim is not None:
            assert got[direction][0] is not None and got[direction][0][0] == claim, (direction, got[direction][0])
        else:
            assert got[direction][0] is not None        # in the domain all the same
    fwd = c.fwd or got["fwd"][0][0]
    if fwd.startswith("igemm"):                         # NULL and one byte short: the same tile, unsplit
        assert {r[0] for r in got["fwd"][1:]} <= {fwd.split("/")[0] + "/S1"}
        assert {r[0] for r in got["dgrad"][1:]} <= {got["dgrad"][0][0].split("/")[0] + "/S1"}
    else:
        assert {r[0] for r in got["fwd"]} == {fwd}
    if ring3:                                           # without the switch the 3x3 shapes stay on conv_bf16_igemm
        assert M.forward(c.shape, M.data_workspace_bytes(c.shape), True, 1)[0].startswith("igemm")
    assert got["wgrad"][1][0].startswith("wgrad_tap<%d,%d>" % (c.R, c.stride))    # dw off a 16-byte boundary


def test_refused_shapes_are_outside_the_mirrors_domain():
    for shape in R.REFUSED:
        for ws in (0, 1 << 30):
            assert M.forward(shape, ws) is None and M.backward_data(shape, ws) is None, shape
            assert M.backward_weight(shape, ws) is None and M.backward_weight(shape, ws, False) is None, shape
    for shape in R.SHORT_WS:
        wws = M.wgrad_workspace_bytes(shape)
        assert M.backward_weight(shape, wws - 1) == M.ENOSPC and M.backward_weight(shape, wws) not in (None, M.ENOSPC)
    assert {M.backward_weight(s, M.wgrad_workspace_bytes(s))[0].split("<")[0] for s in R.SHORT_WS} == {"wgrad_tap", "wgrad_tn"}


REQUIRED = [
    "igemm<2,2,32>/S1", "igemm<2,2,32>/S3", "igemm<2,2,32>/S4", "igemm<2,2,32>/S15", "igemm<2,4,32>/S1", "igemm<2,4,32>/S3",
    "igemm<2,2,32,dgrad>/S1", "igemm<2,2,32,dgrad>/S3", "igemm<2,2,32,dgrad>/S4", "igemm<2,2,32,dgrad>/S15",
    "igemm<2,4,32,dgrad>/S1", "igemm<2,4,32,dgrad>/S3", "igemm<2,2,32>/S2",
    "wgrad_tap<3,1>/S1", "wgrad_tap<3,2>/S1", "wgrad_tap<1,1>/S1", "wgrad_tap<1,2>/S1",
    "wgrad_tap<3,1>/S11", "wgrad_tap<3,2>/S2", "wgrad_tap<1,1>/S2", "wgrad_tap<1,2>/S3",
    "wgrad_tn<v2>/S1", "wgrad_tn<v2>/S4", "ring<4,2,3>", "ring<4,1,3>", "ring<2,2,4>",
]


def test_cases_reach_every_route_the_suite_is_there_for():
    claimed = {label for c in R.CASES for label in (c.fwd, c.dgrad, c.wgrad) if label}
    assert not [r for r in REQUIRED if r not in claimed]
    assert {c.fwd for c in R.RING3_CASES} == {"ring<4,2,3>", "ring<4,1,3>", "ring<2,2,4>"}
    assert any(c.stride == 2 for c in R.RING3_CASES) and all(c.R == 3 for c in R.RING3_CASES)
    small = [c for c in R.CASES if c.dgrad]
    # 3x3 at pad 0, 1, 2 x stride 1, 2; 1x1 at stride 1, 2; H != W; one pixel; several images per pixel tile; N no divisor of 128
    assert {(c.R, c.stride, c.pad) for c in small} == {(3, s, p) for s in (1, 2) for p in (0, 1, 2)} | {(1, 1, 0), (1, 2, 0)}
    assert sum(c.H != c.W for c in small) >= 10 and any(c.H == c.W == 1 and c.pad == 1 for c in small)
    assert any(c.H < c.R and c.W < c.R for c in small) and any(c.stride == 2 and c.H % 2 and not c.W % 2 for c in small)
    assert any(c.N == 3 and c.OH * c.OW < 128 and c.fwd.startswith("igemm") for c in small)
    # the ragged splits: 27 stages in 7, 7, 7, 6; 99 stages in 15 splits of 7 with one stage left for the last
    assert M.plan_split(1, 27) == (4, 7) and M.plan_split(6, 99) == (15, 7)
    # the ring cases sit at the threshold: one pixel tile fewer and the form is gone
    for c in R.CASES[-3:] + R.RING3_CASES:
        m = c.N * c.OH * c.OW
        wgm = int(c.fwd[5])
        assert m % (64 * wgm), c                        # ragged last pixel tile
        assert M.ring_form(m - m % (64 * wgm), c.C, c.K, c.R, True, 3) != tuple(int(v) for v in c.fwd[5:-1].split(",")), c


# ------------------------------------------------------------------------------------------ the library's host-only queries
@pytest.fixture(scope="module")
def L():
    from unlearn_saliency_amd import _lib
    _lib.build()
    return _lib.lib()


def lib_route(L, direction, shape, flags=0, ws_bytes=0):
    buf, ns = ctypes.create_string_buffer(64), ctypes.c_int(-1)
    rc = L.salun_conv2d_bf16_route(direction, *shape, flags, ws_bytes, buf, 64, ctypes.byref(ns))
    return None if rc == EINVAL else M.ENOSPC if rc == ENOSPC else (buf.value.decode(), ns.value)


def test_library_queries_agree_with_the_mirror_on_every_variant(L):
    for c in ALL:
        ring = 3 if c in R.RING3_CASES else 1
        assert L.salun_conv2d_bf16_data_workspace_bytes(*c.shape) == M.data_workspace_bytes(c.shape), c
        wws = L.salun_conv2d_bf16_wgrad_workspace_bytes(*c.shape)
        assert wws == M.wgrad_workspace_bytes(c.shape), c
        for _, ws in R.data_ws_modes(c.shape, "fwd"):
            assert lib_route(L, FWD, c.shape, ring_bits(ring), ws) == M.forward(c.shape, ws, True, ring), (c, ws)
        for _, ws in R.data_ws_modes(c.shape, "dgrad"):
            assert lib_route(L, DGRAD, c.shape, 0, ws) == M.backward_data(c.shape, ws), (c, ws)
        for aligned in (True, False):
            assert lib_route(L, WGRAD, c.shape, 0 if aligned else UNALIGNED, wws) == M.backward_weight(c.shape, wws, aligned), c
    for shape in R.REFUSED:
        for direction in (FWD, DGRAD, WGRAD):
            assert lib_route(L, direction, shape, 0, 1 << 30) is None, (shape, direction)
    for shape in R.SHORT_WS:
        assert lib_route(L, WGRAD, shape, 0, L.salun_conv2d_bf16_wgrad_workspace_bytes(*shape) - 1) == M.ENOSPC
