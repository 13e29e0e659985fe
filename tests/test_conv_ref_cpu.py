"""The float64 convolution model of conv_ref_cpu.py against torch's float64 convolution, the premise of the exact tier
(every partial sum of every integer case below 2^24 units), and the route mirror of conv_routes.py: checked against the
library's host-side queries, and shown to reach, over conv_ref_cpu.CASES, every kernel variant the fp32 convolution
family can pick.  No GPU."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import conv_ref_cpu as R
import conv_routes as M

ODD = [R.Case(*s) for s in [(2, 3, 7, 5, 4, 3, 1, 1), (2, 5, 9, 6, 3, 3, 2, 1), (3, 2, 5, 7, 6, 1, 2, 0),
                            (1, 4, 6, 10, 2, 3, 2, 0), (2, 3, 5, 5, 2, 1, 1, 0), (1, 2, 11, 4, 3, 3, 2, 1)]]
SMALL = [c for c in R.CASES if c.N * c.K * c.P * c.Q * c.C * c.R * c.R <= 10 ** 8]
DIRECTIONS = ("fwd", "dgrad", "wgrad")


def _hi(c):
    """High-side padding (negative: rows / columns no output reads) that makes a pad-0 torch convolution give P x Q."""
    return (c.P - 1) * c.stride + c.R - c.pad - c.H, (c.Q - 1) * c.stride + c.R - c.pad - c.W


def torch_forward(c, x, w):
    hh, hw = _hi(c)
    return F.conv2d(F.pad(x, (c.pad, hw, c.pad, hh)), w, None, c.stride, 0)


def torch_backward_data(c, dy, w):
    hh, hw = _hi(c)
    Hp, Wp = c.pad + c.H + hh, c.pad + c.W + hw
    g = torch.nn.grad.conv2d_input((c.N, c.C, Hp, Wp), w, dy, c.stride, 0)
    full = torch.zeros(c.N, c.C, max(Hp, c.pad + c.H), max(Wp, c.pad + c.W), dtype=torch.float64)
    full[:, :, :Hp, :Wp] = g
    return full[:, :, c.pad:c.pad + c.H, c.pad:c.pad + c.W]


def torch_backward_weight(c, x, dy):
    hh, hw = _hi(c)
    return torch.nn.grad.conv2d_weight(F.pad(x, (c.pad, hw, c.pad, hh)), (c.K, c.C, c.R, c.R), dy, c.stride, 0)


def _close(got, want, exact):
    assert got.shape == want.shape
    if exact:
        assert torch.equal(got, want)
    else:
        assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-300)


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("c", SMALL + ODD, ids=lambda c: c.id)
def test_model_agrees_with_torch_float64(c, kind):
    exact = kind == "int"
    t = R.inputs(c, "fwd", kind)
    conv = torch_forward(c, t.x, t.w)
    _close(R.forward(t.x, t.w, c.stride, c.pad, c.P, c.Q), conv, exact)
    want = ((conv + t.bias[None, :, None, None]) + t.nbias[:, :, None, None]) + t.addend
    _close(R.forward(t.x, t.w, c.stride, c.pad, c.P, c.Q, t.bias, t.nbias, t.addend), want, exact)
    t = R.inputs(c, "dgrad", kind)
    dx = torch_backward_data(c, t.dy, t.w)
    _close(R.backward_data(t.dy, t.w, (c.N, c.C, c.H, c.W), c.stride, c.pad), dx, exact)
    _close(R.backward_data(t.dy, t.w, (c.N, c.C, c.H, c.W), c.stride, c.pad, t.addend), dx + t.addend, exact)
    t = R.inputs(c, "wgrad", kind)
    dw = torch_backward_weight(c, t.x, t.dy)
    _close(R.backward_weight(t.x, t.dy, c.R, c.stride, c.pad), dw, exact)
    _close(R.backward_weight(t.x, t.dy, c.R, c.stride, c.pad, t.dw0), dw + t.dw0, exact)


def test_abs_sum_is_the_sum_of_absolute_terms():
    c = ODD[1]
    t = R.inputs(c, "fwd", "gauss")
    a = R.forward(t.x, t.w, c.stride, c.pad, c.P, c.Q, t.bias, t.nbias, t.addend, absolute=True)
    want = torch_forward(c, t.x.abs(), t.w.abs()) + t.bias.abs()[None, :, None, None] + t.nbias.abs()[:, :, None, None] \
        + t.addend.abs()
    _close(a, want, False)
    assert (a >= R.forward(t.x, t.w, c.stride, c.pad, c.P, c.Q, t.bias, t.nbias, t.addend).abs()).all()
    assert R.bound_gamma(1) == 2.0 ** -24 / (1 - 2.0 ** -24) and R.bound_gamma(4608) < 4608 * 2.0 ** -24 * 1.001


def abs_sums(c, direction, kind):
    t = R.inputs(c, direction, kind)
    if direction == "fwd":
        return t, R.forward(t.x, t.w, c.stride, c.pad, c.P, c.Q, t.bias, t.nbias, t.addend, absolute=True)
    if direction == "dgrad":
        return t, R.backward_data(t.dy, t.w, (c.N, c.C, c.H, c.W), c.stride, c.pad, t.addend, absolute=True)
    return t, R.backward_weight(t.x, t.dy, c.R, c.stride, c.pad, t.dw0, absolute=True)


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.id)
def test_exact_tier_premise_every_partial_sum_below_2_to_24_units(c, direction):
    """The cap is a condition, not a measurement: with every term an integer multiple of the element's unit and the sum
    of their magnitudes below 2^24 units, every fp32 partial sum in every order is exact."""
    t, a = abs_sums(c, direction, "int")
    lg = torch.log2(t.unit)
    assert torch.equal(lg, lg.round()) and float(lg.abs().max()) <= 20
    units = a / t.unit
    assert torch.equal(units, units.round()), "a term is not a whole multiple of its element's unit"
    assert float(units.max()) < 2 ** 24


def test_scales_are_powers_of_two_within_2_to_the_20():
    for n, e in itertools.product((1, 3, 130), (R.IMG_EXP, R.CH_EXP)):
        s = torch.log2(R.scales(n, e))
        assert torch.equal(s, s.round()) and float(s.abs().max()) <= 20
    x = R.integers((5, 4, 2, 2), -3, 3, 1, R.IMG_EXP, R.CH_EXP)
    assert float(x.abs().max()) <= 3 * 2 ** 10 and torch.equal(x[3], x[3].round()) and float(x[0, 0].abs().max()) <= 3


# ------------------------------------------------------------------------------------------ the route mirror
def _lib():
    from unlearn_saliency_amd import _lib
    _lib.build()
    return _lib.lib()


def test_mirror_agrees_with_the_library_queries_on_the_cases():
    L = _lib()
    for c in R.CASES:
        assert L.salun_conv2d_data_workspace_bytes(c.N, c.K, c.P, c.Q, c.R, c.stride) == \
            M.data_ws_bytes(c.N, c.K, c.P, c.Q, c.R, c.stride), c
        assert L.salun_conv2d_data_workspace_bytes(c.N, c.C, c.H, c.W, c.R, 1) == M.data_ws_bytes(c.N, c.C, c.H, c.W, c.R, 1), c
        assert L.salun_conv2d_wgrad_workspace_bytes(c.N, c.C, c.K, c.R, c.P, c.Q) == M.wgrad_ws_bytes(c), c
        # a workspace is offered exactly where a launch may be split; nsplit never exceeds what the query sized
        for label, nbytes in ((M.forward(c, ws=True), M.data_ws_bytes(c.N, c.K, c.P, c.Q, c.R, c.stride)),
                              (M.backward_data(c, ws=True), M.data_ws_bytes(c.N, c.C, c.H, c.W, c.R, 1))):
            if label and label.startswith("igemm") and "/S1" not in label:
                assert nbytes > 0, (c, label)
        for shared in (False, True):
            route, ns = M.backward_weight(c, shared)
            assert 4 * ns * c.K * c.C * c.R * c.R <= M.wgrad_ws_bytes(c), (c, route)
    for N, C, H, W, K in R.RING_CASES:
        for dgrad in (0, 1):
            assert L.salun_conv3x3_pack_bytes(K, C, dgrad) == M.ring_pack_bytes(K, C, dgrad)


def test_mirror_agrees_with_the_library_queries_on_a_sweep():
    L = _lib()
    n = 0
    for N, C, K, H, W, (Rr, s) in itertools.product((1, 2, 3, 5, 24, 128), (3, 8, 64, 130), (3, 32, 64, 72, 130),
                                                     (1, 2, 3, 4, 12, 16, 64), (1, 2, 4, 6, 8, 32, 128, 256),
                                                     ((1, 1), (1, 2), (3, 1), (3, 2))):
        assert L.salun_conv2d_data_workspace_bytes(N, K, H, W, Rr, s) == M.data_ws_bytes(N, K, H, W, Rr, s)
        c = R.Case(N, C, H * s, W * s, K, Rr, s, Rr // 2)
        assert L.salun_conv2d_wgrad_workspace_bytes(N, C, K, Rr, c.P, c.Q) == M.wgrad_ws_bytes(c), c
        assert L.salun_conv3x3_pack_bytes(K, C, N & 1) == M.ring_pack_bytes(K, C, N & 1)
        n += 1
    assert n > 10000


# ------------------------------------------------------ the mirror against the plan the library launches from
FWD, DGRAD, WGRAD = 0, 1, 2                                       # SALUN_ROUTE_*
SHARED, EPI, W_UNAL, OUT_UNAL = 1, 2, 4, 8                        # SALUN_WGRAD_SHARED, SALUN_ROUTE_* flags
AMPLE = 1 << 40                                                   # a backward-weight workspace that is never too small


def lib_route(L, direction, c, flags=0, ws_bytes=0):
    """salun_conv2d_route -> (label or None for SALUN_EINVAL, nsplit)."""
    import ctypes
    buf, ns = ctypes.create_string_buffer(256), ctypes.c_int(-1)
    rc = L.salun_conv2d_route(direction, c.N, c.C, c.H, c.W, c.K, c.R, c.stride, c.pad, c.P, c.Q, flags, ws_bytes, buf,
                              len(buf), ctypes.byref(ns))
    assert rc in (0, -22), (rc, c)
    assert (rc == 0) == bool(buf.value), (rc, buf.value, c)
    return (buf.value.decode() if rc == 0 else None), ns.value


def assert_routes_agree(L, c, variants=True):
    two = (False, True) if variants else (False,)
    fwd_ws = L.salun_conv2d_data_workspace_bytes(c.N, c.K, c.P, c.Q, c.R, c.stride)
    dg_ws = L.salun_conv2d_data_workspace_bytes(c.N, c.C, c.H, c.W, c.R, 1) if c.stride == 1 else 0
    for epi, ws, unal in itertools.product(two, (False, True), two):
        got, _ = lib_route(L, FWD, c, EPI * epi | W_UNAL * unal, fwd_ws if ws else 0)
        assert got == M.forward(c, epi=epi, ws=ws and fwd_ws > 0, w_al=not unal), ("fwd", c, epi, ws, unal)
    for ws, unal, out_unal in itertools.product((False, True), two, two):
        got, _ = lib_route(L, DGRAD, c, W_UNAL * unal | OUT_UNAL * out_unal, dg_ws if ws else 0)
        assert got == M.backward_data(c, ws=ws and dg_ws > 0, w_al=not unal, al=not out_unal), ("dgrad", c, ws, unal, out_unal)
    for shared in (False, True):
        assert lib_route(L, WGRAD, c, SHARED * shared, AMPLE) == M.backward_weight(c, shared), ("wgrad", c, shared)


def test_mirror_agrees_with_the_library_plans_on_the_cases():
    """Every case, in every combination test_conv_exact_gpu.py calls it with: the label of the plan the library would
    execute equals the mirror's, None exactly where the library answers SALUN_EINVAL, and the backward-weight split
    counts are equal."""
    L = _lib()
    for c in R.CASES:
        assert_routes_agree(L, c)


def test_mirror_agrees_with_the_library_plans_on_a_sweep():
    L = _lib()
    n = 0
    for N, C, K, H, W, (Rr, s) in itertools.product((1, 2, 3, 5, 24, 128), (3, 8, 64, 130), (3, 32, 64, 72, 130),
                                                     (1, 2, 3, 4, 12, 16, 64), (1, 2, 4, 6, 8, 32, 128, 256),
                                                     ((1, 1), (1, 2), (3, 1), (3, 2))):
        assert_routes_agree(L, R.Case(N, C, H * s, W * s, K, Rr, s, Rr // 2), variants=False)
        n += 1
    assert n > 10000


# every row of the route table: the variants plan_data, plan_dgrad_s2, plan_wgrad and ring_launch choose
# among.  (Ring tile 4 is absent: its domain is empty, see test_ring_tile_4_has_an_empty_domain.)
REQUIRED = [
    "igemm<3,1>/64/KT1WK2/fast/S1", "igemm<3,1>/64/KT1WK2/fast/S2", "igemm<3,1>/64/KT1WK2/fast/S8",
    "igemm<3,1>/64/KT1WK2/fast/S1/epi", "igemm<3,1>/64/KT1WK2/fast/S2/epi", "igemm<3,1>/64/KT1WK2/fast/S8/epi",
    "igemm<3,1,dgrad>/64/KT1WK2/fast/S1", "igemm<3,1,dgrad>/64/KT1WK2/fast/S2",
    "igemm<1,1>/64/KT1WK2/fast/S1/hw-declined",
    "igemm<3,1>/64/KT1WK2/slow/S1", "igemm<3,1,dgrad>/64/KT1WK2/slow/S1", "igemm<3,1,dgrad>/128/KT1/slow/S1",
    "igemm<3,1>/128/KT4/fast/S1", "igemm<3,1>/128/KT2/fast/S1", "igemm<3,1>/128/KT1/fast/S1", "igemm<3,1>/256/PT2/fast/S1",
    "igemm<3,1>/128/KT4/fast/S1/epi", "igemm<3,1>/128/KT2/fast/S1/epi", "igemm<3,1>/128/KT1/fast/S1/epi",
    "igemm<3,1>/64/KT2WK2/fast/S1", "igemm<3,1>/64/KT2WK2/fast/S1/epi",
    "igemm<1,1>/64/KT1WK2/fast/S1", "igemm<1,1>/64/KT1WK2/fast/S1/epi", "igemm<1,1>/128/KT4/fast/S1",
    "igemm<1,1>/64/KT1WK2/slow/S1", "igemm<1,1,dgrad>/64/KT1WK2/slow/S1",
    "igemm<3,2>/64/KT1WK2/fast/S1", "igemm<3,2>/64/KT1WK2/fast/S2", "igemm<3,2>/64/KT1WK2/slow/S1",
    "igemm<1,2>/64/KT1WK2/fast/S1", "igemm<1,2>/64/KT1WK2/slow/S1", "igemm<3,2>/128/KT4/fast/S1",
    "dgrad_s2<3,pad1>/64/KT1WK2", "dgrad_s2<3,pad0>/64/KT1WK2", "dgrad_s2<3,pad1>/128/KT2", "dgrad_s2<3,pad1>/128/KT1",
    "dgrad_s2<3,pad1>/64/KT2WK2", "dgrad_s2<1,pad0>/64/KT1WK2",
    "dgrad_tap[<1,1>/64/KT1WK2 <1,2>/64/KT1WK2 <2,1>/64/KT1WK2 <2,2>/64/KT1WK2]",
    "dgrad_tap[<2,2>/64/KT1WK2 <2,1>/64/KT1WK2 <1,2>/64/KT1WK2 <1,1>/64/KT1WK2]",
    "dgrad_tap[<1,1>/64/KT1WK2]/empty", "dgrad_tap[<1,1>/128/KT1 <1,2>/128/KT1 <2,1>/128/KT1 <2,2>/128/KT1/P3]",
    "wgrad_1x1<1>", "wgrad_1x1<2>", "wgrad<1,1,false>", "wgrad<1,2,false>",
    "wgrad_smallc<3,1>", "wgrad_smallc<3,2>", "wgrad_smallc<1,1>", "wgrad_smallc<1,2>",
    "wgrad_ring<W4>", "wgrad_ring<W8>", "wgrad_ring<W16>", "wgrad_ring<W32>",
    "wgrad_v<1,5>", "wgrad_v<1,6>", "wgrad_v<1,8>", "wgrad_v<2,9>", "wgrad_v<2,10>",
    "wgrad<3,1,true>", "wgrad<3,1,false>", "wgrad<3,2,true>", "wgrad<3,2,false>",
] + [f"ring<W{w},cfg{cfg}>" for w in (4, 8, 16, 32) for cfg in (1, 2, 3, 5)] \
  + [f"ring<W{w},cfg{cfg}>/NI" for w in (4, 8, 16, 32) for cfg in (1, 2, 3)] + ["ring<W8,cfg5>/NI"]


def routes_of_the_cases():
    seen = set()
    for c in R.CASES:
        for ws, epi in itertools.product((False, True), (False, True)):
            seen.add(M.forward(c, epi=epi, ws=ws))
        seen |= {M.backward_data(c, ws=False), M.backward_data(c, ws=True)}
        seen |= {M.backward_weight(c)[0], M.backward_weight(c, shared=True)[0]}
    for rc in R.RING_CASES:
        seen |= {M.ring(*rc, cfg) for cfg in M.RING_TILES}
    return seen


def test_cases_reach_every_route_of_the_table():
    seen = routes_of_the_cases()
    assert not [r for r in REQUIRED if r not in seen]
    assert None in seen                                    # refusals are exercised too
    # several images per tile with a ragged last tile, in the 64-pixel forward tiling and in the backward-weight chunk
    ragged = [c for c in R.CASES if (g := M.geom(c.N, c.P, c.Q, 64, c.stride, c.R)) and g.NI > 1 and c.N % g.NI]
    assert {g.NI for c in ragged if (g := M.geom(c.N, c.P, c.Q, 64, c.stride, c.R))} >= {2, 4, 16}
    # H != W in every family: forward / backward-data tiles, the merged and per-class stride-2 kernels, backward-weight
    for prefix in ("igemm<3,1>", "igemm<1,1>", "igemm<3,2>", "dgrad_s2", "dgrad_tap", "wgrad_v", "wgrad<", "wgrad_1x1",
                   "wgrad_smallc"):
        assert any(c.H != c.W and any((r or "").startswith(prefix) for r in
                                      (M.forward(c), M.backward_data(c), M.backward_weight(c)[0])) for c in R.CASES), prefix
    assert any(rc[2] != rc[3] for rc in R.RING_CASES)
    # more tiles than the persistent grid of the ring kernel (2 workgroups on each of at most 256 CUs) at cfg 3
    assert any(N * H * W // 64 * M._cdiv(K, 64) > 512 for N, C, H, W, K in R.RING_CASES)


def test_ring_tile_4_has_an_empty_domain():
    """128 pixels x 128 channels needs 2 * (36 KiB of weights + the patch) <= 80 KiB of LDS, i.e. a patch of <= 128 floats
    per channel; a 128-pixel tile with its two halo rows per image is 128 + 2 * NI * W > 128.  The host refuses every
    shape (the mirror over a sweep, the library itself in test_conv_exact_gpu.py)."""
    for N, H, W in itertools.product((1, 2, 3, 8, 64), range(1, 130), (4, 8, 16, 32)):
        assert M.ring(N, 8, H, W, 64, 4) is None
