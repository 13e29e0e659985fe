"""The route mirror of bf16_routes.py (written from the host code before the plans moved into csrc/salun_bf16_plan.h)
against the library's host-only queries salun_conv2d_bf16_route / salun_gemm_bf16_route, its workspace queries and its
*_supported queries: on the shapes the GPU tests of K11 and K16 run, and on a sweep; and the routes those GPU tests'
comments claim, as a list the named cases must reach.  No GPU."""
import ctypes
import itertools

import pytest

import bf16_routes as M
import gemm_bf16_ref_cpu as GB
import test_conv_bf16_gpu as TC
import test_gemm_bf16_gpu as TG

FWD, DGRAD, WGRAD = 0, 1, 2           # SALUN_ROUTE_FORWARD / _BACKWARD_DATA / _BACKWARD_WEIGHT
UNALIGNED = 8                         # SALUN_ROUTE_OUT_UNALIGNED
NT, TN = 0, 1                         # SALUN_GEMM_BF16_NT / _TN
EINVAL, ENOSPC = -22, -28
ring_bits = lambda v: (v + 1) << 8    # SALUN_ROUTE_RING(v)
tn_bits = lambda v: (v + 1) << 12     # SALUN_ROUTE_WGRAD_TN(v)


def _params(fn):
    return [m for m in fn.pytestmark if m.name == "parametrize"]


def _as_tokens(m_shape, C, K):
    """conv_bf16._tokens_nhwc: a Linear layer's tokens as the pixels of one image"""
    m = 1
    for d in m_shape:
        m *= d
    return (1, m // 8, 8, C, K, 1, 1, 0) if m % 8 == 0 else (1, m, 1, C, K, 1, 1, 0)


EPILOGUE = [(N, H, W, C, K, 3, 1, 1) for N, H, W, C, K in _params(TC.test_epilogue_terms)[0].args[1]]
LINEAR = [_as_tokens(ms, C, K) for ms, C, K, _ in _params(TC.test_linear_on_the_1x1_kernels_matches_fp32_linear)[0].args[1]]
WGRAD_DIMS = [(N, H, W, C, K, R, 1, R // 2)
              for N, H, W, C, K, R in _params(TC.test_per_image_channel_sums_ride_on_the_bias_gradient)[0].args[1]]
# what no GPU case above reaches: the 1x1 stride-2 tap kernel, the smallest shape of the TN route, and refusals (the RGB-like
# stem of test_unsupported_shapes_are_refused, a filter of 5)
EXTRA = [(2, 16, 16, 64, 64, 1, 2, 0), (1, 32, 32, 64, 64, 1, 1, 0), (1, 33, 31, 64, 64, 1, 1, 0), (2, 8, 8, 4, 320, 3, 1, 1),
         (2, 8, 8, 64, 64, 5, 1, 2)]
CONV_CASES = list(dict.fromkeys(TC.SHAPES + EPILOGUE + LINEAR + WGRAD_DIMS + EXTRA))
NT_CASES = list(_params(TG.test_gemm_bf16_nt_matches_fp32_matmul_of_the_rounded_operands)[0].args[1]) + \
    [(4096, 640, 320), (4096, 320, 320), (128, 96, 64), (128, 64, 40)]   # test_variants_agree_bitwise_and_shapes_outside_...
TN_CASES = list(_params(TG.test_gemm_bf16_tn_weight_gradient_matches_fp32_matmul_of_the_rounded_operands)[0].args[1]) + \
    [(512, 640, 320), (64, 48, 32)]
# the shapes of the exact-answer tests of K16 (gemm_bf16_ref_cpu.py), refusals included
NT_CASES = list(dict.fromkeys(NT_CASES + [(c.M, c.N, c.K) for c in GB.NT_CASES] + [r[:3] for r in GB.NT_REFUSED] + GB.AGREE))
TN_CASES = list(dict.fromkeys(TN_CASES + [(c.M, c.Na, c.Nb) for c in GB.TN_CASES] + [r[:3] for r in GB.TN_REFUSED]))

CHANNELS = [32, 64, 96, 160, 256, 320, 640, 1280, 2560]
FILTERS = [(1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1), (3, 1, 0), (3, 1, 2)]
# pixel counts on both sides of: one tile, the split target (768 / tiles), 128 ring tiles, 1024 tokens (TN), the chunk
# count of backward-weight, 2^24 pixels, 2^31 elements and bytes; empty batches and extents
PIXELS = [(1, 1, 1), (1, 2, 2), (1, 5, 7), (2, 8, 8), (1, 9, 9), (1, 16, 16), (3, 16, 16), (1, 33, 31), (1, 32, 32),
          (2, 32, 32), (8, 16, 16), (48, 8, 8), (128, 4, 4), (8, 32, 32), (2, 64, 64), (4, 64, 64), (5, 62, 62), (8, 64, 64),
          (16, 64, 64), (64, 64, 64), (4, 128, 128), (2, 2048, 2048), (1, 4095, 4096), (1, 4096, 4096), (0, 8, 8), (1, 0, 5)]
CONV_SWEEP = [(N, H, W, C, K, R, s, p) for (N, H, W), C, K, (R, s, p) in itertools.product(PIXELS, CHANNELS, CHANNELS, FILTERS)]
CONV_SWEEP += [(2, 16, 16, C, K, R, s, p) for C, K, (R, s, p) in
               itertools.product([0, 8, 48, 64], [16, 40, 64], FILTERS + [(5, 1, 2), (3, 3, 1), (3, 1, 3), (1, 1, 1), (2, 1, 0)])]
NT_SWEEP = list(itertools.product([0, 1, 77, 255, 256, 257, 1000, 4096, 8192, 16383, 16384, 16385, 32768, 2 ** 24, 2 ** 25],
                                  [32, 64, 96, 128, 192, 256, 320, 640, 1280, 2560, 5120], [40, 64, 320, 768, 1280, 2 ** 20]))
TN_SWEEP = list(itertools.product([0, 1, 33, 255, 256, 511, 512, 1023, 1024, 4096, 32768, 2 ** 21, 2 ** 24 - 1, 2 ** 24],
                                  CHANNELS + [16, 48], CHANNELS + [48]))


@pytest.fixture(scope="module")
def L():
    from unlearn_saliency_amd import _lib
    _lib.build()
    return _lib.lib()


def _answer(rc, buf, ns):
    if rc == EINVAL:
        return None
    if rc == ENOSPC:
        return M.ENOSPC
    assert rc == 0, rc
    return buf.value.decode(), ns.value


def conv_route(L, direction, shape, flags=0, ws_bytes=0):
    buf, ns = ctypes.create_string_buffer(64), ctypes.c_int(-1)
    return _answer(L.salun_conv2d_bf16_route(direction, *shape, flags, ws_bytes, buf, 64, ctypes.byref(ns)), buf, ns)


def gemm_route(L, op, m, n, k, variant=0, ws_bytes=0):
    buf, ns = ctypes.create_string_buffer(64), ctypes.c_int(-1)
    return _answer(L.salun_gemm_bf16_route(op, m, n, k, variant, ws_bytes, buf, 64, ctypes.byref(ns)), buf, ns)


def _check_conv(L, shape, seen=None):
    """Mirror == query in every direction: with the queried workspace, without one and one byte short; aligned and not;
    under every override of the two switches.  Also what the workspace queries promise."""
    N, H, W, C, K, R, stride, pad = shape
    assert bool(L.salun_conv2d_bf16_supported(C, K, R, stride, pad)) == M.conv_supported(C, K, R, stride, pad), shape
    dws = L.salun_conv2d_bf16_data_workspace_bytes(*shape)
    assert dws == M.data_workspace_bytes(shape), shape
    got = []
    for ws in {0, dws, max(dws - 1, 0)}:
        for al, ring in itertools.product((True, False), (0, 1, 2, 3)):
            g = conv_route(L, FWD, shape, (0 if al else UNALIGNED) | ring_bits(ring), ws)
            assert g == M.forward(shape, ws, al, ring), (shape, ws, al, ring, g)
            got.append(("fwd", g))
        g = conv_route(L, DGRAD, shape, 0, ws)
        assert g == M.backward_data(shape, ws), (shape, ws, g)
        got.append(("dgrad", g))
    assert conv_route(L, FWD, shape, 0, dws) == M.forward(shape, dws, True, 1)  # no override bit: the default switches
    # a split plan fits the workspace the query sized: splits x fp32 copies of the output
    OH, OW = M._out(H, R, stride, pad), M._out(W, R, stride, pad)
    for (what, g), out in zip((("fwd", conv_route(L, FWD, shape, ring_bits(0), dws)), ("dgrad", conv_route(L, DGRAD, shape, 0, dws))),
                              (N * OH * OW * K, N * H * W * C)):
        if g and g[1] > 1:
            assert g[1] * out * 4 <= dws, (shape, what, g)
    for tn in (0, 1):
        wws = M.wgrad_workspace_bytes(shape, tn)
        if tn == 1:
            assert L.salun_conv2d_bf16_wgrad_workspace_bytes(*shape) == wws, shape
        for ws, al in itertools.product({0, wws, max(wws - 1, 0)}, (True, False)):
            g = conv_route(L, WGRAD, shape, (0 if al else UNALIGNED) | tn_bits(tn), ws)
            assert g == M.backward_weight(shape, ws, al, tn), (shape, ws, al, tn, g)
            got.append(("wgrad", g))
            if g and g != M.ENOSPC:
                # [GEMM or tap partials | 128 x K column-sum partials] from the plan's own split: inside the queried size
                label, ns = g
                off = ns * R * R * K * C * 4 if label.startswith("wgrad_tap") else ((ns * K * C * 4 if ns > 1 else 0) + 255) & ~255
                assert (off, off + 128 * K * 4) == M.wgrad_layout(shape, al, tn) and off + 128 * K * 4 <= wws, (shape, g)
    assert conv_route(L, WGRAD, shape, 0, wws) == M.backward_weight(shape, wws, True, 1)
    if seen is not None:
        seen.update(got)


def _check_gemm(L, nt_shapes, tn_shapes, seen=None):
    for m, n, k in nt_shapes:
        assert bool(L.salun_gemm_bf16_supported(m, n, k)) == M.nt_supported(m, n, k), (m, n, k)
        for v in range(-1, 16):
            g = gemm_route(L, NT, m, n, k, v)
            assert g == M.gemm_nt(m, n, k, v), (m, n, k, v, g)
            if seen is not None:
                seen.add(("nt", g))
    for m, na, nb in tn_shapes:
        assert bool(L.salun_gemm_bf16_tn_supported(m, na, nb)) == M.tn_supported(m, na, nb), (m, na, nb)
        for v in range(-1, 5):
            ws = L.salun_gemm_bf16_tn_workspace_bytes(m, na, nb, v) if 0 <= v <= 3 else 0
            assert ws == (M.tn_workspace_bytes(m, na, nb, v) if 0 <= v <= 3 else 0), (m, na, nb, v)
            for w in {0, ws, max(ws - 1, 0)}:
                g = gemm_route(L, TN, m, na, nb, v, w)
                assert g == M.gemm_tn(m, na, nb, v, w), (m, na, nb, v, w, g)
                if seen is not None:
                    seen.add(("tn", g))


@pytest.fixture(scope="module")
def seen(L):
    s = set()
    for shape in CONV_CASES:
        _check_conv(L, shape, s)
    _check_gemm(L, NT_CASES, TN_CASES, s)
    return s


def test_mirror_agrees_with_the_library_queries_on_the_named_cases(seen):
    assert seen


def test_mirror_agrees_with_the_library_queries_on_a_sweep(L):
    assert len(CONV_SWEEP) >= 10000
    for shape in CONV_SWEEP:
        _check_conv(L, shape)
    _check_gemm(L, NT_SWEEP, TN_SWEEP)
    refused = sum(M.forward(s, 0, True, 1) is None for s in CONV_SWEEP)
    assert 1000 < refused < len(CONV_SWEEP) - 5000  # both sides of the domain


# (family, label prefix, split?) - a label of that family starts with the prefix and (split is None or (nsplit > 1) == split)
REQUIRED = [
    # every row of the igemm tile choice of a default build, forward and backward-data, split and unsplit
    *[(d, "igemm<%s,32%s>/" % (t, ",dgrad" if d == "dgrad" else ""), s)
      for d in ("fwd", "dgrad") for t in ("2,2", "2,4") for s in (True, False)],
    # the three ring tile forms
    ("fwd", "ring<4,2,3>", None), ("fwd", "ring<4,1,3>", None), ("fwd", "ring<2,2,4>", None),
    # the four tap kernels, split and straight into dw; the TN route
    ("wgrad", "wgrad_tap<3,1>/", True), ("wgrad", "wgrad_tap<3,2>/", True), ("wgrad", "wgrad_tap<1,1>/", False),
    ("wgrad", "wgrad_tap<1,2>/", None), ("wgrad", "wgrad_tap<3,1>/", False), ("wgrad", "wgrad_tn<v2>/", True),
    # all 13 NT rows, the three TN variants
    *[("nt", M.NT_ARMS[v][0], None) for v in range(1, 14)],
    ("tn", "tn<v1>/", True), ("tn", "tn<v2>/", True), ("tn", "tn<v3>/", True), ("tn", "tn<v2>/S1", False),
]


def _reached(seen, family, prefix, split):
    return any(f == family and g and g != M.ENOSPC and g[0].startswith(prefix) and (split is None or (g[1] > 1) == split)
               for f, g in seen)


def test_named_cases_reach_every_route_of_the_table(seen):
    assert not [r for r in REQUIRED if not _reached(seen, *r)]
    for family in ("fwd", "dgrad", "wgrad", "nt", "tn"):
        assert (family, None) in seen, family   # a refusal in each family


def test_routes_the_gpu_tests_claim(L):
    """What the comments of test_conv_bf16_gpu.py / test_gemm_bf16_gpu.py say about their shapes, in a default process
    (queried workspace, aligned pointers) and under SALUN_CONV_RING=3."""
    def fwd(shape, ring=1):
        return conv_route(L, FWD, shape, ring_bits(ring), L.salun_conv2d_bf16_data_workspace_bytes(*shape))[0]

    def wgrad(shape, flags=0):
        return conv_route(L, WGRAD, shape, flags | tn_bits(1), L.salun_conv2d_bf16_wgrad_workspace_bytes(*shape))[0]
    big = TC.SHAPES[-4:]
    # ">= 128 forward tiles: the 1x1 one takes the LDS-DMA ring kernel by default, all four do under SALUN_CONV_RING=3"
    assert [fwd(s).split("<")[0] for s in big] == ["igemm", "ring", "igemm", "igemm"]
    assert [fwd(s, 3) for s in big] == ["ring<4,2,3>", "ring<4,2,3>", "ring<4,1,3>", "ring<2,2,4>"]  # the tile forms named there
    # the two SD shapes the child process adds
    assert fwd((8, 32, 32, 320, 320, 3, 1, 1), 3) == "ring<4,1,3>" and fwd((8, 16, 16, 640, 1280, 3, 1, 1), 3) == "ring<2,2,4>"
    # nothing else of SHAPES has the tiles for the ring by default
    assert all(fwd(s).startswith("igemm") for s in TC.SHAPES[:-4])
    # test_epilogue_terms: "64 channels -> the reduction is split ...; 32 channels -> nine stages, no split", forward over C
    # and backward-data over K
    for shape in EPILOGUE:
        ws = L.salun_conv2d_bf16_data_workspace_bytes(*shape)
        assert (conv_route(L, FWD, shape, 0, ws)[1] > 1) == (shape[3] > 32), shape
        assert (conv_route(L, DGRAD, shape, 0, ws)[1] > 1) == (shape[4] > 32), shape
    assert conv_route(L, FWD, EPILOGUE[0], 0, 98304) == ("igemm<2,2,32>/S3", 3)
    # test_per_image_channel_sums_...: "the tap kernels (3x3), the dY^T.X GEMM route (1x1 with >= 1024 pixels), ..., the 1x1
    # tap route (few pixels)"
    assert [wgrad(s).split("/")[0] for s in WGRAD_DIMS] == ["wgrad_tap<3,1>", "wgrad_tn<v2>", "wgrad_tap<3,1>", "wgrad_tap<3,1>",
                                                            "wgrad_tap<1,1>", "wgrad_tap<3,1>"]
    # test_gemm_bf16_gpu.py: 1024 tokens is the smallest TN shape; its 2 x 16 x 16 case (512 tokens) stays on the tap kernel
    assert wgrad((1, 32, 32, 64, 64, 1, 1, 0)).startswith("wgrad_tn") and wgrad((1, 33, 31, 64, 64, 1, 1, 0)).startswith("wgrad_tap")
    assert wgrad((1, 32, 32, 64, 64, 1, 1, 0), UNALIGNED).startswith("wgrad_tap<1,1>")
    assert wgrad((2, 16, 16, 320, 640, 1, 1, 0)).startswith("wgrad_tap<1,1>")


def test_a_label_that_does_not_fit_is_refused(L):
    buf = ctypes.create_string_buffer(4)
    assert L.salun_conv2d_bf16_route(FWD, 2, 8, 8, 32, 32, 3, 1, 1, 0, 0, buf, 4, None) == ENOSPC and buf.value == b""
    assert L.salun_gemm_bf16_route(NT, 256, 128, 64, 0, 0, buf, 4, None) == ENOSPC and buf.value == b""
    assert L.salun_gemm_bf16_route(7, 256, 128, 64, 0, 0, buf, 4, None) == EINVAL
    assert L.salun_conv2d_bf16_route(3, 2, 8, 8, 32, 32, 3, 1, 1, 0, 0, buf, 4, None) == EINVAL
