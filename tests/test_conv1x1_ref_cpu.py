"""conv1x1_ref_cpu.py against torch's float64 conv2d, and the premises test_conv1x1_infer_gpu.py rests on (no GPU)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import conv1x1_ref_cpu as P

_id = lambda c: c.id


@pytest.mark.parametrize("c", P.CASES, ids=_id)
def test_model_is_the_pointwise_product_in_float64(c):
    t = P.inputs(c, "gauss")
    want = torch.einsum("kc,nchw->nkhw", t.w[:, :, 0, 0], t.x)
    assert (c.P, c.Q) == (c.H, c.W)
    got = P.forward(t.x, t.w, c)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12 * float(want.abs().max()))
    assert torch.allclose(got, F.conv2d(t.x, t.w), rtol=1e-12, atol=1e-12 * float(want.abs().max()))


@pytest.mark.parametrize("c", P.CASES, ids=_id)
def test_integer_inputs_stay_below_2_to_24_grid_steps(c):
    """The premise of the exact tier, for the longest chain (C = 2048) too."""
    t = P.inputs(c, "int")
    for v in (t.x, t.w, t.scale, t.shift, t.addend):
        assert torch.equal(v.float().double(), v)
    abs_sum = P.forward(t.x, t.w, c, t.scale, t.shift, t.addend, absolute=True)
    steps = abs_sum / t.unit
    assert torch.equal(steps, steps.round()) and float(steps.max()) < 2 ** 24
    for names in P.EPILOGUES:
        y = P.forward(t.x, t.w, c, **P.terms_of(t, names), relu=True)
        assert torch.equal(y.float().double(), y)


def test_route_mirror_covers_every_tile_and_every_staging_path():
    labels = {P.route(c, tile) for c in P.CASES for tile in (0,) + P.TILES}
    assert None not in labels
    for piece in ("pw/64x64/", "pw/128x64/", "pw/128x128/", "/vec16/", "/vec4/"):
        assert any(piece in s for s in labels), piece
    assert "/vec4/" in P.route(P.CASES[0]) and "/vec4/" in P.route(P.CASES[5])          # HW = 49
    assert "/vec16/" in P.route(P.SKEWED) and "/vec4/" in P.route(P.SKEWED, aligned16=False)
    assert "/scalar/" in P.route(P.SKEWED, w_aligned16=False)
    assert P.route(P.CASES[0], 1) == "pw/64x64/vec4/B3"                                    # 147 pixels: a tail tile
    assert P.route(P.CASES[4], 3) == "pw/128x128/vec16/B50"                                # 24.5 pixel tiles x 2
    for name, change in P.REFUSED.items():
        assert P.route(P.CASES[0]._replace(**change)) is None, name
    # ResNet-50 at batch 64: the plan picks the tile from the problem
    assert "128x128" in P.route(P.R.Case(64, 64, 56, 56, 256, 1, 1, 0))
    assert "vec4" in P.route(P.R.Case(64, 2048, 7, 7, 512, 1, 1, 0))


def test_route_query_of_the_library_is_host_only_and_equals_the_mirror():
    from unlearn_saliency_amd import _lib, ops_infer
    _lib.build()
    for c in P.CASES:
        for tile in (0,) + P.TILES:
            for a16, w16 in ((True, True), (False, True), (True, False)):
                assert ops_infer.conv1x1_infer_route(c.N, c.C, c.H * c.W, c.K, tile, a16, w16) == P.route(c, tile, a16, w16)
    for change in P.REFUSED.values():
        r = P.CASES[0]._replace(**change)
        assert ops_infer.conv1x1_infer_route(r.N, r.C, r.H * r.W, r.K) is None
    assert ops_infer.conv1x1_infer_route(1, 8, 4, 32, 9) is None                           # unknown tile
    buf = ctypes.create_string_buffer(96)
    assert _lib.lib().salun_conv1x1_infer_route(1, 8, ctypes.c_int64(4), 32, 0, 1, 1, buf, 4) == -28
