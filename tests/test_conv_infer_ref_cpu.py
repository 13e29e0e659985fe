"""conv_infer_ref_cpu.py against torch's float64 operators, and the premises the GPU tests rest on (no GPU needed)."""
import pytest
import torch
import torch.nn.functional as F

import conv_infer_ref_cpu as R

_id = lambda c: c.id
SMALL = [c for c in R.CASES if c.H <= 56]


@pytest.mark.parametrize("c", R.CASES, ids=_id)
def test_model_equals_torch_conv2d_in_float64(c):
    t = R.inputs(c, "gauss")
    want = F.conv2d(t.x, t.w, None, c.stride, c.pad)
    assert want.shape == (c.N, c.K, c.P, c.Q)
    got = R.forward(t.x, t.w, c)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12 * float(want.abs().max()))
    full = R.forward(t.x, t.w, c, t.scale, t.shift, t.addend, relu=True)
    ref = F.relu(want * t.scale.view(1, -1, 1, 1) + t.shift.view(1, -1, 1, 1) + t.addend)
    assert torch.allclose(full, ref, rtol=1e-12, atol=1e-12 * float(ref.abs().max()))


@pytest.mark.parametrize("c", R.CASES, ids=_id)
def test_integer_inputs_stay_below_2_to_24_grid_steps(c):
    """The premise of the exact tier: abs_sum / unit < 2^24 and every input is an fp32 number on its grid."""
    t = R.inputs(c, "int")
    for v in (t.x, t.w, t.scale, t.shift, t.addend):
        assert torch.equal(v.float().double(), v)
    assert bool((t.scale != 0).all())
    abs_sum = R.forward(t.x, t.w, c, t.scale, t.shift, t.addend, absolute=True)
    steps = abs_sum / t.unit
    assert torch.equal(steps, steps.round()) and float(steps.max()) < 2 ** 24
    for names in R.EPILOGUES:
        y = R.forward(t.x, t.w, c, **R.terms_of(t, names), relu=True)
        assert torch.equal(y / t.unit, (y / t.unit).round()) and torch.equal(y.float().double(), y)


def test_route_mirror_covers_every_tile_and_both_orders():
    labels = {R.route(c, tile) for c in R.CASES for tile in (0,) + R.TILES}
    assert None not in labels
    for piece in ("64x64", "128x64", "128x128", "/fast/", "/generic/", "infer<7,2>", "infer<1,2>", "infer<3,1>", "infer<3,2>"):
        assert any(piece in s for s in labels), piece
    c = R.CASES[0]
    for name, change in R.REFUSED.items():
        assert R.route(c._replace(**change)) is None, name
    # the tail tile is masked, not refused; more than one pixel tile and more than one channel tile occur
    assert R.CASES[0].N * R.CASES[0].P * R.CASES[0].Q == 147
    assert R.route(R.CASES[5], 1).endswith("/B49") and R.route(R.CASES[9], 1).endswith("/B8")
    # the problem picks the tile: a full-size layer1 / layer4 call at the script's default batch
    assert "128x64" in R.route(R.Case(64, 64, 56, 56, 64, 3, 1, 1)) and "64x64" in R.route(R.Case(64, 512, 7, 7, 512, 3, 1, 1))
    assert "128x128" in R.route(R.Case(64, 128, 28, 28, 128, 3, 1, 1))


@pytest.mark.parametrize("shape", [(3, 7, 7), (2, 5, 9), (1, 1, 1), (2, 112, 112), (2, 6, 4)], ids=str)
def test_pool_model_equals_torch_max_pool2d(shape):
    x = R.pool_data(shape)
    want = F.max_pool2d(x[None], 3, 2, 1)[0]
    got = R.maxpool3x3s2(x)
    assert got.shape == want.shape
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    x64 = torch.randn(shape, dtype=torch.float64)
    assert torch.equal(R.maxpool3x3s2(x64), F.max_pool2d(x64[None], 3, 2, 1)[0])
    if shape[-1] > 4:
        assert bool(torch.isnan(x).any()) and bool((x == float("-inf")).any())


def test_fold_bn_equals_batch_norm_in_float64():
    g = torch.Generator().manual_seed(0)
    K = 32
    gamma, var = torch.rand(K, generator=g, dtype=torch.float64) + 0.5, torch.rand(K, generator=g, dtype=torch.float64) + 0.5
    beta, mean = torch.randn(K, generator=g, dtype=torch.float64) * 0.1, torch.randn(K, generator=g, dtype=torch.float64) * 0.1
    x = torch.randn(2, K, 5, 7, generator=g, dtype=torch.float64)
    scale, shift = R.fold_bn(gamma, beta, mean, var, 1e-5)
    want = F.batch_norm(x, mean, var, gamma, beta, False, 0.0, 1e-5)
    assert torch.allclose(x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), want, rtol=1e-13, atol=1e-13)


def test_normalize_model_is_totensor_then_normalize():
    u = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1).repeat(1, 1, 1, 3)
    got = R.normalize_u8(u, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    assert got.shape == (1, 3, 16, 16) and got.dtype == torch.float32
    assert float(got.min()) == -1.0 and float(got.max()) == 1.0
    want = ((u[0, :, :, 0].float() / 255) - 0.5) / 0.5
    assert torch.equal(got[0, 1], want)


def test_eval_figures_are_the_references_formulas():
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(7, 10, generator=g, dtype=torch.float64) * 3
    f = R.eval_figures(logits, 2)
    probs = F.softmax(logits, -1)
    assert abs(f.entropy_sum - float(-(probs * torch.log(probs)).sum())) < 1e-12
    assert abs(f.prob_sum - float(probs[:, 2].sum())) < 1e-12
    assert f.hits == int((torch.argmax(logits, -1) == 2).sum()) and f.count == 7
    assert bool((R.top_two_gap(logits) >= 0).all())
