"""The yardstick of tests/test_attn_exact_gpu.py, validated on the CPU before it judges the kernel (attn_ref_cpu.py):
the float64 kernel model stays inside the first-order bound B1 of the exact answer, the same model run in float32 — a
correct fp32 implementation's noise — stays inside the sharp tier the device is held to, and the one-hot construction
has the score gap it claims."""
import pytest
import torch

import attn_ref_cpu as R

# amplitude of q and k (v and dO stay at 1) x key order; the forced orders are built for amplitude 1
VARIANTS = [(a, o) for a in (1.0, 2.5, 4.0) for o in (None, "asc", "desc")] + [(1.0, "grow"), (1.0, "settle")]
NAMES = ("o", "dq", "dk", "dv")


def _id(shape):
    return "x".join(map(str, shape))


def _vid(variant):
    return f"a{variant[0]}-{variant[1] or 'drawn'}"


@pytest.fixture(scope="module")
def cases():
    memo = {}

    def get(shape, amp, order):
        key = (shape, amp, order)
        if key not in memo:
            q, k, v, d_o, scale = R.gaussian(shape, amp, order)
            ex = R.exact(q, k, v, d_o, scale)
            memo[key] = SimpleCase(ex, R.bounds(ex, q, k, v, d_o, scale), R.emulate(q, k, v, d_o, scale, torch.float64),
                                   R.emulate(q, k, v, d_o, scale, torch.float32))
        return memo[key]

    return get


class SimpleCase:
    def __init__(self, ex, b1, e64, e32):
        self.ex, self.b1, self.e64, self.e32 = ex, b1, e64, e32


def test_number_format_helpers():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -3.0, 0.0, 200.0],
                     dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.0, 0.0, 200.0], dtype=torch.float64)
    assert torch.equal(R.bf16_round(x), want)            # ties to even; one rounding (the 2^-40 is not lost on the way)
    assert torch.equal(R.bf16_round(x.float()).double(), R.bf16_round(x.float().double()))
    assert torch.equal(R.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, -0.75, 0.0])),
                       torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 0.0], dtype=torch.float64))
    r = torch.randn(4096, dtype=torch.float64)
    assert torch.equal(R.bf16_round(r.float().double()), r.float().to(torch.bfloat16).double())
    assert ((R.bf16_round(r) - r).abs() <= R.U * r.abs()).all()


@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
@pytest.mark.parametrize("shape", R.SHAPES, ids=_id)
def test_float64_model_is_within_b1_of_the_exact_answer(cases, shape, variant):
    c = cases(shape, *variant)
    for n in NAMES:
        err, b1 = (getattr(c.e64, n) - getattr(c.ex, n)).abs(), getattr(c.b1, n)
        assert (err <= b1).all(), f"{n}: worst ratio {float((err / b1.clamp_min(1e-300)).max()):.3f}"
    assert (c.e64.lse2 - c.ex.lse2).abs().max() <= 2.0 ** -22 * max(1.0, float(c.ex.lse2.abs().max()))  # one fp32 rounding


@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
@pytest.mark.parametrize("shape", R.SHAPES, ids=_id)
def test_fp32_noise_model_stays_inside_the_sharp_tier(cases, shape, variant):
    """Share of elements beyond ulp_bf16 + B1/8 at most 1 % per tensor, none beyond ulp_bf16 + 2*B1.  The elements
    between the two lines are dominant p values sitting on a bf16 tie: inherent, hence a share cap and not a hard line."""
    c = cases(shape, *variant)
    for n in NAMES:
        e64, b1 = getattr(c.e64, n), getattr(c.b1, n)
        err, ulp = (getattr(c.e32, n) - e64).abs(), R.ulp_bf16(e64)
        share = float((err > ulp + b1 / 8).double().mean())
        assert share <= 0.01, f"{n}: share {share:.4f}"
        assert (err <= ulp + 2 * b1).all(), f"{n}: worst {float(((err - ulp) / b1.clamp_min(1e-300)).max()):.2f} B1"


@pytest.mark.parametrize("shape", [s for s in R.SHAPES if s[3] > R.KT], ids=_id)
def test_forced_key_orders_reach_both_regimes_of_the_running_maximum(shape):
    """"grow": every query's maximum grows on every tile after the first (the rescale branch always runs); "settle":
    on none (it never runs again).  Both keep |s * scale| <= 60, the range the lse bound is derived for."""
    for order, want in (("grow", True), ("settle", False)):
        q, k, v, d_o, scale = R.gaussian(shape, 1.0, order)
        assert all(R.is_bf16(t) for t in (q, k))
        s = q @ k.transpose(-1, -2) * scale
        assert float(s.abs().max()) <= 60
        tile_max = torch.stack([s[..., j:j + R.KT].max(-1).values for j in range(0, shape[3], R.KT)], -1)
        running = tile_max.cummax(-1).values
        grew = tile_max[..., 1:] > running[..., :-1]
        assert bool(grew.all()) if want else not bool(grew.any())


@pytest.mark.parametrize("shape", [s for s in R.SHAPES if s[3] <= R.onehot_capacity(s[4])], ids=_id)
def test_onehot_construction(shape):
    B, H, Nq, Nk, D = shape
    q, k, v, d_o, scale, sel, A = R.onehot_code(shape)
    assert all(R.is_bf16(t) for t in (q, k, v, d_o))
    s2 = (q @ k.transpose(-1, -2)) * (scale * R.LOG2E)                   # scaled scores in log2 units
    top = s2.topk(min(2, Nk), -1)
    assert torch.equal(top.indices[..., 0], sel.expand(B, H, Nq))
    assert torch.equal(top.values[..., 0], torch.full((B, H, Nq), 2 * A * A * scale * R.LOG2E, dtype=torch.float64))
    if Nk > 1:
        assert (top.values[..., 0] - top.values[..., 1]).min() >= 200
    assert sel.unique().numel() == min(Nq, Nk)                          # every key wins once there are queries enough
    ex = R.exact(q, k, v, d_o, scale)
    want_o = v[:, :, sel]
    want_dv = torch.zeros_like(v).index_add_(2, sel, d_o)
    tiny = 2.0 ** -190                                                  # float64 keeps the losers' 2^-200: not bitwise
    assert max(float((ex.o - want_o).abs().max()), float((ex.dv - want_dv).abs().max())) < tiny
    assert max(float(ex.dq.abs().max()), float(ex.dk.abs().max())) < tiny
    e = R.emulate(q, k, v, d_o, scale)
    assert torch.equal(e.o, want_o) and torch.equal(e.dv, want_dv) and not e.dq.any() and not e.dk.any()


@pytest.mark.parametrize("shape", R.SHAPES, ids=_id)
def test_uniform_construction(shape):
    B, H, Nq, Nk, D = shape
    q, k, v, d_o, scale, count = R.uniform_counts(shape)
    assert int(count.sum()) == Nk and count.max() - count.min() <= 1
    ex = R.exact(q, k, v, d_o, scale)
    assert torch.allclose(ex.o, (count / Nk).expand(B, H, Nq, D), rtol=1e-14, atol=0)
    assert torch.allclose(ex.lse2, torch.full((B, H, Nq), float(torch.log2(torch.tensor(float(Nk), dtype=torch.float64))),
                                              dtype=torch.float64), rtol=0, atol=1e-12)
    assert not ex.dk.any()
