"""salun_lms_step (csrc/salun_sampler.hip, ops_sampler.lms_step) against the numpy fp32 statement of its operation
order, and a chain of SD/lms.py's LMSSampler with a stand-in model against the closed-form latent."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = np.float32


def lms_np(x, eu, ec, scale, hist, slot, coeffs, den):
    """The kernel's statement, every operation an fp32 numpy operation of its own.  hist is updated in place."""
    d = ec
    if eu is not None:
        df = ec - eu
        sd = F32(scale) * df
        d = eu + sd
    hist[slot] = d
    a = x + F32(coeffs[0]) * d
    for j in range(1, len(coeffs)):
        t = F32(coeffs[j]) * hist[(slot - j) % 4]
        a = a + t
    return a, a / F32(den)


@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
def test_one_step_is_bit_equal_to_the_numpy_statement(guided):
    from unlearn_saliency_amd import ops_sampler
    r = np.random.default_rng(3)
    shape = (2, 4, 8, 8)
    x = r.standard_normal(shape).astype(F32) * 5
    hist = r.standard_normal((4,) + shape).astype(F32)
    hist_d = torch.from_numpy(hist).cuda()
    for order in (1, 2, 3, 4):
        for slot in (0, 1, 3):
            eps = r.standard_normal((4 if guided else 2,) + shape[1:]).astype(F32)
            coeffs = list(r.standard_normal(order) * 0.3)
            den = 1.0 + float(r.random()) * 3
            eu, ec = (eps[:2], eps[2:]) if guided else (None, eps)
            want, want_in = lms_np(x, eu, ec, 7.5, hist, slot, coeffs, den)
            x_in = torch.full(eps.shape, float("nan"), device="cuda")
            got = ops_sampler.lms_step(torch.from_numpy(x).cuda(), torch.from_numpy(eps).cuda(), 7.5 if guided else 1.0,
                                       hist_d, slot, coeffs, den, x_in=x_in)
            assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), (order, slot)
            assert np.array_equal(hist_d.cpu().numpy().view(np.int32), hist.view(np.int32)), (order, slot)
            for half in range(2 if guided else 1):
                assert np.array_equal(x_in[2 * half:2 * half + 2].cpu().numpy().view(np.int32), want_in.view(np.int32))
            x = want
    # in place, and without the next input
    xd = torch.from_numpy(x).cuda()
    eps = torch.from_numpy(r.standard_normal(shape).astype(F32)).cuda()
    want, _ = lms_np(x, None, eps.cpu().numpy(), 1.0, hist, 2, [0.25, -0.5], 2.0)
    assert ops_sampler.lms_step(xd, eps, 1.0, hist_d, 2, [0.25, -0.5], 2.0, out=xd) is xd
    assert np.array_equal(xd.cpu().numpy(), want)


def test_refusals():
    from unlearn_saliency_amd import ops_sampler
    from unlearn_saliency_amd._lib import SalunError
    x = torch.zeros(2, 4, 8, 8, device="cuda")
    hist = torch.zeros(4, 2, 4, 8, 8, device="cuda")
    with pytest.raises(ValueError):
        ops_sampler.lms_step(x, x.clone(), 1.0, hist, 0, [0.1] * 5, 1.0)
    with pytest.raises(SalunError):
        ops_sampler.lms_step(x, x.clone(), 1.0, hist, 4, [0.1], 1.0)
    with pytest.raises(SalunError):
        ops_sampler.lms_step(x, x.clone(), 2.0, hist, 0, [0.1], 1.0)          # a scale without guidance
    with pytest.raises(SalunError):
        ops_sampler.lms_step(x, x.clone(), 1.0, hist, 0, [0.1], 0.0)


def test_a_chain_with_a_linear_model_ends_at_the_closed_form():
    """eps = a + b sigma: step 0 (order 1) is an Euler step, every later step (order >= 2) integrates the line exactly,
    so x_end = x_0 + h_0 (a + b sigma_0) - a sigma_1 - b sigma_1^2 / 2 in exact arithmetic.  The device chain is allowed
    the distance of the fp32 numpy chain (the same operation order) from that value, measured here."""
    from unlearn_saliency_amd.SD.lms import LMSSampler, LMSSchedule
    steps, B, shape = 6, 2, (4, 8, 8)
    r = np.random.default_rng(9)
    a = r.standard_normal((B,) + shape).astype(F32)
    b = (0.1 * r.standard_normal((B,) + shape)).astype(F32)
    noise = r.standard_normal((B,) + shape).astype(F32)
    sch = LMSSchedule().set_timesteps(steps)
    sig = sch.sigmas.astype(np.float64)
    eps_of = lambda i: a + b * F32(sch.sigmas[i])                     # fp32, two roundings

    seen = []

    def model(x_in, t, context):
        i = len(seen)
        seen.append((x_in.clone(), float(t[0])))
        assert t.shape == (2 * B,) and context.shape[0] == 2 * B
        e = torch.from_numpy(eps_of(i)).cuda()
        return torch.cat([e, e])

    ctx = torch.zeros(B, 3, 8, device="cuda")
    sampler = LMSSampler(None, LMSSchedule())
    got = sampler.sample(ctx, ctx, 7.5, torch.from_numpy(noise).cuda(), steps, eps_fn=model).cpu().numpy()
    assert sampler.last_steps == steps and [t for _, t in seen] == [float(F32(t)) for t in sch.timesteps]   # fp32 rows

    # the fp32 numpy chain
    x = noise * F32(sch.init_noise_sigma)
    x0 = x.astype(np.float64)
    hist = np.zeros((4, B) + shape, F32)
    assert np.array_equal(seen[0][0][:B].cpu().numpy(), x / F32(sch.input_divisor(0)))
    for i in range(steps):
        e = eps_of(i)
        x, x_in = lms_np(x, e, e, 7.5, hist, i % 4, sch.coefficients(i), sch.input_divisor(i + 1))
        if i + 1 < steps:   # what the next pass read: both halves
            assert all(np.array_equal(seen[i + 1][0][h * B:(h + 1) * B].cpu().numpy(), x_in) for h in (0, 1)), i
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    closed = x0 + (sig[1] - sig[0]) * (a64 + b64 * sig[0]) - a64 * sig[1] - b64 * sig[1] ** 2 / 2
    margin = float(np.abs(x.astype(np.float64) - closed).max())
    err = float(np.abs(got.astype(np.float64) - closed).max())
    print(f"lms chain, {steps} steps: fp32 numpy chain {margin:.3e}, device {err:.3e} from the closed form "
          f"(max |x| {float(np.abs(closed).max()):.2f})")
    assert margin < 1e-4 * float(np.abs(closed).max())                # the numpy chain itself integrates the line
    assert err <= margin
