"""The schedule and the coefficients of the linear multistep sampler (SD/lms.py) on the host."""
import numpy as np
import pytest


def schedule(n):
    from unlearn_saliency_amd.SD.lms import LMSSchedule
    return LMSSchedule().set_timesteps(n)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 100, 1000])
def test_sigmas_decrease_to_a_final_zero(n):
    s = schedule(n)
    assert s.sigmas.dtype == np.float32 and s.sigmas.shape == (n + 1,) and len(s) == n
    assert s.sigmas[-1] == 0 and bool((np.diff(s.sigmas.astype(np.float64)) < 0).all())
    assert s.init_noise_sigma == float(s.sigmas[0]) == float(s.sigmas.max())
    assert s.timesteps[-1] == 0 and (n == 1 or s.timesteps[0] == 999)
    if n == 100:       # fractional timesteps; the published schedule's ends
        assert abs(s.timesteps[1] - (999 - 999 / 99)) < 1e-9
        assert abs(s.init_noise_sigma - 14.6146) < 1e-3 and abs(float(s.sigmas[-2]) - 0.0292) < 1e-3


@pytest.mark.parametrize("n", [1, 2, 5, 100])
def test_coefficients_sum_to_the_step(n):
    s = schedule(n)
    sig = s.sigmas.astype(np.float64)
    for i in range(n):
        for order in range(1, min(i + 1, 4) + 1):
            c = s.coefficients(i, order)
            h = sig[i + 1] - sig[i]
            assert c.shape == (order,) and abs(c.sum() - h) <= 1e-12 * abs(h), (i, order)
        assert len(s.coefficients(i)) == min(i + 1, 4)
    with pytest.raises(ValueError):
        s.coefficients(0, 2)


def test_a_cubic_derivative_is_integrated_exactly_from_step_3_on():
    s = schedule(20)
    sig = s.sigmas.astype(np.float64)
    p = np.poly1d([0.3, -1.1, 0.7, 2.0])
    P = np.polyint(p)
    for i in range(3, 20):
        c = s.coefficients(i)
        vals = np.array([p(sig[i - j]) for j in range(4)])
        got, want = float(c @ vals), float(P(sig[i + 1]) - P(sig[i]))
        scale = float(np.abs(c) @ np.abs(vals)) + abs(P(sig[i])) + abs(P(sig[i + 1]))
        assert abs(got - want) <= 1e-12 * scale, i
    # and a lower order is NOT exact for it: the test can tell the orders apart
    c2 = s.coefficients(5, 2)
    assert abs(float(c2 @ [p(sig[5]), p(sig[4])]) - float(P(sig[6]) - P(sig[5]))) > 1e-6


def test_one_and_two_step_chains():
    """dx/dsigma = 1: the chain ends at x0 - sigma_0 whatever the number of steps."""
    for n in (1, 2):
        s = schedule(n)
        x = 5.0
        for i in range(n):
            x += float(s.coefficients(i).sum())
        assert abs(x - (5.0 - float(s.sigmas[0]))) < 1e-12 * 20
        assert s.input_divisor(n) == 1.0 and s.input_divisor(0) == float(np.sqrt(np.float32(s.sigmas[0]) ** 2 + np.float32(1)))
