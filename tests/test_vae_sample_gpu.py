"""salun_vae_posterior_sample (csrc/salun_vae.hip) against its definition in float64.

The kernel computes, every operation rounded to fp32 by itself and s = fp32(scale),
    z = fl(s * fl(mean + fl(sd^ * e))),   sd^ = expf(0.5 * clamp(logvar, -30, 20))     (0.5 * . is exact)
with e the value salun_sampler_noise writes for the key (seed, image id, step = draw) at the element's index.  With
sd = exp(0.5 clamp(logvar)) in float64, u = 2^-24, gamma_k = k u / (1 - k u) and expf within EXP_ULP["expf"] u:
    |z - s (mean + sd e)| <= (EXP_ULP u (1 + gamma_3) + gamma_3) |s sd e| + gamma_2 |s mean|
(one expf and three roundings on the e term, two roundings on the mean term).  `deterministic`: |z - s mean| <= u |s mean|."""
import pytest
import torch

import norm_ref_cpu as R

pytestmark = pytest.mark.gpu

B, ZC, HW = 3, 4, 64
SCALE = 0.18215
IDS = (5, 9, 2)


def ops():
    from unlearn_saliency_amd import ops_infer, ops_sampler
    return ops_infer, ops_sampler


def moments(Cm, seed=0):
    """[B, Cm, 8, 8] fp32: means of order one; log-variances across [-40, 25] with both clamps acting, -40, 25 and the
    clamp points themselves present; channels past 2 zc hold NaN (they must be ignored)."""
    g = torch.Generator().manual_seed(seed)
    m = torch.full((B, Cm, 8, 8), float("nan"))
    m[:, :ZC] = torch.randn(B, ZC, 8, 8, generator=g)
    lv = torch.rand(B, ZC, 8, 8, generator=g) * 65 - 40
    lv.view(-1)[:6] = torch.tensor([-40.0, 25.0, -30.0, 20.0, 0.0, -1e-30])
    m[:, ZC:2 * ZC] = lv
    return m


def model(m, eps, s):
    mean, lv = m[:, :ZC].double(), m[:, ZC:2 * ZC].double()
    sd = torch.exp(0.5 * lv.clamp(-30.0, 20.0))
    t_e, t_m = s * sd * eps.double(), s * mean
    bound = (R.EXP_ULP["expf"] * R.U * (1 + R.gam(3)) + R.gam(3)) * t_e.abs() + R.gam(2) * t_m.abs()
    return t_m + t_e, bound


@pytest.mark.parametrize("Cm", [8, 32])
def test_every_element_within_its_bound(Cm):
    oi, os_ = ops()
    m = moments(Cm)
    assert float(m[:, ZC:2 * ZC].min()) < -30 and float(m[:, ZC:2 * ZC].max()) > 20
    ids = torch.tensor(IDS, dtype=torch.int64, device="cuda")
    s = float(torch.tensor(SCALE, dtype=torch.float32))
    z = oi.vae_posterior_sample(m.cuda(), ZC, ids, seed=7, draw=3, scale=SCALE).cpu()
    eps = os_.sampler_noise(ids, (ZC, 8, 8), 7, step=3).cpu()
    want, bound = model(m, eps, s)
    assert z.shape == (B, ZC, 8, 8) and bool(torch.isfinite(z).all())
    err = (z.double() - want).abs()
    print("posterior sample: worst err / bound", float((err / bound).max()))
    assert bool((err <= bound).all())
    # the mode: one rounding
    zd = oi.vae_posterior_sample(m.cuda(), ZC, None, seed=7, draw=3, scale=SCALE, deterministic=True).cpu()
    sm = s * m[:, :ZC].double()
    assert bool(((zd.double() - sm).abs() <= R.U * sm.abs()).all())
    assert torch.equal(zd, (torch.tensor(SCALE, dtype=torch.float32) * m[:, :ZC]))


def test_keying():
    oi, _ = ops()
    m = moments(8).cuda()
    bits = lambda t: t.view(torch.int32)
    run = lambda mm, ids, seed=7, draw=3: oi.vae_posterior_sample(mm, ZC, torch.tensor(ids, dtype=torch.int64, device="cuda"),
                                                                  seed=seed, draw=draw, scale=SCALE)
    z = run(m, IDS)
    assert torch.equal(bits(run(m, IDS)), bits(z))                              # the same bits again
    perm = [2, 0, 1]
    zp = run(m[perm].contiguous(), [IDS[i] for i in perm])
    assert torch.equal(bits(zp), bits(z[perm]))                                  # an image's latent follows the image
    alone = run(m[1:2].contiguous(), IDS[1:2])
    assert torch.equal(bits(alone[0]), bits(z[1]))
    for other in (run(m, IDS, draw=4), run(m, IDS, seed=8), run(m, (5, 9, 3))[2:]):
        ref = z if other.shape[0] == B else z[2:]
        assert float((bits(other) != bits(ref)).float().mean()) > 0.9           # a fresh draw, nearly every element


def test_moments_of_the_draw():
    """Over 2^17 draws the mean and variance of e are within 5 standard errors of 0 and 1.  e is a centred sum of twelve
    uniforms: excess kurtosis -0.1, so the standard error of the variance is sqrt(1.9 / n)."""
    oi, os_ = ops()
    b, hw = 8, 64
    n = b * ZC * hw * hw
    assert n == 1 << 17
    m = torch.zeros(b, 8, hw, hw, device="cuda")                                 # mean 0, log-variance 0: z = e
    ids = torch.arange(100, 100 + b, dtype=torch.int64, device="cuda")
    z = oi.vae_posterior_sample(m, ZC, ids, seed=11, draw=0, scale=1.0)
    eps = os_.sampler_noise(ids, (ZC, hw, hw), 11, step=0)
    assert bool(((z.double() - eps.double()).abs() <= (R.EXP_ULP["expf"] * R.U * (1 + R.gam(3)) + R.gam(3)) * eps.double().abs()).all())
    e = eps.double().cpu().view(-1)
    assert abs(float(e.mean())) <= 5 * (1.0 / n) ** 0.5
    assert abs(float(e.var(unbiased=False)) - 1.0) <= 5 * (1.9 / n) ** 0.5


def test_refusals():
    from unlearn_saliency_amd._lib import SalunError
    oi, _ = ops()
    ids = torch.tensor(IDS, dtype=torch.int64, device="cuda")
    with pytest.raises(SalunError):
        oi.vae_posterior_sample(torch.zeros(B, 6, 8, 8, device="cuda"), ZC, ids, 0, 0, 1.0)      # Cm < 2 zc
    with pytest.raises(SalunError):
        oi.vae_posterior_sample(torch.zeros(B, 8, 8, 8, device="cuda"), ZC, ids, 0, -1, 1.0)     # draw < 0
    with pytest.raises(ValueError):
        oi.vae_posterior_sample(torch.zeros(B, 8, 8, 8, device="cuda"), ZC, None, 0, 0, 1.0)     # no ids for a sample
