"""salun_adam_ema_step (K20: masked Adam + EMA shadow in one pass) on the device.

  * bit-identity with what it replaces — `salun_masked_adam_step[_coef]` followed by `shadow.lerp_(p, 1 - mu)` — on
    clones: p, m1, v AND the shadow, over sizes that cover the scalar tail, less than one float4, one wave, several
    workgroups with a ragged end and (2^23 + 4101: more tiles than the grid cap of 2048 x 4096 elements) a grid-stride
    loop that runs twice; with and without mask, clip and weight decay; steps 1-3 through salun_adam_coefficients;
  * the aliasing guard; `FusedMaskedAdam.attach_ema` against the plain optimizer + `EMAHelper.update`;
  * two steps of `--mode train` against the reference's (tests/golden/ddpm_train_step.npz);
  * `EMAHelper.ema()` against a stale packed weight image.
"""

import numpy as np
import pytest
import torch

import adam_ema_ref_cpu as A
from fixtures import ddpm_batch, ddpm_small_config, fill_params, flat_params

pytestmark = pytest.mark.gpu

# the last: a second grid-stride pass whose first tile has two full sub-vectors, a third with 100 live lanes and a fourth
# with none, then a 3-element tail
SIZES = [1, 3, 4, 1023, 4096 + 5, 2 ** 20 + 1, 2 ** 23 + 4101, 2048 * 4096 + 4 * (2 * 256 + 100) + 3]
B1, B2, EPS, LR = 0.9, 0.999, 1e-8, 2e-4
MOMENT_TOL = 4.5e-5  # tests/test_ddpm_gpu.py's bound for the Adam moments of a replayed reference run
STRIDE = 997


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _shift(t, offset):
    """`t` in an allocation of its own, `offset` elements in (offset 1: 4-byte aligned only, the kernel's scalar route)."""
    return torch.cat([t.new_zeros(offset), t])[offset:] if offset else t.contiguous()


def _state(n, seed, offset=0):
    """p, m1, v, shadow and a u8 0/1 mask of n elements."""
    from unlearn_saliency_amd import ops
    p = ops.fill_normal(n, seed, 0.0, 0.05)
    shadow = p + ops.fill_normal(n, seed + 1, 0.0, 1e-3)
    m1, v = ops.fill_normal(n, seed + 2, 0.0, 1e-3), ops.fill_normal(n, seed + 3, 0.0, 1e-3).square_()
    mask = ops.fill_u8(n, seed + 4) & 1
    return tuple(_shift(t, offset) for t in (p, m1, v, shadow, mask))


def _grad(n, seed, offset=0):
    from unlearn_saliency_amd import ops
    return _shift(ops.fill_normal(n, seed, 0.0, 0.02), offset)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_k20_is_bit_identical_to_adam_then_lerp(n, masked, clip, wd):
    from unlearn_saliency_amd import ops
    mu = 0.9999
    p, m1, v, sh, mask = _state(n, 1000 + n % 977)
    mask = mask if masked else None
    q, n1, w, th = p.clone(), m1.clone(), v.clone(), sh.clone()
    step_a = torch.zeros(1, dtype=torch.int64, device="cuda")
    step_b = torch.zeros(1, dtype=torch.int64, device="cuda")
    coef_a, coef_b = torch.zeros(2, device="cuda"), torch.zeros(2, device="cuda")
    sq = torch.zeros(1, device="cuda")
    for step in (1, 2, 3):
        g = _grad(n, 2000 + 7 * step + n % 977)
        sqn = ops.grad_sqnorm(g, sq) if clip else None
        ops.adam_coefficients(step_a, LR, B1, B2, coef_a)
        ops.adam_ema_step_coef(p, g, m1, v, sh, mask, coef_a, B1, B2, EPS, wd, mu, sqnorm=sqn, max_norm=0.5)
        ops.adam_coefficients(step_b, LR, B1, B2, coef_b)
        ops.masked_adam_step_coef(q, g, n1, w, mask, coef_b, B1, B2, EPS, wd, sqnorm=sqn, max_norm=0.5)
        th.lerp_(q, 1.0 - mu)
        assert _same(p, q) and _same(m1, n1) and _same(v, w), (n, step)
        assert _same(sh, th), (n, step, int((_bits(sh) != _bits(th)).sum()))
    assert int(step_a) == 3 and not _same(sh, _state(n, 1000 + n % 977)[3])
    if masked and wd == 0.0:
        # no gradient enters a masked-out element: its first moment only decays, b1 * m1 three times over (the weight
        # itself still moves, by the momentum it started with)
        m0 = _state(n, 1000 + n % 977)[1]
        assert _same(m1[mask == 0], (m0 * B1 * B1 * B1)[mask == 0])


@pytest.mark.parametrize("mu", [0.9999, 0.999, 0.9, 0.51])
@pytest.mark.parametrize("offset", [0, 1])
def test_k20_host_step_twin_rates_and_unaligned_pointers(mu, offset):
    """`salun_adam_ema_step` (lr, step on the host) against `salun_masked_adam_step` + lerp_, for rates down to the edge
    of lerp's small-weight form, on 16-byte aligned vectors and on vectors one float into their allocation."""
    from unlearn_saliency_amd import ops
    n = 4096 + 5
    p, m1, v, sh, mask = _state(n, 31, offset)
    q, n1, w, th = (_shift(t.clone(), offset) for t in (p, m1, v, sh))
    assert all(t.data_ptr() % 16 == 4 * offset for t in (p, m1, v, sh, q, n1, w, th))
    for step in (1, 2, 3):
        g = _grad(n, 77 + step, offset)
        ops.adam_ema_step(p, g, m1, v, sh, mask, LR, B1, B2, EPS, 1e-2, mu, step)
        ops.masked_adam_step(q, g, n1, w, mask, LR, B1, B2, EPS, 1e-2, step)
        th.lerp_(q, 1.0 - mu)
        assert _same(p, q) and _same(m1, n1) and _same(v, w) and _same(sh, th), (mu, offset, step)


def test_k20_against_the_cpu_restatement(oracle_mod):
    """p, m1, v exact (the oracle's Adam); the shadow within the one ulp the numpy fma can be off by (double rounding)."""
    from unlearn_saliency_amd import ops
    n, mu = 4096 + 5, 0.999
    p, m1, v, sh, mask = _state(n, 500)
    hp, hm, hv, hs, hmask = (t.cpu().numpy().copy() for t in (p, m1, v, sh, mask))
    for step in (1, 2):
        g = _grad(n, 600 + step)
        ops.adam_ema_step(p, g, m1, v, sh, mask, LR, B1, B2, EPS, 0.0, mu, step, gscale=0.7)
        A.adam_ema_step(hp, g.cpu().numpy(), hm, hv, hs, hmask, 0.7, LR, B1, B2, EPS, 0.0, mu, step)
    for dev, host in ((p, hp), (m1, hm), (v, hv)):
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), host.view(np.uint32))
    ulps = np.abs(sh.cpu().numpy().view(np.int32).astype(np.int64) - hs.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1, int(ulps.max())


def test_k20_refuses_aliased_buffers_without_launching():
    from unlearn_saliency_amd import _lib, ops
    from unlearn_saliency_amd._lib import c_double, c_int, c_int64, c_void_p
    n = 1023
    bufs = dict(zip(("p", "m1", "v", "shadow"), _state(n, 9)[:4]))
    g = _grad(n, 10)
    coef = torch.tensor([1.0, -1e-3], device="cuda")
    before = {k: t.clone() for k, t in bufs.items()}
    L = _lib.lib()
    names = list(bufs)
    for i in range(4):
        for j in range(i + 1, 4):
            a = dict(bufs)
            a[names[j]] = a[names[i]]
            ptr = {k: c_void_p(t.data_ptr()) for k, t in a.items()}
            common = (c_void_p(g.data_ptr()), ptr["m1"], ptr["v"], ptr["shadow"], c_void_p(None), c_void_p(None),
                      c_double(1.0), c_double(1.0))
            tail = (c_double(B1), c_double(B2), c_double(EPS), c_double(0.0), c_double(0.999))
            rc = L.salun_adam_ema_step_coef(ptr["p"], *common, c_void_p(coef.data_ptr()), *tail, c_int64(n), c_void_p(None))
            assert rc == _lib.SALUN_EINVAL, (names[i], names[j], rc)
            rc = L.salun_adam_ema_step(ptr["p"], *common, c_double(LR), *tail, c_int(1), c_int64(n), c_void_p(None))
            assert rc == _lib.SALUN_EINVAL, (names[i], names[j], rc)
    with pytest.raises(_lib.SalunError):
        ops.adam_ema_step(bufs["p"], g, bufs["m1"], bufs["v"], bufs["p"], None, LR, B1, B2, EPS, 0.0, 0.999, 1)
    torch.cuda.synchronize()
    assert all(_same(bufs[k], before[k]) for k in bufs)  # nothing ran


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(5, 7)
        self.b = torch.nn.Parameter(torch.zeros(3))


def _toy(attach, mu=0.9999):
    from unlearn_saliency_amd import rng
    from unlearn_saliency_amd.DDPM.models.ema import EMAHelper
    from unlearn_saliency_amd.flat import arena_of
    from unlearn_saliency_amd.optim import FusedMaskedAdam
    m = Toy()
    with torch.no_grad():
        for i, p in enumerate(m.parameters()):
            p.copy_(torch.from_numpy(rng.normal(p.numel(), 11 + i, 0.0, 0.5)).view_as(p))
    m = m.cuda()
    arena = arena_of(m)
    opt = FusedMaskedAdam(arena, lr=1e-3, weight_decay=1e-2, grad_clip=1.0)
    ema = EMAHelper(mu=mu)
    ema.register(m)
    if attach:
        assert ema.attach_to(opt, m)
    return m, arena, opt, ema


def _count(monkeypatch, names):
    from unlearn_saliency_amd import _lib
    L, calls = _lib.lib(), {}
    for name in names:
        fn = getattr(L, name)
        calls[name] = 0

        def counted(*a, _fn=fn, _name=name):
            calls[_name] += 1
            return _fn(*a)

        monkeypatch.setattr(L, name, counted)
    return calls


@pytest.mark.parametrize("device_step", [False, True])
def test_attach_ema_equals_the_plain_optimizer_plus_ema_update(monkeypatch, device_step):
    from unlearn_saliency_amd import ops
    calls = _count(monkeypatch, ["salun_masked_adam_step", "salun_masked_adam_step_coef", "salun_adam_ema_step",
                                 "salun_adam_ema_step_coef"])
    (ma, aa, oa, ea), (mb, ab, ob, eb) = _toy(True), _toy(False)
    assert aa.n == 5 * 7 + 7 + 3
    mask = (ops.fill_u8(aa.n, 3) & 1).contiguous()
    for o in (oa, ob):
        o.set_mask(mask)
        if device_step:
            o.use_device_step()
    for k in range(5):
        g = ops.fill_normal(aa.n, 40 + k, 0.0, 0.3)
        for arena, opt, ema, model in ((aa, oa, ea, ma), (ab, ob, eb, mb)):
            arena.grads.copy_(g)
            opt.clip_grad_norm_(1.0)
            opt.step()
            ema.update(model)
        assert _same(aa.params, ab.params) and _same(oa.exp_avg, ob.exp_avg) and _same(oa.exp_avg_sq, ob.exp_avg_sq), k
        assert _same(ea._flat, eb._flat), k
    assert not _same(ea._flat, aa.params)
    folded, plain = ("salun_adam_ema_step_coef", "salun_masked_adam_step_coef") if device_step else \
        ("salun_adam_ema_step", "salun_masked_adam_step")
    # the optimizer without attach_ema still goes through the entry point it always used; the attached one never does
    assert calls == {**dict.fromkeys(calls, 0), folded: 5, plain: 5}, calls


def test_two_training_steps_on_the_device_match_the_reference(golden_dir):
    """Tolerances: those of tests/test_ddpm_gpu.py::test_saliency_unlearn_matches_reference.  The shadow after two steps
    is mu^2 s0 + mu w p1 + w p2 (w = 1 - mu), linear in the weights: their movement bounds times w (1 + mu)."""
    from test_ddpm_train_host import _train_golden_run
    from unlearn_saliency_amd.DDPM.runners import diffusion as RD
    g, cfg, runner, model, before = _train_golden_run(RD, golden_dir, torch.device("cuda"), library_conv=False)
    losses = np.array([float(v) for v in runner.step_losses], np.float64)
    rel = np.abs(losses - g["step_loss"]) / np.abs(g["step_loss"])
    print(f"step losses {losses}, reference {g['step_loss']}, rel. deviation {rel}")
    assert rel.max() <= 1e-5, rel
    opt, ema = runner.last_optimizer, runner.last_ema
    assert opt._ema_shadow is ema._flat  # the run took the folded path
    m1, v = opt.exp_avg.cpu().numpy(), opt.exp_avg_sq.cpu().numpy()
    s1, s2 = np.abs(g["exp_avg_sample"]).max(), np.abs(g["exp_avg_sq_sample"]).max()
    d1 = np.abs(m1[::STRIDE] - g["exp_avg_sample"]) / s1
    d2 = np.abs(v[::STRIDE] - g["exp_avg_sq_sample"]) / s2
    print(f"exp_avg max dev {d1.max():.2e} of scale, exp_avg_sq max dev {d2.max():.2e} of scale")
    assert d1.max() <= MOMENT_TOL and d2.max() <= MOMENT_TOL, (d1.max(), d2.max())
    assert abs(np.linalg.norm(m1.astype(np.float64)) - float(g["exp_avg_norm"])) <= 1e-5 * float(g["exp_avg_norm"])
    assert abs(v.astype(np.float64).sum() - float(g["exp_avg_sq_sum"])) <= 2e-5 * float(g["exp_avg_sq_sum"])
    lr = cfg.optim.lr
    after = flat_params(model)
    p0 = before[::STRIDE]
    got, ref = after[::STRIDE], g["param_sample"]
    dgot, dref = got - p0, ref - p0
    bad = np.abs(dgot - dref) > 1e-4 * np.abs(dref) + 1e-3 * lr
    print(f"weights: movement differs by more than 1e-4 relative + 1e-3 lr on {int(bad.sum())} of {bad.size}")
    assert bad.mean() <= 5e-3, bad.mean()
    assert np.abs(got - ref).max() <= 2 * 2 * lr
    sums = np.array([float(p.detach().double().sum()) for p in model.parameters()])
    assert np.allclose(sums, g["tensor_sums"], rtol=1e-4, atol=3e-3)
    mu = float(g["ema_rate"])
    k = (1.0 - mu) * (1.0 + mu)
    sh = ema._flat.cpu().numpy()
    got, ref = sh[::STRIDE], g["shadow_sample"]
    dgot, dref = got - p0, ref - p0
    bad = np.abs(dgot - dref) > 1e-4 * np.abs(dref) + k * 1e-3 * lr
    print(f"shadow: movement differs by more than 1e-4 relative + {k:.2f}e-3 lr on {int(bad.sum())} of {bad.size}; "
          f"largest reference movement {np.abs(dref).max():.2e}")
    assert np.abs(dref).max() > 0.01 * lr and bad.mean() <= 5e-3, bad.mean()
    assert np.abs(got - ref).max() <= k * 2 * 2 * lr
    assert abs(sh.astype(np.float64).sum() - float(g["shadow_sum"])) <= 1e-4 * abs(float(g["shadow_sum"])) + 3e-3


def test_ema_copy_is_not_served_stale_weight_images():
    """The snapshot model reads packed images of its 3x3 weights.  `ema()` rewrites the weights: a forward pass after it
    must see them — equal, bit for bit, to a freshly built model loaded with the shadow."""
    from unlearn_saliency_amd import weightimg
    from unlearn_saliency_amd.conv import use_salun_convs
    from unlearn_saliency_amd.DDPM.models.diffusion import Conditional_Model
    from unlearn_saliency_amd.DDPM.models.ema import EMAHelper
    cfg = ddpm_small_config()
    model = fill_params(Conditional_Model(cfg), 7000).cuda()
    ema = EMAHelper(mu=0.9)
    ema.register(model)
    x, c = (torch.from_numpy(v).cuda() for v in ddpm_batch(4, 200))
    x, t = 2 * x - 1, torch.tensor([5.0, 400.0, 750.0, 999.0], device="cuda")
    fwd = lambda m: m(x, t, c, mode="test", cond_scale=2.0)
    with torch.no_grad():
        copy = ema.ema_copy(model).eval()
        assert use_salun_convs(copy) > 0
        packs = weightimg.RING_LAUNCHES[0]
        first = fwd(copy)  # packs the images of the copy's weights
        assert weightimg.RING_LAUNCHES[0] > packs
        ema._flat.mul_(1.25)  # the average moves on
        packs = weightimg.RING_LAUNCHES[0]
        ema.ema(copy)
        second = fwd(copy)
        assert weightimg.RING_LAUNCHES[0] > packs  # re-packed
        fresh = Conditional_Model(cfg).cuda().eval()  # never packed an image before it holds the shadow's weights
        for n, p in fresh.named_parameters():
            p.copy_(ema.shadow[n])
        assert use_salun_convs(fresh) > 0
        want = fwd(fresh)
    assert not torch.equal(first, second)
    assert torch.equal(second, want), float((second - want).abs().max())
