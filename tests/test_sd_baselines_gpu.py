"""SD baselines on the device: the K21 kernels (salun_ldm_ddim_step, salun_esd_loss) bit for bit against their numpy
restatement (esd_ref_cpu.py), the frozen copy's weight images, the latent DDIM sampler's step counts, and `train_esd` /
`gradient_ascent` replaying the draws of the REFERENCE's own runs (tests/golden/sd_baselines.npz, written by
tests/golden/make_golden_sd_baselines.py) against its float64 values.

Tolerances of the replayed runs: the fixture holds, per quantity, the reference's OWN fp32-versus-float64 gap
(`rel_max`: max |a - b| / max |b|) and 4x that gap as the device's bound — its MFMA convolutions and GEMMs sum in another
order than the host's.  The bounds are read from the fixture, not restated here (DESIGN.md §9f lists them).
"""
import os
import random

import numpy as np
import pytest
import torch

import esd_ref_cpu as R
from fixtures import SD_GLUE_PROMPTS, fill_params, replay_draws, sd_glue_batches, sd_glue_class_contexts, \
    sd_glue_contexts, sd_tiny_config
from unlearn_saliency_amd import rng

pytestmark = pytest.mark.gpu


def _bits(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint32)


def _np(seed, *shape):
    return rng.normal(int(np.prod(shape)), seed).reshape(shape)


def rel_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.fixture(scope="module")
def base(golden_dir):
    return np.load(os.path.join(golden_dir, "sd_baselines.npz"))


# ------------------------------------------------------------------------------------------------ 1a
CHW = (1, 3, 4, 1023, 256, 4096 + 5, 16384)
COEF = (0.6153, 0.7883, 0.5871, 0.8095)   # c_s1m, c_sqrt_at, c_dir, c_sqrt_aprev: any fp32 values do


@pytest.mark.parametrize("chw", CHW)
@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("scale", [1.0, 3.0, 7.5])
def test_ldm_ddim_step_bit_identical(chw, B, scale):
    """scale 1.0: a single eps of B rows (the reference's no-guidance branch); else the two halves of a 2B-row eps."""
    from unlearn_saliency_amd import ops_sampler as S
    x = _np(10 + chw, B, chw)
    eps = _np(20 + chw, B if scale == 1.0 else 2 * B, chw)
    z = _np(30 + chw, B, chw)
    dx, de, dz = (torch.from_numpy(v).cuda() for v in (x, eps, z))
    for sigma, zz, dzz in ((0.0, None, None), (0.3171, z, dz)):
        want, want0 = R.ldm_ddim_step(x, eps, scale, *COEF, sigma, zz)
        x0 = torch.empty_like(dx)
        got = S.ldm_ddim_step(dx, de, scale, *COEF, sigma, dzz, x0=x0)
        assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(x0), _bits(want0)), (sigma,)
        got = S.ldm_ddim_step(dx, de, scale, *COEF, sigma, dzz)            # without x0_out
        assert np.array_equal(_bits(got), _bits(want))
        assert np.array_equal(_bits(dx), _bits(x))                          # inputs untouched
        alias = dx.clone()
        assert S.ldm_ddim_step(alias, de, scale, *COEF, sigma, dzz, out=alias) is alias   # x_prev aliasing x
        assert np.array_equal(_bits(alias), _bits(want))


@pytest.mark.parametrize("which", ["x", "eps", "z", "out", "x0"])
def test_ldm_ddim_step_scalar_route_when_one_pointer_is_4_bytes_off(which):
    from unlearn_saliency_amd import ops_sampler as S
    B, chw = 2, 256
    x, eps, z = _np(1, B, chw), _np(2, 2 * B, chw), _np(3, B, chw)

    def dev(a, off):   # a device tensor whose storage starts 4 bytes past a 16-byte boundary when `off`
        buf = torch.empty(a.size + 4, dtype=torch.float32, device="cuda")
        t = buf[1:1 + a.size] if off else buf[:a.size]
        assert t.data_ptr() % 16 == (4 if off else 0)
        return t.view(a.shape).copy_(torch.from_numpy(a))

    dx, de, dz = dev(x, which == "x"), dev(eps, which == "eps"), dev(z, which == "z")
    out, x0 = dev(np.zeros_like(x), which == "out"), dev(np.zeros_like(x), which == "x0")
    want, want0 = R.ldm_ddim_step(x, eps, 7.5, *COEF, 0.25, z)
    S.ldm_ddim_step(dx, de, 7.5, *COEF, 0.25, dz, out=out, x0=x0)
    assert np.array_equal(_bits(out), _bits(want)) and np.array_equal(_bits(x0), _bits(want0))


def test_ldm_ddim_step_rejects_what_the_header_says():
    from unlearn_saliency_amd import ops_sampler as S
    from unlearn_saliency_amd._lib import SalunError
    x, eps = torch.zeros(2, 8, device="cuda"), torch.zeros(4, 8, device="cuda")
    with pytest.raises(SalunError, match="invalid argument"):       # sigma != 0 without z
        S.ldm_ddim_step(x, eps, 3.0, *COEF, 0.1, None)
    with pytest.raises(SalunError, match="invalid argument"):       # a single eps is the scale == 1 branch
        S.ldm_ddim_step(x, eps[:2].contiguous(), 3.0, *COEF)
    with pytest.raises(ValueError):
        S.ldm_ddim_step(x, torch.zeros(3, 8, device="cuda"), 3.0, *COEF)
    assert S.ldm_ddim_step(x[:0], eps[:0], 1.0, *COEF).shape == (0, 8)   # empty batch: nothing launched


# ------------------------------------------------------------------------------------------------ 1b
# 64 segments of 1024 floats is where salun_esd_loss goes from one launch to two: 65536 elements, one more, and 80 segments
@pytest.mark.parametrize("B,chw", [(B, chw) for chw in CHW for B in (1, 3)] + [(4, 16384), (1, 65537), (5, 16384)])
def test_esd_loss_target_gradient_and_sum(chw, B):
    from unlearn_saliency_amd import ops
    e_n, e_0p = _np(40 + chw, B, chw), _np(50 + chw, 2 * B, chw)
    dn, d0p = torch.from_numpy(e_n).cuda(), torch.from_numpy(e_0p).cuda()
    for ng in (1.0, 0.35):
        loss, d, tgt = ops.esd_loss_raw(dn, d0p, ng, want_target=True)
        # the torch expression on the device, one operation per line
        e_0, e_p = d0p[:B], d0p[B:]
        diff = e_p - e_0
        sc = ng * diff
        target = e_0 - sc
        dd = dn - target
        grad = (2.0 / dn.numel()) * dd
        assert np.array_equal(_bits(tgt), _bits(target)) and np.array_equal(_bits(d), _bits(grad))
        wl, wd, wt = R.esd_loss(e_n, e_0p, ng)
        assert np.array_equal(_bits(tgt), _bits(wt)) and np.array_equal(_bits(d), _bits(wd))
        # the loss against the float64 sum: salun_sqerr_loss's bound (tests/test_kernels_gpu.py::test_sqerr_loss_and_grad)
        assert abs(loss.item() - wl) <= 1e-6 * abs(wl), (loss.item(), wl)
        again, d2, _ = ops.esd_loss_raw(dn, d0p, ng)
        assert np.array_equal(_bits(again), _bits(loss)) and np.array_equal(_bits(d2), _bits(d))   # deterministic


def test_esd_loss_autograd_only_e_n_and_grad_out_scaling():
    from unlearn_saliency_amd import ops
    B, chw = 2, 1023
    e_n = torch.from_numpy(_np(1, B, chw)).cuda().requires_grad_(True)
    e_0p = torch.from_numpy(_np(2, 2 * B, chw)).cuda().requires_grad_(True)
    loss = ops.esd_loss(e_n, e_0p, 1.0)
    (loss * 0.25).backward()
    assert e_0p.grad is None
    _, d, _ = ops.esd_loss_raw(e_n.detach(), e_0p.detach(), 1.0)
    assert np.array_equal(_bits(e_n.grad), _bits(d * 0.25))
    ref_n = e_n.detach().clone().requires_grad_(True)
    ref = torch.nn.MSELoss()(ref_n, e_0p[:B].detach() - (1.0 * (e_0p[B:].detach() - e_0p[:B].detach())))
    (ref * 0.25).backward()
    assert abs(loss.item() - ref.item()) <= 1e-6 * abs(ref.item())
    assert torch.allclose(e_n.grad, ref_n.grad, rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        ops.esd_loss(e_n, e_0p[:3].detach().contiguous(), 1.0)


# ------------------------------------------------------------------------------------------------ models
def _tiny(bf16=False):
    from unlearn_saliency_amd.SD.ldm_lite import LatentDiffusionLite
    m = LatentDiffusionLite(sd_tiny_config(), bf16=bf16)
    fill_params(m.model.diffusion_model, 9000)
    m = m.cuda()
    assert m.use_mfma_convs() >= 8
    return m


def _flat(m):
    return torch.cat([p.detach().reshape(-1) for p in m.model.diffusion_model.parameters()]).cpu().numpy()


def _contexts(device="cuda"):
    return {k: torch.from_numpy(v).unsqueeze(0).to(device) for k, v in sd_glue_contexts().items()}


def test_frozen_copy_packs_once_and_never_moves():
    """bf16 configuration (its packed weight images are counted by weightimg.BF16_LAUNCHES): over three optimizer steps
    on the trained model the frozen copy packs on its first pass only and computes the same bits every time; the trained
    model re-packs after every step and its output changes."""
    from unlearn_saliency_amd import ops, weightimg
    from unlearn_saliency_amd.optim import FusedMaskedAdam
    from unlearn_saliency_amd.SD import train_scripts as TS
    m = _tiny(bf16=True)
    frozen = m.frozen_copy()
    assert not frozen.training and not any(p.requires_grad for p in frozen.parameters())
    assert all(getattr(p, "_salun_frozen", False) for p in frozen.parameters())
    assert not any(hasattr(p, "_salun_frozen") for p in m.parameters())
    assert np.array_equal(_bits(_flat(frozen)), _bits(_flat(m)))
    arena = TS._unet_arena(m)
    opt = FusedMaskedAdam(arena, lr=1e-3)
    z = torch.from_numpy(_np(1, 2, 4, 8, 8)).cuda()
    c = torch.from_numpy(_np(2, 2, 7, 24)).cuda()
    t = torch.tensor([3, 700]).cuda()
    noise = torch.from_numpy(_np(3, 2, 4, 8, 8)).cuda()
    m.train()
    f_packs, t_packs, f_out, t_out = [], [], [], []
    for _ in range(3):
        n0 = weightimg.BF16_LAUNCHES[0]
        with torch.no_grad():
            f_out.append(frozen.apply_model(z, t, c).clone())
        n1 = weightimg.BF16_LAUNCHES[0]
        opt.zero_grad()
        out = m.apply_model(z, t, c)
        n2 = weightimg.BF16_LAUNCHES[0]
        ops.mse_loss(noise, out).backward()
        opt.step()
        t_out.append(out.detach().clone())
        f_packs.append(n1 - n0)
        t_packs.append(n2 - n1)
    print("pack launches per pass: frozen", f_packs, "trained", t_packs)
    # (the first stale image met packs every stale image of the registry: on pass 1 that is the frozen copy's pass)
    assert f_packs[0] > 0 and f_packs[1:] == [0, 0], f_packs
    assert t_packs[1] > 0 and t_packs[2] > 0, t_packs
    assert np.array_equal(_bits(f_out[0]), _bits(f_out[1])) and np.array_equal(_bits(f_out[0]), _bits(f_out[2]))
    assert not np.array_equal(_bits(t_out[0]), _bits(t_out[1])) and not np.array_equal(_bits(t_out[1]), _bits(t_out[2]))


def test_ddim_sample_step_counts(base):
    """The exit rule at every till_T, as recorded by the reference run (S = 5: `timesteps[:t_start]` leaves 4 positions)."""
    from unlearn_saliency_amd.SD.ddim import DDIMSampler
    S = int(base["ddim_steps"])
    m = _tiny()
    smp = DDIMSampler(m).make_schedule(S, 0.0)
    ctx = _contexts()
    x_T = torch.from_numpy(base["esd_full_mask__start"][0]).cuda()
    keep = x_T.clone()
    recorded = {int(k): int(s) for tag in ("esd_full_mask", "esd_xattn", "esd_noxattn")
                for k, s in zip(base[f"{tag}__randint"][0::2], base[f"{tag}__steps"])}
    assert {0, S - 1} <= set(recorded)
    for till, want in sorted(recorded.items()) + [(None, S - 1), (1, S - 1)]:
        z = smp.sample(ctx[SD_GLUE_PROMPTS[0]], ctx[""], 3.0, x_T, till_T=till)
        assert smp.last_steps == want, (till, smp.last_steps, want)
        assert z.shape == x_T.shape and torch.isfinite(z).all() and torch.equal(x_T, keep)
    smp.sample(ctx[SD_GLUE_PROMPTS[0]], None, 1.0, x_T, till_T=S - 1)   # no guidance: B rows, one step
    assert smp.last_steps == 1


class replay_esd:
    """train_esd's draws in the reference's order: random.sample -> the recorded word, torch.randint -> t_enc and the
    DDPM timestep alternately, torch.randn -> the recorded start codes."""

    def __init__(self, base, tag):
        self.words = [str(w) for w in base[f"{tag}__words"]]
        self.ints = [int(v) for v in base[f"{tag}__randint"]]
        self.starts = [v for v in base[f"{tag}__start"]]

    def __enter__(self):
        self.real = (random.sample, torch.randint, torch.randn)
        w, i, s = self.words, self.ints, self.starts
        random.sample = lambda pop, k: [w.pop(0)]
        torch.randint = lambda *a, device=None, **k: torch.tensor([i.pop(0)], device=device or "cpu")
        torch.randn = lambda *a, **k: torch.from_numpy(s.pop(0).astype(np.float32))
        return self

    def __exit__(self, et, ev, tb):
        random.sample, torch.randint, torch.randn = self.real
        if et is None:
            assert not self.words and not self.ints and not self.starts, "recorded draws left over: the call order differs"


def _saliency_mask_file(m, base, path):
    unet = m.model.diffusion_model
    n = sum(p.numel() for p in unet.parameters())
    assert n == int(base["n_params"])
    bits = (rng.u8(n, int(base["mask_seed"])) & 1).astype(np.int64)
    off, mask = 0, {}
    for name, p in unet.named_parameters():
        mask[name] = torch.from_numpy(bits[off:off + p.numel()]).view_as(p)
        off += p.numel()
    torch.save(mask, path)
    return bits


def _check_state(base, tag, m, init, sel_bits, figures):
    """Adam moments and final weights against the reference's float64 run on the strided sample, at the fixture's
    bounds; untouched elements bit-identical to the initial weights, with zero moments."""
    stride = int(base["stride"])
    opt = m._salun_last_optimizer
    w = _flat(m)
    m1, m2 = opt.exp_avg.cpu().numpy(), opt.exp_avg_sq.cpu().numpy()
    for q, got in (("exp_avg", m1), ("exp_avg_sq", m2), ("weights", w)):
        figures[q] = (rel_max(got[::stride], base[f"{tag}_f64__{q}_s"]), float(base[f"{tag}__gap_{q}"]),
                      float(base[f"{tag}__bound_{q}"]))
    off = sel_bits == 0
    assert np.array_equal(_bits(w[off]), _bits(init[off])), "weights outside the selection / mask moved"
    assert not m1[off].any() and not m2[off].any(), "Adam moments outside the selection / mask"
    assert (w != init)[~off].mean() > 0.5, "selected weights did not move"


def _report_and_assert(tag, figures):
    for q, (err, gap, bound) in figures.items():
        print(f"{tag}: {q}: device vs float64 {err:.3e}; reference fp32 vs float64 {gap:.3e}; bound (4x) {bound:.3e}")
    bad = {q: v for q, v in figures.items() if not v[0] <= v[2]}
    assert not bad, bad


@pytest.mark.parametrize("tag,method,masked", [("esd_full_mask", "full", True), ("esd_xattn", "xattn", False),
                                               ("esd_noxattn", "noxattn", False)])
def test_train_esd_replays_the_reference_run(base, tag, method, masked, tmp_path):
    from unlearn_saliency_amd.SD import train_scripts as TS
    m = _tiny()
    init = _flat(m).copy()
    names = [n for n, _ in m.model.diffusion_model.named_parameters()]
    assert names == [str(n) for n in base["param_names"]]
    sizes = [p.numel() for p in m.model.diffusion_model.parameters()]
    sel = np.concatenate([np.full(s, TS.esd_selects(n, method), np.int64) for n, s in zip(names, sizes)])
    mask_path = None
    if masked:
        mask_path = str(tmp_path / "mask.pt")
        sel = sel & _saliency_mask_file(m, base, mask_path)
    S, iters = int(base["ddim_steps"]), len(base[f"{tag}__steps"])
    trace = []
    with replay_esd(base, tag):
        model, losses = TS.train_esd(str(base["prompt"]), method, 3.0, 1.0, iters, float(base["lr"]), None, None,
                                     mask_path, None, ["cuda:0", "cuda:0"], seperator=str(base["seperator"]),
                                     image_size=64, ddim_steps=S, model=m, contexts=_contexts(), trace=trace)
    assert model is m and len(losses) == iters and not m.training
    assert [t["steps"] for t in trace] == list(base[f"{tag}__steps"])
    assert [t["word"] for t in trace] == [str(w) for w in base[f"{tag}__words"]]
    figures = {"losses": (rel_max(losses, base[f"{tag}__losses__f64"]), float(base[f"{tag}__gap_losses"]),
                          float(base[f"{tag}__bound_losses"]))}
    z = np.stack([t["z"].cpu().numpy() for t in trace])
    e_0p = np.stack([t["e_0p"].cpu().numpy() for t in trace])
    for q, got in (("z", z), ("e_0", e_0p[:, :1]), ("e_p", e_0p[:, 1:])):
        figures[q] = (rel_max(got, base[f"{tag}__{q}__f64"]), float(base[f"{tag}__gap_{q}"]), float(base[f"{tag}__bound_{q}"]))
    _check_state(base, tag, m, init, sel, figures)
    _report_and_assert(tag, figures)


@pytest.mark.parametrize("tag,masked", [("ga_masked", True), ("ga_unmasked", False)])
def test_gradient_ascent_replays_the_reference_run(base, tag, masked, tmp_path):
    from unlearn_saliency_amd.SD import train_scripts as TS
    m = _tiny()
    init = _flat(m).copy()
    n = init.size
    sel = np.ones(n, np.int64)
    mask_path = None
    if masked:
        mask_path = str(tmp_path / "mask.pt")
        sel = _saliency_mask_file(m, base, mask_path)
    _, _, forget, remain = sd_glue_batches()
    cls = [torch.from_numpy(c) for c in sd_glue_class_contexts()]
    fdl = [(z.cuda(), cls[3].unsqueeze(0).repeat(len(z), 1, 1).cuda()) for z in forget]
    rdl = [(z.cuda(), torch.stack([cls[int(l)] for l in labs]).cuda()) for z, labs in zip(remain, base["ga__remain_labels"])]
    with replay_draws(base[f"{tag}__randint"], base[f"{tag}__randn"]):
        model, losses = TS.gradient_ascent(3, "full", 0.5, 4, 2, float(base["lr"]), None, None, mask_path, None, "cuda",
                                           image_size=8, model=m, forget_dl=fdl, remain_dl=rdl)
    assert model is m and len(losses) == 6
    figures = {"losses": (rel_max(losses, base[f"{tag}__losses__f64"]), float(base[f"{tag}__gap_losses"]),
                          float(base[f"{tag}__bound_losses"]))}
    _check_state(base, tag, m, init, sel, figures)
    _report_and_assert(tag, figures)


def test_train_esd_bf16_smoke(base, tmp_path):
    """One ESD iteration in the bf16 configuration: finite loss, masked weights untouched.  No parity claim."""
    from unlearn_saliency_amd.SD import train_scripts as TS
    m = _tiny(bf16=True)
    init = _flat(m).copy()
    mask_path = str(tmp_path / "mask.pt")
    bits = _saliency_mask_file(m, base, mask_path)
    torch.manual_seed(0)
    random.seed(0)
    _, losses = TS.train_esd(SD_GLUE_PROMPTS[0], "full", 3.0, 1.0, 1, 1e-4, None, None, mask_path, None, ["cuda:0"],
                             image_size=64, ddim_steps=5, model=m, contexts=_contexts())
    w = _flat(m)
    assert len(losses) == 1 and np.isfinite(losses[0])
    assert np.array_equal(_bits(w[bits == 0]), _bits(init[bits == 0])) and (w != init)[bits == 1].any()


@pytest.mark.parametrize("script", ["train-esd", "gradient_ascent"])
def test_baseline_command_lines_end_to_end(tmp_path, script):
    """train-esd.py (2 iterations) and gradient_ascent.py (1 epoch) with --synthetic on the tiny configuration: the files
    the reference names appear."""
    import subprocess
    import sys
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.path.join(root, "unlearn_saliency_amd", "SD", "train-scripts")
    cfg = {"model": {"params": {"unet_config": {"params": {k: (list(v) if isinstance(v, tuple) else v)
                                                             for k, v in sd_tiny_config().items()}}}}}
    with open(tmp_path / "tiny.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    env = dict(os.environ, PYTHONPATH=root)
    common = ["--config_path", str(tmp_path / "tiny.yaml"), "--ckpt_path", "none", "--synthetic", "2", "--lr", "1e-4"]
    if script == "train-esd":
        argv = ["--prompt", "Van Gogh, Kilian Eng", "--seperator", ",", "--train_method", "xattn", "--iterations", "2",
                "--devices", "0,0", "--image_size", "64", "--ddim_steps", "5"]
        name = "compvis-esd-method_xattn-lr_0.0001"
    else:
        argv = ["--class_to_forget", "0", "--train_method", "full", "--epochs", "1", "--batch_size", "4", "--device", "0"]
        name = "compvis-ga-method_full-alpha_0.1-epoch_1-lr_0.0001"
    r = subprocess.run([sys.executable, os.path.join(d, script + ".py")] + argv + common, cwd=str(tmp_path),
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    folder = tmp_path / "models" / name
    sd = torch.load(folder / f"{name}.pt", weights_only=False, map_location="cpu")
    assert any(k.startswith("model.diffusion_model.") for k in sd) and not any("ddim" in k for k in sd)
    assert (folder / f"{name.replace('compvis', 'diffusers')}.pt").exists()
    assert len(open(folder / "loss.txt").read()) > 0
