"""Host side of DDPM training from scratch (`train.py --mode train | retrain`): the command line, the loop of
`Diffusion._train` and its checkpoint, the remain-only loader of `retrain`, one training step against the reference's own
(tests/golden/make_golden_ddpm_train.py) and the handshake between `FusedMaskedAdam.attach_ema` and `EMAHelper.update`.
CPU: the kernels are replaced by the oracle (tests/cpu_standins.py) and by the restatement of salun_adam_ema_step
(tests/adam_ema_ref_cpu.py) for the duration of a test; the sampler kernels have no stand-in, so the snapshot's
`sample_visualization` is recorded instead of run."""
import glob
import logging
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import yaml

import adam_ema_ref_cpu as A
import ddpm_ref_cpu as R
from fixtures import ddpm_batch, ddpm_small_config, fill_params, flat_params

STRIDE = 997


@pytest.fixture()
def host_kernels():
    """The CPU stand-ins behind `ops` for one test; the module is put back as it was."""
    from unlearn_saliency_amd import ops
    saved = dict(vars(ops))
    epoch = ops.PARAM_EPOCH[0]
    A.install()
    A.CALLS.update(adam_ema_step=0, masked_adam_step=0)
    yield A.CALLS
    for k in [k for k in vars(ops) if k not in saved]:
        delattr(ops, k)
    for k, v in saved.items():
        setattr(ops, k, v)
    ops.PARAM_EPOCH[0] = max(ops.PARAM_EPOCH[0], epoch)


@pytest.fixture()
def host_runner(monkeypatch, host_kernels):
    """`Diffusion(args, config)` on the host: the constructor's tables on the CPU instead of the GPU check."""
    from unlearn_saliency_amd.DDPM.runners import diffusion as RD

    def init(self, args, config):
        self.args, self.config = args, config
        self._setup(torch.device("cpu"))

    monkeypatch.setattr(RD.Diffusion, "__init__", init)
    seen = []

    def visualization(self, model, name, cond_scale):
        seen.append((name, cond_scale, model.training, flat_params(model)))

    monkeypatch.setattr(RD.Diffusion, "sample_visualization", visualization)
    root = logging.getLogger()
    handlers, level = list(root.handlers), root.level
    yield SimpleNamespace(RD=RD, visualizations=seen)
    for h in [h for h in root.handlers if h not in handlers]:
        root.removeHandler(h)
        h.close()
    root.setLevel(level)


def _as_dict(ns):
    return {k: _as_dict(v) if hasattr(v, "__dict__") else v for k, v in vars(ns).items()}


def _small_yaml(path, **training):
    """The reduced U-Net of the DDPM goldens with ch_mult [1, 1], the EMA on, as a settings file."""
    cfg = ddpm_small_config()
    cfg.model.ch_mult = [1, 1]
    cfg.model.ema, cfg.model.ema_rate = True, 0.9
    cfg.training.log_freq = 1
    for k, v in training.items():
        setattr(cfg.training, k, v)
    with open(path, "w") as f:
        yaml.safe_dump(_as_dict(cfg), f)
    return cfg


def _tiny_set(n=40, size=16):
    """CIFAR-shaped uint8 set with balanced labels i % 10, as `synthetic_cifar10` returns it."""
    from unlearn_saliency_amd import rng
    x = rng.u8(n * size * size * 3, 4242).reshape(n, size, size, 3)
    y = (np.arange(n) % 10).astype(np.int64)
    return (x, y), (x[:10], y[:10])


@pytest.mark.parametrize("mode", ["train", "retrain"])
def test_train_and_retrain_run_and_write_a_checkpoint_sample_py_loads(tmp_path, monkeypatch, host_runner, mode):
    from unlearn_saliency_amd.DDPM import datasets, sample, train
    cfg_path = str(tmp_path / "small.yml")
    _small_yaml(cfg_path, n_iters=3, snapshot_freq=2)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(datasets, "synthetic_cifar10", _tiny_set)
    argv = ["--config", cfg_path, "--mode", mode, "--synthetic", "--library_conv", "--timesteps", "2"]
    if mode == "retrain":
        argv += ["--label_to_forget", "3"]
    assert train.main(argv) == 0  # 1 = the run raised (NotImplementedError before these modes existed)
    runs = glob.glob(str(tmp_path / "results" / "cifar10" / "*"))
    assert len(runs) == 1
    log = open(os.path.join(runs[0], "logs", "stdout.txt")).read()
    assert "NotImplementedError" not in log and "Traceback" not in log
    assert log.count("step: ") == 3  # log_freq 1: every step reports its loss
    states = torch.load(os.path.join(runs[0], "ckpts", "ckpt.pth"), weights_only=False)
    assert isinstance(states, list) and len(states) == 4
    model_sd, opt_sd, step, ema_sd = states
    assert step == 1  # snapshot_freq 2 over steps 0..2: written after step 1, as the reference numbers it
    assert model_sd and all(k.startswith("module.") for k in model_sd)
    from unlearn_saliency_amd.DDPM.functions import load_config
    from unlearn_saliency_amd.DDPM.models.diffusion import Conditional_Model
    names = [n for n, _ in Conditional_Model(load_config(cfg_path)).named_parameters()]
    assert list(ema_sd) == names  # the reference's EMAHelper registers the unwrapped module: no prefix
    assert all("module." + n in model_sd and ema_sd[n].shape == model_sd["module." + n].shape for n in names)
    assert any(not torch.equal(ema_sd[n], model_sd["module." + n]) for n in names)  # the average lags the weights
    assert set(opt_sd["state"][0]) == {"exp_avg", "exp_avg_sq", "step"} and float(opt_sd["state"][0]["step"]) == 2.0
    # the snapshot sampled the EMA copy, in eval mode, named by the step, at the command line's guidance scale
    assert len(host_runner.visualizations) == 1
    name, scale, training, weights = host_runner.visualizations[0]
    assert (name, scale, training) == (1, 2.0, False)
    assert np.array_equal(weights, np.concatenate([ema_sd[n].reshape(-1).numpy() for n in names]))
    # sample.py's loader takes it: the model gets states[0], the model it samples gets the EMA dict
    args, config = sample.parse_args_and_config(["--config", cfg_path, "--ckpt_folder", runs[0], "--mode",
                                                 "visualization", "--library_conv"])
    model, test_model = host_runner.RD.Diffusion(args, config).load_ema_model()
    assert test_model is not model and not test_model.training
    for n, p in model.named_parameters():
        assert torch.equal(p, model_sd["module." + n]), n
    for n, p in test_model.named_parameters():
        assert torch.equal(p, ema_sd[n]), n


def test_retrain_never_draws_the_class_to_forget(monkeypatch, host_runner):
    """Two passes over the remain split of a tiny synthetic set, through `Diffusion.retrain`'s own loader."""
    from unlearn_saliency_amd.DDPM import datasets
    monkeypatch.setattr(datasets, "synthetic_cifar10", _tiny_set)
    cfg = ddpm_small_config()
    cfg.model.ch_mult = [1, 1]
    cfg.training.batch_size = 6  # 36 remaining samples: 6 batches a pass
    cfg.training.n_iters = 12
    args = SimpleNamespace(label_to_forget=7, synthetic=True, library_conv=True, cond_scale=2.0)
    runner = host_runner.RD.Diffusion(args, cfg)
    consumed = []
    step = runner.train_step

    def recording_step(model, optimizer, batch, loader=None):
        consumed.append(batch[1].clone())
        return step(model, optimizer, batch, loader)

    monkeypatch.setattr(runner, "train_step", recording_step)
    runner.retrain()
    labels = torch.cat(consumed)
    assert labels.numel() == 72 and len(consumed) == 12  # 2 passes x 36
    assert not (labels == 7).any()
    counts = torch.bincount(labels, minlength=10)
    assert counts[7] == 0 and all(int(counts[k]) == 8 for k in range(10) if k != 7)  # every remaining sample, twice
    # `train` over the same set does draw it
    consumed.clear()
    cfg.training.n_iters = 7  # 40 samples in batches of 6: one pass
    runner.train()
    assert (torch.cat(consumed) == 7).sum() == 4


def _train_golden_run(runner_mod, golden_dir, device, library_conv=True):
    g = np.load(os.path.join(golden_dir, "ddpm_train_step.npz"))
    from unlearn_saliency_amd.DDPM.models.diffusion import Conditional_Model
    cfg = ddpm_small_config()
    cfg.training.n_iters = int(g["n_iters"])
    cfg.model.ema, cfg.model.ema_rate = True, float(g["ema_rate"])
    args = SimpleNamespace(label_to_forget=0, synthetic=True, library_conv=library_conv, cond_scale=2.0)
    runner = runner_mod.Diffusion(args, cfg)
    model = fill_params(Conditional_Model(cfg), 7000).to(device)
    before = flat_params(model)
    batches = [tuple(torch.from_numpy(v).to(device) for v in ddpm_batch(4, 300 + i)) for i in range(2)]
    with R.replay(randn=g["randn"], randint=g["randint"], keep=g["keep"]):
        model = runner._train(batches, model=model)
    return g, cfg, runner, model, before


def test_two_training_steps_match_the_reference(golden_dir, host_runner):
    """Tolerances: those of test_ddpm_oracle_vs_golden.py for ddpm_unlearn_rl.npz.  The shadow after two steps is
    mu^2 s0 + mu w p1 + w p2 (w = 1 - mu): linear in the weights, so it inherits their bounds times w (1 + mu)."""
    g, cfg, runner, model, before = _train_golden_run(host_runner.RD, golden_dir, torch.device("cpu"))
    assert host_kernels_used(A.CALLS) == ("folded", 2)
    losses = np.array([float(v) for v in runner.step_losses], np.float64)
    assert np.allclose(losses, g["step_loss"], rtol=1e-5, atol=0), (losses, g["step_loss"])
    opt, ema = runner.last_optimizer, runner.last_ema
    m1, v = opt.exp_avg.numpy(), opt.exp_avg_sq.numpy()
    s1, s2 = np.abs(g["exp_avg_sample"]).max(), np.abs(g["exp_avg_sq_sample"]).max()
    assert np.allclose(m1[::STRIDE], g["exp_avg_sample"], rtol=1e-4, atol=1e-5 * s1)
    assert np.allclose(v[::STRIDE], g["exp_avg_sq_sample"], rtol=2e-4, atol=1e-5 * s2)
    assert abs(np.linalg.norm(m1.astype(np.float64)) - float(g["exp_avg_norm"])) <= 1e-5 * float(g["exp_avg_norm"])
    assert abs(v.astype(np.float64).sum() - float(g["exp_avg_sq_sum"])) <= 2e-5 * float(g["exp_avg_sq_sum"])
    lr = cfg.optim.lr
    got, ref = flat_params(model)[::STRIDE], g["param_sample"]
    close = np.abs(got - ref) <= 0.02 * lr + 1e-6 * np.abs(ref)
    assert close.mean() > 0.995, close.mean()
    assert np.abs(got - ref).max() <= 2.5 * lr * 2
    sums = np.array([float(p.detach().double().sum()) for p in model.parameters()])
    assert np.allclose(sums, g["tensor_sums"], rtol=1e-4, atol=2e-3)
    mu = float(g["ema_rate"])
    k = (1.0 - mu) * (1.0 + mu)
    assert list(ema.state_dict()) == [str(n) for n in g["shadow_keys"]]
    sh = ema._flat.numpy()
    got, ref = sh[::STRIDE], g["shadow_sample"]
    assert np.abs(ref - before[::STRIDE]).max() > 0.01 * lr  # the captured average did move
    close = np.abs(got - ref) <= k * 0.02 * lr + 1e-6 * np.abs(ref)
    assert close.mean() > 0.995, close.mean()
    assert np.abs(got - ref).max() <= k * 2.5 * lr * 2
    assert abs(sh.astype(np.float64).sum() - float(g["shadow_sum"])) <= 1e-4 * abs(float(g["shadow_sum"])) + 2e-3


def host_kernels_used(calls):
    if calls["adam_ema_step"] and not calls["masked_adam_step"]:
        return "folded", calls["adam_ema_step"]
    if calls["masked_adam_step"] and not calls["adam_ema_step"]:
        return "plain", calls["masked_adam_step"]
    return "mixed", calls["adam_ema_step"] + calls["masked_adam_step"]


# ------------------------------------------------------------------------------------------ the EMA handshake
class Toy(nn.Module):
    """Three parameter tensors of sizes no multiple of four."""

    def __init__(self):
        super().__init__()
        self.a = nn.Linear(5, 7)
        self.b = nn.Parameter(torch.zeros(3))

    def forward(self, x):
        return self.a(x).sum() + (self.b * self.b).sum()


def _toy(seed=11, frozen=False):
    from unlearn_saliency_amd import rng
    from unlearn_saliency_amd.DDPM.models.ema import EMAHelper
    from unlearn_saliency_amd.flat import arena_of
    from unlearn_saliency_amd.optim import FusedMaskedAdam
    m = Toy()
    with torch.no_grad():
        for i, p in enumerate(m.parameters()):
            p.copy_(torch.from_numpy(rng.normal(p.numel(), seed + i, 0.0, 0.5)).view_as(p))
    if frozen:
        m.b.requires_grad_(False)  # the shadow then skips `b` and no longer lines up with the arena
    arena = arena_of(m)
    opt = FusedMaskedAdam(arena, lr=1e-2, grad_clip=1.0)
    ema = EMAHelper(mu=0.9)
    ema.register(m)
    return m, arena, opt, ema


def _set_grads(arena, seed):
    from unlearn_saliency_amd import rng
    arena.grads.copy_(torch.from_numpy(rng.normal(arena.n, seed, 0.0, 0.3)))


def _lerp_ref(shadow, p, mu, times=1):
    s = shadow.copy()
    for _ in range(times):
        A.ema_lerp(s, p, mu)
    return s


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()


@pytest.mark.parametrize("attach", [True, False])
def test_step_then_update_moves_the_shadow_exactly_once(host_kernels, attach):
    m, arena, opt, ema = _toy()
    if attach:
        assert ema.attach_to(opt, m)
    s0 = ema._flat.numpy().copy()
    for k in range(3):
        _set_grads(arena, 50 + k)
        opt.step()
        ema.update(m)
        want = _lerp_ref(s0, arena.params.numpy(), 0.9)
        got = ema._flat.numpy()
        # torch's host lerp_ may or may not fuse the multiply-add: one ulp; zero or two applications are ~1e-3 away
        assert _ulps(got, want) <= 1, (k, _ulps(got, want))
        assert np.abs(got - s0).max() > 1e-4 and np.abs(_lerp_ref(s0, arena.params.numpy(), 0.9, 2) - got).max() > 1e-5
        s0 = got.copy()
    assert host_kernels_used(host_kernels) == (("folded", 3) if attach else ("plain", 3))
    assert opt.steps == 3


def test_a_second_update_after_one_step_is_applied_on_the_plain_path(host_kernels):
    m, arena, opt, ema = _toy()
    assert ema.attach_to(opt, m)
    s0 = ema._flat.numpy().copy()
    _set_grads(arena, 60)
    opt.step()
    ema.update(m)  # the step's own: consumed
    once = ema._flat.numpy().copy()
    assert _ulps(once, _lerp_ref(s0, arena.params.numpy(), 0.9)) == 0
    ema.update(m)  # a further one: the average is taken again, by EMAHelper itself
    twice = ema._flat.numpy()
    assert _ulps(twice, _lerp_ref(once, arena.params.numpy(), 0.9)) <= 1
    assert np.abs(twice - once).max() > 1e-5
    # a folded step whose update() never comes does not swallow a later step's
    _set_grads(arena, 61)
    opt.step()
    _set_grads(arena, 62)
    opt.step()
    before = ema._flat.numpy().copy()
    ema.update(m)
    assert np.array_equal(ema._flat.numpy(), before)
    ema.update(m)
    assert not np.array_equal(ema._flat.numpy(), before)


def test_a_shadow_that_does_not_line_up_with_the_arena_is_not_attached(host_kernels):
    m, arena, opt, ema = _toy(frozen=True)
    assert ema._arena_params(m) is None and not ema.attach_to(opt, m)
    s0 = {k: v.clone() for k, v in ema.shadow.items()}
    _set_grads(arena, 70)
    opt.step()
    ema.update(m)
    assert host_kernels_used(host_kernels) == ("plain", 1)
    for k, p in m.named_parameters():
        if p.requires_grad:
            assert torch.allclose(ema.shadow[k], 0.9 * s0[k] + 0.1 * p.detach(), rtol=1e-6, atol=1e-7)
    with pytest.raises(ValueError):
        opt.attach_ema(torch.zeros(arena.n - 1), 0.9)
    with pytest.raises(ValueError):
        opt.attach_ema(torch.zeros(arena.n), 0.3)  # 1 - mu >= 0.5: lerp takes its other form


def test_ema_writes_are_seen_by_the_weight_image_cache():
    """`ema()` used to write through `param.data`, which bumps neither the parameter's version nor the epoch."""
    from unlearn_saliency_amd import weightimg
    from unlearn_saliency_amd.DDPM.models.ema import EMAHelper
    m = Toy()
    ema = EMAHelper(mu=0.9)
    ema.register(m)
    with torch.no_grad():
        for v in ema.shadow.values():
            v.add_(1.0)
    keys = [weightimg.key(p) for p in m.parameters()]
    ema.ema(m)
    assert all(weightimg.key(p) != k for p, k in zip(m.parameters(), keys))
    assert all(torch.equal(p, ema.shadow[n]) for n, p in m.named_parameters())
    assert all(p.requires_grad and p.is_leaf for p in m.parameters())
