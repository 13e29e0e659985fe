"""The STL-10 diffusion runs on the device: the five-level U-Net at 64 x 64 (ch 128 x [1, 2, 2, 2, 4], attention at
16 x 16, one ResnetBlock per level) against the REFERENCE's model and runner (tests/golden/ddpm_stl10.npz, made by
tests/golden/make_golden_ddpm_stl10.py; inputs and draws from tests/stl10_fixture.py), then sampling, the mask and the
data path end to end.

Bounds.  The goldens are the reference's fp64 run; e32_* in the fixture is how far the reference's own fp32 run is from
it on the same inputs.  Each bound is max(the CIFAR-10 test's constant, 4 x e32) — 4 is the margin of
profiles/svc_bounds_measured.txt; the constants are tests/test_ddpm_gpu.py's FWD_TOL = 2.5e-5 of the output's scale,
1e-5 relative for the loss, and rtol 1e-4 / atol 3e-3 for the per-tensor sums.  Every test prints what it measured
(profiles/stl10_bounds_measured.txt)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ddpm_ref_cpu as R
import resample_ref_cpu as RS
import stl10_fixture as SF
from fixtures import fill_params

pytestmark = pytest.mark.gpu

FWD_TOL, LOSS_RTOL, SUM_RTOL, SUM_ATOL, MARGIN = 2.5e-5, 1e-5, 1e-4, 3e-3, 4.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def t_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "ddpm_stl10.npz"))


@pytest.fixture()
def counters(monkeypatch):
    """Library-convolution calls from zero, and every attention call that goes to this package's GEMM counted."""
    from unlearn_saliency_amd import conv as sconv
    from unlearn_saliency_amd import gemm
    calls = {"attn": 0}
    real = gemm.attention_f32

    def counted(*a, **k):
        calls["attn"] += 1
        return real(*a, **k)

    monkeypatch.setattr(gemm, "attention_f32", counted)
    sconv.reset_library_conv_calls()
    return calls


def check_routes(model, calls, passes):
    """No library convolution; every ResnetBlock ran as the fused node for every shape it saw; every AttnBlock call of
    `passes` model passes went to the own GEMM."""
    from unlearn_saliency_amd import conv as sconv
    from unlearn_saliency_amd.DDPM.models.diffusion import AttnBlock, ResnetBlock
    assert sconv.library_conv_calls() == 0, sconv.LIBRARY_CONV_CALLS
    blocks = [m for m in model.modules() if isinstance(m, ResnetBlock)]
    attns = [m for m in model.modules() if isinstance(m, AttnBlock)]
    assert len(blocks) == 5 + 2 + 10 and len(attns) == 1 + 1 + 2
    for b in blocks:
        assert b.fused_node and b.__dict__.get("_fused_shapes"), "a ResnetBlock never reached the fused node"
        assert all(b._fused_shapes.values()), {k[0]: v for k, v in b._fused_shapes.items()}
    assert model.own_gemm and all(a.own_gemm for a in attns)
    assert calls["attn"] == passes * len(attns), (calls, passes)


def sums_close(got, ref, e32):
    """|got - ref| <= max(SUM_ATOL + SUM_RTOL |ref|, MARGIN e32 scale) per tensor; -> the worst excess over |ref| terms"""
    bound = np.maximum(SUM_ATOL + SUM_RTOL * np.abs(ref), MARGIN * e32 * np.abs(ref).max())
    dev = np.abs(got - ref)
    return dev, bound


def test_unet_forward_matches_the_reference(golden, counters):
    from unlearn_saliency_amd.conv import use_salun_convs
    from unlearn_saliency_amd.DDPM.models.diffusion import Conditional_Model
    model = fill_params(Conditional_Model(SF.config()), SF.PARAM_SEED).cuda().eval()
    assert use_salun_convs(model) > 0
    xb, cb = SF.batch(200)
    with torch.no_grad():
        out = model(t_(2 * xb - 1), torch.tensor(SF.FWD_T, device="cuda"), t_(cb), mode="test", cond_scale=2.0)
    out = out.double().cpu().numpy()
    ref = golden["fwd_test_s2"]
    assert out.shape == ref.shape == (SF.BATCH, 3, SF.SIDE, SF.SIDE)
    err = float(np.abs(out - ref).max() / np.abs(ref).max())
    tol = max(FWD_TOL, MARGIN * float(golden["e32_fwd"]))
    print(f"STL-10 U-Net forward vs the reference's fp64 output: max |err| = {err:.2e} of the output's scale "
          f"(bound {tol:.2e}; the reference's own fp32 run: {float(golden['e32_fwd']):.2e})")
    assert err <= tol, (err, tol)
    check_routes(model, counters, passes=2)  # eps(x, c) and eps(x, null)


@pytest.fixture()
def workdir(tmp_path):
    from unlearn_saliency_amd.DDPM.models.diffusion import Conditional_Model
    from unlearn_saliency_amd.DDPM.runners import diffusion as RD
    os.makedirs(tmp_path / "ckpts")
    init = fill_params(Conditional_Model(SF.config()), SF.PARAM_SEED)
    torch.save([RD.add_prefix(init.state_dict()), None, 0], str(tmp_path / "ckpts" / "ckpt.pth"))
    return str(tmp_path)


def _args(d, **kw):
    base = dict(ckpt_folder=d, label_to_forget=0, cond_scale=2.0, mask_path=None, method=None, alpha=1.0,
                mask_dir=os.path.join(d, "mask"), synthetic=True, library_conv=False)
    base.update(kw)
    return SimpleNamespace(**base)


def _loader(batches):
    return [tuple(t_(v) for v in b) for b in batches]


def _check_step(tag, golden, runner, model):
    loss = float(runner.step_losses[-1])
    ref = float(golden[f"{tag}_loss"])
    rel = abs(loss - ref) / abs(ref)
    tol = max(LOSS_RTOL, MARGIN * float(golden[f"e32_{tag}_loss"]))
    sums = np.array([float(p.detach().double().sum()) for p in model.parameters()])
    dev, bound = sums_close(sums, golden[f"{tag}_tensor_sums"], float(golden[f"e32_{tag}_sums"]))
    print(f"STL-10 {tag} step: loss {loss!r} vs {ref!r}, relative deviation {rel:.2e} (bound {tol:.2e}); per-tensor sums: "
          f"max |dev| {dev.max():.2e}, max dev / bound {float((dev / bound).max()):.2e} "
          f"(the reference's own fp32 run: {float(golden[f'e32_{tag}_sums']):.2e} of scale)")
    assert rel <= tol, (loss, ref, rel)
    assert (dev <= bound).all(), (int((dev > bound).sum()), float((dev / bound).max()))


def test_saliency_unlearn_rl_step_matches_the_reference(golden, workdir, counters, monkeypatch):
    from unlearn_saliency_amd.DDPM.runners import diffusion as RD
    monkeypatch.setattr(RD, "get_forget_dataset",
                        lambda *a, **k: (_loader(SF.remain_batches()), _loader(SF.forget_batches())))
    cfg = SF.config(n_iters=1)
    cfg.ckpt_dir = os.path.join(workdir, "out")
    os.makedirs(cfg.ckpt_dir)
    runner = RD.Diffusion(_args(workdir, method="rl", alpha=float(golden["alpha"])), cfg)
    with R.replay(**SF.draws(*golden["rl_draw_counts"])):
        model = runner.saliency_unlearn()
    _check_step("rl", golden, runner, model)
    check_routes(model, counters, passes=3)  # remain, forget, the no-grad target


def test_train_step_matches_the_reference(golden, workdir, counters):
    from unlearn_saliency_amd.DDPM.models.diffusion import Conditional_Model
    from unlearn_saliency_amd.DDPM.runners import diffusion as RD
    cfg = SF.config(n_iters=1)
    cfg.ckpt_dir = os.path.join(workdir, "out")
    os.makedirs(cfg.ckpt_dir)
    runner = RD.Diffusion(_args(workdir), cfg)
    model = fill_params(Conditional_Model(cfg), SF.PARAM_SEED).cuda()
    with R.replay(**SF.draws(*golden["train_draw_counts"])):
        model = runner._train(_loader(SF.remain_batches()), model=model)
    _check_step("train", golden, runner, model)
    check_routes(model, counters, passes=1)


def test_sample_classes_writes_64x64_pngs(tmp_path, monkeypatch):
    from PIL import Image
    from unlearn_saliency_amd.DDPM import sample
    monkeypatch.chdir(tmp_path)
    out = str(tmp_path / "run")
    assert sample.main(["--config", "stl10_sample.yml", "--ckpt_folder", out, "--mode", "sample_classes", "--timesteps",
                        "2", "--n_samples_per_class", "1", "--synthetic"]) == 0
    for cl in range(10):
        files = os.listdir(os.path.join(out, "class_samples", str(cl)))
        assert files == [f"{cl}.png"], (cl, files)
        img = Image.open(os.path.join(out, "class_samples", str(cl), files[0]))
        assert img.size == (64, 64) and img.mode == "RGB"
        assert np.asarray(img).shape == (64, 64, 3)


def _small_synthetic(monkeypatch):
    """The stand-in cut to 20 + 20 images: class 0 then has 4 of them, two batches of two."""
    from unlearn_saliency_amd.DDPM.datasets import stl10
    real = stl10.synthetic_stl10
    monkeypatch.setattr(stl10, "synthetic_stl10", lambda: real(20, 20))
    return real(20, 20)


def test_generate_mask_on_two_batches(workdir, monkeypatch, capsys):
    from unlearn_saliency_amd import conv as sconv
    from unlearn_saliency_amd.DDPM.runners import diffusion as RD
    _small_synthetic(monkeypatch)
    sconv.reset_library_conv_calls()
    runner = RD.Diffusion(_args(workdir), SF.config())
    masks = runner.generate_mask()
    assert "36 4" in capsys.readouterr().out          # remain / forget counts, printed as the reference prints them
    assert len(runner._forget_loader) == 2
    md = torch.load(os.path.join(workdir, "mask", "0", "with_0.5.pt"), weights_only=False)
    n = sum(v.numel() for v in md.values())
    ones = sum(int(v.sum()) for v in md.values())
    assert all(k.startswith("module.") and v.dtype == torch.int64 for k, v in md.items())
    assert ones == int(0.5 * n) == int(masks[0.5].sum()), (ones, n)
    assert sconv.library_conv_calls() == 0, sconv.LIBRARY_CONV_CALLS


def test_data_path_is_the_pillow_resize_on_the_device(monkeypatch):
    """`get_dataset` / `get_forget_dataset` on the stand-in: K26's bytes are the restatement's, ToTensor'd; the frozen
    flip of the forget path is the mirror of those bytes."""
    from unlearn_saliency_amd.DDPM import datasets as DS
    x96, y = _small_synthetic(monkeypatch)
    want = torch.from_numpy(RS.resize_u8(x96, (64, 64))).permute(0, 3, 1, 2).contiguous()
    # the loaders hold byte / 255 in fp32 (the device's division may differ from the host's in the last bit): back to bytes
    u8 = lambda x: (x.cpu() * 255).round().to(torch.uint8)
    cfg = SF.config()
    loader = DS.get_dataset(None, cfg, synthetic=True)
    assert loader.x.shape == (40, 3, 64, 64) and loader.x.is_cuda and loader.x.dtype == torch.float32
    assert float((loader.x.cpu() - want.float() / 255).abs().max()) <= 2.0 ** -24
    assert torch.equal(u8(loader.x), want) and torch.equal(loader.c.cpu(), torch.from_numpy(y))
    cfg.data.random_flip = True
    np.random.seed(3)
    flip = np.random.rand(40) < 0.5
    assert flip.any() and not flip.all()
    np.random.seed(3)
    remain, forget = DS.get_forget_dataset(None, cfg, 0, synthetic=True)
    mirrored = torch.where(torch.from_numpy(flip)[:, None, None, None], want.flip(3), want)
    assert torch.equal(u8(forget.x), mirrored[torch.from_numpy(y == 0)])
    assert torch.equal(u8(remain.x), mirrored[torch.from_numpy(y != 0)])
