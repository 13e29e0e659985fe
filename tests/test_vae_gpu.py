"""The first-stage encoder on the device (SD/autoencoder.py: EncoderPlan on K27 / K28 / K15 and the posterior kernel).

(a) the Downsample layer as ONE K27 call: pad = 0 with the caller's P = H / 2 - taps past the high edge read zero;
(b) the golden's tiny encoder against the reference-run float64 moments;
(c) the v1 ddconfig on one 64 x 64 image against a float64 copy of our own module on the CPU;
(d) first_stage(seed) plugged into LatentDiffusionLite;
(e) encode_images.py --synthetic writes a file _common.batches loads.

The tolerance of (b) and (c) is vae_fixture.DEVICE_FACTOR times the distance of the SAME module in fp32 on the CPU
library from the float64 answer (largest absolute difference) - recorded in the golden for (b), computed here for (c).
The measured figures are logged (profiles/vae_bounds_measured.txt)."""
import json
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

import conv_infer_ref_cpu as CR
import vae_fixture as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def log(line):
    print(line)
    d = os.environ.get("SALUN_MEASURED_DIR")
    if d and os.path.isdir(d):
        with open(os.path.join(d, "vae_bounds_measured.txt"), "a") as f:
            f.write(line + "\n")


def _script(name):
    import importlib.util
    d = os.path.join(ROOT, "unlearn_saliency_amd", "SD", "train-scripts")
    if d not in sys.path:
        sys.path.insert(0, d)
    spec = importlib.util.spec_from_file_location("sd_cli_" + name.replace("-", "_"), os.path.join(d, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def counters_zero():
    from unlearn_saliency_amd import conv_infer, norm
    return conv_infer.library_infer_calls() == 0 and all(v == 0 for v in norm.LIBRARY_GN_SPLIT_CALLS.values())


def reset_counters():
    from unlearn_saliency_amd import conv_infer, norm
    from unlearn_saliency_amd.SD import autoencoder
    conv_infer.reset_library_infer_calls()
    norm.reset_library_gn_split_calls()
    for k in autoencoder.ATTENTION_ROUTES:
        autoencoder.ATTENTION_ROUTES[k] = 0


def tiny_plan():
    from unlearn_saliency_amd.SD.autoencoder import AutoencoderKLLite, EncoderPlan
    return EncoderPlan(X.load_filled(AutoencoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM)).cuda())


# ------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("side,asked", [(6, (3, 3)), (7, None)], ids=["6x6 high-side zeros", "7x7 no tap outside"])
def test_downsample_is_one_k27_call(side, asked):
    """x [1, 8, side, side], 3 x 3 / 2, pad = 0, P = Q = 3 against F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, 2) in float64;
    every element within gamma_(2 n + 1) * abs_sum (n = C R R products, one epilogue addition)."""
    from unlearn_saliency_amd import conv_infer
    reset_counters()
    g = torch.Generator().manual_seed(side)
    x = torch.randn(1, 8, side, side, generator=g)
    w = torch.randn(32, 8, 3, 3, generator=g)
    b = torch.randn(32, generator=g)
    xp = F.pad(x.double(), (0, 1, 0, 1))
    want = F.conv2d(xp, w.double(), b.double(), 2)[:, :, :3, :3]
    abs_sum = F.conv2d(xp.abs(), w.double().abs(), b.double().abs(), 2)[:, :, :3, :3]
    assert want.shape == (1, 32, 3, 3)
    y = conv_infer.conv_bn_act(x.cuda(), w.cuda(), None, b.cuda(), stride=2, pad=0, out_size=asked)
    assert y.shape == (1, 32, 3, 3) and conv_infer.library_infer_calls() == 0
    err = (y.cpu().double() - want).abs()
    n = 8 * 3 * 3
    log(f"downsample on K27 {side} x {side}: worst |got - exact| = {float((err / (CR.U * abs_sum)).max()):.3f} u * abs_sum "
        f"(bound {CR.bound_gamma(2 * n + 1) / CR.U:.1f})")
    assert bool((err <= CR.bound_gamma(2 * n + 1) * abs_sum).all())
    if asked is not None:          # the last row and column saw the zeros: they differ from a convolution that wraps or clamps
        inner = F.conv2d(x.double(), w.double(), b.double(), 2)
        assert inner.shape[-1] == 2 and torch.allclose(y.cpu().double()[:, :, :2, :2], inner, rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------ (b)
def test_tiny_encoder_against_the_reference_run():
    from unlearn_saliency_amd.SD import autoencoder
    g = X.golden()
    plan = tiny_plan()
    reset_counters()
    x = torch.from_numpy(g["x"]).cuda()
    got = plan.encode_moments(x)
    want = torch.from_numpy(g["moments64"])
    yard = float((torch.from_numpy(g["moments32"]).double() - want).abs().max())
    err = float((got.cpu().double() - want).abs().max())
    log(f"tiny encoder: fp32 CPU library {yard:.3e}, device {err:.3e} of max |moment| {float(want.abs().max()):.3f} "
        f"(allowed {X.DEVICE_FACTOR} x the library's)")
    assert got.shape == (1, 8, 8, 8) and err <= X.DEVICE_FACTOR * yard
    assert counters_zero()
    assert autoencoder.ATTENTION_ROUTES == {"k15": 1, "library": 0}            # 64 tokens: K15
    padded = plan.encode_moments_padded(x)
    assert padded.shape == (1, 32, 8, 8) and bool((padded[:, 8:] == 0).all()) and torch.equal(padded[:, :8], got)
    assert torch.equal(plan.encode_moments(x), got)                             # the same bits again
    # mode(): scale * mean, one rounding
    z = plan.encode(x, None, seed=0, deterministic=True, scale=1.0)
    assert torch.equal(z, got[:, :4])
    # uint8 input: the device normalisation feeds the same encoder
    u8 = ((torch.from_numpy(g["x"]) * 0.5 + 0.5) * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    xn = CR.normalize_u8(u8, (0.5,) * 3, (0.5,) * 3)
    assert torch.equal(plan.encode_moments(u8.cuda()), plan.encode_moments(xn.cuda()))
    assert counters_zero()


def test_an_image_does_not_depend_on_its_batch():
    plan = tiny_plan()
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(3, 3, 32, 32, generator=g) * 2 - 1).cuda()
    ids = [7, 8, 9]
    z = plan.encode(x, ids, seed=5, draw=1)
    assert z.shape == (3, 4, 8, 8)
    assert torch.equal(plan.encode(x[1:2], ids[1:2], seed=5, draw=1)[0], z[1])
    assert torch.equal(plan.encode(x.flip(0), ids[::-1], seed=5, draw=1), z.flip(0))
    assert not torch.equal(plan.encode(x, ids, seed=5, draw=2), z)


# ------------------------------------------------------------------------------------------ (c)
def test_v1_encoder_against_float64():
    from unlearn_saliency_amd.SD import autoencoder
    from unlearn_saliency_amd.SD.autoencoder import AutoencoderKLLite, EncoderPlan
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model = X.load_filled(AutoencoderKLLite())
    g = torch.Generator().manual_seed(4)
    x = (torch.rand(1, 3, 64, 64, generator=g) * 2 - 1)
    with torch.no_grad():
        m32 = model(x).double()
        plan = EncoderPlan(model.cuda())
        reset_counters()
        got = plan.encode_moments(x.cuda()).cpu().double()
        want = model.cpu().double()(x.double())
    yard, err = float((m32 - want).abs().max()), float((got - want).abs().max())
    log(f"v1 encoder, 64 x 64: fp32 CPU library {yard:.3e}, device {err:.3e} of max |moment| {float(want.abs().max()):.3f} "
        f"(allowed {X.DEVICE_FACTOR} x the library's)")
    assert got.shape == (1, 8, 8, 8) and err <= X.DEVICE_FACTOR * yard
    assert counters_zero() and autoencoder.ATTENTION_ROUTES == {"k15": 1, "library": 0}


# ------------------------------------------------------------------------------------------ (d)
def test_first_stage_in_latent_diffusion_lite():
    from fixtures import sd_tiny_config
    from unlearn_saliency_amd.SD.ldm_lite import LatentDiffusionLite
    seed = 12
    ctx = torch.zeros(2, 77, 8)
    m = LatentDiffusionLite(sd_tiny_config(), first_stage=tiny_plan().first_stage(seed), cond_stage=lambda txt: ctx.cuda()).cuda()
    g = torch.Generator().manual_seed(6)
    batch = {"jpg": torch.rand(2, 32, 32, 3, generator=g) * 2 - 1, "txt": ["a", "b"]}
    z1, c1 = m.get_input(batch)
    z2, _ = m.get_input(batch)
    assert z1.shape == (2, 4, 8, 8) and z1.is_cuda and c1.shape == (2, 77, 8)
    assert not torch.equal(z1, z2)                                              # every fetch draws afresh
    x = batch["jpg"].permute(0, 3, 1, 2).cuda()
    ref = tiny_plan()
    assert torch.equal(z1, ref.encode(x, [0, 1], seed, 0, False, 1.0) * m.scale_factor)
    assert torch.equal(z2, ref.encode(x, [2, 3], seed, 0, False, 1.0) * m.scale_factor)
    assert m.scale_factor == 0.18215


# ------------------------------------------------------------------------------------------ (e)
def test_encode_images_synthetic_writes_a_latents_file(tmp_path):
    out = tmp_path / "latents.pt"
    cli = _script("encode_images")
    cli.main(["--synthetic", "2", "--ddconfig", json.dumps(X.TINY_DDCONFIG), "--image_size", "32", "--batch_size", "2",
              "--context_dim", "8", "--seed", "1", "--out", str(out)])
    common = _script("_common")
    args = types.SimpleNamespace(latents=str(out), synthetic=0, batch_size=2)
    data = common.batches(args, "cuda:0", {"forget": 3, "remain": 2})
    assert len(data["forget"]) == 2 and len(data["remain"]) == 2
    for kind, n in (("forget", 3), ("remain", 2)):
        for b in data[kind]:
            assert len(b) == n and b[0].shape == (2, 4, 8, 8) and all(c.shape == (2, 77, 8) for c in b[1:])
            assert all(t.dtype == torch.float32 and t.device == torch.device("cuda:0") for t in b)
            assert bool(torch.isfinite(b[0]).all())
    assert not torch.equal(data["forget"][0][0], data["forget"][1][0])
    again = tmp_path / "again.pt"
    cli.main(["--synthetic", "2", "--ddconfig", json.dumps(X.TINY_DDCONFIG), "--image_size", "32", "--batch_size", "4",
              "--context_dim", "8", "--seed", "1", "--out", str(again)])
    one = torch.load(again, weights_only=False)["forget"][0][0]
    assert torch.equal(one[:2], data["forget"][0][0].cpu())                     # a latent does not depend on --batch_size
