"""The first-stage decoder on the device (SD/autoencoder.py: DecoderPlan on K27 - plain and with the nearest-2x input -,
K28, K15 and the byte kernel).

(a) the golden's tiny decoder against the reference-run float64 image;
(b) the v1 ddconfig on one [1, 4, 8, 8] latent against a float64 copy of our own module on the CPU;
(c) decode_u8 is the byte kernel applied to decode; an image's pixels do not depend on its batch; no CPU path.

The tolerance of (a) and (b) is vae_fixture.DEVICE_FACTOR times the distance of the SAME module in fp32 on the CPU
library from the float64 answer (largest absolute difference) - recorded in the golden for (a), computed here for (b).
The measured figures are logged (profiles/vae_dec_bounds_measured.txt)."""
import os

import pytest
import torch

import vae_dec_fixture as X

pytestmark = pytest.mark.gpu


def log(line):
    print(line)
    d = os.environ.get("SALUN_MEASURED_DIR")
    if d and os.path.isdir(d):
        with open(os.path.join(d, "vae_dec_bounds_measured.txt"), "a") as f:
            f.write(line + "\n")


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
    from unlearn_saliency_amd.SD.autoencoder import DecoderKLLite, DecoderPlan
    return DecoderPlan(X.load_filled(DecoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM)).cuda())


def test_tiny_decoder_against_the_reference_run():
    from unlearn_saliency_amd.SD import autoencoder
    g = X.golden()
    plan = tiny_plan()
    reset_counters()
    z = torch.from_numpy(g["z"]).cuda()
    got = plan.decode(z, scale=1.0)
    want = torch.from_numpy(g["image64"])
    yard = float((torch.from_numpy(g["image32"]).double() - want).abs().max())
    err = float((got.cpu().double() - want).abs().max())
    log(f"tiny decoder: fp32 CPU library {yard:.3e}, device {err:.3e} of max |pixel| {float(want.abs().max()):.3f} "
        f"(allowed {X.DEVICE_FACTOR} x the library's)")
    assert got.shape == (1, 3, 32, 32) and err <= X.DEVICE_FACTOR * yard
    assert counters_zero()
    assert autoencoder.ATTENTION_ROUTES == {"k15": 1, "library": 0}            # 64 tokens: K15
    padded = plan.decode_padded(z, scale=1.0)
    assert padded.shape == (1, 32, 32, 32) and bool((padded[:, 3:] == 0).all()) and torch.equal(padded[:, :3], got)
    assert torch.equal(plan.decode(z, scale=1.0), got)                          # the same bits again
    # the scale: 1 / scale * z in one rounding, then the same decoder
    s = autoencoder.SCALE_FACTOR
    assert torch.equal(plan.decode(z), plan.decode((1.0 / s) * z, scale=1.0))
    assert counters_zero()


def test_v1_decoder_against_float64():
    from unlearn_saliency_amd.SD import autoencoder
    from unlearn_saliency_amd.SD.autoencoder import DecoderKLLite, DecoderPlan
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model = X.load_filled(DecoderKLLite())
    z = torch.from_numpy(X.tiny_latent())
    with torch.no_grad():
        i32 = model(z).double()
        plan = DecoderPlan(model.cuda())
        reset_counters()
        got = plan.decode(z.cuda(), scale=1.0).cpu().double()
        calls_zero, routes = counters_zero(), dict(autoencoder.ATTENTION_ROUTES)
        want = model.cpu().double()(z.double())
    yard, err = float((i32 - want).abs().max()), float((got - want).abs().max())
    log(f"v1 decoder, 8 x 8 latent: fp32 CPU library {yard:.3e}, device {err:.3e} of max |pixel| "
        f"{float(want.abs().max()):.3f} (allowed {X.DEVICE_FACTOR} x the library's)")
    assert got.shape == (1, 3, 64, 64) and err <= X.DEVICE_FACTOR * yard
    assert calls_zero and routes == {"k15": 1, "library": 0}


def test_decode_u8_batch_independence_and_no_cpu_path():
    from unlearn_saliency_amd import ops_infer
    from unlearn_saliency_amd.SD.autoencoder import DecoderKLLite, DecoderPlan
    plan = tiny_plan()
    g = torch.Generator().manual_seed(5)
    z = (torch.randn(3, 4, 8, 8, generator=g) * 0.5).cuda()
    reset_counters()
    img = plan.decode(z)
    u8 = plan.decode_u8(z)
    assert u8.dtype == torch.uint8 and u8.shape == (3, 32, 32, 3)
    assert torch.equal(u8, ops_infer.decoded_to_u8(img))
    assert len(torch.unique(u8)) > 50                                           # an image, not a constant
    assert torch.equal(plan.decode(z[1:2])[0], img[1])
    assert torch.equal(plan.decode(z.flip(0)), img.flip(0))
    assert torch.equal(plan.decode_u8(z[2:3])[0], u8[2])
    assert counters_zero()
    with pytest.raises(RuntimeError, match="no CPU path"):
        DecoderPlan(DecoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM))
    with pytest.raises(ValueError):
        plan.decode(torch.zeros(1, 3, 8, 8).cuda())
