"""The first-stage decoder's module tree on the CPU (SD/autoencoder.py: DecoderKLLite) against the reference run of
tests/golden/vae_decoder.npz: the state_dict keys and shapes, the forward, the checkpoint loader."""
import pytest
import torch

import vae_dec_fixture as X


def shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def tiny():
    from unlearn_saliency_amd.SD.autoencoder import DecoderKLLite
    return X.load_filled(DecoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM))


def test_keys_and_shapes_are_the_references():
    from unlearn_saliency_amd.SD.autoencoder import DecoderKLLite
    g = X.golden()
    assert shapes(DecoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM)) == X.unpack_keys(g["tiny_keys"], g["tiny_shapes"])
    v1 = shapes(DecoderKLLite())
    assert v1 == X.unpack_keys(g["v1_keys"], g["v1_shapes"])
    assert all(k.startswith(("decoder.", "post_quant_conv.")) for k in v1)
    assert v1["decoder.up.3.upsample.conv.weight"] == (512, 512, 3, 3) and "decoder.up.0.upsample.conv.weight" not in v1


def test_forward_matches_the_reference_run():
    g = X.golden()
    with torch.no_grad():
        got = tiny()(torch.from_numpy(g["z"]))
    want32, want64 = torch.from_numpy(g["image32"]), torch.from_numpy(g["image64"])
    assert got.shape == (1, 3, 32, 32)
    yard = float((want32.double() - want64).abs().max())
    # the same library ops in the same order: a few ulps of threading differences at most
    assert float((got - want32).abs().max()) <= 2 * yard
    assert float((got.double() - want64).abs().max()) <= 2 * yard


def test_load_compvis_ignores_the_encoder_and_names_a_missing_key():
    from unlearn_saliency_amd.SD.autoencoder import AutoencoderKLLite, DecoderKLLite
    src = tiny()
    sd = {"first_stage_model." + k: v.clone() for k, v in src.state_dict().items()}
    enc = AutoencoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM)
    sd.update({"first_stage_model." + k: v for k, v in enc.state_dict().items()})      # encoder.*, quant_conv.*
    sd["first_stage_model.loss.logvar"] = torch.zeros(())
    sd["first_stage_model.model_ema.decay"] = torch.zeros(())
    sd["model.diffusion_model.out.2.bias"] = torch.zeros(4)
    dst = DecoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM).load_compvis({"state_dict": sd})
    assert all(torch.equal(v, src.state_dict()[k]) for k, v in dst.state_dict().items())
    bare = DecoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM).load_compvis(dict(src.state_dict(), **enc.state_dict()))
    assert all(torch.equal(v, src.state_dict()[k]) for k, v in bare.state_dict().items())
    missing = {k: v for k, v in sd.items() if k != "first_stage_model.decoder.up.1.upsample.conv.bias"}
    with pytest.raises(KeyError, match="decoder.up.1.upsample.conv.bias"):
        DecoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM).load_compvis(missing)
    bad = dict(sd)
    bad["first_stage_model.post_quant_conv.weight"] = torch.zeros(4, 8, 1, 1)
    with pytest.raises(ValueError, match="post_quant_conv.weight"):
        DecoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM).load_compvis(bad)
    extra = dict(sd)
    extra["first_stage_model.decoder.up.9.block.0.conv1.weight"] = torch.zeros(1)
    with pytest.raises(KeyError, match="decoder.up.9"):
        DecoderKLLite(X.TINY_DDCONFIG, X.TINY_EMBED_DIM).load_compvis(extra)
    # the encoder's tree and keys are what they were
    assert all(k.startswith(("encoder.", "quant_conv.")) for k in enc.state_dict())
