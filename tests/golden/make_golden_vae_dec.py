"""Reference-run golden for the Stable-Diffusion first-stage decoder (SD/autoencoder.py: DecoderKLLite, DecoderPlan).

    python tests/golden/make_golden_vae_dec.py          ->  tests/golden/vae_decoder.npz

EXECUTES the reference's own class, imported from /root/reference/SD (build container only):

    ldm.modules.diffusionmodules.model.Decoder                          (model.py:496-625)

on the CPU, with the tiny configuration of tests/vae_fixture.py (ch 32, ch_mult (1, 2, 2), one block per level - two in
the decoder, which adds one -, resolution 32, z_channels 4) behind a Conv2d(4, 4, 1) post_quant_conv, as
AutoencoderKL.decode chains them (ldm/models/autoencoder.py).  Weights are filled by name from vae_fixture.fill_by_name;
the latent is vae_dec_fixture.tiny_latent().

Stored: data only - the key / shape list of the tiny tree and of the v1 first_stage_config
(configs/stable-diffusion/v1-inference.yaml), the latent, the float64 image and the image of the same module in fp32
(its distance from float64 is the tests' yardstick).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE),):
    if p not in sys.path:
        sys.path.insert(0, p)
import vae_dec_fixture as X  # noqa: E402

REF_SD = "/root/reference/SD"
sys.dont_write_bytecode = True
torch.set_num_threads(8)


class _RefKL(torch.nn.Module):
    """The two members of AutoencoderKL its `decode` uses, under their names."""

    def __init__(self, Decoder, ddconfig, embed_dim):
        super().__init__()
        self.decoder = Decoder(**ddconfig)
        self.post_quant_conv = torch.nn.Conv2d(embed_dim, ddconfig["z_channels"], 1)

    def forward(self, z):
        return self.decoder(self.post_quant_conv(z))


def main():
    sys.path.insert(0, REF_SD)
    from ldm.modules.diffusionmodules.model import Decoder

    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}
    tiny = X.load_filled(_RefKL(Decoder, X.TINY_DDCONFIG, X.TINY_EMBED_DIM)).eval()
    z = torch.from_numpy(X.tiny_latent())
    with torch.no_grad():
        i32 = tiny(z)
        i64 = tiny.double()(z.double())
    v1 = _RefKL(Decoder, X.V1_DDCONFIG, 4)
    tk, ts = X.pack_keys(shapes(tiny))
    vk, vs = X.pack_keys(shapes(v1))
    print("tiny:", len(tk), "tensors, image", tuple(i64.shape), "fp32 error", float((i32.double() - i64).abs().max()),
          "of max", float(i64.abs().max()), "; v1:", len(vk), "tensors")
    np.savez_compressed(X.GOLDEN, tiny_keys=tk, tiny_shapes=ts, v1_keys=vk, v1_shapes=vs, z=z.numpy(),
                        image64=i64.numpy(), image32=i32.numpy())


if __name__ == "__main__":
    main()
