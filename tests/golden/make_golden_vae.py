"""Reference-run golden for the Stable-Diffusion first-stage encoder (SD/autoencoder.py).

    python tests/golden/make_golden_vae.py          ->  tests/golden/vae_encoder.npz

EXECUTES the reference's own classes, imported from /root/reference/SD (build container only):

    ldm.modules.diffusionmodules.model.Encoder                          (model.py:379-493)
    ldm.modules.distributions.distributions.DiagonalGaussianDistribution (distributions.py:24-)

on the CPU, with the tiny configuration of tests/vae_fixture.py (ch 32, ch_mult (1, 2, 2), one block per level,
resolution 32, z_channels 4) followed by a Conv2d(8, 8, 1) quant_conv, as AutoencoderKL.encode chains them
(ldm/models/autoencoder.py).  Weights are filled by name from vae_fixture.fill_by_name; the input is
vae_fixture.tiny_input().

Stored: data only - the key / shape list of the tiny tree and of the v1 first_stage_config
(configs/stable-diffusion/v1-inference.yaml: ch 128, ch_mult 1,2,4,4, two blocks per level), the input, the float64
moments and mode(), and the moments of the same module in fp32 (its distance from float64 is the tests' yardstick).
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
import vae_fixture as X  # noqa: E402

REF_SD = "/root/reference/SD"
sys.dont_write_bytecode = True
torch.set_num_threads(8)


class _RefKL(torch.nn.Module):
    """The two members of AutoencoderKL its `encode` uses, under their names."""

    def __init__(self, Encoder, ddconfig, embed_dim):
        super().__init__()
        self.encoder = Encoder(**ddconfig)
        self.quant_conv = torch.nn.Conv2d(2 * ddconfig["z_channels"], 2 * embed_dim, 1)

    def forward(self, x):
        return self.quant_conv(self.encoder(x))


def main():
    sys.path.insert(0, REF_SD)
    from ldm.modules.diffusionmodules.model import Encoder
    from ldm.modules.distributions.distributions import DiagonalGaussianDistribution

    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}
    tiny = X.load_filled(_RefKL(Encoder, X.TINY_DDCONFIG, X.TINY_EMBED_DIM)).eval()
    x = torch.from_numpy(X.tiny_input())
    with torch.no_grad():
        m32 = tiny(x)
        m64 = tiny.double()(x.double())
        mode = DiagonalGaussianDistribution(m64).mode()
    v1 = _RefKL(Encoder, X.V1_DDCONFIG, 4)
    tk, ts = X.pack_keys(shapes(tiny))
    vk, vs = X.pack_keys(shapes(v1))
    print("tiny:", len(tk), "tensors, moments", tuple(m64.shape), "fp32 error", float((m32.double() - m64).abs().max()),
          "of max", float(m64.abs().max()), "; v1:", len(vk), "tensors")
    np.savez_compressed(X.GOLDEN, tiny_keys=tk, tiny_shapes=ts, v1_keys=vk, v1_shapes=vs, x=x.numpy(),
                        moments64=m64.numpy(), moments32=m32.numpy(), mode64=mode.numpy())


if __name__ == "__main__":
    main()
