"""Shared by the first-stage decoder tests (test_vae_decoder_host.py, test_vae_decoder_gpu.py) and
tests/golden/make_golden_vae_dec.py: the golden's path and loader and the seeded latent.  The tiny configuration, the
weights filled by name, the key packing and the tolerance rule (DEVICE_FACTOR) are vae_fixture's."""
import functools
import os

import numpy as np

import vae_fixture as X
from vae_fixture import (DEVICE_FACTOR, TINY_DDCONFIG, TINY_EMBED_DIM, V1_DDCONFIG, fill_by_name, load_filled,  # noqa: F401
                         pack_keys, unpack_keys)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vae_decoder.npz")
LATENT_SEED = 31


def tiny_latent() -> np.ndarray:
    """[1, 4, 8, 8] float32: an UNSCALED latent (what post_quant_conv reads), a smooth field plus noise, a few units wide
    as the first stage's are."""
    r = np.random.default_rng(LATENT_SEED)
    yy, xx = np.mgrid[0:8, 0:8] / 8.0
    base = np.stack([np.sin(5.0 * xx + c) * np.cos(3.0 * yy - c) for c in range(4)])
    return (3.0 * base + 1.5 * r.standard_normal((4, 8, 8))).astype(np.float32)[None]


@functools.lru_cache(None)
def golden():
    return dict(np.load(GOLDEN))
