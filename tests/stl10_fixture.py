"""Inputs shared by tests/golden/make_golden_ddpm_stl10.py (which feeds them to the reference) and
tests/test_ddpm_stl10_gpu.py (which feeds them to the HIP path): the reduced STL-10 U-Net config, its batches and every
random draw of the captured steps.  All of it comes from the counter-based generator, so nothing but the reference's
results has to be stored."""
import numpy as np
import torch

from fixtures import ddpm_small_config
from unlearn_saliency_amd import rng

BATCH = 2
SIDE = 64
PARAM_SEED = 7000
FWD_T = (5.0, 750.0)


def config(n_iters=1):
    """The STL-10 U-Net with one ResnetBlock per level: ch 128 x [1, 2, 2, 2, 4], attention at 16 x 16, 64 x 64."""
    cfg = ddpm_small_config()
    cfg.data.dataset, cfg.data.image_size = "STL10", SIDE
    cfg.model.ch_mult, cfg.model.num_res_blocks, cfg.model.attn_resolutions = [1, 2, 2, 2, 4], 1, [16]
    cfg.training.batch_size, cfg.training.n_iters = BATCH, n_iters
    cfg.sampling.batch_size = BATCH
    return cfg


def batch(seed, label=None):
    """(x fp32 [2, 3, 64, 64] in [0, 1], c int64 [2])"""
    x = rng.uniform(BATCH * 3 * SIDE * SIDE, seed, 0.0, 1.0).reshape(BATCH, 3, SIDE, SIDE)
    c = (rng.u8(BATCH, seed + 1) % 10).astype(np.int64) if label is None else np.full(BATCH, label, np.int64)
    return x, c


def remain_batches():
    return [batch(300)]


def forget_batches():
    return [batch(400, label=0)]


# the i-th call of each kind, whichever run makes it
def randn_draw(i):
    return rng.normal(BATCH * 3 * SIDE * SIDE, 5000 + 10 * i).reshape(BATCH, 3, SIDE, SIDE)


def randint_draw(i):
    """BATCH // 2 + 1 timesteps in [0, 1000)"""
    v = rng.u8(2 * (BATCH // 2 + 1), 6000 + 10 * i).astype(np.int64)
    return (v[0::2] * 256 + v[1::2]) % 1000


def keep_draw(i):
    """the label-drop keep mask of one model call: sample 0 keeps its label, sample 1 alternates"""
    return np.array([True, i % 2 == 0])


def draws(n_randn, n_randint, n_keep):
    return dict(randn=[torch.from_numpy(randn_draw(i)) for i in range(n_randn)],
                randint=[torch.from_numpy(randint_draw(i)) for i in range(n_randint)],
                keep=[torch.from_numpy(keep_draw(i)) for i in range(n_keep)])
