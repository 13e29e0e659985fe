"""Shared by the first-stage encoder tests (test_vae_host.py, test_vae_gpu.py) and tests/golden/make_golden_vae.py: the
tiny encoder configuration, the seeded weights filled BY NAME (so the reference's module and ours get the same numbers
whatever order they register their parameters in), the golden's loader, and the tolerance rule.

The tolerance of the network comparisons is not a fixed number: the device may be DEVICE_FACTOR = 8 times as far from
the float64 moments as the SAME module tree in fp32 on the CPU library is (the largest absolute difference) - the
factor and form of classifier_eval_fixture.py - because its kernels sum in another order through every layer."""
import functools
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vae_encoder.npz")
DEVICE_FACTOR = 8
WEIGHT_SEED, INPUT_SEED = 28, 29
TINY_DDCONFIG = dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=(1, 2, 2),
                     num_res_blocks=1, attn_resolutions=(), dropout=0.0)
TINY_EMBED_DIM = 4
V1_DDCONFIG = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=(1, 2, 4, 4),
                   num_res_blocks=2, attn_resolutions=(), dropout=0.0)


def fill_by_name(shapes: dict, seed: int = WEIGHT_SEED) -> dict:
    """name -> float32 array.  Names are visited in sorted order, each from its own child of one seeded generator.
    Convolution weights are N(0, 1 / fan_in) (activations keep their size through the depth), norm weights 1 + 0.1 N,
    every bias 0.1 N."""
    out = {}
    for i, name in enumerate(sorted(shapes)):
        r = np.random.default_rng([seed, i])
        shape = tuple(int(v) for v in shapes[name])
        if name.endswith("bias"):
            a = 0.1 * r.standard_normal(shape)
        elif len(shape) == 1:
            a = 1.0 + 0.1 * r.standard_normal(shape)
        else:
            a = r.standard_normal(shape) / np.sqrt(np.prod(shape[1:]))
        out[name] = a.astype(np.float32)
    return out


def load_filled(module: torch.nn.Module, seed: int = WEIGHT_SEED) -> torch.nn.Module:
    sd = module.state_dict()
    filled = fill_by_name({k: tuple(v.shape) for k, v in sd.items()}, seed)
    module.load_state_dict({k: torch.from_numpy(filled[k]).to(sd[k].dtype) for k in sd})
    return module


def tiny_input() -> np.ndarray:
    """[1, 3, 32, 32] float32 in [-1, 1]: a smooth field plus noise."""
    r = np.random.default_rng(INPUT_SEED)
    yy, xx = np.mgrid[0:32, 0:32] / 32.0
    base = np.stack([np.sin(6.0 * xx + c) * np.cos(4.0 * yy - c) for c in range(3)])
    return np.clip(0.7 * base + 0.2 * r.standard_normal((3, 32, 32)), -1, 1).astype(np.float32)[None]


def pack_keys(shapes: dict):
    """A key/shape list as two arrays (names, shapes padded with 0 to four entries)."""
    names = sorted(shapes)
    return np.array(names), np.array([list(shapes[n]) + [0] * (4 - len(shapes[n])) for n in names], np.int64)


def unpack_keys(names, shapes) -> dict:
    return {str(n): tuple(int(v) for v in s if v) for n, s in zip(names, shapes)}


@functools.lru_cache(None)
def golden():
    return dict(np.load(GOLDEN))
