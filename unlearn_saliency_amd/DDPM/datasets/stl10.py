"""STL-10 for the DDPM runs (reference DDPM/datasets/__init__.py:55-69, 145-159): the binary files torchvision's STL10
reads, train followed by test (5,000 + 8,000 images: "use both train and test sets due to its small size"), and the
reference's `transforms.Resize(config.data.image_size)` done ONCE, on the device, on the uint8 originals, by K26
(ops_resample.resize_u8: Pillow's antialiased bilinear resample, bit for bit).

The reference resizes and then flips, per fetch.  Here the set is resized once and flipped where the CIFAR-10 path flips
(per pass in `get_dataset`, frozen once in `get_forget_dataset`).  That is the same image: the resample's coefficient
tables are mirror-symmetric (output column OW-1-i reads the mirrored taps of column i with the same integer weights,
tests/test_resample_ref_cpu.py), so resize(mirror(x)) == mirror(resize(x)) byte for byte, and the originals never have
to stay resident.

No torchvision, no download: the files are read with numpy, and when they are absent (or under --synthetic) the
counter-based stand-in of the same size and shape goes through the same K26 call."""
from __future__ import annotations

import os

import numpy as np
import torch

from ...Classification.dataset import SYNTHETIC_SEED, _u8_chunked

SIDE = 96
N_TRAIN, N_TEST = 5_000, 8_000
FOLDER = "stl10_binary"


def have_stl10(data_dir: str) -> bool:
    return all(os.path.exists(os.path.join(data_dir, FOLDER, f"{s}_{k}.bin")) for s in ("train", "test") for k in "Xy")


def _read_split(base: str, split: str):
    """One split -> (x uint8 [N, 96, 96, 3], y int64 [N] in 0..9).  The file stores each image as three planes, each
    plane COLUMN-major: [N, 3, col, row].  Swapping the last two axes gives [N, 3, row, col]; then channels go last."""
    y = np.fromfile(os.path.join(base, f"{split}_y.bin"), dtype=np.uint8)
    x = np.fromfile(os.path.join(base, f"{split}_X.bin"), dtype=np.uint8)
    if x.size != y.size * 3 * SIDE * SIDE:
        raise ValueError(f"{base}/{split}_X.bin: {x.size} bytes for {y.size} labels (expected {3 * SIDE * SIDE} per image)")
    x = x.reshape(-1, 3, SIDE, SIDE).transpose(0, 3, 2, 1)  # [N, 3, col, row] -> [N, row, col, 3]
    return np.ascontiguousarray(x), y.astype(np.int64) - 1   # labels are stored 1..10


def load_stl10_files(data_dir: str):
    """(x uint8 NHWC, y int64): the train split followed by the test split, as the reference's ConcatDataset."""
    base = os.path.join(data_dir, FOLDER)
    (xtr, ytr), (xte, yte) = _read_split(base, "train"), _read_split(base, "test")
    return np.concatenate([xtr, xte]), np.concatenate([ytr, yte])


def synthetic_stl10(n_train: int = N_TRAIN, n_test: int = N_TEST, seed: int = SYNTHETIC_SEED):
    """STL-10-shaped stand-in, made the way `synthetic_cifar10` makes CIFAR-10's: uint8 pixels from the counter-based
    generator, balanced labels i % 10, train part followed by test part.  -> (x uint8 NHWC, y int64)."""
    px = SIDE * SIDE * 3
    x = np.empty((n_train + n_test, SIDE, SIDE, 3), np.uint8)
    x[:n_train] = _u8_chunked(n_train * px, seed).reshape(n_train, SIDE, SIDE, 3)
    x[n_train:] = _u8_chunked(n_test * px, seed + 1_000_003).reshape(n_test, SIDE, SIDE, 3)
    y = np.concatenate([np.arange(n_train) % 10, np.arange(n_test) % 10]).astype(np.int64)
    return x, y


def resize_target(h: int, w: int, size: int):
    """(OH, OW) of `transforms.Resize(size)` with an int: the smaller edge becomes `size`, the aspect ratio stays."""
    if h <= w:
        return size, int(size * w / h)
    return int(size * h / w), size


def device_arrays(config, synthetic, device):
    """(x uint8 [N, S, S, 3] on `device`, y int64 [N] on `device`), S = config.data.image_size: the whole set uploaded
    as uint8 and resized by one K26 launch."""
    from ... import ops_resample
    use_syn = synthetic if synthetic is not None else not have_stl10(config.data.path)
    x, y = synthetic_stl10() if use_syn else load_stl10_files(config.data.path)
    xd = torch.from_numpy(x).to(device)
    size = resize_target(x.shape[1], x.shape[2], int(config.data.image_size))
    if size != tuple(x.shape[1:3]):  # (Pillow returns a copy when the size does not change)
        xd = ops_resample.resize_u8(xd, size)
    return xd, torch.from_numpy(y).to(device)
