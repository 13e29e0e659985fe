"""CIFAR-10 and STL-10 loaders for the DDPM runs (`config.data.dataset`; STL-10's reader and its one-time device resize
are in stl10.py): the whole training set (`get_dataset`, reference DDPM/datasets/__init__.py:30-77)
and the class-split forget / remain sets (reference :120-177, 241-255).  The reference materialises both splits once
as Python lists of (ToTensor image, label) with the random flip frozen at materialisation time; here both splits are device-resident fp32 tensors built once
(flip drawn once, like the reference) and batches are index gathers on the GPU.  Falls back to the
counter-based synthetic stand-in of the configured set when the dataset files are absent (no network on the GPU box)."""
from __future__ import annotations

import numpy as np
import torch

from ...Classification.dataset import _load_cifar10_files, have_cifar10, synthetic_cifar10
from ... import dist as sdist
from . import stl10


class TensorLoader:
    """Shuffling batch iterator over device tensors (x: (N,3,S,S) fp32 in [0,1], c: (N,) int64)."""

    def __init__(self, x, c, batch_size, shuffle=True, rank=0, world_size=1, flip=False):
        self.x, self.c, self.batch_size, self.shuffle = x, c, int(batch_size), shuffle
        self.rank, self.world_size = rank, world_size
        self.flip = flip  # RandomHorizontalFlip(0.5) per sample and pass, drawn for the global batch like the order
        self.last_shard = None  # (lo, hi, b): this rank holds samples [lo, hi) of the global batch of b just yielded

    def __len__(self):
        return (len(self.x) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        n = len(self.x)
        g = torch.Generator()
        g.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
        order = (torch.randperm(n, generator=g) if self.shuffle else torch.arange(n)).to(self.x.device)
        for s in range(0, n, self.batch_size):
            idx = order[s:s + self.batch_size]
            b = idx.numel()
            lo, hi = sdist.balanced_slice(b, self.rank, self.world_size) if self.world_size > 1 else (0, b)
            self.last_shard = (lo, hi, b)
            idx = idx[lo:hi]
            x = self.x[idx]
            if self.flip:
                mirror = (torch.rand(b, generator=g) < 0.5)[lo:hi].to(x.device)
                x = torch.where(mirror[:, None, None, None], x.flip(3), x)
            yield x, self.c[idx]


def _train_arrays(config, synthetic):
    """(x uint8 NHWC, y int64) of the CIFAR-10 training set, or of its synthetic stand-in."""
    use_syn = synthetic if synthetic is not None else not have_cifar10(config.data.path)
    (x, y), _ = synthetic_cifar10() if use_syn else _load_cifar10_files(config.data.path)
    return x, y


def _dataset_name(config) -> str:
    name = config.data.dataset
    if name not in ("CIFAR10", "STL10"):
        raise ValueError(f"data.dataset {name!r}: the DDPM runs read CIFAR10 or STL10")
    return name


def _u8_to_float(xd):
    """device uint8 NHWC -> fp32 NCHW in [0, 1] (ToTensor)."""
    return xd.permute(0, 3, 1, 2).float().div_(255).contiguous()


def _to_device(x, y, device):
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(device).permute(0, 3, 1, 2).float().div_(255).contiguous()
    return xt, torch.from_numpy(y).to(device)


def get_dataset(args, config, device=None, synthetic=None):
    """-> loader over the whole training set (`--mode train`): shuffled every pass; with `data.random_flip` each sample
    is mirrored with probability 0.5 every time it is drawn, as the reference's transform does."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    if _dataset_name(config) == "STL10":
        xd, yt = stl10.device_arrays(config, synthetic, device)
        xt = _u8_to_float(xd)
    else:
        xt, yt = _to_device(*_train_arrays(config, synthetic), device)
    return TensorLoader(xt, yt, config.training.batch_size, True, sdist.rank(), sdist.world_size(),
                        flip=bool(getattr(config.data, "random_flip", True)))


def get_forget_dataset(args, config, label_to_drop, device=None, synthetic=None):
    """-> (remain_loader, forget_loader) split by class `label_to_drop`."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    if _dataset_name(config) == "STL10":
        # resized first (once, on the uint8 originals), mirrored after: the same bytes as the reference's
        # Resize -> RandomHorizontalFlip, because the resample commutes with a mirror (stl10.py)
        xd, yt = stl10.device_arrays(config, synthetic, device)
        if getattr(config.data, "random_flip", True):  # frozen once, as in the reference's materialised lists
            flip = torch.from_numpy(np.random.rand(len(xd)) < 0.5).to(device)
            xd = torch.where(flip[:, None, None, None], xd.flip(2), xd)
        xt = _u8_to_float(xd)
    else:
        x, y = _train_arrays(config, synthetic)
        if getattr(config.data, "random_flip", True):  # frozen once, as in the reference's materialised lists
            flip = np.random.rand(len(x)) < 0.5
            x = np.where(flip[:, None, None, None], x[:, :, ::-1, :], x)
        xt, yt = _to_device(x, y, device)
    forget = yt == int(label_to_drop)
    print(int((~forget).sum()), int(forget.sum()))
    rk, ws = sdist.rank(), sdist.world_size()
    bs = config.training.batch_size
    return (TensorLoader(xt[~forget], yt[~forget], bs, True, rk, ws),
            TensorLoader(xt[forget], yt[forget], bs, True, rk, ws))


def data_transform(config, X):
    """[0,1] -> model range (reference datasets/__init__.py:241-255)."""
    if config.data.uniform_dequantization:
        X = X / 256.0 * 255.0 + torch.rand_like(X) / 256.0
    if config.data.gaussian_dequantization:
        X = X + torch.randn_like(X) * 0.01
    if config.data.rescaled:
        X = 2 * X - 1.0
    elif config.data.logit_transform:
        lam = 1e-6
        X = lam + (1 - 2 * lam) * X
        X = torch.log(X) - torch.log1p(-X)
    if hasattr(config, "image_mean"):
        return X - config.image_mean.to(X.device)[None, ...]
    return X
