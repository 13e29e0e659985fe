"""Inputs shared by tests/golden/make_golden_datasets.py (which feeds them to the reference) and by
tests/test_datasets_host.py / tests/test_datasets_gpu.py (which feed them to this package).  Everything derives from the
counter-based generator or from index arithmetic, so it regenerates identically anywhere."""
import numpy as np
import torch

from fixtures import TinyCNN
from unlearn_saliency_amd import rng

SPLIT_SEEDS = (1, 2)
RANDOM_COUNT = 37           # `class_to_replace=-1` with this many samples marked
CLASS_NONE = {"cifar100": 7, "svhn": 3}   # a class forgotten with `num_indexes_to_replace=None`
SVHN_BIG_CLASS = 1          # >= 4454 training samples after the split, forgotten with the count 4454
CIFAR100_CLASS_COUNT = (11, 20)  # (class, count): cifar100's test set stays whole whenever a count is given


def index_images(n, side=2):
    """[n, side, side, 3] uint8 whose first three bytes spell the sample's index: a split is read back from pixels."""
    x = np.zeros((n, side, side, 3), np.uint8)
    i = np.arange(n)
    x[:, 0, 0, 0], x[:, 0, 0, 1], x[:, 0, 0, 2] = i & 255, (i >> 8) & 255, (i >> 16) & 255
    return x


def image_index(x):
    x = np.asarray(x).astype(np.int64)
    return x[:, 0, 0, 0] | (x[:, 0, 0, 1] << 8) | (x[:, 0, 0, 2] << 16)


def split_source(name):
    """((xtr, ytr), (xte, yte)) small enough to run the reference's loaders in a moment.  cifar100: 100 classes x 30
    shuffled; svhn: class 1 holds 5,000 samples (4,500 after the split: the 4454 rule can be asked for), the others
    50."""
    if name == "cifar100":
        ytr = np.repeat(np.arange(100), 30)
        yte = np.repeat(np.arange(100), 5)
    elif name == "svhn":
        ytr = np.concatenate([np.full(5000 if c == SVHN_BIG_CLASS else 50, c) for c in range(10)])
        yte = np.concatenate([np.full(300 if c == SVHN_BIG_CLASS else 30, c) for c in range(10)])
    else:
        raise ValueError(name)
    ytr = ytr[np.argsort(rng.uniform(len(ytr), 4100), kind="stable")].astype(np.int64)
    yte = yte[np.argsort(rng.uniform(len(yte), 4200), kind="stable")].astype(np.int64)
    return (index_images(len(ytr)), ytr), (index_images(len(yte)), yte)


def split_cases(name):
    """(tag, loader keyword arguments) of every recorded marked-loader call, per seed."""
    cases = [("random", dict(class_to_replace=-1, num_indexes_to_replace=RANDOM_COUNT)),
             ("class_none", dict(class_to_replace=CLASS_NONE[name], num_indexes_to_replace=None))]
    if name == "svhn":
        cases.append(("class_4454", dict(class_to_replace=SVHN_BIG_CLASS, num_indexes_to_replace=4454)))
    else:
        c, k = CIFAR100_CLASS_COUNT
        cases.append(("class_count", dict(class_to_replace=c, num_indexes_to_replace=k)))
    return cases


# ------------------------------------------------------------------ merged RL (rl_merged.npz)
RL_CLASSES = 16
RL_BATCH = 32
RL_EPOCHS = 2
RL_NUMPY_SEED = 7
RL_TORCH_SEED = 5


def rl_merged_datasets():
    """41 forget + 90 retain uint8 8x8 images, 16 classes, no augmentation: 131 samples = 5 steps of batch 32, the last
    one ragged (3 samples)."""
    from unlearn_saliency_amd.Classification.dataset import ArrayDataset
    fx = rng.u8(41 * 8 * 8 * 3, 5100).reshape(41, 8, 8, 3)
    fy = (rng.u8(41, 5101) % RL_CLASSES).astype(np.int64)
    rx = rng.u8(90 * 8 * 8 * 3, 5102).reshape(90, 8, 8, 3)
    ry = (rng.u8(90, 5103) % RL_CLASSES).astype(np.int64)
    return ArrayDataset(fx, fy, transform="test"), ArrayDataset(rx, ry, transform="test")


def rl_model(seed=41):
    """TinyCNN with a 16-way head, parameters from the counter-based generator."""
    m = TinyCNN(num_classes=RL_CLASSES)
    sd = m.state_dict()
    for j, (k, v) in enumerate(sd.items()):
        if not v.dtype.is_floating_point:
            continue
        s = seed + 1000 * j
        if "running_var" in k:
            v.copy_(torch.from_numpy(rng.uniform(v.numel(), s, 0.5, 1.5)).view_as(v))
        elif k.startswith("bn") and k.endswith("weight"):
            v.copy_(torch.from_numpy(rng.uniform(v.numel(), s, 0.8, 1.2)).view_as(v))
        else:
            v.copy_(torch.from_numpy(rng.normal(v.numel(), s, 0.0, 0.2)).view_as(v))
    m.load_state_dict(sd)
    return m


def rl_mask_flat(n):
    return (rng.u8(n, 5200) & 1).astype(np.int64)


def rl_args(**kw):
    from types import SimpleNamespace
    base = dict(unlearn_lr=0.013, momentum=0.9, weight_decay=5e-4, decreasing_lr="91,136", rewind_epoch=0,
                imagenet_arch=False, unlearn="RL", unlearn_epochs=RL_EPOCHS, dataset="cifar100",
                num_classes=RL_CLASSES, warmup=0, print_freq=50, batch_size=RL_BATCH)
    base.update(kw)
    return SimpleNamespace(**base)


# ------------------------------------------------------------------ crop / flip restatement
def crop_flip(img, dy, dx, flip, pad=4):
    """RandomCrop(H, padding=pad) at offset (dy, dx) of the zero-padded image, then the horizontal flip: [H, W, 3] uint8
    in, [3, H, W] float32 (/255) out."""
    h, w = img.shape[:2]
    padded = np.zeros((h + 2 * pad, w + 2 * pad, 3), np.uint8)
    padded[pad:pad + h, pad:pad + w] = img
    out = padded[dy:dy + h, dx:dx + w]
    if flip:
        out = out[:, ::-1]
    return np.ascontiguousarray(out.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)
