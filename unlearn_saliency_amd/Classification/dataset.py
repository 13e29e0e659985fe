"""Input pipelines for the SalUn classification path: CIFAR-10, CIFAR-100, SVHN and Tiny-ImageNet
(no torchvision needed).  `DATASETS` is the one table of what differs between them.

Mirrors the *observable behaviour* of the reference's loader
(Classification/dataset.py:529-705): 45,000 / 5,000 stratified train/val split drawn
with ``np.random.RandomState(seed)``, forget-set marking by negated labels
(``-label-1``) with ``RandomState(seed-1)``, class-wise test-set filtering, and loaders
whose ``.dataset`` exposes ``.data`` (N,32,32,3 uint8), ``.targets`` (ndarray) and
``.transform`` so the entry scripts can slice forget/retain sets exactly as the
reference scripts do (main_random.py:50-110).

Two batch paths:

* host path (default) — per-sample RandomCrop(32, padding=4) + RandomHorizontalFlip +
  ToTensor consuming the global torch RNG in torchvision's order (two ``randint`` then
  one ``rand`` per sample), shuffling like ``torch.utils.data.RandomSampler``; this is
  the reference's K0 pipeline kept for RNG-stream compatibility;
* device path (``device_resident=True``) — the whole uint8 set lives in HBM
  (45,000 x 3,072 B = 138 MB) and ``salun_image_batch`` assembles the fp32 batch
  (gather + crop + flip + /255) in one kernel, removing the single-threaded host loop
  that otherwise bounds steps/s.

Both paths take the image size from the data: 32 x 32 for the CIFAR sets and SVHN, 64 x 64 for
Tiny-ImageNet (crop padding 4 either way).  The loaders of the other three datasets
(`cifar100_dataloaders`, `svhn_dataloaders`, `tiny_imagenet_dataloaders`) reproduce the reference's
observable behaviour, oddities included (dataset.py:73-178, 181-294, 372-526); each says which.
"""
from __future__ import annotations

import copy
import os
import pickle
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from .. import rng as salun_rng

TRAIN_TRANSFORM = "train"  # RandomCrop(H, 4) + RandomHorizontalFlip + ToTensor
TEST_TRANSFORM = "test"    # ToTensor only
CROP_PAD = 4

SYNTHETIC_SEED = 2


class DatasetSpec(NamedTuple):
    """What `--dataset NAME` fixes: the head's width, the image side, the model's normalisation layer (reference
    utils.py:112-225) and the real set's sizes, which the synthetic stand-in copies."""
    classes: int
    image: int
    mean: Tuple[float, float, float]
    std: Tuple[float, float, float]
    n_train: int
    n_test: int


DATASETS = {
    "cifar10": DatasetSpec(10, 32, (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616), 50_000, 10_000),
    "svhn": DatasetSpec(10, 32, (0.4377, 0.4438, 0.4728), (0.1201, 0.1231, 0.1052), 73_257, 26_032),
    "cifar100": DatasetSpec(100, 32, (0.5071, 0.4866, 0.4409), (0.2673, 0.2564, 0.2762), 50_000, 10_000),
    "TinyImagenet": DatasetSpec(200, 64, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), 100_000, 10_000),
}


class ArrayDataset:
    """In-memory image set with torchvision-CIFAR10-like attributes."""

    def __init__(self, data: np.ndarray, targets: np.ndarray, transform: str = TEST_TRANSFORM, train: bool = True):
        assert data.dtype == np.uint8 and data.ndim == 4 and data.shape[-1] == 3
        self.data = data
        self.targets = np.asarray(targets)
        self.transform = transform
        self.train = train

    def __len__(self):
        return len(self.data)

    def __getitem__(self, i):
        img = self.data[i]
        if self.transform == TRAIN_TRANSFORM:
            # torchvision order: RandomCrop.get_params (randint i, randint j), then flip (rand < 0.5)
            h, w, p = img.shape[0], img.shape[1], CROP_PAD
            dy = int(torch.randint(0, 2 * p + 1, size=(1,)).item())
            dx = int(torch.randint(0, 2 * p + 1, size=(1,)).item())
            flip = bool(torch.rand(1) < 0.5)
            padded = np.zeros((h + 2 * p, w + 2 * p, 3), np.uint8)
            padded[p:p + h, p:p + w] = img
            img = padded[dy:dy + h, dx:dx + w]
            if flip:
                img = img[:, ::-1]
        x = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).to(torch.float32).div(255)
        return x, int(self.targets[i])


class BatchLoader:
    """The subset of torch.utils.data.DataLoader the unlearning loops rely on:
    iteration over (image[B,3,H,W] fp32, target[B] int64), ``len()``, ``.dataset``,
    ``.batch_size``; H and W are the data's.  An empty dataset iterates zero batches.  `shuffle=True` draws one
    permutation per epoch the way RandomSampler does (a 64-bit seed from the global generator, then randperm)."""

    def __init__(self, dataset: ArrayDataset, batch_size: int, shuffle: bool, device_resident: bool = False,
                 device: Optional[torch.device] = None, rank: int = 0, world_size: int = 1):
        self.dataset = dataset
        self.batch_size = int(batch_size)
        self.shuffle = shuffle
        self.device_resident = device_resident
        self.device = device
        self.rank, self.world_size = rank, world_size
        # device copies of the dataset, images and labels cached apart: [key, host array, device tensor] each.  Swapping
        # `dataset.targets` (RL's per-epoch relabelling of a merged set) uploads the label vector alone, not the images.
        # The host array is held so that its id cannot be handed to another array while the entry lives.
        self._dev_data = None
        self._dev_targets = None
        # (lo, hi, b) of the batch just yielded: this rank holds samples [lo, hi) of a global batch of b — what the
        # callers need to draw per-batch randomness for the GLOBAL batch (then slice) and to count-weight the loss
        self.last_shard = None
        self.image_uploads = 0  # times the device path copied the images to the device

    def _slice(self, b: int):
        if self.world_size <= 1:
            return 0, b
        return self.rank * b // self.world_size, (self.rank + 1) * b // self.world_size

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def _order(self) -> torch.Tensor:
        n = len(self.dataset)
        # DataLoader draws a base seed when the iterator is created, RandomSampler another when started
        torch.empty((), dtype=torch.int64).random_()
        if not self.shuffle:
            return torch.arange(n)
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
        g = torch.Generator()
        g.manual_seed(seed)
        return torch.randperm(n, generator=g)

    def _resident(self):
        ds = self.dataset
        dev = self.device or torch.device("cuda", torch.cuda.current_device())
        key = (id(ds.data), ds.data.shape)
        if self._dev_data is None or self._dev_data[0] != key:
            self._dev_data = (key, ds.data, torch.from_numpy(np.ascontiguousarray(ds.data)).to(dev))
            self.image_uploads += 1
        key = (id(ds.targets), len(ds.targets))
        if self._dev_targets is None or self._dev_targets[0] != key:
            self._dev_targets = (key, ds.targets, torch.from_numpy(np.asarray(ds.targets).astype(np.int64)).to(dev))
        return self._dev_data[2], self._dev_targets[2]

    def __iter__(self):
        order = self._order()
        n, bs = len(self.dataset), self.batch_size
        if self.device_resident:
            from .. import ops
            data, targets = self._resident()
            order = order.to(data.device)
            train = self.dataset.transform == TRAIN_TRANSFORM
            for s in range(0, n, bs):
                idx = order[s:s + bs]
                b = idx.numel()
                lo, hi = self._slice(b)  # contiguous, balanced shard of the global batch
                crop = flip = None
                if train:
                    # augmentation is drawn for the GLOBAL batch on every rank (identically seeded generators), then
                    # sliced: ranks stay in lock-step whatever their shard sizes, and the global batch sees b
                    # independent draws, not the same b/ws draws on every rank
                    crop = torch.randint(0, 2 * CROP_PAD + 1, (b, 2), device=data.device,
                                         dtype=torch.int32)[lo:hi].contiguous()
                    flip = (torch.rand(b, device=data.device) < 0.5).to(torch.uint8)[lo:hi].contiguous()
                idx = idx[lo:hi].contiguous()
                self.last_shard = (lo, hi, b)
                yield ops.image_batch(data, idx, crop, flip, pad=CROP_PAD), targets[idx]
        else:
            order = order.tolist()
            for s in range(0, n, bs):
                idx = order[s:s + bs]
                lo, hi = self._slice(len(idx))
                self.last_shard = (lo, hi, len(idx))
                idx = idx[lo:hi]
                items = [self.dataset[i] for i in idx]
                x = (torch.stack([it[0] for it in items]) if items
                     else torch.empty((0, 3) + tuple(self.dataset.data.shape[1:3])))
                y = torch.tensor([it[1] for it in items], dtype=torch.int64)
                yield x, y


# ------------------------------------------------------------------------- sources
def _load_cifar10_files(data_dir: str):
    """Standard `cifar-10-batches-py` pickles (what torchvision's CIFAR10 reads; no download here)."""
    base = os.path.join(data_dir, "cifar-10-batches-py")

    def read(names):
        xs, ys = [], []
        for nm in names:
            with open(os.path.join(base, nm), "rb") as f:
                d = pickle.load(f, encoding="latin1")
            xs.append(np.asarray(d["data"], dtype=np.uint8))
            ys.extend(d["labels"] if "labels" in d else d["fine_labels"])
        x = np.vstack(xs).reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)
        return np.ascontiguousarray(x), np.asarray(ys, dtype=np.int64)

    return read([f"data_batch_{i}" for i in range(1, 6)]), read(["test_batch"])


def synthetic_cifar10(n_train: int = 50_000, n_test: int = 10_000, seed: int = SYNTHETIC_SEED):
    """CIFAR-shaped stand-in: uint8 pixels ~ U{0..255} from the counter-based
    generator, balanced labels i % 10.  After the 10 % validation split: 45,000 train, 4,500/class."""
    xtr = salun_rng.u8(n_train * 3072, seed).reshape(n_train, 32, 32, 3)
    xte = salun_rng.u8(n_test * 3072, seed + 1_000_003).reshape(n_test, 32, 32, 3)
    ytr = (np.arange(n_train) % 10).astype(np.int64)
    yte = (np.arange(n_test) % 10).astype(np.int64)
    return (xtr, ytr), (xte, yte)


def have_cifar10(data_dir: str) -> bool:
    return os.path.exists(os.path.join(data_dir, "cifar-10-batches-py", "data_batch_1"))


def _u8_chunked(n: int, seed: int, chunk_words: int = 1 << 22) -> np.ndarray:
    """`rng.u8(n, seed)`, built in pieces so that the temporaries stay small at Tiny-ImageNet size (1.2 GB):
    the generator is index-addressed, so words [w0, w1) are the words of seed + w0."""
    if n <= 8 * chunk_words:
        return salun_rng.u8(n, seed)
    out = np.empty(n, np.uint8)
    for w0 in range(0, (n + 7) // 8, chunk_words):
        lo = 8 * w0
        hi = min(n, lo + 8 * chunk_words)
        out[lo:hi] = salun_rng.u8(hi - lo, seed + w0)
    return out


def synthetic_images(dataset: str, n_train: Optional[int] = None, n_test: Optional[int] = None,
                     seed: int = SYNTHETIC_SEED):
    """Stand-in for any entry of `DATASETS`, made the way `synthetic_cifar10` makes CIFAR-10's: counter-based uint8
    pixels, balanced labels i % classes, and the real set's sizes unless `n_train` / `n_test` shrink them."""
    spec = DATASETS[dataset]
    n_train = spec.n_train if n_train is None else int(n_train)
    n_test = spec.n_test if n_test is None else int(n_test)
    px = spec.image * spec.image * 3
    xtr = _u8_chunked(n_train * px, seed).reshape(n_train, spec.image, spec.image, 3)
    xte = _u8_chunked(n_test * px, seed + 1_000_003).reshape(n_test, spec.image, spec.image, 3)
    ytr = (np.arange(n_train) % spec.classes).astype(np.int64)
    yte = (np.arange(n_test) % spec.classes).astype(np.int64)
    return (xtr, ytr), (xte, yte)


def have_cifar100(data_dir: str) -> bool:
    return os.path.exists(os.path.join(data_dir, "cifar-100-python", "train"))


def _load_cifar100_files(data_dir: str):
    """`cifar-100-python/{train,test}` pickles, labels from `fine_labels` (what torchvision's CIFAR100 reads)."""
    def read(name):
        with open(os.path.join(data_dir, "cifar-100-python", name), "rb") as f:
            d = pickle.load(f, encoding="latin1")
        x = np.asarray(d["data"], dtype=np.uint8).reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)
        return np.ascontiguousarray(x), np.asarray(d["fine_labels"], dtype=np.int64)

    return read("train"), read("test")


def have_svhn(data_dir: str) -> bool:
    return os.path.exists(os.path.join(data_dir, "train_32x32.mat"))


def _load_svhn_files(data_dir: str):
    """`train_32x32.mat` / `test_32x32.mat`: X is [32, 32, 3, N], y is [N, 1] with the digit 0 stored as 10
    (torchvision's SVHN maps it back to 0, so the reference never sees a 10)."""
    try:
        from scipy.io import loadmat
    except ImportError as e:
        raise ImportError("reading SVHN's .mat files needs scipy; without it run with --synthetic") from e

    def read(name):
        m = loadmat(os.path.join(data_dir, name))
        x = np.ascontiguousarray(np.asarray(m["X"], dtype=np.uint8).transpose(3, 0, 1, 2))
        y = np.asarray(m["y"]).astype(np.int64).reshape(-1)
        y[y == 10] = 0
        return x, y

    return read("train_32x32.mat"), read("test_32x32.mat")


_IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")


def have_tiny_imagenet(data_dir: str) -> bool:
    return os.path.isdir(os.path.join(data_dir, "train")) and (
        os.path.isdir(os.path.join(data_dir, "val", "images")) or os.path.isdir(os.path.join(data_dir, "test")))


def _image_files(root: str):
    """Every image file under `root`, in the order an ImageFolder lists a class directory (sorted walk)."""
    out = []
    for d, _, names in sorted(os.walk(root, followlinks=True)):
        out.extend(os.path.join(d, nm) for nm in sorted(names) if nm.lower().endswith(_IMAGE_EXTENSIONS))
    return out


def tiny_imagenet_file_lists(data_dir: str):
    """-> (classes, [(path, label)] train, [(path, label)] test) of a Tiny-ImageNet folder; reads no image and
    writes nothing.  Classes are the sorted wnids of `train/`.  The test set is either the layout the reference leaves
    behind (`test/<wnid>/images/*`) or, for a pristine download (`val/images` + `val_annotations.txt`), what its split
    would be: per class and in sorted file-name order the first 25 files are validation (unused), the rest test.  The
    reference moves the user's files to get there (dataset.py:399-430); this computes the same split in memory."""
    train_root = os.path.join(data_dir, "train")
    classes = sorted(d for d in os.listdir(train_root) if os.path.isdir(os.path.join(train_root, d)))
    label = {c: i for i, c in enumerate(classes)}
    train = [(p, label[c]) for c in classes for p in _image_files(os.path.join(train_root, c))]
    val_images = os.path.join(data_dir, "val", "images")
    test = []
    if os.path.isdir(val_images):
        per_class = {c: [] for c in classes}
        with open(os.path.join(data_dir, "val", "val_annotations.txt")) as f:
            for line in f:
                parts = line.split("\t")
                if len(parts) >= 2 and parts[1] in per_class:
                    per_class[parts[1]].append(parts[0])
        for c in classes:
            names = sorted(nm for nm in per_class[c] if os.path.exists(os.path.join(val_images, nm)))
            test.extend((os.path.join(val_images, nm), label[c]) for nm in names[25:])
    else:
        test_root = os.path.join(data_dir, "test")
        test_classes = sorted(d for d in os.listdir(test_root) if os.path.isdir(os.path.join(test_root, d)))
        for i, c in enumerate(test_classes):  # an ImageFolder numbers the classes of the folder it is given
            test.extend((p, i) for p in _image_files(os.path.join(test_root, c)))
    return classes, train, test


def _load_tiny_imagenet_files(data_dir: str):
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("decoding the Tiny-ImageNet folder needs PIL (pillow); without it run with "
                          "--synthetic") from e
    _, train, test = tiny_imagenet_file_lists(data_dir)

    def read(files):
        x = np.empty((len(files), 64, 64, 3), np.uint8)
        for i, (path, _) in enumerate(files):
            with Image.open(path) as im:
                x[i] = np.asarray(im.convert("RGB"), dtype=np.uint8)
        return x, np.asarray([lab for _, lab in files], dtype=np.int64)

    return read(train), read(test)


# ---------------------------------------------------------------- forget marking
def replace_indexes(dataset, indexes, seed=0, only_mark: bool = False):
    """only_mark: flag forget samples by label -> -label-1 (the -1 keeps class 0 markable);
    otherwise overwrite them with random other samples (reference dataset.py:648-671)."""
    indexes = np.asarray(indexes)
    if only_mark:
        dataset.targets[indexes] = -dataset.targets[indexes] - 1
        return
    rng = np.random.RandomState(seed)
    pool = list(set(range(len(dataset))) - set(indexes.tolist()))
    new_indexes = rng.choice(pool, size=len(indexes))
    dataset.data[indexes] = dataset.data[new_indexes]
    dataset.targets[indexes] = dataset.targets[new_indexes]


def replace_class(dataset, class_to_replace: int, num_indexes_to_replace: Optional[int] = None, seed: int = 0,
                  only_mark: bool = False):
    """class -1 = "any class" (random-data forgetting); reference dataset.py:674-705."""
    targets = np.asarray(dataset.targets)
    if class_to_replace == -1:
        indexes = np.flatnonzero(np.ones_like(targets))
    else:
        indexes = np.flatnonzero(targets == class_to_replace)
    if num_indexes_to_replace is not None:
        if num_indexes_to_replace > len(indexes):
            raise AssertionError(f"Want to replace {num_indexes_to_replace} indexes but only {len(indexes)} "
                                 "samples in dataset")
        rng = np.random.RandomState(seed)
        indexes = rng.choice(indexes, size=num_indexes_to_replace, replace=False)
        print(f"Replacing indexes {indexes}")
    replace_indexes(dataset, indexes, seed, only_mark)


def cifar10_dataloaders(batch_size=128, data_dir="datasets/cifar10", num_workers=2, random_to_replace=None,
                        class_to_replace: Optional[int] = None, num_indexes_to_replace=None,
                        indexes_to_replace=None, seed: int = 1, only_mark: bool = False, shuffle=True,
                        no_aug=False, synthetic: bool = False, device_resident: bool = False):
    """(train_loader, val_loader, test_loader), same splits as reference dataset.py:529-645."""
    if synthetic or not have_cifar10(data_dir):
        if not synthetic:
            print(f"CIFAR-10 files not found under {data_dir!r}: using the synthetic CIFAR-shaped set")
        (xtr, ytr), (xte, yte) = synthetic_cifar10()
    else:
        (xtr, ytr), (xte, yte) = _load_cifar10_files(data_dir)
    print("Dataset information: CIFAR-10\t 45000 images for training \t 5000 images for validation\t")
    print("10000 images for testing\t no normalize applied in data_transform")

    rng = np.random.RandomState(seed)
    valid_idx = []
    for c in range(int(ytr.max()) + 1):
        class_idx = np.where(ytr == c)[0]
        valid_idx.append(rng.choice(class_idx, int(0.1 * len(class_idx)), replace=False))
    valid_idx = np.hstack(valid_idx)
    train_idx = np.asarray(sorted(set(range(len(xtr))) - set(valid_idx.tolist())), dtype=np.int64)

    train_tf = TEST_TRANSFORM if no_aug else TRAIN_TRANSFORM
    train_set = ArrayDataset(xtr[train_idx], ytr[train_idx].copy(), train_tf, train=True)
    valid_set = ArrayDataset(xtr[valid_idx], ytr[valid_idx].copy(), train_tf, train=True)
    test_set = ArrayDataset(xte, yte.copy(), TEST_TRANSFORM, train=False)

    if class_to_replace is not None and indexes_to_replace is not None:
        raise ValueError("Only one of `class_to_replace` and `indexes_to_replace` can be specified")
    if class_to_replace is not None:
        replace_class(train_set, class_to_replace, num_indexes_to_replace=num_indexes_to_replace, seed=seed - 1,
                      only_mark=only_mark)
        if num_indexes_to_replace is None or num_indexes_to_replace == 4500:
            keep = test_set.targets != class_to_replace
            test_set.data, test_set.targets = test_set.data[keep], test_set.targets[keep]
    if indexes_to_replace is not None:
        replace_indexes(train_set, indexes_to_replace, seed=seed - 1, only_mark=only_mark)

    mk = lambda ds, sh: BatchLoader(ds, batch_size, sh, device_resident=device_resident)
    return mk(train_set, True), mk(valid_set, False), mk(test_set, False)


def _split_mark_load(source, *, val_fraction, train_tf, valid_tf, test_filter_counts, val_is_test, batch_size,
                     class_to_replace, num_indexes_to_replace, indexes_to_replace, seed, only_mark, device_resident):
    """The body the reference's three loaders share (dataset.py:105-178, 222-294, 449-526): a per-class validation
    split of `val_fraction` from RandomState(seed) (drawn for every class even when it takes nothing, so the stream
    is the reference's), forget marking from RandomState(seed - 1), and the test set without `class_to_replace` when
    `num_indexes_to_replace` is None or one of `test_filter_counts`."""
    (xtr, ytr), (xte, yte) = source
    rng = np.random.RandomState(seed)
    valid_idx = []
    for c in range(int(ytr.max()) + 1):
        class_idx = np.where(ytr == c)[0]
        valid_idx.append(rng.choice(class_idx, int(val_fraction * len(class_idx)), replace=False))
    valid_idx = np.hstack(valid_idx).astype(np.int64)
    train_idx = np.asarray(sorted(set(range(len(xtr))) - set(valid_idx.tolist())), dtype=np.int64)

    # an empty validation split leaves the training images as they are: share them (1.2 GB for Tiny-ImageNet) unless
    # the forget samples are to be overwritten in place
    writes_images = not only_mark and (class_to_replace is not None or indexes_to_replace is not None)
    train_data = xtr if len(valid_idx) == 0 and not writes_images else xtr[train_idx]
    train_set = ArrayDataset(train_data, ytr[train_idx].copy(), train_tf, train=True)
    valid_set = ArrayDataset(xtr[valid_idx], ytr[valid_idx].copy(), valid_tf, train=True)
    test_set = ArrayDataset(xte, yte.copy(), TEST_TRANSFORM, train=False)

    if class_to_replace is not None and indexes_to_replace is not None:
        raise ValueError("Only one of `class_to_replace` and `indexes_to_replace` can be specified")
    if class_to_replace is not None:
        replace_class(train_set, class_to_replace, num_indexes_to_replace=num_indexes_to_replace, seed=seed - 1,
                      only_mark=only_mark)
        if num_indexes_to_replace is None or num_indexes_to_replace in test_filter_counts:
            keep = test_set.targets != class_to_replace
            test_set.data, test_set.targets = test_set.data[keep], test_set.targets[keep]
    if indexes_to_replace is not None:
        replace_indexes(train_set, indexes_to_replace, seed=seed - 1, only_mark=only_mark)

    mk = lambda ds, sh: BatchLoader(ds, batch_size, sh, device_resident=device_resident)
    return mk(train_set, True), mk(test_set if val_is_test else valid_set, False), mk(test_set, False)


def _source(dataset, label, have, load, data_dir, synthetic, n_train, n_test):
    if synthetic or not have(data_dir):
        if not synthetic:
            print(f"{label} files not found under {data_dir!r}: using the synthetic {label}-shaped set")
        return synthetic_images(dataset, n_train, n_test)
    return load(data_dir)


def cifar100_dataloaders(batch_size=128, data_dir="datasets/cifar100", num_workers=2,
                         class_to_replace: Optional[int] = None, num_indexes_to_replace=None, indexes_to_replace=None,
                         seed: int = 1, only_mark: bool = False, shuffle=True, no_aug=False, synthetic: bool = False,
                         device_resident: bool = False, n_train: Optional[int] = None, n_test: Optional[int] = None,
                         source=None):
    """(train_loader, val_loader, test_loader) as reference dataset.py:181-294: 10 % per-class validation split,
    crop + flip unless `no_aug`, and the test set loses `class_to_replace` only when `num_indexes_to_replace` is None
    (CIFAR-10's loader also does for a whole class's count; this one does not).  `source` = ((xtr, ytr), (xte, yte))
    hands over arrays already read; `n_train` / `n_test` size the synthetic set."""
    source = source or _source("cifar100", "CIFAR-100", have_cifar100, _load_cifar100_files, data_dir, synthetic,
                               n_train, n_test)
    print("Dataset information: CIFAR-100\t 45000 images for training \t 500 images for validation\t")
    print("10000 images for testing\t no normalize applied in data_transform")
    print("Data augmentation = randomcrop(32,4) + randomhorizontalflip")
    train_tf = TEST_TRANSFORM if no_aug else TRAIN_TRANSFORM
    return _split_mark_load(source, val_fraction=0.1, train_tf=train_tf, valid_tf=train_tf, test_filter_counts=(),
                            val_is_test=False, batch_size=batch_size, class_to_replace=class_to_replace,
                            num_indexes_to_replace=num_indexes_to_replace, indexes_to_replace=indexes_to_replace,
                            seed=seed, only_mark=only_mark, device_resident=device_resident)


def svhn_dataloaders(batch_size=128, data_dir="datasets/svhn", num_workers=2, class_to_replace: Optional[int] = None,
                     num_indexes_to_replace=None, indexes_to_replace=None, seed: int = 1, only_mark: bool = False,
                     shuffle=True, no_aug=False, synthetic: bool = False, device_resident: bool = False,
                     n_train: Optional[int] = None, n_test: Optional[int] = None, source=None):
    """As reference dataset.py:73-178: the same split, NO augmentation ever (`no_aug` is ignored), and the test set
    filtered when `num_indexes_to_replace` is None or 4454.  torchvision's SVHN calls its label vector `.labels`; the
    sets here call it `.targets`, which is what the reference's scripts try first."""
    source = source or _source("svhn", "SVHN", have_svhn, _load_svhn_files, data_dir, synthetic, n_train, n_test)
    print("Dataset information: SVHN\t 45000 images for training \t 5000 images for validation\t")
    return _split_mark_load(source, val_fraction=0.1, train_tf=TEST_TRANSFORM, valid_tf=TEST_TRANSFORM,
                            test_filter_counts=(4454,), val_is_test=False, batch_size=batch_size,
                            class_to_replace=class_to_replace, num_indexes_to_replace=num_indexes_to_replace,
                            indexes_to_replace=indexes_to_replace, seed=seed, only_mark=only_mark,
                            device_resident=device_resident)


def tiny_imagenet_dataloaders(batch_size=128, data_dir="./tiny-imagenet-200", num_workers=2,
                              class_to_replace: Optional[int] = None, num_indexes_to_replace=None,
                              indexes_to_replace=None, seed: int = 1, only_mark: bool = False, shuffle=True,
                              no_aug=False, synthetic: bool = False, device_resident: bool = False,
                              n_train: Optional[int] = None, n_test: Optional[int] = None, source=None):
    """As reference dataset.py:372-526 (`TinyImageNet(args).data_loaders`): a 0 % validation split (still drawn per
    class), so the validation set is empty and `val_loader` IS the test set; crop(64, 4) + flip always (`no_aug` is
    ignored); the test set filtered when `num_indexes_to_replace` is None or 500.  `data_dir` is the folder (the
    reference reads it from `--data_dir`); the user's files are only read, never moved."""
    source = source or _source("TinyImagenet", "Tiny-ImageNet", have_tiny_imagenet, _load_tiny_imagenet_files,
                               data_dir, synthetic, n_train, n_test)
    loaders = _split_mark_load(source, val_fraction=0.0, train_tf=TRAIN_TRANSFORM, valid_tf=TRAIN_TRANSFORM,
                               test_filter_counts=(500,), val_is_test=True, batch_size=batch_size,
                               class_to_replace=class_to_replace, num_indexes_to_replace=num_indexes_to_replace,
                               indexes_to_replace=indexes_to_replace, seed=seed, only_mark=only_mark,
                               device_resident=device_resident)
    print(f"Traing loader: {len(loaders[0].dataset)} images, Test loader: {len(loaders[2].dataset)} images")
    return loaders


def split_marked(marked_dataset: ArrayDataset):
    """forget (targets < 0, restored to -t-1) / retain (targets >= 0) copies of a marked set —
    the slicing the reference scripts do inline (generate_mask.py:148-164, main_random.py:77-93)."""
    forget = copy.deepcopy(marked_dataset)
    sel = forget.targets < 0
    forget.data, forget.targets = forget.data[sel], -forget.targets[sel] - 1
    retain = copy.deepcopy(marked_dataset)
    sel = retain.targets >= 0
    retain.data, retain.targets = retain.data[sel], retain.targets[sel]
    return forget, retain
