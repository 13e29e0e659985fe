"""Plumbing the drop-in must reproduce (reference Classification/utils.py): seeds, meters,
top-k accuracy, checkpoint naming, and `setup_model_dataset` (one branch per `dataset.DATASETS` entry)."""
from __future__ import annotations

import os
import random
import shutil

import numpy as np
import torch

from . import dataset as dataset_mod
from .dataset import (DATASETS, TEST_TRANSFORM, TRAIN_TRANSFORM, cifar10_dataloaders, cifar100_dataloaders,
                      svhn_dataloaders, tiny_imagenet_dataloaders)
from .models import model_dict
from .models.resnet_cifar import NormalizeByChannelMeanStd

__all__ = ["setup_model_dataset", "setup_seed", "AverageMeter", "accuracy", "save_checkpoint", "load_checkpoint",
           "NormalizeByChannelMeanStd", "dataset_convert_to_test", "dataset_convert_to_train", "warmup_lr"]


def setup_seed(seed: int) -> None:
    """All four generators + deterministic conv algorithms (reference utils.py:288-294)."""
    print("setup random seed = {}".format(seed))
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)
    torch.backends.cudnn.deterministic = True


class AverageMeter:
    """Running sample-weighted mean: .val (last), .avg, .sum, .count."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def accuracy(output: torch.Tensor, target: torch.Tensor, topk=(1,)):
    """precision@k in percent, one 1-element tensor per k (reference utils.py:321-334)."""
    kmax = max(topk)
    pred = output.topk(kmax, dim=1, largest=True, sorted=True).indices.t()  # (kmax, B)
    hit = pred.eq(target.view(1, -1).expand_as(pred))
    n = target.size(0)
    return [hit[:k].reshape(-1).float().sum(0).mul_(100.0 / n) for k in topk]


def warmup_lr(epoch, step, optimizer, one_epoch_step, args):
    overall = args.warmup * one_epoch_step
    lr = min(args.lr * (step + epoch * one_epoch_step) / overall, args.lr)
    for group in optimizer.param_groups:
        group["lr"] = lr


def save_checkpoint(state, is_SA_best, save_path, pruning, filename="checkpoint.pth.tar"):
    """{save_path}/{pruning}{filename} — e.g. RLcheckpoint.pth.tar (reference utils.py:44-52)."""
    path = os.path.join(save_path, str(pruning) + filename)
    torch.save(state, path)
    if is_SA_best:
        shutil.copyfile(path, os.path.join(save_path, str(pruning) + "model_SA_best.pth.tar"))


def load_checkpoint(device, save_path, pruning, filename="checkpoint.pth.tar"):
    path = os.path.join(save_path, str(pruning) + filename)
    if not os.path.exists(path):
        print("Checkpoint not found! path:{}".format(path))
        return None
    print("Load checkpoint from:{}".format(path))
    return torch.load(path, map_location=device, weights_only=False)


def _innermost(dataset):
    while hasattr(dataset, "dataset"):
        dataset = dataset.dataset
    return dataset


def dataset_convert_to_train(dataset):
    ds = _innermost(dataset)
    ds.transform = TRAIN_TRANSFORM
    ds.train = False


def dataset_convert_to_test(dataset, args=None):
    """Switch a (possibly wrapped) dataset to the evaluation transform (reference utils.py:97-109)."""
    ds = _innermost(dataset)
    ds.transform = TEST_TRANSFORM
    ds.train = False


def _model_for(args, classes: int):
    if args.imagenet_arch:
        return model_dict[args.arch](num_classes=classes, imagenet=True)
    return model_dict[args.arch](num_classes=classes)


_OUT_OF_SCOPE = {
    "imagenet": "ImageNet needs the lmdb pipeline, dict batches and the 7x7/2 stem (README: --imagenet_arch)",
    "cifar10_no_val": "the *_no_val sets return four values no entry point of this build reads",
    "cifar100_no_val": "the *_no_val sets return four values no entry point of this build reads",
}


def setup_model_dataset(args, synthetic_sizes=None):
    """-> (model, train_full_loader, val_loader, test_loader, marked_loader), one branch per entry of
    `dataset.DATASETS` as reference utils.py:112-225: a full loader, a second set of loaders with the forget samples
    *marked* (labels negated, seed = args.seed so RandomState(seed-1) picks them), the model built for the dataset's
    class count with its normalisation layer installed.  The reference's differences between the branches are kept:
    only cifar10 re-seeds (`train_seed`) around the model construction, `no_aug` reaches the cifar10 and cifar100
    loaders only, and Tiny-ImageNet takes its folder from `--data_dir` and its test loader from the UNMARKED call.

    `synthetic_sizes` = (n_train, n_test) shrinks the synthetic stand-in (tests; there is no flag for it)."""
    name = args.dataset
    if name in _OUT_OF_SCOPE:
        raise NotImplementedError(f"dataset {name!r} is out of scope: {_OUT_OF_SCOPE[name]}")
    if name not in DATASETS:
        raise ValueError("Dataset not supprot yet !")
    spec = DATASETS[name]
    if int(getattr(args, "num_classes", spec.classes)) != spec.classes:
        print(f"warning: --num_classes {args.num_classes} differs from {name}'s {spec.classes} classes; the model is "
              f"built with {spec.classes}, random labels and the Fisher loop use {args.num_classes}")
    synthetic = bool(getattr(args, "synthetic", False))
    resident = bool(getattr(args, "device_loader", False))
    common = dict(batch_size=args.batch_size, data_dir=args.data, num_workers=args.workers, synthetic=synthetic,
                  device_resident=resident)
    marked = dict(class_to_replace=args.class_to_replace, num_indexes_to_replace=args.num_indexes_to_replace,
                  indexes_to_replace=args.indexes_to_replace, seed=args.seed, only_mark=True, shuffle=True)
    normalization = NormalizeByChannelMeanStd(spec.mean, spec.std)

    if name == "cifar10":
        if synthetic_sizes is not None:
            raise ValueError("synthetic_sizes: the cifar10 loader keeps its fixed synthetic set")
        train_full_loader, val_loader, _ = cifar10_dataloaders(**common)
        marked_loader, _, test_loader = cifar10_dataloaders(no_aug=args.no_aug, **marked, **common)
        if args.train_seed is None:
            args.train_seed = args.seed
        setup_seed(args.train_seed)
        model = model_dict[args.arch](num_classes=spec.classes, imagenet=bool(args.imagenet_arch))
        setup_seed(args.train_seed)
        model.normalize = normalization
        return model, train_full_loader, val_loader, test_loader, marked_loader

    # the other three read (or synthesise) their arrays once and hand them to both loader calls
    loaders, have, load, label = {
        "svhn": (svhn_dataloaders, dataset_mod.have_svhn, dataset_mod._load_svhn_files, "SVHN"),
        "cifar100": (cifar100_dataloaders, dataset_mod.have_cifar100, dataset_mod._load_cifar100_files, "CIFAR-100"),
        "TinyImagenet": (tiny_imagenet_dataloaders, dataset_mod.have_tiny_imagenet,
                         dataset_mod._load_tiny_imagenet_files, "Tiny-ImageNet"),
    }[name]
    if name == "TinyImagenet":
        common["data_dir"] = args.data_dir
    n_train, n_test = synthetic_sizes if synthetic_sizes is not None else (None, None)
    common["source"] = dataset_mod._source(name, label, have, load, common["data_dir"], synthetic, n_train, n_test)
    if name == "TinyImagenet":
        train_full_loader, val_loader, test_loader = loaders(**common)
        marked_loader, _, _ = loaders(**marked, **common)
    else:
        train_full_loader, val_loader, _ = loaders(**common)
        if name == "cifar100":
            marked["no_aug"] = args.no_aug
        marked_loader, _, test_loader = loaders(**marked, **common)
    model = _model_for(args, spec.classes)
    model.normalize = normalization
    return model, train_full_loader, val_loader, test_loader, marked_loader
