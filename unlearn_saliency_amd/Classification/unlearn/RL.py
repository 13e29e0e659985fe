"""Random-label (RL) unlearning — SalUn's Phase B when a saliency mask is passed.

The reference has two branches (Classification/unlearn/RL.py), chosen by `--dataset`:

* cifar10 / svhn (RL.py:109-178) — per epoch one pass over the forget loader with *fresh uniform random labels for
  every batch* (`torch.randint(0, num_classes, target.shape)` from the CPU generator, RL.py:125), then one pass over
  the retain loader with the true labels; returns the retain-pass top-1.
* cifar100 / TinyImagenet (RL.py:51-107) — per epoch the WHOLE forget set is relabelled at once with
  `np.random.randint(0, num_classes, n_forget)` (numpy's global generator, seeded by `setup_seed`), concatenated with
  the retain set as [forget, retain], shuffled, and walked in ONE pass of ceil((n_f + n_r) / batch) steps; the meters
  run over every batch, against the labels as assigned.

BatchNorm is in train mode in both; with a mask, every step is the fused masked-SGD launch (impl.py).

The merged branch concatenates the images once per call, not once per epoch: only the label vector changes between
epochs, and the device loader uploads a new label vector without touching the resident images (1.2 GB for
Tiny-ImageNet; `BatchLoader._resident`).
"""
import numpy as np
import torch

from ... import dist as sdist
from .. import utils
from ..dataset import ArrayDataset, BatchLoader
from ._steps import run_pass
from .impl import iterative_unlearn

MERGED_DATASETS = ("cifar100", "TinyImagenet")


class MergedSet:
    """[forget, retain] as one loader whose forget labels are redrawn per epoch.  The images are concatenated here,
    once; `relabel` replaces the label vector alone."""

    def __init__(self, forget_loader, retain_loader, batch_size):
        fd, rd = forget_loader.dataset, retain_loader.dataset
        if not (isinstance(fd, ArrayDataset) and isinstance(rd, ArrayDataset)):
            raise TypeError("RL merges the forget and retain sets: both loaders must wrap an ArrayDataset")
        if fd.transform != rd.transform:
            raise ValueError("RL merges the forget and retain sets: their transforms differ")
        self.sources = (fd.data, rd.data)  # held: `matches` compares identities
        self.n_forget = len(fd)
        self.retain_targets = np.asarray(rd.targets).astype(np.int64)
        self.dataset = ArrayDataset(np.concatenate([fd.data, rd.data]),
                                    np.concatenate([np.zeros(self.n_forget, np.int64), self.retain_targets]),
                                    transform=fd.transform)
        kw = {}
        if isinstance(forget_loader, BatchLoader):
            kw = dict(device_resident=forget_loader.device_resident, device=forget_loader.device)
        self.loader = BatchLoader(self.dataset, batch_size, True, **kw)

    def matches(self, forget_loader, retain_loader, batch_size) -> bool:
        fd, rd = forget_loader.dataset, retain_loader.dataset
        return (self.sources[0] is fd.data and self.sources[1] is rd.data and self.loader.batch_size == int(batch_size)
                and self.dataset.transform == fd.transform
                and np.array_equal(self.retain_targets, np.asarray(rd.targets)))

    def relabel(self, num_classes: int) -> np.ndarray:
        """Draw this epoch's forget labels (RL.py:53) and install [drawn, retain] as the loader's label vector."""
        drawn = np.random.randint(0, num_classes, (self.n_forget,))
        self.dataset.targets = np.concatenate([drawn.astype(np.int64), self.retain_targets])
        return drawn


_merged = None  # the MergedSet of the call in progress: built in epoch 0, dropped after the last epoch


def merged_set(forget_loader, retain_loader, epoch: int, args) -> MergedSet:
    global _merged
    if epoch == 0 or _merged is None or not _merged.matches(forget_loader, retain_loader, args.batch_size):
        _merged = MergedSet(forget_loader, retain_loader, args.batch_size)
    m = _merged
    if epoch >= int(getattr(args, "unlearn_epochs", epoch + 1)) - 1:
        _merged = None
    return m


@iterative_unlearn
def RL(data_loaders, model, criterion, optimizer, epoch, args, mask=None):
    forget_loader = data_loaders["forget"]
    retain_loader = data_loaders["retain"]
    if args.dataset not in MERGED_DATASETS + ("cifar10", "svhn"):
        # the reference falls through both branches and dies at `return top1.avg` (RL.py:178)
        raise NotImplementedError(f"RL has no branch for dataset {args.dataset!r} (RL.py:51, 109)")
    merged = args.dataset in MERGED_DATASETS
    if merged and sdist.world_size() > 1:
        raise NotImplementedError("RL on cifar100 / TinyImagenet walks one merged, relabelled set: not sharded over "
                                  "ranks (run it on one GPU)")
    if epoch < args.warmup:
        # the reference's warm-up here reads an undefined loop variable (RL.py:69-71, 119-121)
        raise NameError("name 'i' is not defined  [reference RL.py:120: warmup>0 is unusable; keep --warmup 0]")
    losses, top1 = utils.AverageMeter(), utils.AverageMeter()
    model.train()
    loader_len = len(forget_loader) + len(retain_loader)

    if merged:
        m = merged_set(forget_loader, retain_loader, epoch, args)
        m.relabel(args.num_classes)
        run_pass(m.loader, model, criterion, optimizer, epoch, args, track=True, losses=losses, top1=top1,
                 loader_len=loader_len, print_offset=len(forget_loader))
        return top1.avg

    def random_labels(target):
        return torch.randint(0, args.num_classes, target.shape)

    run_pass(forget_loader, model, criterion, optimizer, epoch, args, label_fn=random_labels, track=False,
             loader_len=loader_len)
    run_pass(retain_loader, model, criterion, optimizer, epoch, args, track=True, losses=losses, top1=top1,
             loader_len=loader_len)
    return top1.avg
