"""Fisher forgetting (reference Classification/unlearn/fisher.py:50-114, `--unlearn fisher_new`).  Model in eval mode
throughout, and left in eval mode as the reference leaves it:

1. `hessian`: the retain set, unshuffled, in batches of 32 (the last one ragged; `data_loaders["retain"].dataset` with
   its own transforms, through a BatchLoader that keeps the caller's `device_resident` choice).  Per batch and class y
   the reference runs a full backward of CE_mean(output, y) and adds mean_i(prob[i, y]) * grad^2 to every parameter.
   Here `persample.fisher_diag` gets all classes' squared gradients from ONE pass over the activations (DESIGN.md
   §9c) and the K18 kernels (csrc/salun_ff.hip) add them into one fp32 vector F in arena layout.  F is divided by the
   number of batches, not samples, as in the reference.  `criterion` is ignored, as in the reference.
2. `get_mean_var` for every parameter, by shape: var = alpha * clamp(1 / (F + 1e-8), max 1e3 [and 1e2 when shape[0] ==
   num_classes]); its mean over dim 1 when ndim > 1; mu = p; when shape[0] == num_classes and
   (num_indexes_to_replace, dataset) is (4500, cifar10) or (450, cifar100), row `class_to_replace` (default -1: the last
   row) gets mu = 0 and var = 1e-4; then var x10 when shape[0] == num_classes or ndim == 1.
3. p = mu + sqrt(var) z: steps 2 and 3 are one `salun_ff_apply` launch over the flat arena.

The noise z is the package's counter-based normal keyed by `args.seed` and the flat parameter index
(`ops.fill_normal(n, args.seed)` regenerates it), not the reference's `torch.normal_` stream: the draws differ, their
distribution (N(0, 1), independent per element) is the same.  The reference function takes no mask, so a mask
raises; so does a world size above 1.
"""
from __future__ import annotations

import torch

from ... import dist as sdist
from ... import ops_ff
from ...flat import arena_of
from ...persample import fisher_diag
from ..dataset import BatchLoader

HESSIAN_BATCH = 32  # the reference's DataLoader(batch_size=32, shuffle=False) in hessian()


def _override_row(args):
    """The reference's class-row override applies to (num_indexes_to_replace, dataset) = (4500, cifar10) / (450,
    cifar100) only; returns `class_to_replace` then, else None."""
    n, ds = getattr(args, "num_indexes_to_replace", None), getattr(args, "dataset", None)
    if (n == 4500 and ds == "cifar10") or (n == 450 and ds == "cifar100"):
        return int(args.class_to_replace)
    return None


def fisher_grad2(data_loaders, model, num_classes: int, arena=None):
    """Step 1: (F, number of batches) — F is the raw fp32 sum over the batches of sum_y mean_i(prob[i, y]) grad_y^2."""
    arena = arena if arena is not None else arena_of(model)
    dev = arena.device
    loader = data_loaders["retain"]
    batches = BatchLoader(loader.dataset, HESSIAN_BATCH, False,
                          device_resident=bool(getattr(loader, "device_resident", False)), device=dev)
    model.eval()
    F = arena.new_like()
    nb = 0
    for image, _ in batches:
        image = image.to(dev, non_blocking=True)
        if image.size(0) == 0:
            continue
        fisher_diag(model, image, num_classes, F, arena=arena)
        nb += 1
    return F, nb


def fisher_new(data_loaders, model, criterion, args, mask=None):
    """Same name / effect as the reference function: every parameter becomes mu + sqrt(var) * z."""
    if mask is not None:
        raise NotImplementedError("fisher_new takes no mask: the reference's Fisher forgetting perturbs every "
                                  "parameter (run it without --mask)")
    if sdist.world_size() > 1:
        raise NotImplementedError("fisher_new runs on one process: the data-parallel form of the Fisher pass is not "
                                  "implemented; launch it with world size 1")
    arena = arena_of(model)
    if not all(p.requires_grad for p in arena._params):
        raise NotImplementedError("fisher_new: every parameter must require a gradient (the flat layout is the "
                                  "reference's concatenation of the trainable parameters)")
    num_classes = int(args.num_classes)
    F, nb = fisher_grad2(data_loaders, model, num_classes, arena)
    if nb == 0:
        raise ValueError("fisher_new needs a non-empty retain set")
    ops_ff.apply(arena.params, F, [p.shape for p in arena._params], num_classes, _override_row(args), nb,
                 float(args.alpha), int(args.seed))
    model.eval()
    return model
