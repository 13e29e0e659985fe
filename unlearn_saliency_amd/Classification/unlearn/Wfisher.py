"""IU — influence unlearning with the WoodFisher inverse-Hessian approximation (reference
Classification/unlearn/Wfisher.py:99-198, `--unlearn wfisher`).  Model in eval mode throughout:

1. F = sum over forget batches of n_b * grad(mean CE), R the same over the retain set (batch `args.batch_size`,
   unshuffled, the datasets' own transforms); T = |forget|, T2 = |retain|;  v = F / (T + T2) - R T / ((T + T2) T2).
2. The reference walks the retain set at batch 1 (N = 1000, at most 1,002 samples): o = g_0, then per sample
   t = <o, g_i>;  k -= (<k, g_i> / (N + t)) o;  o -= (t / (N + t)) o.  Since o is only ever rescaled, o = s g_0 and
   k = v - beta g_0, and the walk needs only a_i = <g_0, g_i> and b_i = <v, g_i>.  Those come from
   `persample.persample_dots` in batches of `args.batch_size` — no per-sample gradient is formed — and
   `salun_iu_recurrence` turns them into beta on the device.
3. theta += alpha (v - beta g_0) (* mask): one `salun_iu_apply` launch over the flat arena.

F and R accumulate with `salun_saliency_accumulate`; g_0 is one batch-1 backward on the product path.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass

import torch
import torch.nn as nn

from ... import dist as sdist
from ... import ops, ops_iu
from ...flat import arena_of
from ...persample import persample_dots
from ..dataset import BatchLoader

WOODFISHER_N = 1000  # the reference's N (Wfisher.py:50): the walk returns after idx > N, i.e. 1,002 samples


@dataclass
class IUPerturbation:
    """The pieces of the IU step, all on the device: perturbation = v - beta[0] * g0 (beta[1] is the final scale s
    of o = s g0); `n` retain samples were walked."""
    v: torch.Tensor
    g0: torch.Tensor
    beta: torch.Tensor
    ab: torch.Tensor
    n: int


def _head(dataset, n):
    if len(dataset) <= n:
        return dataset
    d = copy.copy(dataset)
    d.data, d.targets = dataset.data[:n], dataset.targets[:n]
    return d


def _loader(loader, dataset, batch_size, device):
    return BatchLoader(dataset, batch_size, False, device_resident=bool(getattr(loader, "device_resident", False)),
                       device=device)


def _check_criterion(criterion):
    ok = (type(criterion) is nn.CrossEntropyLoss and criterion.weight is None and criterion.reduction == "mean"
          and criterion.label_smoothing == 0.0)
    if not ok:
        raise NotImplementedError("wfisher: the per-sample pass computes plain cross-entropy gradients; "
                                  f"criterion {criterion} is not nn.CrossEntropyLoss() with default settings")


def _grad_sum(loader, model, criterion, arena, acc):
    """acc += sum over batches of n_b * grad(criterion); returns the number of samples."""
    dev = arena.device
    total = 0
    for image, target in loader:
        image, target = image.to(dev, non_blocking=True), target.to(dev, non_blocking=True)
        n = image.size(0)
        if n == 0:
            continue
        arena.zero_grad()
        criterion(model(image), target).backward()
        ops.saliency_accumulate(acc, arena.grads, float(n))
        total += n
    return total


def iu_perturbation(data_loaders, model, criterion, args) -> IUPerturbation:
    """Steps 1 and 2: v, g_0 and beta (device) for the model as it stands; the model is left in eval mode."""
    if sdist.world_size() > 1:
        raise NotImplementedError("wfisher (IU) runs on one process: the data-parallel form of the per-sample pass "
                                  "is not implemented; launch it with world size 1")
    _check_criterion(criterion)
    arena = arena_of(model)
    if not all(p.requires_grad for p in arena._params):
        raise NotImplementedError("wfisher: every parameter must require a gradient (the flat layout is the "
                                  "reference's concatenation of the trainable parameters)")
    dev = arena.device
    bs = int(args.batch_size)
    retain_ds, forget_ds = data_loaders["retain"].dataset, data_loaders["forget"].dataset
    model.eval()

    F_ = arena.new_like()
    R_ = arena.new_like()
    T = _grad_sum(_loader(data_loaders["forget"], forget_ds, bs, dev), model, criterion, arena, F_)
    T2 = _grad_sum(_loader(data_loaders["retain"], retain_ds, bs, dev), model, criterion, arena, R_)
    if T == 0 or T2 == 0:
        raise ValueError(f"wfisher needs non-empty forget and retain sets (got {T} / {T2} samples)")
    v = arena.new_like()
    ops.saliency_accumulate(v, F_, 1.0 / (T + T2))
    ops.saliency_accumulate(v, R_, -T / ((T + T2) * T2))
    del F_, R_

    # the reference's batch-1 walk covers samples 0 .. N+1 of the unshuffled retain set
    n = min(len(retain_ds), WOODFISHER_N + 2)
    ab = torch.zeros((max(n - 1, 0), 2), dtype=torch.float64, device=dev)
    g0 = None
    off = 0
    for image, target in _loader(data_loaders["retain"], _head(retain_ds, n), bs, dev):
        image, target = image.to(dev, non_blocking=True), target.to(dev, non_blocking=True)
        if g0 is None:  # sample 0: o = g_0, one batch-1 backward on the product path
            arena.zero_grad()
            criterion(model(image[:1]), target[:1]).backward()
            g0 = arena.grads.clone()
            image, target = image[1:], target[1:]
        b = image.size(0)
        if b:
            persample_dots(model, image, target, g0, v, out=ab[off:off + b], arena=arena)
            off += b
    assert off == ab.shape[0], (off, ab.shape)
    arena.zero_grad()
    beta = ops_iu.recurrence(ab, float(WOODFISHER_N))
    return IUPerturbation(v=v, g0=g0, beta=beta, ab=ab, n=n)


def Wfisher(data_loaders, model, criterion, args, mask=None):
    """Same name / signature / effect as the reference function: theta += alpha * perturbation (* mask)."""
    arena = arena_of(model)
    iu = iu_perturbation(data_loaders, model, criterion, args)
    m = arena.pack_mask(mask) if mask else None  # `if mask:` as the reference (Wfisher.py:34)
    ops_iu.apply(arena.params, iu.v, iu.g0, iu.beta, m, float(args.alpha))
    return model
