"""`train`: one pre-training epoch (reference Classification/trainer/train.py:31-133) on the flat arena, and
`get_optimizer_and_scheduler` (train.py:17-28).

Same signature, same per-iteration `warmup_lr` rule, same print lines as the reference.  The step is

    optimizer.zero_grad()   one memset of the flat gradient
    loss.backward()         K23's two backward launches hand layer4 its gradient; everything accumulates in the arena
    optimizer.step()        one fused mask * SGD-momentum launch

and the meters (loss sum, hits, samples) live on the device: with the fused head (cls_head.use_fused_head) K23 itself
adds to them, so the loop issues no per-step host synchronisation and no meter kernels; they are read only when a line
is printed.  The reference's `Loss val (avg)` / `Accuracy val (avg)` pairs are printed with the running averages in both
places: the last batch's own values would cost the per-step sync the meters exist to avoid.

Checkpoints: `sgd_state_dict` / `load_sgd_state_dict` convert between FusedMaskedSGD's flat momentum vector and the
`torch.optim.SGD.state_dict()` layout (param_groups + state[i]["momentum_buffer"] in named_parameters() order), so a
checkpoint written by either code base resumes in the other.
"""
from __future__ import annotations

import contextlib
import time
from typing import Dict, Optional

import torch

from .. import utils
from ... import wgrad_side
from ...cls_head import HeadMeters, forward_loss
from ...flat import arena_of
from ...optim import FusedMaskedSGD


def get_optimizer_and_scheduler(model, args):
    """SGD(lr, momentum, weight_decay) + MultiStepLR(decreasing_lr, gamma 0.1), or with `--imagenet_arch` the
    reference's warmup-then-cosine LambdaLR (main_train.py:66-84)."""
    optimizer = FusedMaskedSGD(arena_of(model), args.lr, momentum=args.momentum, weight_decay=args.weight_decay)
    if getattr(args, "imagenet_arch", False):
        import math
        warmup, epochs = args.warmup, args.epochs

        def lambda0(cur_iter):
            if cur_iter < warmup:
                return (cur_iter + 1) / warmup
            return 0.5 * (1.0 + math.cos(math.pi * ((cur_iter - warmup) / (epochs - warmup))))

        scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=lambda0)
    else:
        decreasing_lr = list(map(int, str(args.decreasing_lr).split(",")))
        scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=decreasing_lr, gamma=0.1)  # 0.1 is fixed
    return optimizer, scheduler


def _pack_mask(optimizer, mask):
    """The reference multiplies every gradient by mask[name] before the step; here the optimizer applies the flat mask
    inside its launch (as the unlearn drivers do)."""
    if not mask:
        return None
    if isinstance(mask, torch.Tensor):
        return mask
    return optimizer.arena.pack_mask(mask)


def train(train_loader, model, criterion, optimizer, epoch, args, mask=None, l1=False):
    losses, top1 = utils.AverageMeter(), utils.AverageMeter()
    model.train()
    dev = next(model.parameters()).device
    if not isinstance(optimizer, FusedMaskedSGD):
        raise TypeError("train() steps the flat arena: pass the optimizer of get_optimizer_and_scheduler()")
    optimizer.set_mask(_pack_mask(optimizer, mask))
    meters = HeadMeters(dev)
    print_freq = getattr(args, "print_freq", 50)
    steps = len(train_loader)
    start = time.time()
    for i, (image, target) in enumerate(train_loader):
        if epoch < args.warmup:
            utils.warmup_lr(epoch, i + 1, optimizer, one_epoch_step=steps, args=args)
        image = image.to(dev, non_blocking=True)
        target = target.to(dev, non_blocking=True)

        loss, _ = forward_loss(model, image, target, meters, criterion)
        if l1:
            from ..unlearn._steps import l1_regularization
            loss = loss + args.alpha * l1_regularization(model)
        optimizer.zero_grad()
        # the l1 term gives every parameter a second gradient producer on the main stream: the convolution kernels must
        # then accumulate on the main stream too
        with (wgrad_side.overlap_disabled() if l1 else contextlib.nullcontext()):
            loss.backward()
        optimizer.step()

        if (i + 1) % print_freq == 0:
            avg_loss, avg_top1, _ = meters.read()
            end = time.time()
            print("Epoch: [{0}][{1}/{2}]\t"
                  "Loss {loss:.4f} ({loss:.4f})\t"
                  "Accuracy {top1:.3f} ({top1:.3f})\t"
                  "Time {3:.2f}".format(epoch, i, steps, end - start, loss=avg_loss, top1=avg_top1))
            start = time.time()
    avg_loss, avg_top1, n = meters.read()
    if n:
        losses.update(avg_loss, n)
        top1.update(avg_top1, n)
    print("train_accuracy {top1.avg:.3f}".format(top1=top1))
    return top1.avg


# ------------------------------------------------------------------------------- torch.optim.SGD checkpoint layout
def _sgd_group_template(lr: float) -> dict:
    """The keys (and defaults) torch.optim.SGD puts into a param group in this torch version."""
    probe = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    return dict(probe.state_dict()["param_groups"][0])


def momentum_to_per_param(arena, flat: torch.Tensor) -> Dict[int, Dict[str, torch.Tensor]]:
    """Flat momentum vector -> {i: {"momentum_buffer": tensor of parameter i's shape}} in named_parameters() order."""
    return {i: {"momentum_buffer": flat[o:o + k].view(shp).clone()}
            for i, (o, k, shp) in enumerate(zip(arena.offsets, arena.numels, arena.shapes))}


def momentum_to_flat(arena, state: dict, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The inverse: entries missing from `state` (or without a buffer) leave their slice of `out` as it is (zeros for
    a fresh vector)."""
    flat = out if out is not None else arena.new_like()
    for i, (o, k) in enumerate(zip(arena.offsets, arena.numels)):
        ent = state.get(i, state.get(str(i)))
        buf = None if not ent else ent.get("momentum_buffer")
        if buf is not None:
            flat[o:o + k].copy_(buf.reshape(-1).to(device=flat.device, dtype=flat.dtype))
    return flat


def sgd_state_dict(optimizer: FusedMaskedSGD) -> dict:
    """`optimizer`'s state in exactly torch.optim.SGD.state_dict()'s layout."""
    src = optimizer.param_groups[0]
    group = _sgd_group_template(src["lr"])
    for key, val in src.items():
        if key != "params" and (key in group or key == "initial_lr"):
            group[key] = val
    group["params"] = list(range(len(optimizer.arena.names)))
    state = {}
    if optimizer.momentum_buffer is not None and optimizer.steps > 0:
        state = momentum_to_per_param(optimizer.arena, optimizer.momentum_buffer)
    return {"state": state, "param_groups": [group]}


def load_sgd_state_dict(optimizer: FusedMaskedSGD, sd: dict) -> None:
    """Load a torch.optim.SGD state dict (the reference's checkpoints, or `sgd_state_dict`'s)."""
    groups = sd.get("param_groups") or []
    if groups:
        if len(groups) != 1 or len(groups[0]["params"]) != len(optimizer.arena.names):
            raise ValueError("the optimizer state does not describe this model: expected one param group with "
                             f"{len(optimizer.arena.names)} parameters")
        for key, val in groups[0].items():
            if key != "params":
                optimizer.param_groups[0][key] = val
    state = sd.get("state") or {}
    has_buf = any(ent and ent.get("momentum_buffer") is not None for ent in state.values())
    if has_buf and optimizer.momentum_buffer is not None:
        momentum_to_flat(optimizer.arena, state, optimizer.momentum_buffer)
    # torch creates a buffer on a parameter's first step; with buffers present the next step must not re-create them
    optimizer.steps = max(optimizer.steps, 1) if has_buf else 0
    optimizer._first_step = not has_buf
