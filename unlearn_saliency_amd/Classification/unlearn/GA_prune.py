"""Gradient ascent with iterative magnitude pruning and weight rewinding (reference
Classification/unlearn/GA_prune.py:67-209): `pruning_times` states of `epochs` GA epochs; after each state the model is
pruned at `args.rate`, the mask is extracted, and — except after the last state — the weights rewind to the saved
initialisation under that mask with a fresh optimizer and schedule.

Runs on `run_pass` + `FusedMaskedSGD`: the optimizer's mask is the prune mask, a pruning round is K22
(`pruner.pruning_model`).  The reference takes `(data_loaders, model, criterion, args)`; main_random passes a fifth
argument and the reference dies with TypeError — here `mask=None` is accepted and anything else raises TypeError."""
import os
import time
from copy import deepcopy

import numpy as np
import torch

from ...flat import arena_of
from ...optim import FusedMaskedSGD
from .. import pruner, utils
from ..trainer import validate
from .GA import _ga_epoch
from .impl import plot_training_curve


def _no_mask(name, mask):
    if mask is not None:
        raise TypeError(f"{name}() takes 4 positional arguments but 5 were given")


def _fresh_optimizer(model, args, milestones):
    optimizer = FusedMaskedSGD(arena_of(model), args.lr, momentum=args.momentum, weight_decay=args.weight_decay)
    optimizer.set_mask(pruner.optimizer_mask(model))
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=milestones, gamma=0.1)
    return optimizer, scheduler


def _new_result():
    return {"train_ta": [], "test_ta": [], "val_ta": []}


def _epoch(data_loaders, model, criterion, optimizer, scheduler, epoch, args, state, all_result, best_sa, init_weight):
    """GA pass, validate on val and test, scheduler.step(), save_checkpoint with the reference's keys, the plot."""
    start_time = time.time()
    print(optimizer.state_dict()["param_groups"][0]["lr"])
    acc = _ga_epoch(data_loaders, model, criterion, optimizer, epoch, args)
    tacc = validate(data_loaders["val"], model, criterion, args)
    test_tacc = validate(data_loaders["test"], model, criterion, args)
    scheduler.step()
    all_result["train_ta"].append(acc)
    all_result["val_ta"].append(tacc)
    all_result["test_ta"].append(test_tacc)
    is_best_sa = tacc > best_sa
    best_sa = max(tacc, best_sa)
    utils.save_checkpoint({"state": state, "result": all_result, "epoch": epoch + 1, "state_dict": model.state_dict(),
                           "best_sa": best_sa, "optimizer": optimizer.state_dict(),
                           "scheduler": scheduler.state_dict(), "init_weight": init_weight()},
                          is_SA_best=is_best_sa, pruning=state, save_path=args.save_dir)
    plot_training_curve({"train": all_result["train_ta"], "val": all_result["val_ta"], "test": all_result["test_ta"]},
                        args.save_dir, str(state) + "net")
    print("one epoch duration:{}".format(time.time() - start_time))
    return best_sa


def _report(data_loaders, model, criterion, args, all_result):
    pruner.check_sparsity(model)
    print("Performance on the test data set")
    validate(data_loaders["test"], model, criterion, args)
    if len(all_result["val_ta"]) != 0:
        val_pick_best_epoch = np.argmax(np.array(all_result["val_ta"]))
        print("* best SA = {}, Epoch = {}".format(all_result["test_ta"][val_pick_best_epoch], val_pick_best_epoch + 1))


def _prune_round(model, args, optimizer):
    if getattr(args, "random_prune", False):
        print("random pruning")
        pruner.pruning_model_random(model, args.rate, optimizer=optimizer, seed=getattr(args, "seed", 0))
    else:
        print("L1 pruning")
        pruner.pruning_model(model, args.rate, optimizer=optimizer)
    return pruner.check_sparsity(model)


def GA_prune(data_loaders, model, criterion, args, mask=None):
    _no_mask("GA_prune", mask)
    milestones = list(map(int, str(args.decreasing_lr).split(",")))
    all_result, best_sa = _new_result(), 0
    optimizer, scheduler = _fresh_optimizer(model, args, milestones)
    holder = {}

    def init_weight():
        if "w" in holder:
            return holder["w"]
        if args.prune_type == "pt":   # loaded after the first state; the checkpoints before that carry None
            return None
        # lt, or rewind_lt whose rewind epoch has not come: the reference reads a variable it never assigned
        raise NameError("name 'initalization' is not defined")

    print("######################################## Start Standard Training Iterative Pruning "
          "########################################")
    try:
        for state in range(0, args.pruning_times):
            print("******************************************")
            print("pruning state", state)
            print("******************************************")
            pruner.check_sparsity(model)
            for epoch in range(0, args.epochs):
                if state == 0 and epoch == args.rewind_epoch:
                    torch.save(model.state_dict(),
                               os.path.join(args.save_dir, "epoch_{}_rewind_weight.pt".format(epoch + 1)))
                    if args.prune_type == "rewind_lt":
                        holder["w"] = deepcopy(model.state_dict())
                best_sa = _epoch(data_loaders, model, criterion, optimizer, scheduler, epoch, args, state, all_result,
                                 best_sa, init_weight)
            _report(data_loaders, model, criterion, args, all_result)
            all_result, best_sa = _new_result(), 0
            if args.prune_type == "pt":
                print("* loading pretrained weight")
                holder["w"] = torch.load(os.path.join(args.save_dir, "0model_SA_best.pth.tar"),
                                         map_location=next(model.parameters()).device, weights_only=False)["state_dict"]
            _prune_round(model, args, optimizer)
            current_mask = pruner.extract_mask(model.state_dict())
            pruner.remove_prune(model)
            if state < args.pruning_times - 1:
                model.load_state_dict(init_weight(), strict=False)
                pruner.prune_model_custom(model, current_mask)
                optimizer.close()
                optimizer, scheduler = _fresh_optimizer(model, args, milestones)
                for _ in range(args.rewind_epoch):  # learning rate rewinding
                    scheduler.step()
    finally:
        optimizer.close()
    return model
