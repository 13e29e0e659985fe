"""Gradient ascent with a pruning round after every epoch (reference Classification/unlearn/GA_prune_bi.py:67-160): one
optimizer (`args.lr`, momentum, weight decay) and MultiStepLR schedule over `args.epochs`; per epoch the GA pass on the
forget set, validate on val and test, scheduler.step(), save_checkpoint, the plot, then a prune at `args.rate` (or a
random prune) and check_sparsity.  Same fused step and K22 rounds as GA_prune; `mask=None` only."""
from .. import pruner
from .GA_prune import _epoch, _fresh_optimizer, _new_result, _no_mask, _prune_round, _report


def GA_prune_bi(data_loaders, model, criterion, args, mask=None):
    _no_mask("GA_prune_bi", mask)
    milestones = list(map(int, str(args.decreasing_lr).split(",")))
    all_result, best_sa = _new_result(), 0
    optimizer, scheduler = _fresh_optimizer(model, args, milestones)
    print("######################################## Start Standard Training Iterative Pruning "
          "########################################")
    try:
        pruner.check_sparsity(model)
        state = 0
        for epoch in range(0, args.epochs):
            best_sa = _epoch(data_loaders, model, criterion, optimizer, scheduler, epoch, args, state, all_result,
                             best_sa, lambda: None)
            _report(data_loaders, model, criterion, args, all_result)
            _prune_round(model, args, optimizer)
    finally:
        optimizer.close()
    return model
