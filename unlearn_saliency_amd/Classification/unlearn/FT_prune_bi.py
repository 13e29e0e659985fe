"""Fine-tuning with gradual magnitude pruning (reference Classification/unlearn/FT_prune_bi.py:9-29): every second
epoch, counted back from the last, prunes `prune_rate` of the remaining convolution weights so that the rounds compound
to `args.rate`, then runs the FT pass on the retain set.

The reference declares the plugin without `mask` while its epoch driver always passes one, so through the registry it
raises TypeError (the quirk of GA_l1).  Here it runs; with a saliency mask the optimizer's mask is that
mask AND the prune mask.  A round is `pruner.pruning_model` (K22) and the step stays the one fused launch."""
from .. import pruner
from .FT import FT_iter
from .impl import iterative_unlearn

prune_step = 2


def prune_schedule(unlearn_epochs: int, rate: float):
    """-> (prune_rate of each round, the epochs at whose start a round fires)."""
    rounds = (unlearn_epochs - 1) // prune_step + 1
    prune_rate = 1 - (1 - rate) ** (1 / rounds)
    return prune_rate, [e for e in range(unlearn_epochs) if (unlearn_epochs - e) % prune_step == 0]


@iterative_unlearn
def FT_prune_bi(data_loaders, model, criterion, optimizer, epoch, args, mask=None):
    model.train()
    prune_rate, _ = prune_schedule(args.unlearn_epochs, args.rate)
    fire = (args.unlearn_epochs - epoch) % prune_step == 0
    if epoch == 0:
        # the packed saliency mask the epoch driver just installed on this run's optimizer (or None); later epochs find
        # the optimizer's mask already combined with the prune mask
        optimizer._saliency_u8 = optimizer.mask_u8
    st = pruner.prune_state(model, create=fire)
    if st is not None:
        # refreshed on every call: a model that arrives pruned (--resume, an earlier FT_prune_bi call) must neither keep
        # that run's saliency mask nor lose this one
        st.saliency = getattr(optimizer, "_saliency_u8", None)
        if not fire:
            optimizer.set_mask(pruner.optimizer_mask(model))   # a firing epoch installs it after its round
    if fire:
        if getattr(args, "random_prune", False):
            print("random pruning")
            pruner.pruning_model_random(model, prune_rate, optimizer=optimizer, seed=getattr(args, "seed", 0))
        else:
            print("L1 pruning")
            pruner.pruning_model(model, prune_rate, optimizer=optimizer)
    pruner.check_sparsity(model)
    return FT_iter(data_loaders, model, criterion, optimizer, epoch, args, mask)
