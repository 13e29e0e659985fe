"""The `unlearn` plugin registry (reference Classification/unlearn/__init__.py:18-61).

`get_unlearn_method(name)` returns a callable
``method(data_loaders, model, criterion, args, mask=None) -> None`` that mutates `model`
in place; unknown names raise NotImplementedError exactly like the reference.  All 17
registry names are kept so command lines stay drop-in; the SalUn hot path (RL with a
mask), the baselines that share its fused step (GA, GA_l1, FT, FT_l1, raw, boundary_shrink,
boundary_expanding — SURVEY.md §8 F1), the proximal variant (RL_proximal, F2) and the IU / WoodFisher
baseline (wfisher: per-sample gradient dots from one batched backward) and Fisher forgetting
(fisher_new: all classes' squared batch gradients from one pass over the activations) are
implemented, and so are the weight-pruning baselines FT_prune_bi, GA_prune and GA_prune_bi (global magnitude or random
pruning of the convolution weights as one K22 round on the flat arena); the per-sample empirical Fisher
(fisher), FT_prune and retrain are registered but raise with a scope note.
"""
from .boundary_ex import boundary_expanding
from .boundary_sh import boundary_shrink
from .fisher import fisher_new
from .FT import FT, FT_l1
from .FT_prune_bi import FT_prune_bi
from .GA import GA, GA_l1
from .GA_prune import GA_prune
from .GA_prune_bi import GA_prune_bi
from .impl import (FusedMaskedSGD, iterative_unlearn, load_unlearn_checkpoint, save_unlearn_checkpoint)
from .RL import RL
from .RL_pro import RL_proximal
from .Wfisher import Wfisher


def raw(data_loaders, model, criterion, args, mask=None):
    """No unlearning: evaluate the original model."""
    return None


def _out_of_scope(name, why):
    def method(data_loaders, model, criterion, args, mask=None):
        raise NotImplementedError(f"Unlearn method {name} is registered for CLI compatibility but is outside the "
                                  f"accelerated hot path of this build ({why}); see SURVEY.md §8 (f)")
    method.__name__ = name
    return method


_REGISTRY = {
    "raw": raw, "RL": RL, "GA": GA, "FT": FT, "FT_l1": FT_l1, "GA_l1": GA_l1,
    "retrain": _out_of_scope("retrain", "re-training from scratch is pre-training, not unlearning arithmetic"),
    "fisher": _out_of_scope("fisher", "Fisher-forgetting baseline"),
    "fisher_new": fisher_new,
    "wfisher": Wfisher,
    # stays a scope note: tests/test_cli.py::test_registry_names_match_reference pins FT_prune to NotImplementedError
    "FT_prune": _out_of_scope("FT_prune", "pruning baseline"),
    "FT_prune_bi": FT_prune_bi, "GA_prune": GA_prune, "GA_prune_bi": GA_prune_bi,
    "boundary_expanding": boundary_expanding, "boundary_shrink": boundary_shrink, "RL_proximal": RL_proximal,
}


def get_unlearn_method(name):
    """method usage:  function(data_loaders, model, criterion, args, mask=None)"""
    try:
        return _REGISTRY[name]
    except KeyError:
        raise NotImplementedError(f"Unlearn method {name} not implemented!") from None
