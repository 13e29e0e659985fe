"""Global weight pruning on the flat arena (reference Classification/pruner/utils.py:23-175, which drives
torch.nn.utils.prune over every nn.Conv2d weight).

The reference re-parametrises each convolution (`weight = weight_orig * weight_mask`, recomputed by a forward pre-hook
on every forward) and ranks with a cat + torch.topk + per-layer scatter per round.  Here a `PruneState` hangs on the
model: one u8 `keep` vector over the arena (1 outside the convolution weights), the device table of the convolution
weights' (offset, length) ranges and the host count `alive` of weights still standing.  A round is
`ops.prune_global` (K22: gather, select, scatter) and costs nothing per step afterwards: the arena holds the effective
weights, and `FusedMaskedSGD` keeps a weight whose mask byte is 0 at its value — zero — with zero momentum.

While a state exists `model.state_dict()` reads like a hooked torch model: `<conv>.weight_orig` and `<conv>.weight_mask`
(float 0/1) stand in for `<conv>.weight`, and `load_state_dict` accepts that form.  `weight_orig` holds the effective
weights (pruned entries are 0; the reference keeps weight-decayed leftovers there that nothing reads).
"""
from __future__ import annotations

import copy
from collections import OrderedDict
from typing import Dict, Optional

import torch
import torch.nn as nn

from ... import ops
from ...flat import FlatArena, arena_of

__all__ = ["pruning_model", "pruning_model_random", "prune_model_custom", "remove_prune", "extract_mask",
           "reverse_mask", "check_sparsity", "check_sparsity_dict", "prune_state", "optimizer_mask", "PruneState"]

_STATE_ATTR = "_salun_prune_state"
_ROUNDS_ATTR = "_salun_prune_rounds"  # survives remove_prune: the random variant's keys differ from round to round


def conv_weight_names(model: nn.Module) -> list:
    """`<module>.weight` of every nn.Conv2d, the set the reference prunes (pruner/utils.py:26-28)."""
    return [name + ".weight" if name else "weight" for name, m in model.named_modules() if isinstance(m, nn.Conv2d)]


class _Segments:
    """The convolution weights' ranges in the arena, ascending, and their device table.  Cached on the arena."""

    def __init__(self, model: nn.Module, arena: FlatArena):
        at = {n: i for i, n in enumerate(arena.names)}
        idx = sorted(at[n] for n in conv_weight_names(model) if n in at)
        if not idx:
            raise ValueError("the model has no nn.Conv2d weight to prune")
        self.names = [arena.names[i] for i in idx]
        self.ranges = [(arena.offsets[i], arena.numels[i]) for i in idx]
        self.shapes = [arena.shapes[i] for i in idx]
        self.table = torch.tensor(self.ranges, dtype=torch.int64, device=arena.device).reshape(-1, 2)
        self.n_sel = sum(k for _, k in self.ranges)


def _segments(model: nn.Module) -> tuple:
    arena = arena_of(model)
    if not arena.params.is_cuda:
        raise RuntimeError("pruning runs on the flat arena of a device model; there is no CPU path")
    sg = getattr(arena, "_salun_conv_segs", None)
    if sg is None:
        sg = arena._salun_conv_segs = _Segments(model, arena)
    return arena, sg


class PruneState:
    """keep / segment table / alive count of one model's arena."""

    def __init__(self, model: nn.Module):
        arena, sg = _segments(model)
        self.arena: FlatArena = arena
        self.names, self.ranges, self.shapes, self.segs, self.n_sel = sg.names, sg.ranges, sg.shapes, sg.table, sg.n_sel
        self.keep = torch.ones(arena.n, dtype=torch.uint8, device=arena.device)
        self.alive = self.n_sel
        self.saliency: Optional[torch.Tensor] = None  # flat u8 saliency mask the optimizer mask is ANDed with
        self.seed = 0
        self._hooks: list = []

    def mask_of(self, j: int) -> torch.Tensor:
        o, k = self.ranges[j]
        return self.keep[o:o + k].view(self.shapes[j])

    def recount(self) -> None:
        """alive from a popcount (one host sync): after a custom mask or a checkpoint was loaded."""
        outside = self.arena.n - self.n_sel
        self.alive = ops.mask_popcount(self.keep) - outside


def prune_state(model: nn.Module, create: bool = False) -> Optional[PruneState]:
    st = getattr(model, _STATE_ATTR, None)
    if st is not None and arena_of(model) is not st.arena:
        raise RuntimeError("the model's parameters were re-homed while it was pruned (model.to(...) after pruning?)")
    if st is None and create:
        st = PruneState(model)
        st._hooks = [model._register_state_dict_hook(_state_dict_hook),
                     model._register_load_state_dict_pre_hook(_load_pre_hook, with_module=True)]
        object.__setattr__(model, _STATE_ATTR, st)
    return st


def optimizer_mask(model: nn.Module) -> Optional[torch.Tensor]:
    """What `FusedMaskedSGD.set_mask` gets: keep, ANDed with the saliency mask if the state carries one; None if the
    model is not pruned."""
    st = prune_state(model)
    if st is None:
        return None
    return st.keep if st.saliency is None else st.keep & st.saliency


# ------------------------------------------------------------------ state_dict in the hooked-model layout
def _state_dict_hook(module, state_dict, prefix, local_metadata):
    st = getattr(module, _STATE_ATTR, None)
    if st is None:
        return state_dict
    conv = {prefix + n: j for j, n in enumerate(st.names)}
    out = OrderedDict()
    for key, val in state_dict.items():
        j = conv.get(key)
        if j is None:
            out[key] = val
        else:
            out[key + "_orig"] = val
            out[key + "_mask"] = st.mask_of(j).to(val.dtype)
    meta = getattr(state_dict, "_metadata", None)
    if meta is not None:
        out._metadata = meta
    return out


def _load_pre_hook(module, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
    st = getattr(module, _STATE_ATTR, None)
    if st is None:
        return
    changed = False
    for j, n in enumerate(st.names):
        key = prefix + n
        if key + "_orig" not in state_dict:
            continue
        w = state_dict.pop(key + "_orig")
        m = state_dict.pop(key + "_mask", None)
        if m is not None:
            w = w * m.to(w.dtype)
            st.mask_of(j).copy_((m != 0).to(torch.uint8))
            changed = True
        state_dict[key] = w
    if changed:
        st.recount()


# ------------------------------------------------------------------ pruning operations
def _round_key(model: nn.Module, seed: int) -> int:
    r = getattr(model, _ROUNDS_ATTR, 0)
    object.__setattr__(model, _ROUNDS_ATTR, r + 1)
    # salun_fill_uniform draws element i from splitmix64(key + i): rounds sit 2^34 apart, far more than any n_sel
    return (int(seed) * 0x9E3779B97F4A7C15 + (r << 34)) & 0xFFFFFFFFFFFFFFFF


def _prune(model: nn.Module, px, optimizer, rnd_seed: Optional[int]) -> int:
    st = prune_state(model, create=True)
    if isinstance(px, int) and not isinstance(px, bool):
        if not 0 <= px <= st.alive:
            raise ValueError(f"amount={px} should be smaller than the number of parameters to prune={st.alive}")
        k = px
    else:
        k = ops.prune_amount(px, st.alive)
    if k:
        rnd = None   # (a round that prunes nothing launches nothing and does not use up a round key)
        if rnd_seed is not None:
            rnd = ops.fill_uniform(st.n_sel, _round_key(model, rnd_seed), device=st.arena.device)
        buf = getattr(optimizer, "momentum_buffer", None) if optimizer is not None else None
        ops.prune_global(st.arena.params, buf, st.keep, st.segs, st.n_sel, st.alive, k, rnd=rnd)
        st.alive -= k
    if optimizer is not None:
        optimizer.set_mask(optimizer_mask(model))
    return k


def pruning_model(model: nn.Module, px, optimizer=None) -> None:
    """global_unstructured(L1Unstructured, amount=px) over every conv weight.  `optimizer` (a FusedMaskedSGD on this
    model's arena): its momentum is zeroed at the pruned weights and its mask becomes `optimizer_mask(model)`."""
    print("Apply Unstructured L1 Pruning Globally (all conv layers)")
    _prune(model, px, optimizer, None)


def pruning_model_random(model: nn.Module, px, optimizer=None, seed: Optional[int] = None) -> None:
    """global_unstructured(RandomUnstructured, amount=px): uniform without replacement among the alive conv weights.
    The keys come from salun_fill_uniform keyed by (seed, pruning round of this model) — not by rank, so every data-parallel
    rank prunes the same set — and do not reproduce torch's generator (the draws.py convention)."""
    print("Apply Unstructured Random Pruning Globally (all conv layers)")
    st = prune_state(model, create=True)
    _prune(model, px, optimizer, st.seed if seed is None else seed)


def prune_model_custom(model: nn.Module, mask_dict: Dict[str, torch.Tensor]) -> None:
    """CustomFromMask per conv layer, keys `<conv>.weight_mask`."""
    print("Pruning with custom mask (all conv layers)")
    st = prune_state(model, create=True)
    with torch.no_grad():
        for j, n in enumerate(st.names):
            mask_name = n + "_mask"
            if mask_name not in mask_dict:
                print("Can not find [{}] in mask_dict".format(mask_name))
                continue
            m = (mask_dict[mask_name].to(st.arena.device) != 0).reshape(st.shapes[j])
            o, k = st.ranges[j]
            st.mask_of(j).mul_(m.to(torch.uint8))
            st.arena.params[o:o + k].mul_(m.reshape(-1).to(torch.float32))  # a torch write: the weight images see it
    st.recount()


def remove_prune(model: nn.Module) -> None:
    """Drops the state; the zeros stay in the weights (prune.remove makes `weight_orig * weight_mask` the weight)."""
    print("Remove hooks for multiplying masks (all conv layers)")
    st = getattr(model, _STATE_ATTR, None)
    if st is None:
        raise ValueError("Parameter 'weight' of the model's convolutions has to be pruned before pruning can be removed")
    for h in st._hooks:
        h.remove()
    object.__delattr__(model, _STATE_ATTR)


# ------------------------------------------------------------------ mask dictionaries (host)
def extract_mask(model_dict):
    return {key: copy.deepcopy(val) for key, val in model_dict.items() if "mask" in key}


def reverse_mask(mask_dict):
    return {key: 1 - val for key, val in mask_dict.items()}


def _report(zero_sum: float, sum_list: float):
    if zero_sum:
        remain_weight_ratie = 100 * (1 - zero_sum / sum_list)
        print("* remain weight ratio = ", 100 * (1 - zero_sum / sum_list), "%")
    else:
        print("no weight for calculating sparsity")
        remain_weight_ratie = None
    return remain_weight_ratie


def check_sparsity(model: nn.Module):
    """100 * (1 - zeros / weights) over the conv layers, None when there is no zero.  One counting launch over the
    segments on a device model (and one read-back); a host model is counted by torch."""
    convs = [m for m in model.modules() if isinstance(m, nn.Conv2d)]
    if not convs:
        return _report(0.0, 0.0)
    if not convs[0].weight.is_cuda or hasattr(convs[0], "weight_orig"):  # a host model, or one torch's own hooks prune
        return _report(float(sum(int(torch.sum(m.weight == 0)) for m in convs)),
                       float(sum(m.weight.nelement() for m in convs)))
    arena, sg = _segments(model)
    p, segs, n_sel = arena.params, sg.table, sg.n_sel
    zeros = int(ops.prune_count_zeros(p, segs, n_sel).item())
    if zeros < 0:
        raise RuntimeError("salun_prune_count_zeros refused the segment table")
    return _report(float(zeros), float(n_sel))


def check_sparsity_dict(state_dict):
    sum_list = 0
    zero_sum = 0
    for key in state_dict.keys():
        if "mask" in key:
            sum_list += float(state_dict[key].nelement())
            zero_sum += float(torch.sum(state_dict[key] == 0))
    return _report(zero_sum, sum_list)
