"""One global pruning round at ResNet-18 size (n_sel = 11.16 M convolution weights), this build's K22 round against
torch.nn.utils.prune.global_unstructured on the same device, and what a pruned model costs per step afterwards: forward
+ backward of the hooked torch model (20 weight_orig * weight_mask multiplies per forward, and their autograd) against
the same torch model with the masks folded in (prune.remove) and against this build's pruned model.

    python tools/prune_bench.py [--reps 7] [--batch 256] [--out profiles/prune_bench.json]

A round is timed on the host clock around a synchronise — this build's round ends in its status check, which
synchronises anyway — over `--reps` repetitions after two warm-up rounds, the two implementations alternating (and swapping which goes first), each
repetition on freshly restored weights.  Forward + backward is timed with device events, the three models alternating in a rotating order.
Medians are reported, with min and max.  Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn
import torch.nn.utils.prune as tprune

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unlearn_saliency_amd.Classification import pruner  # noqa: E402
from unlearn_saliency_amd.Classification.models import model_dict  # noqa: E402
from unlearn_saliency_amd.conv import use_salun_convs  # noqa: E402
from unlearn_saliency_amd.flat import arena_of  # noqa: E402
from unlearn_saliency_amd.norm import use_fused_bn  # noqa: E402

WARMUP = 2


def now():
    torch.cuda.synchronize()
    return time.perf_counter()


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def torch_prune(model, amount):
    tprune.global_unstructured([(m, "weight") for m in model.modules() if isinstance(m, nn.Conv2d)],
                               pruning_method=tprune.L1Unstructured, amount=amount)


def time_rounds(own, plain, amount, reps):
    arena = arena_of(own)
    saved = arena.params.clone()
    t_own, t_torch = [], []
    def own_round():
        arena.params.copy_(saved)
        if pruner.prune_state(own) is not None:
            pruner.remove_prune(own)
        pruner.prune_state(own, create=True)          # the keep vector and the table: built once per model, not per round
        t0 = now()
        pruner.pruning_model(own, amount)
        return (now() - t0) * 1e3

    def torch_round():
        victim = copy.deepcopy(plain)
        t0 = now()
        torch_prune(victim, amount)
        return (now() - t0) * 1e3

    for r in range(WARMUP + reps):
        if r % 2 == 0:   # alternate which side goes first: neither always inherits the other's cache and clock state
            a, b = own_round(), torch_round()
        else:
            b, a = torch_round(), own_round()
        if r >= WARMUP:
            t_own.append(a)
            t_torch.append(b)
    return stats(t_own), stats(t_torch)


def time_steps(models, x, y, reps):
    out = {k: [] for k in models}
    for r in range(WARMUP + reps):
        order = list(models.items())
        order = order[r % len(order):] + order[:r % len(order)]   # rotate the order from repetition to repetition
        for name, m in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if name == "own_pruned":
                arena_of(m).zero_grad()        # its gradients are views of the flat vector: one memset
            else:
                m.zero_grad(set_to_none=True)
            e0.record()
            nn.functional.cross_entropy(m(x), y).backward()
            e1.record()
            e1.synchronize()
            if r >= WARMUP:
                out[name].append(e0.elapsed_time(e1))
    return {k: stats(v) for k, v in out.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join("profiles", "prune_bench.json"))
    a = ap.parse_args(argv)
    torch.manual_seed(0)
    plain = model_dict["resnet18"](num_classes=10).cuda().train()
    own = model_dict["resnet18"](num_classes=10).cuda().train()
    own.load_state_dict(plain.state_dict())
    use_salun_convs(own)
    use_fused_bn(own)
    x = torch.rand(a.batch, 3, 32, 32, device="cuda")
    y = torch.randint(0, 10, (a.batch,), device="cuda")
    res = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "reps": a.reps, "amounts": {}}
    for amount in (0.2, 0.95):
        r_own, r_torch = time_rounds(own, plain, amount, a.reps)
        hooked = copy.deepcopy(plain)
        torch_prune(hooked, amount)
        folded = copy.deepcopy(hooked)
        for m in folded.modules():
            if isinstance(m, nn.Conv2d):
                tprune.remove(m, "weight")
        st = pruner.prune_state(own)
        steps = time_steps({"torch_hooked": hooked, "torch_masks_folded": folded, "own_pruned": own}, x, y, a.reps)
        res["amounts"][str(amount)] = {"n_sel": st.n_sel, "alive_after": st.alive, "round_own": r_own,
                                       "round_torch": r_torch, "fwd_bwd": steps}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
