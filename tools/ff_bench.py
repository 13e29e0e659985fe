"""Wall time of Fisher forgetting (`--unlearn fisher_new`) on full-size ResNet-18, per phase, for both forms of the
activation pass (`persample.fisher_diag`: "replicate" = the batch repeated once per class and one backward, "loop" =
one forward and one backward per class over the retained graph), next to the reference's literal loop on the product
path (per batch of 32: one forward, then per class a full backward and F += mean(prob[:, y]) * grad^2).

    python tools/ff_bench.py [--retain 45000] [--batches 40] [--ref-batches 10]

Inputs: synthetic CIFAR-shaped images (uniform [0, 1)), batches of 32 as the reference's hessian().  Each phase is
timed over `--batches` batches (`--ref-batches` for the literal loop) after one warm-up batch and scaled to the
ceil(retain / 32) batches of a `--retain`-sample set; the apply kernel runs once on the real arena.  Prints one JSON
line.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unlearn_saliency_amd import ops_ff  # noqa: E402
from unlearn_saliency_amd.Classification.models import model_dict  # noqa: E402
from unlearn_saliency_amd.conv import use_salun_convs  # noqa: E402
from unlearn_saliency_amd.flat import arena_of  # noqa: E402
from unlearn_saliency_amd.norm import use_fused_bn  # noqa: E402
from unlearn_saliency_amd.persample import _fisher_capture, _fisher_square, _slicer  # noqa: E402

BATCH = 32


def now():
    torch.cuda.synchronize()
    return time.perf_counter()


def fused_phases(model, arena, xs, C, form):
    """Seconds spent per phase over the batches xs: capture forward, activation backward, K18 grouped squares."""
    F = arena.new_like()
    sl = _slicer(arena)
    t = {"forward": 0.0, "backward": 0.0, "k18": 0.0}
    for x in xs:
        mark = {}
        t0 = now()
        records, w = _fisher_capture(model, x, C, form, loss_hook=lambda: mark.setdefault("fwd", now()))
        t1 = now()
        _fisher_square(records, w, x.shape[0], F, sl)
        t2 = now()
        t["forward"] += mark["fwd"] - t0
        t["backward"] += t1 - mark["fwd"]
        t["k18"] += t2 - t1
        del records
    return t, F


def literal_loop(model, arena, xs, C):
    """The reference's hessian() inner loop on the product path (library autograd through the package's layers)."""
    model.eval()
    F = arena.new_like()
    t0 = now()
    for x in xs:
        out = model(x)
        prob = torch.softmax(out, dim=-1).detach()
        for y in range(C):
            arena.zero_grad()
            Fn.cross_entropy(out, torch.full((x.shape[0],), y, dtype=torch.int64, device=x.device)).backward(
                retain_graph=y + 1 < C)
            g = arena.grads
            F.addcmul_(g * prob[:, y].mean(), g)
    return now() - t0, F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--retain", type=int, default=45000)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--ref-batches", type=int, default=10)
    ap.add_argument("--num_classes", type=int, default=10)
    a = ap.parse_args()
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    model = model_dict["resnet18"](num_classes=a.num_classes).to(dev)
    use_salun_convs(model)
    use_fused_bn(model)
    arena = arena_of(model)
    model.eval()
    C = a.num_classes
    nb_total = math.ceil(a.retain / BATCH)
    xs = [torch.rand(BATCH, 3, 32, 32, device=dev) for _ in range(max(a.batches, a.ref_batches) + 1)]
    res = {"retain": a.retain, "batches_total": nb_total, "batches_timed": a.batches, "ref_batches_timed": a.ref_batches}
    for form in ("replicate", "loop"):
        fused_phases(model, arena, xs[:1], C, form)  # warm-up
        t, _ = fused_phases(model, arena, xs[1:a.batches + 1], C, form)
        per = {k: v / a.batches for k, v in t.items()}
        res[form] = {f"{k}_ms_per_batch": round(1e3 * v, 3) for k, v in per.items()}
        res[form]["total_s"] = round(sum(per.values()) * nb_total, 2)
    F = arena.new_like()
    F.fill_(1e-3)
    ops_ff.apply(arena.params.clone(), F, [p.shape for p in arena._params], C, -1, nb_total, 0.2, 2)  # warm-up
    p = arena.params.clone()
    t0 = now()
    ops_ff.apply(p, F, [q.shape for q in arena._params], C, -1, nb_total, 0.2, 2)
    res["apply_ms"] = round(1e3 * (now() - t0), 3)
    for form in ("replicate", "loop"):
        res[form]["total_s"] = round(res[form]["total_s"] + res["apply_ms"] / 1e3, 2)
    literal_loop(model, arena, xs[:1], C)  # warm-up
    tl, _ = literal_loop(model, arena, xs[1:a.ref_batches + 1], C)
    res["literal"] = {"ms_per_batch": round(1e3 * tl / a.ref_batches, 3),
                      "total_s": round(tl / a.ref_batches * nb_total, 2)}
    res["param_count"] = arena.n
    print(json.dumps(res))


if __name__ == "__main__":
    main()
