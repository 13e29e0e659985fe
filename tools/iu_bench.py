"""Wall time of the IU / WoodFisher baseline (`--unlearn wfisher`) on full-size ResNet-18, per phase, next to the
reference's literal loop (batch-1 autograd passes in plain PyTorch on the same device) and the apply kernel's
achieved bandwidth.

    python tools/iu_bench.py [--batch_size 256] [--ref-samples 1002] [--repeats 3]

Data: the synthetic CIFAR-shaped set with 4,500 forget / 40,500 retain samples (`--num_indexes_to_replace 4500`),
device-resident loader.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unlearn_saliency_amd import conv as sconv  # noqa: E402
from unlearn_saliency_amd import ops, ops_iu  # noqa: E402
from unlearn_saliency_amd.Classification import arg_parser, utils  # noqa: E402
from unlearn_saliency_amd.Classification.dataset import BatchLoader, split_marked  # noqa: E402
from unlearn_saliency_amd.Classification.unlearn.Wfisher import WOODFISHER_N  # noqa: E402
from unlearn_saliency_amd.conv import use_salun_convs  # noqa: E402
from unlearn_saliency_amd.flat import arena_of  # noqa: E402
from unlearn_saliency_amd.norm import use_fused_bn  # noqa: E402
from unlearn_saliency_amd.persample import persample_dots  # noqa: E402

W = sys.modules["unlearn_saliency_amd.Classification.unlearn.Wfisher"]  # the module (the package re-exports the function)


def sync_time(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t


def phases(model, forget_ds, retain_ds, bs, dev, device_resident):
    """The plugin's steps, timed one by one (same calls as Wfisher.iu_perturbation / Wfisher)."""
    arena = arena_of(model)
    crit = nn.CrossEntropyLoss()
    mk = lambda ds: BatchLoader(ds, bs, False, device_resident=device_resident, device=dev)
    model.eval()
    out = {}
    F_, R_ = arena.new_like(), arena.new_like()
    (T, out["F_sum_s"]) = sync_time(lambda: W._grad_sum(mk(forget_ds), model, crit, arena, F_))
    (T2, out["R_sum_s"]) = sync_time(lambda: W._grad_sum(mk(retain_ds), model, crit, arena, R_))
    v = arena.new_like()
    ops.saliency_accumulate(v, F_, 1.0 / (T + T2))
    ops.saliency_accumulate(v, R_, -T / ((T + T2) * T2))
    n = min(len(retain_ds), W.WOODFISHER_N + 2)
    head = W._head(retain_ds, n)
    batches = [(x.to(dev), y.to(dev)) for x, y in mk(head)]

    def g0_fn():
        arena.zero_grad()
        crit(model(batches[0][0][:1]), batches[0][1][:1]).backward()
        return arena.grads.clone()

    g0, out["g0_s"] = sync_time(g0_fn)
    ab = torch.zeros((n - 1, 2), dtype=torch.float64, device=dev)

    def ps():
        off = 0
        for i, (x, y) in enumerate(batches):
            if i == 0:
                x, y = x[1:], y[1:]
            persample_dots(model, x, y, g0, v, out=ab[off:off + x.shape[0]], arena=arena)
            off += x.shape[0]

    _, out["persample_s"] = sync_time(ps)
    beta, out["beta_s"] = sync_time(lambda: ops_iu.recurrence(ab, float(W.WOODFISHER_N)))
    p_save = arena.params.clone()
    _, out["apply_s"] = sync_time(lambda: ops_iu.apply(arena.params, v, g0, beta, None, 0.2))
    arena.params.copy_(p_save)
    out["total_s"] = sum(out[k] for k in ("F_sum_s", "R_sum_s", "g0_s", "persample_s", "beta_s", "apply_s"))
    return out, (v, g0, beta)


def apply_bandwidth(arena, v, g0, beta, masked, reps=20):
    m = torch.ones(arena.n, dtype=torch.uint8, device=v.device) if masked else None
    p_save = arena.params.clone()
    ops_iu.apply(arena.params, v, g0, beta, m, 0.0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ops_iu.apply(arena.params, v, g0, beta, m, 0.0)
    e1.record()
    torch.cuda.synchronize()
    arena.params.copy_(p_save)
    sec = e0.elapsed_time(e1) / 1e3 / reps
    return sec, arena.n * (17 if masked else 16) / sec / 1e9


def literal_reference(model_plain, retain_ds, v, nsamp, dev):
    """The reference's woodfisher loop (Wfisher.py:47-70): batch 1, autograd.grad, two dots and two axpys per sample."""
    model_plain.eval()
    params = [p for p in model_plain.parameters() if p.requires_grad]
    loader = BatchLoader(W._head(retain_ds, nsamp), 1, False, device_resident=True, device=dev)
    crit = nn.CrossEntropyLoss()

    def run():
        k = v.clone()
        o = None
        N = 1000
        for idx, (x, y) in enumerate(loader):
            model_plain.zero_grad()
            g = torch.cat([t.view(-1) for t in torch.autograd.grad(crit(model_plain(x), y), params)])
            with torch.no_grad():
                if o is None:
                    o = g.clone()
                else:
                    t = torch.dot(o, g)
                    k -= (torch.dot(k, g) / (N + t)) * o
                    o -= (t / (N + t)) * o
            if idx > N:
                break
        return k

    return sync_time(run)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--ref-samples", type=int, default=1002, help="samples of the literal loop (0: skip it)")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    args = arg_parser.parse_args(["--synthetic", "--device_loader", "--num_indexes_to_replace", "4500",
                                  "--batch_size", str(a.batch_size), "--save_dir", "/tmp/iu_bench_unused"])
    utils.setup_seed(args.seed)
    model, _, _, _, marked = utils.setup_model_dataset(args)
    model.to(dev)
    plain = copy.deepcopy(model)
    use_salun_convs(model)
    use_fused_bn(model)
    forget_ds, retain_ds = split_marked(marked.dataset)
    sconv.reset_library_conv_calls()
    runs = []
    for _ in range(a.repeats + 1):  # the first run warms up kernels and the allocator
        r, (v, g0, beta) = phases(model, forget_ds, retain_ds, a.batch_size, dev, True)
        runs.append(r)
    runs = runs[1:]
    best = {k: min(r[k] for r in runs) for k in runs[0]}
    arena = arena_of(model)
    res = {"workload": "wfisher_resnet18", "forget": len(forget_ds), "retain": len(retain_ds),
           "batch_size": a.batch_size, "repeats": a.repeats, "best": best, "runs": runs,
           "library_conv_calls": sconv.library_conv_calls()}
    for masked in (False, True):
        sec, gbs = apply_bandwidth(arena, v, g0, beta, masked)
        res[f"apply_{'masked' if masked else 'unmasked'}"] = {"s": sec, "GB_per_s": gbs, "n": arena.n}
    if a.ref_samples:
        _, sec = literal_reference(plain, retain_ds, v, a.ref_samples, dev)
        # timing only: the retain set's RandomCrop / flip draws differ between the two walks, so their results do not
        # compare here (tests/test_iu_gpu.py pins the values on augmentation-free data)
        res["reference_loop"] = {"samples": min(a.ref_samples, W.WOODFISHER_N + 2), "s": sec}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
