"""Golden vectors for the pruning baselines, produced by calling the REFERENCE's own functions (imported from
/root/reference through the stubs of make_golden.py; build container only):

    GA_prune_bi  (Classification/unlearn/GA_prune_bi.py:67-160)   2 epochs
    GA_prune     (Classification/unlearn/GA_prune.py:67-209)      pruning_times 2, rewind_lt at epoch 0, 2 epochs each
                 (as shipped it dies in its GA epoch: `utils` names pruner.utils there; recorded, then re-bound)
    FT_prune_bi  (Classification/unlearn/FT_prune_bi.py:9-29)     3 epochs (one round fires) and 4 epochs (two fire)

    python tests/golden/make_golden_prune.py

FT_prune_bi is declared without `mask` while the epoch driver always passes one: through the registry it raises
TypeError (recorded).  Its goldens come from driving the undecorated epoch function — pruner.pruning_model + FT_iter —
with the driver's own optimizer / scheduler construction, the loop the wrapper would run.

Capture condition: at every pruning round the gap between the smallest kept and the largest pruned |w| must be at least
20 x the absolute tolerance of the GPU comparison (1e-4), so that rounding differences between implementations cannot
move a weight across the threshold.  The script re-seeds the initial weights until every round of every run satisfies it
and stores the gaps.  Fixtures are data only.
"""
from __future__ import annotations

import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import prune_ref_cpu as PR  # noqa: E402
from fixtures import tiny_batches  # noqa: E402

GPU_ATOL = 1e-4
MIN_GAP = 20 * GPU_ATOL
LOADERS = {"forget": (2, 700), "retain": (3, 800), "val": (2, 900), "test": (2, 1000)}


_GA_PRUNE: dict = {}


class GapTooSmall(Exception):
    pass


def _args(d, **kw):
    base = dict(lr=0.004, unlearn_lr=0.004, momentum=0.9, weight_decay=5e-4, decreasing_lr="91,136", rewind_epoch=0,
                imagenet_arch=False, epochs=2, unlearn_epochs=3, rate=0.3, random_prune=False, pruning_times=2,
                prune_type="rewind_lt", dataset="cifar10", num_classes=10, warmup=0, print_freq=50, batch_size=16,
                save_dir=d, gpu=0, no_l1_epochs=0, alpha=0.0)
    base.update(kw)
    return SimpleNamespace(**base)


def _loaders():
    return {k: MG._ListLoader(PR.loaders_from(tiny_batches(nb, 16, seed))) for k, (nb, seed) in LOADERS.items()}


def _conv_modules(model):
    return [m for m in model.modules() if isinstance(m, nn.Conv2d)]


def _recording(real, log):
    """Wrap the reference's pruning_model: after it ran, record the compact mask and the threshold gap."""
    def wrapped(model, px):
        before = [getattr(m, "weight_mask", torch.ones_like(m.weight)).clone() for m in _conv_modules(model)]
        mags = torch.cat([m.weight.detach().abs().reshape(-1) for m in _conv_modules(model)])
        real(model, px)
        after = torch.cat([m.weight_mask.reshape(-1) for m in _conv_modules(model)])
        was = torch.cat([b.reshape(-1) for b in before])
        new = (was == 1) & (after == 0)
        gap = float(mags[after == 1].min() - mags[new].max()) if new.any() else float("inf")
        if gap < MIN_GAP:
            raise GapTooSmall(gap)
        log.append((after.numpy().astype(np.uint8), gap))
    return wrapped


def _effective(model):
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    out = {}
    for k, v in sd.items():
        if k.endswith("weight_mask"):
            continue
        if k.endswith("weight_orig"):
            out[k[:-5]] = (v * sd[k[:-4] + "mask"]).numpy()
        else:
            out[k] = v.numpy()
    return out


def _save(tag, init, args, log, accs, model, extra=None):
    keys = ("lr", "unlearn_lr", "momentum", "weight_decay", "decreasing_lr", "rewind_epoch", "epochs", "unlearn_epochs",
            "rate", "pruning_times")
    names = list(LOADERS)
    np.savez(os.path.join(HERE, f"prune_{tag}.npz"), rounds=len(log), gpu_atol=GPU_ATOL,
             gaps=np.array([g for _, g in log]), accs=np.asarray(accs, np.float64),
             loader_names=np.array(names), loader_nb=np.array([LOADERS[n][0] for n in names]),
             loader_seed=np.array([LOADERS[n][1] for n in names]),
             **{f"mask_r{i}": m for i, (m, _) in enumerate(log)},
             **{"arg_" + k: np.array(getattr(args, k)) for k in keys},
             **{"init_" + k: v.numpy() for k, v in init.items()},
             **{"sd_" + k: v for k, v in _effective(model).items()}, **(extra or {}))


def capture(seed, ref_unlearn, write):
    crit = nn.CrossEntropyLoss()
    init = PR.prune_cnn_state(seed)
    fresh = lambda: (lambda m: (m.load_state_dict(init), m)[1])(PR.PruneCNN())
    import pruner as ref_pruner
    out = []
    with tempfile.TemporaryDirectory() as d:
        for tag, modname in (("ga_prune_bi", "unlearn.GA_prune_bi"), ("ga_prune", "unlearn.GA_prune")):
            mod, log = sys.modules[modname], []
            real = mod.pruning_model
            extra = None
            if tag == "ga_prune":
                # GA_prune.py binds `utils` to pruner.utils (its star import of pruner runs last over that name), so its
                # GA epoch dies on utils.AverageMeter: record that, then capture with the name bound to the module meant
                if "died" not in _GA_PRUNE:
                    try:
                        mod.GA_prune(_loaders(), fresh(), crit, _args(d))
                        _GA_PRUNE["died"] = ""
                    except AttributeError as e:
                        _GA_PRUNE["died"] = str(e)
                    assert "AverageMeter" in _GA_PRUNE["died"], _GA_PRUNE["died"]
                    mod.utils = sys.modules["utils"]
                extra = {"reference_error": np.array(_GA_PRUNE["died"])}
            mod.pruning_model = _recording(real, log)
            try:
                model, args = fresh(), _args(d)
                getattr(mod, tag.replace("ga", "GA"))(_loaders(), model, crit, args)
            finally:
                mod.pruning_model = real
            last = torch.load(os.path.join(d, ("1" if tag == "ga_prune" else "0") + "checkpoint.pth.tar"), weights_only=False)
            r = last["result"]
            accs = list(zip(r["train_ta"], r["val_ta"], r["test_ta"]))   # the last state's epochs
            out.append((tag, init, args, log, accs, model, extra))
        raised = None
        try:
            ref_unlearn.FT_prune_bi(_loaders(), fresh(), crit, _args(d), None)
        except TypeError as e:
            raised = str(e)
        assert raised and "positional argument" in raised, raised
        inner = ref_unlearn.FT_prune_bi.__closure__[0].cell_contents
        for E in (3, 4):
            log = []
            real = ref_pruner.pruning_model
            ref_pruner.pruning_model = _recording(real, log)
            try:
                model, a = fresh(), _args(d, unlearn_epochs=E)
                opt = torch.optim.SGD(model.parameters(), a.unlearn_lr, momentum=a.momentum, weight_decay=a.weight_decay)
                sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[91, 136], gamma=0.1)
                accs = []
                for epoch in range(E):
                    accs.append((float(inner(_loaders(), model, crit, opt, epoch, a)),))
                    sched.step()
            finally:
                ref_pruner.pruning_model = real
            out.append((f"ft_prune_bi_e{E}", init, a, log, accs, model, {"reference_registry_error": np.array(raised)}))
    if write:
        for item in out:
            _save(*item[:6], extra=item[6])
    return out


def main():
    _, ref_unlearn = MG.import_reference_classification()
    for seed in range(1000):
        try:
            capture(seed, ref_unlearn, write=False)
        except GapTooSmall:
            continue
        out = capture(seed, ref_unlearn, write=True)
        print("seed", seed, {t: [round(g, 5) for _, g in log] for t, _, _, log, *_ in out})
        return
    raise SystemExit("no seed satisfies the gap condition")


if __name__ == "__main__":
    main()
