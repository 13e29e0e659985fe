"""Golden vectors for Fisher forgetting (`--unlearn fisher_new`), produced by calling the REFERENCE's own `hessian` and
`get_mean_var` (Classification/unlearn/fisher.py:50-101; imported through the stubs of make_golden.py, build container
only) on the fixture network TinyCNN:

    python tests/golden/make_golden_ff.py

Retain set: 300 samples (tests/ff_ref_cpu.py), i.e. nine batches of 32 and a ragged batch of 12.  Every case runs
twice: as shipped in fp32, and on a `.double()` model with fp64 images (the reference follows the parameters' dtype),
which is the fp64 truth.  Stored per case in ff_<case>.npz, per parameter name: grad2 (grad2_acc after the division
by the batch count), mu and var, for both runs (g2_32_* / mu_32_* / var_32_*, *_64_*), the initial state_dict and the
fp32 run's own relative error against the fp64 run.  Cases (ff_ref_cpu.CASES): the (4500, cifar10, class -1) last-row
override, the same with an explicit class, and a configuration where the override does not apply.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (stubs + reference import; also puts the repo root on sys.path)
sys.path.insert(0, os.path.dirname(HERE))
import ff_ref_cpu as FF  # noqa: E402
from fixtures import TinyCNN, tiny_state  # noqa: E402


class _Typed:
    """A dataset whose images come out in `dtype` (the fp64 run)."""

    def __init__(self, ds, dtype):
        self.ds, self.dtype = ds, dtype

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        x, y = self.ds[i]
        return x.to(self.dtype), y


def run_reference(fmod, args, dtype):
    model = TinyCNN()
    model.load_state_dict(tiny_state(FF.MODEL_SEED))
    model = model.to(dtype)
    for p in model.parameters():
        p.data0 = p.data.clone()
    fmod.hessian(_Typed(FF.retain_dataset(), dtype), model, nn.CrossEntropyLoss(), args)
    out = {}
    for n, p in model.named_parameters():
        mu, var = fmod.get_mean_var(p, args, False)
        out[n] = (p.grad2_acc.detach().clone(), mu.detach().clone(), var.detach().clone())
    return out


def main():
    MG.import_reference_classification()
    fmod = sys.modules["unlearn.fisher"]
    sd = tiny_state(FF.MODEL_SEED)
    for name, *_ in FF.CASES:
        args = FF.case_args(name)
        r32 = run_reference(fmod, args, torch.float32)
        r64 = run_reference(fmod, args, torch.float64)
        g32 = torch.cat([r32[n][0].reshape(-1).double() for n in r32])
        g64 = torch.cat([r64[n][0].reshape(-1) for n in r64])
        rel = float((g32 - g64).norm() / g64.norm())
        arrays = {}
        for n in r32:
            for j, tag in enumerate(("g2", "mu", "var")):
                arrays[f"{tag}_32_{n}"] = r32[n][j].numpy()
                arrays[f"{tag}_64_{n}"] = r64[n][j].numpy()
        np.savez(os.path.join(HERE, f"ff_{name}.npz"), n_retain=FF.N_RETAIN, batch_size=FF.BATCH, alpha=FF.ALPHA,
                 model_seed=FF.MODEL_SEED, num_indexes_to_replace=args.num_indexes_to_replace, dataset=args.dataset,
                 class_to_replace=args.class_to_replace, fp32_rel_err_grad2=rel,
                 **{"sd_" + k: v.numpy() for k, v in sd.items()}, **arrays)
        print(f"ff_{name}: |grad2_64| {float(g64.norm()):.6g}  fp32 rel err {rel:.3g}")


if __name__ == "__main__":
    main()
