"""Golden vectors for the IU / WoodFisher baseline (`--unlearn wfisher`), produced by calling the REFERENCE's own
`unlearn.Wfisher` (Classification/unlearn/Wfisher.py:99-198; imported through the stubs of make_golden.py, build
container only) on the fixture network TinyCNN:

    python tests/golden/make_golden_iu.py

Cases: retain 1,100 samples (the walk returns after 1,002) and retain 300 (the walk runs out), each unmasked and
masked, alpha = 0.2, batch 64, 40 forget samples.  Every case runs twice: as shipped in fp32, and on a `.double()`
model with fp64 images (the reference follows the parameters' dtype), which is the fp64 truth.  Stored per case in
iu_<retain>_<masked|unmasked>.npz: the seeds, v and the perturbation k (captured at the reference's woodfisher call),
the final state_dict, and the fp32 run's own relative error against the fp64 run.  Inputs come from the
counter-based generator (tests/iu_ref_cpu.py); fixtures are data only.
"""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (stubs + reference import; also puts the repo root on sys.path)
import iu_ref_cpu as IU  # noqa: E402
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


def run_reference(ref_unlearn, n_retain, masked, dtype):
    forget, retain = IU.iu_datasets(n_retain)
    model = TinyCNN()
    model.load_state_dict(tiny_state(IU.MODEL_SEED))
    model = model.to(dtype)
    mflat = IU.mask_flat(sum(p.numel() for p in model.parameters()))
    off = np.cumsum([0] + [p.numel() for p in model.parameters()])
    maskd = {n: torch.from_numpy(mflat[off[i]:off[i + 1]]).view_as(p)
             for i, (n, p) in enumerate(model.named_parameters())}
    loaders = {"forget": SimpleNamespace(dataset=_Typed(forget, dtype)),
               "retain": SimpleNamespace(dataset=_Typed(retain, dtype))}
    args = SimpleNamespace(batch_size=IU.BATCH, gpu=0, imagenet_arch=False, alpha=IU.ALPHA)
    wmod = sys.modules["unlearn.Wfisher"]
    real = wmod.woodfisher
    seen = {}

    def spy(model, train_dl, device, criterion, v, args, mask=None):
        seen["v"] = v.detach().clone()
        k = real(model, train_dl, device, criterion, v, args, mask)
        seen["k"] = k.detach().clone()
        return k

    wmod.woodfisher = spy
    try:
        ref_unlearn.Wfisher(loaders, model, nn.CrossEntropyLoss(), args, maskd if masked else None)
    finally:
        wmod.woodfisher = real
    return seen["v"], seen["k"], {k: v.detach().clone() for k, v in model.state_dict().items()}, mflat


def main():
    _, ref_unlearn = MG.import_reference_classification()
    for n_retain in IU.CASES:
        for masked in (False, True):
            v32, k32, sd32, mflat = run_reference(ref_unlearn, n_retain, masked, torch.float32)
            v64, k64, sd64, _ = run_reference(ref_unlearn, n_retain, masked, torch.float64)
            rel = lambda a, b: float((a.double() - b).norm() / b.norm())
            tag = f"iu_{n_retain}_{'masked' if masked else 'unmasked'}"
            np.savez(os.path.join(HERE, tag + ".npz"),
                     n_retain=n_retain, n_forget=IU.N_FORGET, batch_size=IU.BATCH, alpha=IU.ALPHA, N=IU.N_WF,
                     model_seed=IU.MODEL_SEED, mask_seed=IU.MASK_SEED, data_seeds=np.array([1500, 1501, 1502, 1503]),
                     mask=mflat.astype(np.uint8) if masked else np.zeros(0, np.uint8),
                     v32=v32.numpy(), k32=k32.numpy(), v64=v64.numpy(), k64=k64.numpy(),
                     fp32_rel_err_v=rel(v32, v64), fp32_rel_err_k=rel(k32, k64),
                     **{"sd32_" + k: t.numpy() for k, t in sd32.items()},
                     **{"sd64_" + k: t.numpy() for k, t in sd64.items()})
            print(f"{tag}: |k64| {float(k64.norm()):.6g}  fp32 rel err v {rel(v32, v64):.3g} k {rel(k32, k64):.3g}")


if __name__ == "__main__":
    main()
