"""Golden values of the reference's VGG-16-BN (Classification/models/VGG_LTH.py: `vgg16_bn_lth`), float64 on the CPU.

    python tests/golden/make_golden_vgg.py

Writes vgg16_bn_lth.json (the reference model's state_dict names and shapes, in order) and vgg16_bn_lth.npz: for the
weights and the batch of tests/vgg_fixture.py, the reference model's float64 logits in train mode and in eval mode and,
in each mode, the float64 gradients of the mean cross-entropy for the tensors of vgg_fixture.GRAD_NAMES (the last
convolution's weight gradient sampled: every 97th element).  In train mode the gradient of a convolution bias ahead of
a BatchNorm is zero in exact arithmetic: `grad_train_features.0.bias` holds the float64 rounding noise of that zero.
Data only; the reference is called, never copied.
Build-container tool: pytest does not collect it.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (the module loader; also puts the repo root and tests/ on sys.path)
import vgg_fixture as VF  # noqa: E402


def decision_margin(model, train):
    """The smallest |BatchNorm output| ahead of a ReLU and the smallest gap between a positive window maximum and its
    runner-up ahead of a MaxPool2d, over the fixture batch in the float64 reference."""
    import torch.nn as nn
    VF.fill_state(model)
    model.train(train)
    h, worst = model.normalize(VF.batch()[0].double()), float("inf")
    with torch.no_grad():
        for mod in model.features:
            if isinstance(mod, nn.ReLU):
                worst = min(worst, float(h.abs().min()))
            if isinstance(mod, nn.MaxPool2d):
                N, C, H, W = h.shape
                s = h.view(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4)
                s = s.sort(dim=1, descending=True).values
                worst = min(worst, float((s[:, 0] - s[:, 1])[s[:, 0] > 0].min()))
            h = mod(h)
    return worst


def main():
    ref = MG._load("ref_vgg_lth", MG.REF + "/Classification/models/VGG_LTH.py")
    torch.manual_seed(0)
    model = ref.vgg16_bn_lth(num_classes=10)
    sd = model.state_dict()
    meta = {"names": list(sd), "shapes": [list(v.shape) for v in sd.values()],
            "param_names": [n for n, _ in model.named_parameters()],
            "modules": [type(m).__name__ for m in model.features],
            "seed": VF.SEED, "batch_seed": VF.BATCH_SEED, "batch": VF.BATCH, "sample_stride": VF.SAMPLE_STRIDE}
    model = model.double()
    margins = {mode: decision_margin(model, mode == "train") for mode in ("eval", "train")}
    assert min(margins.values()) >= VF.DECISION_MARGIN, margins   # (see vgg_fixture.BATCH_SEED)
    meta["decision_margin"] = margins
    out = {}
    for mode in ("eval", "train"):
        logits, grads = VF.run(model, train=mode == "train", want_grads=True)
        out["logits_" + mode] = logits.numpy()
        for n, g in grads.items():
            out[f"grad_{mode}_{n}"] = g.numpy().copy()
    for k, v in out.items():
        assert v.dtype == np.float64 and np.isfinite(v).all(), k
    np.savez_compressed(os.path.join(HERE, "vgg16_bn_lth.npz"), **out)
    with open(os.path.join(HERE, "vgg16_bn_lth.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print({k: v.shape for k, v in out.items()}, float(np.abs(out["logits_train"]).max()))


if __name__ == "__main__":
    main()
