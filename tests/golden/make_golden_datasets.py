"""Golden vectors for the CIFAR-100 / SVHN loaders and for RL's merged branch, captured from the REFERENCE's own
functions (build container only; nothing here is copied from the reference, it is only *called*).

    python tests/golden/make_golden_datasets.py

datasets_splits.npz   the reference's `cifar100_dataloaders` / `svhn_dataloaders` on the small index-coded sets of
                      tests/datasets_fixture.py (torchvision's CIFAR100 / SVHN classes stubbed: the only thing stubbed
                      is where the arrays come from).  Per dataset and seed: validation indices, training indices in the
                      reference's order, and per marked call the training label vector and the test-set length.
rl_merged.npz         the reference's `RL` with dataset="cifar100" on 41 forget + 90 retain samples, 2 epochs, batch
                      32, with and without a mask (keys `masked_*` / `unmasked_*`): the labels it drew per epoch,
                      the labels of every step's batch, the trained state_dict.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (import shims for the reference)
import datasets_fixture as dfx  # noqa: E402


def make_splits(ref_dataset):
    out = {}
    for name in ("cifar100", "svhn"):
        source = dfx.split_source(name)

        class StubCIFAR100:
            def __init__(self, root, train=True, transform=None, download=False):
                x, y = source[0 if train else 1]
                self.data, self.targets, self.transform = x.copy(), list(y), transform

            def __len__(self):
                return len(self.data)

        class StubSVHN:
            def __init__(self, root, split="train", transform=None, download=False):
                x, y = source[0 if split == "train" else 1]
                self.data, self.labels, self.transform = x.copy(), y.copy(), transform

            def __len__(self):
                return len(self.data)

        ref_dataset.CIFAR100, ref_dataset.SVHN = StubCIFAR100, StubSVHN
        loaders = getattr(ref_dataset, name + "_dataloaders")
        labels_of = lambda ds: np.asarray(ds.targets if hasattr(ds, "targets") else ds.labels)
        for seed in dfx.SPLIT_SEEDS:
            train, val, test = loaders(batch_size=16, seed=seed)
            key = f"{name}_s{seed}_"
            out[key + "valid_idx"] = dfx.image_index(val.dataset.data).astype(np.int32)
            out[key + "train_idx"] = dfx.image_index(train.dataset.data).astype(np.int32)
            out[key + "test_len"] = np.int64(len(test.dataset))
            for tag, kw in dfx.split_cases(name):
                train, val, test = loaders(batch_size=16, seed=seed, only_mark=True, **kw)
                out[key + tag + "_train_targets"] = labels_of(train.dataset).astype(np.int16)
                out[key + tag + "_test_len"] = np.int64(len(test.dataset))
                out[key + tag + "_test_targets"] = labels_of(test.dataset).astype(np.int16)
    np.savez_compressed(os.path.join(HERE, "datasets_splits.npz"), **out)
    print("datasets_splits.npz:", len(out), "arrays")


def make_rl_merged(ref_unlearn):
    from torch.utils.data import DataLoader
    out = {}
    for tag, use_mask in (("masked", True), ("unmasked", False)):
        model = dfx.rl_model()
        init = {k: v.clone() for k, v in model.state_dict().items()}
        fds, rds = dfx.rl_merged_datasets()
        forget, retain = DataLoader(fds, dfx.RL_BATCH, shuffle=True), DataLoader(rds, dfx.RL_BATCH, shuffle=True)
        sizes = [p.numel() for p in model.parameters()]
        mflat = dfx.rl_mask_flat(sum(sizes))
        off = np.cumsum([0] + sizes)
        maskd = {n: torch.from_numpy(mflat[off[i]:off[i + 1]]).view_as(p)
                 for i, (n, p) in enumerate(model.named_parameters())} if use_mask else None
        drawn, seen = [], []
        real_randint = np.random.randint

        def rec_randint(*a, **k):
            v = real_randint(*a, **k)
            drawn.append(np.asarray(v).copy())
            return v

        ce = nn.CrossEntropyLoss()

        def criterion(out, tgt):
            seen.append(tgt.detach().numpy().copy())
            return ce(out, tgt)

        np.random.seed(dfx.RL_NUMPY_SEED)
        torch.manual_seed(dfx.RL_TORCH_SEED)
        np.random.randint = rec_randint
        try:
            ref_unlearn.RL({"forget": forget, "retain": retain}, model, criterion, dfx.rl_args(), maskd)
        finally:
            np.random.randint = real_randint
        assert len(drawn) == dfx.RL_EPOCHS and len(seen) == dfx.RL_EPOCHS * 5
        out.update({f"{tag}_drawn": np.stack(drawn), f"{tag}_step_targets": np.concatenate(seen),
                    f"{tag}_step_sizes": np.array([len(s) for s in seen])})
        out.update({f"{tag}_sd_{k}": v.numpy() for k, v in model.state_dict().items()})
    out.update({"init_" + k: v.numpy() for k, v in init.items()})
    np.savez_compressed(os.path.join(HERE, "rl_merged.npz"), **out)
    print("rl_merged.npz written")


if __name__ == "__main__":
    _, ref_unlearn = mg.import_reference_classification()
    make_splits(sys.modules["dataset"])
    make_rl_merged(ref_unlearn)
