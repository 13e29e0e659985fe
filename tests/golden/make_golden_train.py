"""Golden vectors for the pre-training epoch, produced by calling the REFERENCE's own `trainer.train` and
`get_optimizer_and_scheduler` (Classification/trainer/train.py:17-133, imported from /root/reference through the stubs of
make_golden.py; build container only):

    python tests/golden/make_golden_train.py

Two epochs on the tiny BN CNN of tests/fixtures.py over three fixed batches of 16, the first epoch inside `--warmup 1`,
MultiStepLR milestones 1,2 stepped after each epoch as main_train.py:116-120 does.  tests/golden/train_epoch.npz holds
the seeds of the inputs, the initial and final state dicts, the final momentum buffers, the learning rate of every
optimizer step, the returned accuracies, the SGD state-dict layout of the run, and the key set of the checkpoint that
the reference's main_train.py writes (read from the dict literal it passes to save_checkpoint).  Data only.
"""
from __future__ import annotations

import ast
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
from fixtures import TinyCNN, tiny_batches, tiny_state  # noqa: E402

STATE_SEED, BATCH_SEED, NB, BS, EPOCHS = 41, 1200, 3, 16, 2
ARGS = dict(lr=0.05, momentum=0.9, weight_decay=5e-4, decreasing_lr="1,2", warmup=1, print_freq=2, imagenet_arch=False,
            alpha=0.0, epochs=EPOCHS)


def checkpoint_keys():
    """The string keys of the dict literal main_train.py hands to save_checkpoint."""
    tree = ast.parse(open(MG.REF + "/Classification/main_train.py").read())
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "id", None) == "save_checkpoint":
            for arg in node.args:
                if isinstance(arg, ast.Dict):
                    return [k.value for k in arg.keys]
    raise RuntimeError("save_checkpoint call not found")


def main():
    MG.import_reference_classification()
    tt = sys.modules["trainer.train"]
    torch.manual_seed(0)
    model = TinyCNN()
    init = tiny_state(STATE_SEED)
    model.load_state_dict(init)
    init = {k: v.clone() for k, v in init.items()}
    args = SimpleNamespace(**ARGS)
    batches = tiny_batches(NB, BS, BATCH_SEED)
    loader = MG._ListLoader([(torch.from_numpy(x), torch.from_numpy(y)) for x, y in batches])
    optimizer, scheduler = tt.get_optimizer_and_scheduler(model, args)
    lrs = []
    real_step = optimizer.step

    def step(*a, **k):
        lrs.append(optimizer.param_groups[0]["lr"])
        return real_step(*a, **k)

    optimizer.step = step
    accs, epoch_lr = [], []
    for epoch in range(EPOCHS):
        epoch_lr.append(optimizer.state_dict()["param_groups"][0]["lr"])
        accs.append(tt.train(loader, model, nn.CrossEntropyLoss(), optimizer, epoch, args))
        scheduler.step()
    osd = optimizer.state_dict()
    names = [n for n, _ in model.named_parameters()]
    out = {"state_seed": STATE_SEED, "batch_seed": BATCH_SEED, "nb": NB, "bs": BS, "epochs": EPOCHS,
           "args": json.dumps(ARGS), "lr_steps": np.asarray(lrs, np.float64), "lr_epoch_start": np.asarray(epoch_lr),
           "lr_after": float(optimizer.param_groups[0]["lr"]), "acc": np.asarray(accs, np.float64),
           "names": np.asarray(names), "checkpoint_keys": np.asarray(checkpoint_keys()),
           "sgd_top_keys": np.asarray(sorted(osd.keys())),
           "sgd_group_keys": np.asarray(sorted(osd["param_groups"][0].keys())),
           "sgd_state_keys": np.asarray(sorted(osd["state"][0].keys())),
           "sgd_state_index": np.asarray(sorted(osd["state"].keys()), np.int64),
           "sgd_group_params": np.asarray(osd["param_groups"][0]["params"], np.int64)}
    for i, (x, y) in enumerate(batches):
        out[f"x{i}"], out[f"y{i}"] = x, y
    for k, v in init.items():
        out["init_" + k] = v.numpy()
    for k, v in model.state_dict().items():
        out["sd_" + k] = v.detach().numpy()
    for i, n in enumerate(names):
        out["mom_" + n] = osd["state"][i]["momentum_buffer"].numpy()
    path = os.path.join(HERE, "train_epoch.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; acc", accs, "lr", lrs)


if __name__ == "__main__":
    main()
