"""Host side of Classification/main_train.py: the reference's command line parses, the checkpoint has the reference's keys
and torch.optim.SGD's state layout (tests/golden/train_epoch.npz records both from the reference), the momentum
conversion flat <-> per-parameter is exact, and the entry point refuses to run without a GPU.  CPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fixtures import TinyCNN, tiny_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "train_epoch.npz"))


def test_parser_accepts_the_reference_command_line():
    """The README command of the reference: python main_train.py --arch resnet18 --dataset cifar10 --lr 0.1
    --epochs 182 --save_dir DIR (plus the resume pair)."""
    from unlearn_saliency_amd.Classification import arg_parser, main_train
    a = arg_parser.parse_args(["--arch", "resnet18", "--dataset", "cifar10", "--lr", "0.1", "--epochs", "182",
                               "--save_dir", "out", "--resume", "--checkpoint", "out/0checkpoint.pth.tar"])
    assert (a.arch, a.dataset, a.lr, a.epochs, a.save_dir, a.resume) == ("resnet18", "cifar10", 0.1, 182, "out", True)
    assert (a.momentum, a.weight_decay, a.decreasing_lr, a.warmup, a.print_freq) == (0.9, 5e-4, "91,136", 0, 50)
    assert callable(main_train.main)


def test_checkpoint_keys_equal_the_references(golden):
    from unlearn_saliency_amd.Classification import main_train
    assert list(main_train.CHECKPOINT_KEYS) == [str(k) for k in golden["checkpoint_keys"]]
    src = open(os.path.join(ROOT, "unlearn_saliency_amd", "Classification", "main_train.py")).read()
    for k in main_train.CHECKPOINT_KEYS:
        assert f'"{k}":' in src, k                                   # the dict main() saves spells the same keys


class _Arena:
    """A CPU stand-in with the arena's layout fields (the conversion functions read nothing else)."""

    def __init__(self, model):
        ps = list(model.named_parameters())
        self.names = [n for n, _ in ps]
        self.shapes = [tuple(p.shape) for _, p in ps]
        self.numels = [p.numel() for _, p in ps]
        self.offsets = list(np.cumsum([0] + self.numels[:-1]))
        self.n = sum(self.numels)

    def new_like(self):
        return torch.zeros(self.n)


def test_momentum_round_trip_is_exact(golden):
    from unlearn_saliency_amd.Classification.trainer.train import momentum_to_flat, momentum_to_per_param
    model = TinyCNN()
    arena = _Arena(model)
    assert arena.names == [str(n) for n in golden["names"]]
    flat = torch.cat([torch.from_numpy(golden["mom_" + n]).reshape(-1) for n in arena.names])
    state = momentum_to_per_param(arena, flat)
    assert sorted(state) == list(golden["sgd_state_index"]) == list(range(len(arena.names)))
    for i, n in enumerate(arena.names):
        assert sorted(state[i]) == [str(k) for k in golden["sgd_state_keys"]]
        assert state[i]["momentum_buffer"].shape == arena.shapes[i]
        assert np.array_equal(state[i]["momentum_buffer"].numpy().view(np.uint32), golden["mom_" + n].view(np.uint32))
    back = momentum_to_flat(arena, state)
    assert torch.equal(back.view(torch.int32), flat.view(torch.int32))
    back = momentum_to_flat(arena, {str(i): v for i, v in state.items()})      # keys as strings (a JSON round trip)
    assert torch.equal(back.view(torch.int32), flat.view(torch.int32))
    # and it loads into torch.optim.SGD, whose own state_dict then has the recorded layout
    sgd = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
    group = dict(sgd.state_dict()["param_groups"][0])
    sgd.load_state_dict({"state": state, "param_groups": [group]})
    sd = sgd.state_dict()
    assert sorted(sd) == [str(k) for k in golden["sgd_top_keys"]]
    assert sorted(sd["param_groups"][0]) == [str(k) for k in golden["sgd_group_keys"] if str(k) != "initial_lr"]
    assert sd["param_groups"][0]["params"] == list(golden["sgd_group_params"])


def test_sgd_state_dict_layout_equals_the_references(golden, monkeypatch):
    """sgd_state_dict on a FusedMaskedSGD-shaped object: the recorded top-level keys, group keys and state keys."""
    from types import SimpleNamespace
    import importlib
    T = importlib.import_module("unlearn_saliency_amd.Classification.trainer.train")   # (the package exports the function)
    model = TinyCNN()
    model.load_state_dict(tiny_state(41))
    arena = _Arena(model)
    flat = torch.arange(arena.n, dtype=torch.float32)
    group = dict(lr=0.005, momentum=0.9, weight_decay=5e-4, initial_lr=0.05, params=list(model.parameters()))
    opt = SimpleNamespace(param_groups=[group], arena=arena, momentum_buffer=flat, steps=6)
    sd = T.sgd_state_dict(opt)
    assert sorted(sd) == [str(k) for k in golden["sgd_top_keys"]]
    assert sorted(sd["param_groups"][0]) == [str(k) for k in golden["sgd_group_keys"]]
    assert sd["param_groups"][0]["params"] == list(golden["sgd_group_params"])
    assert (sd["param_groups"][0]["lr"], sd["param_groups"][0]["initial_lr"]) == (0.005, 0.05)
    assert sorted(sd["state"]) == list(golden["sgd_state_index"])
    assert all(sorted(e) == [str(k) for k in golden["sgd_state_keys"]] for e in sd["state"].values())
    # before the first step torch has no state either
    assert T.sgd_state_dict(SimpleNamespace(param_groups=[group], arena=arena, momentum_buffer=flat, steps=0))["state"] == {}
    # loading it back: buffers land in the flat vector, the next step does not re-create them
    dst = SimpleNamespace(param_groups=[dict(lr=0.1, momentum=0.9, weight_decay=0.0, params=[])], arena=arena,
                          momentum_buffer=torch.zeros(arena.n), steps=0, _first_step=True)
    T.load_sgd_state_dict(dst, sd)
    assert torch.equal(dst.momentum_buffer, flat) and dst._first_step is False and dst.steps >= 1
    assert dst.param_groups[0]["lr"] == 0.005 and dst.param_groups[0]["weight_decay"] == 5e-4
    with pytest.raises(ValueError, match="does not describe this model"):
        T.load_sgd_state_dict(dst, {"state": {}, "param_groups": [dict(group, params=[0, 1])]})


def test_entry_point_refuses_to_run_without_a_gpu(tmp_path):
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the entry point would run")
    r = subprocess.run([sys.executable, "-m", "unlearn_saliency_amd.Classification.main_train", "--synthetic",
                        "--save_dir", str(tmp_path), "--epochs", "1"], cwd=str(tmp_path), capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    assert r.returncode != 0
    assert "needs a ROCm device" in (r.stderr + r.stdout), (r.stderr[-800:], r.stdout[-400:])
