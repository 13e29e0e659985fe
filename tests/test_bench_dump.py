"""`bench.py --dump-outputs DIR`: what the timed path leaves its caller, written as float32 / float64 .npy files.

CPU-side: dump_outputs() on a small flat-arena model, and the argument checks that run before any device work."""
import os
import subprocess
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_writes_float_arrays_of_the_last_step(tmp_path):
    bench = _bench()
    from unlearn_saliency_amd.flat import arena_of
    torch.manual_seed(0)
    model = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.Flatten(), nn.Linear(4 * 6 * 6, 10))
    arena = arena_of(model, torch.device("cpu"))
    opt = types.SimpleNamespace(momentum_buffer=torch.arange(arena.n, dtype=torch.float32))
    logits = model(torch.rand(2, 3, 8, 8))
    loss = nn.functional.cross_entropy(logits, torch.tensor([1, 2]))
    info = bench.dump_outputs(str(tmp_path / "out"), model, arena, opt, [logits, loss])
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == info["files"] == ["bn_running_stats.npy", "logits.npy", "loss.npy", "momentum_sample.npy",
                                      "params.npy"]
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in files}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert np.array_equal(got["params"], arena.params.numpy())
    assert np.array_equal(got["logits"], logits.detach().numpy())
    assert got["loss"][0] == float(loss.detach())
    assert got["bn_running_stats"].size == 8  # running mean + var of 4 channels
    # the sample is the whole (small) vector in index order, since the sample size exceeds it
    assert np.array_equal(got["momentum_sample"], np.arange(arena.n, dtype=np.float32))
    assert info["bytes"] == sum(v.nbytes for v in got.values()) <= bench.DUMP_MAX_BYTES


def test_full_size_dump_fits_the_budget():
    bench = _bench()
    bn_floats = 9606  # ResNet-18: running mean + var of its BatchNorm layers
    total = 4 * bench.N18 + 4 * bench.DUMP_MOMENTUM_SAMPLE + 4 * 256 * 10 + 8 + 4 * bn_floats
    assert total <= bench.DUMP_MAX_BYTES


def _run(args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          timeout=300, cwd=ROOT)


def test_steps_below_one_are_refused():
    r = _run(["--gpus", "1", "--steps", "0", "--warmup", "0"])
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr + r.stdout


def test_dump_outputs_is_refused_for_other_workloads(tmp_path):
    r = _run(["--gpus", "1", "--workload", "ddpm", "--dump-outputs", str(tmp_path)])
    assert r.returncode != 0 and "resnet18 workload only" in r.stderr + r.stdout
