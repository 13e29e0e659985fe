"""`bench.py` without `--full` is a plain run: set-up, mask, warm-up, the timed steps, --dump-outputs and the result line.
The secondary figures (timed mask generation, event calibration, CPU baselines, the ddpm / sd / dp_ws1 blocks) are
measured with `--full` only."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_full_is_off_by_default():
    bench = _bench()
    assert bench.parse([]).full is False
    assert bench.parse(["--full"]).full is True


@pytest.mark.gpu
def test_plain_line_has_the_headline_and_no_secondary_figures(tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE",
              "SALUN_FORCE_COLLECTIVES"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=600, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["unit"] == "steps/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["value"] > 0 and out["steps"] == 4 and out["warmup"] == 2
    assert abs(out["ms_per_step"] * out["value"] - 1e3) < 1e-6 * 1e3
    assert out["mask_gen"] is None and out["mask_gen_sec"] is None
    assert out["roofline"]["achieved"] > 0 and out["roofline"]["event_pair_overhead_us"] is None
    assert not {"cpu_baseline", "ddpm", "sd", "dp_ws1"} & set(out)
    assert out["dump_outputs"]["files"] == sorted(os.listdir(tmp_path / "out"))
