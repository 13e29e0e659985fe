"""streams.py: a side stream handed out by `concurrent_stream` really runs beside the current stream (its own hardware
queue), beside the side streams handed out before it, and — in a process with an RCCL process group, where the
communicator's streams used to push the backward-weight side stream onto the compute stream's queue (round 6: every
kernel of the data-parallel step back to back, 10.03 ms against 8.53) — the data-parallel ResNet-18 step stays within a
few per cent of the single-process one (`bench.py --force_collectives`, short windows in subprocesses)."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_SIDE_STREAMS = """
import torch
from unlearn_saliency_amd import streams
dev = torch.device("cuda", torch.cuda.current_device())
main = torch.cuda.current_stream(dev)
a = streams.concurrent_stream(dev)
b = streams.concurrent_stream(dev)
assert a.cuda_stream != b.cuda_stream and a.cuda_stream != main.cuda_stream
buf = torch.empty(32 * 1024 * 1024, dtype=torch.float32, device=dev).zero_()
flag = torch.zeros(1, dtype=torch.float32, device=dev)
assert streams._beside_main(main, a, buf, flag)
if streams.STATS.get("fallbacks", 0) == 0:
    assert streams._beside_main(main, b, buf, flag)
    assert streams._beside_main(a, b, buf, flag)  # the second one was also probed against the first
else:
    # no candidate ran beside both (too few hardware queues for main + two side streams): the probe says so and
    # hands out a stream that shares a queue — which the check must then see
    assert not (streams._beside_main(main, b, buf, flag) and streams._beside_main(a, b, buf, flag))
# what the probe rejects: the stream itself is certainly not concurrent with itself
assert not streams._beside_main(a, a, buf, flag)
print("side streams ok", streams.STATS)
"""


def test_side_streams_get_a_queue_of_their_own():
    """In a fresh process, where a run hands its side streams out: in this one, the streams earlier tests and the
    libraries they loaded created have already decided which hardware queues new streams land on.  The first side stream
    always gets a queue of its own; a second one does only where the runtime provides enough queues, and where it does
    not, the probe must report the fallback (STATS) instead of claiming a queue it did not find."""
    r = subprocess.run([sys.executable, "-c", _SIDE_STREAMS], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "side streams ok" in r.stdout, r.stderr[-3000:]
    print(r.stdout)


def _line(extra, port):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "LOCAL_WORLD_SIZE", "SALUN_FORCE_COLLECTIVES"):
        env.pop(k, None)
    env["MASTER_PORT"] = str(port)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "10",
                        "--no_cpu_baseline", "--no_ddpm", "--no_sd", "--no_dp", "--no_mask_gen"] + extra,
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_data_parallel_step_at_world_size_one_is_not_serialised():
    plain = _line([], 29631)
    dp = _line(["--force_collectives"], 29632)
    assert dp["backend"] == "nccl" and dp["collectives"] is True
    ratio = dp["ms_per_step"] / plain["ms_per_step"]
    # measured 1.02; the serialised state this guards against was 1.17
    assert ratio < 1.08, (plain["ms_per_step"], dp["ms_per_step"])
