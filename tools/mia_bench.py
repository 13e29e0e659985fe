"""SVC_MIA on the host (sklearn) and on the device (K25, csrc/salun_svc.hip) at the benchmark's sizes, on one GPU.

  10,000 shadow-train + 10,000 shadow-test images, 4,500 target images (the forget set of the flagship run), ResNet-18
  on the HIP path, batch 256, the five features of Classification/evaluation/svc_mia.py.  The images are the
  counter-based synthetic CIFAR-shaped set with the non-member populations darkened (x `--shade`).  The network is
  untrained: `correctness`, `m_entropy` and `prob` separate the populations, `confidence` and `entropy` do not, and
  there every alpha ends at C — the longest kind of SMO run, and one that leaves the threshold rho undetermined, so the
  two backends may report different accuracies for those two features.  Both are printed.

  Both backends run in ONE process, alternated `--reps` times after one untimed device call; each call is timed with a
  host clock around device-synchronised work.  The device path also reports its stages (collect, gram, fit, decision:
  synchronised around each, summed over the five features) and the SMO updates per feature.  A machine without sklearn
  times the device path alone and says so.

    python tools/mia_bench.py [--reps 2] [--shadow 10000] [--target 4500] [--shade 0.5] [--out profiles/mia_bench.json]

Prints one JSON line and writes it to `--out`."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--shadow", type=int, default=10_000, help="points per shadow class")
    ap.add_argument("--target", type=int, default=4_500)
    ap.add_argument("--shade", type=float, default=0.5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mia_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mia_bench needs a ROCm device: a timing taken anywhere else says nothing")
    from unlearn_saliency_amd import rng as salun_rng
    from unlearn_saliency_amd.Classification.dataset import ArrayDataset, BatchLoader
    from unlearn_saliency_amd.Classification.evaluation import SVC_MIA
    from unlearn_saliency_amd.Classification.models.resnet_cifar import resnet18
    from unlearn_saliency_amd.conv import use_salun_convs
    from unlearn_saliency_amd.norm import use_fused_bn
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = resnet18(num_classes=10).to(dev)
    use_salun_convs(model), use_fused_bn(model)

    def images(n, seed, shade):
        x = salun_rng.u8(n * 3072, seed).reshape(n, 32, 32, 3)
        if shade != 1.0:
            x = (x.astype(np.float32) * shade).astype(np.uint8)
        return ArrayDataset(x, (np.arange(n) % 10).astype(np.int64))

    sets = dict(shadow_train=images(a.shadow, 71, 1.0), shadow_test=images(a.shadow, 72, a.shade),
                target_test=images(a.target, 73, a.shade))

    def run(backend, stages=None):
        resident = backend == "device"
        ld = {k: BatchLoader(d, a.batch, False, device_resident=resident, device=dev) for k, d in sets.items()}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = SVC_MIA(shadow_train=ld["shadow_train"], shadow_test=ld["shadow_test"], target_train=None,
                    target_test=ld["target_test"], model=model, backend=backend, stages=stages)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, m

    try:
        import sklearn
        backends, note = ("device", "sklearn"), f"sklearn {sklearn.__version__}"
    except ImportError:
        backends, note = ("device",), "sklearn is not installed on this machine: device path only"
    run("device")  # untimed: code objects, allocator, clocks
    times = {b: [] for b in backends}
    results, stage_runs = {}, []
    for _ in range(a.reps):
        for b in backends:  # alternated: both see the same clocks and the same neighbours
            stages = {} if b == "device" else None
            t, results[b] = run(b, stages)
            times[b].append(t)
            print(f"{b}: {t:.3f} s", file=sys.stderr, flush=True)
            if stages is not None:
                stage_runs.append(stages)
    fmt = lambda ts: {"s_median": round(statistics.median(ts), 4), "s_min": round(min(ts), 4), "s_max": round(max(ts), 4)}
    out = {"workload": "svc_mia", "shadow_per_class": a.shadow, "target": a.target, "batch": a.batch, "shade": a.shade,
           "reps": a.reps, "host_library": note, "gpu": torch.cuda.get_device_name(0)}
    for b in backends:
        out[b] = dict(fmt(times[b]), accuracies={k: round(float(v), 6) for k, v in results[b].items()})
    out["device"]["stages_s_median"] = {k: round(statistics.median(s[k] for s in stage_runs), 4)
                                        for k in ("collect", "gram", "fit", "decision")}
    out["device"]["smo_updates_per_feature"] = stage_runs[-1]["iterations"]
    if "sklearn" in out:
        out["sklearn_over_device"] = round(out["sklearn"]["s_median"] / out["device"]["s_median"], 2)
        out["max_accuracy_difference"] = round(max(abs(results["device"][k] - results["sklearn"][k])
                                                   for k in results["device"]), 6)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
