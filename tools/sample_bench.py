"""Sampling throughput of `Diffusion.sample_image` on the full-size CFG-DDPM U-Net (configs/cifar10_sample.yml, random
weights): the tensor-op loop and the fused step kernel (`fused=True`), alternated in ONE process at the config's batch
size for a short `--timesteps`; prints one JSON line with images/s of both (median and range over `--reps`).

    python tools/sample_bench.py [--timesteps 8] [--reps 5] [--batch N] [--sample_type generalized|ddpm_noisy]
    python tools/sample_bench.py --launches      kernel launches per reverse step of both paths, from
                                                 `rocprofv3 --kernel-trace --stats` runs of their own (one child process
                                                 per path and step count; the difference of two step counts divided by
                                                 the difference of the steps leaves out everything that is not a step)
"""
import argparse, csv, glob, json, os, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def runner(a):
    import torch
    from types import SimpleNamespace
    from unlearn_saliency_amd.DDPM.functions import load_config
    from unlearn_saliency_amd.DDPM.runners.diffusion import Diffusion
    cfg = load_config(os.path.join(ROOT, "unlearn_saliency_amd", "DDPM", "configs", "cifar10_sample.yml"))
    args = SimpleNamespace(ckpt_folder=None, synthetic=True, seed=1234, sample_type=a.sample_type, skip_type="uniform",
                           timesteps=a.timesteps, eta=1.0, cond_scale=2.0, library_conv=a.library_conv)
    torch.manual_seed(0)
    r = Diffusion(args, cfg)
    model = r._load_model().eval()
    n = a.batch or cfg.sampling.batch_size
    ids = torch.arange(n, dtype=torch.int64, device=r.device)
    c = (ids % cfg.data.n_classes).contiguous()
    from unlearn_saliency_amd import ops_sampler
    x = ops_sampler.sampler_noise(ids, (cfg.data.channels, cfg.data.image_size, cfg.data.image_size), 1234)
    run = {"loop": lambda: r.sample_image(x, model, c, 2.0),
           "fused": lambda: r.sample_image(x, model, c, 2.0, fused=True, image_ids=ids)}
    return torch, run, n


def bench(a):
    torch, run, n = runner(a)
    with torch.no_grad():
        for k in run:  # warm-up: kernel selection, workspaces
            run[k]()
        torch.cuda.synchronize()
        times = {k: [] for k in run}
        for _ in range(a.reps):
            for k in run:  # alternated: both see the same clocks and temperature
                t0 = time.perf_counter()
                run[k]()
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
    out = {"workload": "ddpm_sample_image", "batch": n, "timesteps": a.timesteps, "sample_type": a.sample_type,
           "reps": a.reps}
    for k, ts in times.items():
        ips = sorted(n / t for t in ts)
        out[k] = {"images_per_s_median": round(statistics.median(ips), 2), "images_per_s_min": round(ips[0], 2),
                  "images_per_s_max": round(ips[-1], 2)}
    out["fused_median_not_below_loop_range"] = out["fused"]["images_per_s_median"] >= out["loop"]["images_per_s_min"]
    print(json.dumps(out))


def worker(a):
    torch, run, _ = runner(a)
    with torch.no_grad():
        run[a.worker]()
    torch.cuda.synchronize()


def launches(a):
    counts = {}
    steps = (a.timesteps, 2 * a.timesteps)
    for path in ("loop", "fused"):
        for t in steps:
            with tempfile.TemporaryDirectory() as d:
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "s", "--",
                       sys.executable, os.path.abspath(__file__), "--worker", path, "--timesteps", str(t),
                       "--batch", str(a.batch or 16), "--sample_type", a.sample_type]
                subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
                files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
                if not files:
                    raise RuntimeError("rocprofv3 wrote no kernel_stats.csv")
                counts[(path, t)] = sum(int(r["Calls"]) for r in csv.DictReader(open(files[0])))
    per = {p: (counts[(p, steps[1])] - counts[(p, steps[0])]) / float(steps[1] - steps[0]) for p in ("loop", "fused")}
    print(json.dumps({"workload": "ddpm_sample_image_launches", "sample_type": a.sample_type,
                      "launches_per_step_loop": per["loop"], "launches_per_step_fused": per["fused"],
                      "launches_removed_per_step": per["loop"] - per["fused"]}))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--timesteps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None, help="default: the config's sampling.batch_size")
    ap.add_argument("--sample_type", default="generalized")
    ap.add_argument("--library_conv", action="store_true")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--worker", choices=["loop", "fused"], default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a)
    elif a.launches:
        launches(a)
    else:
        bench(a)


if __name__ == "__main__":
    main()
