"""The Stable-Diffusion first-stage encoder at 512 x 512 on one GPU: K28 per GroupNorm shape, and SD/autoencoder.py's
EncoderPlan (K27 / K28 / attention / posterior) beside the same module on library ops.

  gn       every distinct GroupNorm(32) shape of the v1 encoder at a `--side` image, batch 1 and `--batch`: K28
           (salun_gn_split_forward, GroupNorm + SiLU in two launches), `F.group_norm` + `F.silu` (the library's two ops),
           and salun_gn_forward where it accepts the shape; alternated in ONE process, device events around `--group`
           back-to-back calls, median and range over `--reps`.  `of_hbm_peak` is the algorithmic traffic of the
           two-phase form, 12 B per element (read, read, write), over the median time, as a fraction of 8 TB/s.
  encoder  seconds per image of EncoderPlan.encode_moments and of `model(x)` under torch.no_grad(), batch 1 and
           `--batch`, alternated; and one instrumented pass of the plan with device events around every call, summed by
           kind: the share of K27 (all convolutions), K28 (all GroupNorms) and the attention product.

    python tools/vae_bench.py [--side 512] [--batch 4] [--reps 9] [--group 3] [--out profiles/vae_bench.json]

Weights are seeded random numbers (timing does not depend on them).  Prints one JSON line and writes it to `--out`."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8e12
GN_SHAPES = [(128, 1), (128, 2), (256, 2), (256, 4), (512, 4), (512, 8)]     # (channels, side divisor), G = 32


def _event_times(run, reps, group):
    import torch
    for fn in run.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in run}
    for _ in range(reps):
        for k, fn in run.items():                 # alternated: all see the same clocks and the same neighbours
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(group):
                fn()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e) * 1e-3 / group)
    return {k: sorted(v) for k, v in times.items()}


def _stats(t, scale=1e6, unit="us"):
    return {f"{unit}_median": round(statistics.median(t) * scale, 3), f"{unit}_min": round(t[0] * scale, 3),
            f"{unit}_max": round(t[-1] * scale, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--group", type=int, default=3, help="back-to-back calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_bench.json"))
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("vae_bench needs a ROCm device: a timing taken anywhere else says nothing")
    from unlearn_saliency_amd import conv_infer, norm, ops, ops_infer
    from unlearn_saliency_amd.SD import autoencoder
    from unlearn_saliency_amd.SD.autoencoder import AutoencoderKLLite, EncoderPlan

    torch.manual_seed(0)
    gn = []
    for C, div in GN_SHAPES:
        side = a.side // div
        for N in (1, a.batch):
            x = torch.randn(N, C, side, side, device="cuda")
            g, b = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.1
            y = torch.empty_like(x)
            run = {"k28": lambda: ops_infer.gn_split_forward(x, g, b, 32, 1e-6, True, y),
                   "library": lambda: F.silu(F.group_norm(x, 32, g, b, 1e-6))}
            if ops.gn_forward(x, g, b, 32, 1e-6, True) is not None:
                run["salun_gn_forward"] = lambda: ops.gn_forward(x, g, b, 32, 1e-6, True)
            t = _event_times(run, a.reps, a.group)
            rec = {"shape": [N, C, side, side], "slabs": ops_infer.gn_split_slabs(C, side * side, 32),
                   "workgroups": N * 32 * ops_infer.gn_split_slabs(C, side * side, 32)}
            for k in run:
                med = statistics.median(t[k])
                rec[k] = dict(_stats(t[k]), of_hbm_peak=round(12.0 * x.numel() / med / HBM_PEAK, 3))
            rec["library_over_k28"] = round(statistics.median(t["library"]) / statistics.median(t["k28"]), 3)
            gn.append(rec)
            del x, y

    model = AutoencoderKLLite().cuda()
    plan = EncoderPlan(model)
    enc = []
    for N in (1, a.batch):
        x = torch.rand(N, 3, a.side, a.side, device="cuda") * 2 - 1

        def lib():
            with torch.no_grad():
                return model(x)

        conv_infer.reset_library_infer_calls()
        norm.reset_library_gn_split_calls()
        for k in autoencoder.ATTENTION_ROUTES:
            autoencoder.ATTENTION_ROUTES[k] = 0
        own = plan.encode_moments(x)
        counts = {"LIBRARY_INFER_CALLS": dict(conv_infer.LIBRARY_INFER_CALLS),
                  "LIBRARY_GN_SPLIT_CALLS": dict(norm.LIBRARY_GN_SPLIT_CALLS), "ATTENTION_ROUTES": dict(autoencoder.ATTENTION_ROUTES)}
        ref = lib()
        agree = float((own - ref).abs().max() / ref.abs().max())
        t = _event_times({"plan": lambda: plan.encode_moments(x), "library": lib}, a.reps, 1)

        # one instrumented pass: device events around every call of a kind
        spans = {"k27": [], "k28": [], "attention": []}

        def timed(kind, fn):
            def wrapper(*args, **kw):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                out = fn(*args, **kw)
                e.record()
                spans[kind].append((s, e))
                return out
            return wrapper

        saved = plan._conv, plan._gn, plan._product
        plan._conv, plan._gn, plan._product = timed("k27", saved[0]), timed("k28", saved[1]), timed("attention", saved[2])
        s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0.record()
        plan.encode_moments(x)
        e0.record()
        torch.cuda.synchronize()
        plan._conv, plan._gn, plan._product = saved
        total = s0.elapsed_time(e0)
        parts = {k: sum(s.elapsed_time(e) for s, e in v) for k, v in spans.items()}
        enc.append({"batch": N, "side": a.side,
                    "plan_ms_per_image": round(statistics.median(t["plan"]) * 1e3 / N, 3),
                    "library_ms_per_image": round(statistics.median(t["library"]) * 1e3 / N, 3),
                    "plan": _stats(t["plan"], 1e3, "ms"), "library": _stats(t["library"], 1e3, "ms"),
                    "library_over_plan": round(statistics.median(t["library"]) / statistics.median(t["plan"]), 3),
                    "instrumented_pass_ms": round(total, 3), "calls": {k: len(v) for k, v in spans.items()},
                    "share": {k: round(v / total, 3) for k, v in parts.items()},
                    "max_moment_difference_over_max_moment": agree, **counts})
        del x
    line = json.dumps({"workload": "sd_vae_encoder", "reps": a.reps, "group": a.group, "gn": gn, "encoder": enc})
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
