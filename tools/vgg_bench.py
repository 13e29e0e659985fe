"""VGG-16-BN (`--arch vgg16_bn_lth`) on one GPU: the masked RL step, K24 (csrc/salun_pool.hip) beside the library's
pooling, and the thirteen convolutions one by one.

  step    steps/s of the masked random-label step at batch 256 (forward -> cross-entropy on random labels -> zero_grad ->
          backward -> fused masked SGD step) on this package's kernels (MFMA convolutions, fused BN + ReLU, K24) and on
          the same model with plain library modules, alternated in blocks of `--steps` in ONE process; the library
          convolution / pooling calls of one own-kernel step are counted.
  pool    K24 forward and backward at the four pool shapes of the network beside F.max_pool2d and its autograd on the
          same tensors: HIP events around `--group` back-to-back calls, alternated, median and range over `--reps`; the
          bytes each direction has to move (x + y + idx forward, dy + idx + dx backward) over the median time, and that
          rate as a fraction of 8.0 TB/s (the HBM3E peak) and of 6.29 TB/s (a float4 copy on this chip).
  convs   every convolution of the own-kernel model at its batch-256 shape: forward, and backward (data + weight +
          bias) through the module, host clock around `--group` calls ending in a synchronise.

    python tools/vgg_bench.py [--steps 10] [--blocks 5] [--batch 256] [--block-seconds 30] [--reps 21] [--group 20]
                              [--out profiles/vgg_bench.json]

Prints one JSON line and writes it to `--out`."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12     # bytes/s: spec, and what a float4 copy reaches
POOL_SHAPES = ((64, 32), (128, 16), (256, 8), (512, 4))   # (channels, height = width) of the four pool inputs


def build(own):
    import torch
    from unlearn_saliency_amd.Classification.models import model_dict
    from unlearn_saliency_amd.conv import use_salun_convs
    from unlearn_saliency_amd.norm import use_fused_bn
    torch.manual_seed(0)
    model = model_dict["vgg16_bn_lth"](num_classes=10).cuda().train()
    if own:
        use_salun_convs(model), use_fused_bn(model)
    return model


def step_rates(a):
    import torch
    import torch.nn.functional as F
    from unlearn_saliency_amd import conv as sconv
    from unlearn_saliency_amd import pool
    from unlearn_saliency_amd.flat import arena_of
    from unlearn_saliency_amd.optim import FusedMaskedSGD
    x = torch.rand(a.batch, 3, 32, 32, device="cuda")
    y = torch.randint(0, 10, (a.batch,), device="cuda")       # the random labels of an RL step
    runs = {}
    for name, own in (("own", True), ("library", False)):
        model = build(own)
        arena = arena_of(model)
        opt = FusedMaskedSGD(arena, 0.01, momentum=0.9, weight_decay=5e-4)
        opt.set_mask((torch.arange(arena.n, device="cuda") % 2).to(torch.uint8))
        runs[name] = (model, opt)

    def block(name, steps):
        model, opt = runs[name]
        torch.cuda.synchronize()
        t0, done = time.perf_counter(), 0
        for _ in range(steps):
            loss = F.cross_entropy(model(x), y)
            opt.zero_grad()
            loss.backward()
            opt.step()
            done += 1
            if time.perf_counter() - t0 > a.block_seconds:
                break
        torch.cuda.synchronize()
        return done / (time.perf_counter() - t0), done

    for name in runs:                     # warm-up of both paths: code objects, workspaces, library algorithm search
        block(name, 3)
    sconv.reset_library_conv_calls()
    pool.reset_library_pool_calls()
    block("own", 1)
    counts = {"library_conv_calls": dict(sconv.LIBRARY_CONV_CALLS), "LIBRARY_POOL_CALLS": dict(pool.LIBRARY_POOL_CALLS)}
    rates = {n: [] for n in runs}
    short = 0
    for _ in range(a.blocks):
        for name in runs:                 # alternated: both see the same clocks and the same neighbours
            r, done = block(name, a.steps)
            rates[name].append(r)
            short += done < a.steps
    for _, opt in runs.values():
        opt.close()
    fmt = lambda xs: {"steps_per_s_median": round(statistics.median(xs), 3), "steps_per_s_min": round(min(xs), 3),
                      "steps_per_s_max": round(max(xs), 3)}
    out = {"batch": a.batch, "steps_per_block": a.steps, "blocks": a.blocks, "blocks_cut_short": short,
           "own_kernels": fmt(rates["own"]), "library_modules": fmt(rates["library"]), **counts}
    out["own_over_library"] = round(out["own_kernels"]["steps_per_s_median"] /
                                    out["library_modules"]["steps_per_s_median"], 4)
    return out


def _event_times(run, reps, group):
    import torch
    for fn in run.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in run}
    for _ in range(reps):
        for k, fn in run.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(group):
                fn()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e) * 1e-3 / group)
    return {k: sorted(v) for k, v in times.items()}


def pool_times(a):
    import torch
    import torch.nn.functional as F
    from unlearn_saliency_amd import ops
    out = []
    for C, H in POOL_SHAPES:
        x = torch.randn(a.batch, C, H, H, device="cuda")
        y, idx = ops.maxpool2x2_forward(x)
        dy = torch.randn_like(y)
        xl = x.clone().requires_grad_()
        yl = F.max_pool2d(xl, 2, 2)
        run = {"k24_forward": lambda: ops.maxpool2x2_forward(x),
               "library_forward": lambda: F.max_pool2d(x, 2, 2),
               "k24_backward": lambda: ops.maxpool2x2_backward(dy, idx),
               "library_backward": lambda: torch.autograd.grad(yl, xl, dy, retain_graph=True)}
        ts = _event_times(run, a.reps, a.group)
        nbytes = {"k24_forward": x.numel() * 4 + y.numel() * 5, "k24_backward": y.numel() * 5 + x.numel() * 4}
        rec = {"shape": [a.batch, C, H, H], "reps": a.reps, "calls_per_rep": a.group}
        for k, t in ts.items():
            rec[k] = {"us_median": round(statistics.median(t) * 1e6, 2), "us_min": round(t[0] * 1e6, 2),
                      "us_max": round(t[-1] * 1e6, 2)}
            if k in nbytes:
                rate = nbytes[k] / statistics.median(t)
                rec[k].update(bytes=nbytes[k], tb_per_s=round(rate / 1e12, 3), of_hbm_peak=round(rate / HBM_PEAK, 3),
                              of_float4_copy=round(rate / HBM_COPY, 3))
        out.append(rec)
    return out


def conv_times(a):
    import torch
    import torch.nn as nn
    from unlearn_saliency_amd.flat import arena_of
    model = build(True)
    arena_of(model)                        # the gradients land in the flat arena, as in the step
    out, h = [], 32
    for i, m in enumerate(model.features):
        if isinstance(m, nn.MaxPool2d):
            h //= 2
        if not isinstance(m, nn.Conv2d):
            continue
        x = torch.randn(a.batch, m.in_channels, h, h, device="cuda").requires_grad_(i > 0)
        dy = torch.randn(a.batch, m.out_channels, h, h, device="cuda")

        def timed(fn):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.group):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.group

        def fwd():
            with torch.no_grad():
                m(x)

        t_f = timed(fwd)
        t_fb = timed(lambda: m(x).backward(dy))
        flop = 2.0 * a.batch * m.out_channels * m.in_channels * 9 * h * h
        out.append({"layer": f"features.{i}", "shape": [a.batch, m.in_channels, h, h, m.out_channels],
                    "forward_us": round(t_f * 1e6, 1), "backward_us": round((t_fb - t_f) * 1e6, 1),
                    "forward_tflops": round(flop / t_f / 1e12, 2)})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--block-seconds", type=float, default=30.0, help="a block stops early after this long")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--group", type=int, default=20, help="back-to-back calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vgg_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vgg_bench needs a ROCm device: a timing taken anywhere else says nothing")
    line = json.dumps({"workload": "vgg16_bn_lth_masked_rl", "step": step_rates(a), "pool": pool_times(a),
                       "convs": conv_times(a)})
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
