"""The ResNet-34 of DDPM/classifier_evaluation.py at 224 x 224 on one GPU: this package's InferencePlan (K26 resize,
normalise, K27 convolutions, 3 x 3 pool, evaluation head) beside the same module on library modules.

  forward  seconds per batch-`--batch` forward from normalised fp32 images to logits: InferencePlan.forward and
           `model(x)` under torch.no_grad(), alternated in ONE process, device events around `--group` back-to-back
           forwards, median and range over `--reps`; the library calls of one plan forward are counted
           (LIBRARY_INFER_CALLS).
  convs    every distinct convolution shape of the network at that batch: K27 (with the folded-BatchNorm epilogue and
           ReLU it carries in the network) and F.conv2d alone (the library's convolution WITHOUT the BatchNorm and ReLU
           kernels that follow it in the library model), alternated, events around `--group` calls; time, and TFLOP/s
           from 2 N K C R R P Q over the median time, and that rate as a fraction of 157.3 TFLOP/s (the fp32 matrix
           peak).  `count` is how often the shape occurs in the network.
  end_to_end  seconds for classifier_evaluation.main on `--pngs` PNG files of 32 x 32 (read with PIL, uploaded once,
           resized on the device, batch `--batch`), host clock, the CSV write included; the first run of the process
           and a second one (code objects and buffers warm).

    python tools/classifier_eval_bench.py [--batch 64] [--reps 11] [--group 5] [--pngs 500]
                                          [--out profiles/classifier_eval_bench.json]

Prints one JSON line and writes it to `--out`."""
import argparse, contextlib, io, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_MATRIX_PEAK = 157.3e12


def _event_times(run, reps, group):
    import torch
    for fn in run.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in run}
    for _ in range(reps):
        for k, fn in run.items():                 # alternated: both see the same clocks and the same neighbours
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(group):
                fn()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e) * 1e-3 / group)
    return {k: sorted(v) for k, v in times.items()}


def _stats(t, scale=1e3, unit="ms"):
    return {f"{unit}_median": round(statistics.median(t) * scale, 4), f"{unit}_min": round(t[0] * scale, 4),
            f"{unit}_max": round(t[-1] * scale, 4)}


def conv_shapes(model, side):
    """[(N-free shape (C, H, W, K, R, stride, pad), count)] of the network's convolutions, in network order."""
    import torch
    import torch.nn as nn
    seen, order = {}, []
    hooks = []

    def hook(m, inp, out):
        x = inp[0]
        key = (m.in_channels, x.shape[2], x.shape[3], m.out_channels, m.kernel_size[0], m.stride[0], m.padding[0])
        if key not in seen:
            order.append(key)
        seen[key] = seen.get(key, 0) + 1

    for m in model.modules():
        if isinstance(m, nn.Conv2d):
            hooks.append(m.register_forward_hook(hook))
    with torch.no_grad():
        model(torch.zeros(1, 3, side, side))
    for h in hooks:
        h.remove()
    return [(k, seen[k]) for k in order]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--side", type=int, default=224)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--group", type=int, default=5, help="back-to-back calls per timed window")
    ap.add_argument("--pngs", type=int, default=500)
    ap.add_argument("--tile-sweep", action="store_true", help="also time K27 with each tile forced, per shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classifier_eval_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("classifier_eval_bench needs a ROCm device: a timing taken anywhere else says nothing")
    from unlearn_saliency_amd import conv_infer, ops_infer
    from unlearn_saliency_amd.DDPM import classifier_evaluation as ce
    from unlearn_saliency_amd.DDPM import pngio
    from unlearn_saliency_amd.DDPM.models.resnet34 import InferencePlan, resnet34, standin_state_dict

    model = resnet34(10)
    model.load_state_dict(standin_state_dict(0))
    model.eval()
    shapes = conv_shapes(model, a.side)
    plan = InferencePlan(model, "cuda", a.side)
    lib = model.cuda()
    torch.manual_seed(0)
    x = torch.randn(a.batch, 3, a.side, a.side, device="cuda")

    def lib_forward():
        with torch.no_grad():
            return lib(x)

    conv_infer.reset_library_infer_calls()
    own, _ = plan.forward(x)
    counts = dict(conv_infer.LIBRARY_INFER_CALLS)
    ref = lib_forward()
    agree = float((own - ref).abs().max() / ref.abs().max())
    ts = _event_times({"own": lambda: plan.forward(x), "library": lib_forward}, a.reps, a.group)
    forward = {"batch": a.batch, "side": a.side, "reps": a.reps, "forwards_per_rep": a.group,
               "own_kernels": _stats(ts["own"]), "library_modules": _stats(ts["library"]),
               "library_over_own": round(statistics.median(ts["library"]) / statistics.median(ts["own"]), 4),
               "LIBRARY_INFER_CALLS": counts, "max_logit_difference_over_max_logit": agree}

    convs = []
    for (C, H, W, K, R, stride, pad), count in shapes:
        xi = torch.randn(a.batch, C, H, W, device="cuda")
        w = torch.randn(K, C, R, R, device="cuda") * (2.0 / (K * R * R)) ** 0.5
        scale, shift = torch.rand(K, device="cuda") + 0.5, torch.randn(K, device="cuda") * 0.1
        P, Q = ops_infer.conv_out_size(H, R, stride, pad), ops_infer.conv_out_size(W, R, stride, pad)
        out = torch.empty(a.batch, K, P, Q, device="cuda")
        run = {"k27": lambda: ops_infer.conv2d_infer(xi, w, scale, shift, None, True, stride, pad, out),
               "library": lambda: F.conv2d(xi, w, None, stride, pad)}
        forced = {name: (lambda tile=tile: ops_infer.conv2d_infer(xi, w, scale, shift, None, True, stride, pad, out, tile))
                  for tile, name in ((1, "64x64"), (2, "128x64"), (3, "128x128"))} if a.tile_sweep else {}
        t = _event_times({**run, **forced}, a.reps, a.group)
        flop = 2.0 * a.batch * K * C * R * R * P * Q
        rec = {"shape": [a.batch, C, H, W, K, R, stride, pad], "count": count, "gflop": round(flop / 1e9, 3),
               "route": ops_infer.conv2d_infer_route(a.batch, C, H, W, K, R, stride, pad, P, Q)}
        for k in run:
            med = statistics.median(t[k])
            rec[k] = dict(_stats(t[k], 1e6, "us"), tflops=round(flop / med / 1e12, 2),
                          of_fp32_matrix_peak=round(flop / med / FP32_MATRIX_PEAK, 3))
        rec["library_over_k27"] = round(statistics.median(t["library"]) / statistics.median(t["k27"]), 3)
        if forced:       # every tile forced: what the plan's choice (`route`) is measured against
            rec["forced_tile_us_median"] = {k: round(statistics.median(t[k]) * 1e6, 2) for k in forced}
        convs.append(rec)
    del lib

    e2e = {}
    with tempfile.TemporaryDirectory() as d:
        folder = os.path.join(d, "run", "cfg", "class_samples", "0")
        os.makedirs(folder)
        r = np.random.default_rng(0)
        for i in range(a.pngs):
            pngio.write_png(os.path.join(folder, f"{i}.png"), r.integers(0, 256, (32, 32, 3)).astype(np.uint8))
        argv = ["--sample_path", folder, "--dataset", "cifar10", "--synthetic", "-b", str(a.batch), "--entropy_zero_safe",
                "--result_csv", os.path.join(d, "result.csv")]
        for tag in ("first_run_s", "second_run_s"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):      # (its three report lines are not this tool's output)
                ce.main(argv)
            torch.cuda.synchronize()
            e2e[tag] = round(time.perf_counter() - t0, 3)
    e2e["pngs"] = a.pngs
    line = json.dumps({"workload": "resnet34_classifier_evaluation", "forward": forward, "convs": convs, "end_to_end": e2e})
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
