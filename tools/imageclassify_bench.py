"""The ResNet-50 of SD/eval-scripts/imageclassify.py at 224 x 224 on one GPU: K30 (the pointwise convolution) beside K27
and the library, the whole forward beside the library modules, and the command line end to end.

  pointwise  every distinct 1 x 1 / stride-1 shape of the network at batch `--batch`: K30, K27 (both with the folded
           BatchNorm, and the ReLU, in their epilogue) and `F.conv2d` followed by the epilogue as torch ops
           (`* scale + shift`, `relu`), alternated in ONE process, device events around `--group` back-to-back calls,
           median and range over `--reps`.  `k30_wins`: K30's median is below K27's by more than the overlap of the two
           ranges (k30 max < k27 min is the plain case); the plan keeps a shape on K27 where it is false
           (SD/resnet50.POINTWISE_ON_K27).  `count` is how often the shape occurs in the network.
  forward  seconds per batch-`--batch` forward from normalised fp32 images to logits: InferencePlan50.forward as routed,
           the same plan with every pointwise layer on K27, and `model(x)` under torch.no_grad(), alternated.
  end_to_end  seconds for imageclassify.main --synthetic on `--pngs` PNG files of 512 x 512 (decoded with Pillow, resized
           on the device), host clock, the CSV write included; the first run of the process and a second one.

    python tools/imageclassify_bench.py [--batch 64] [--reps 11] [--group 5] [--pngs 500]
                                        [--out profiles/imageclassify_bench.json]

Prints one JSON line and writes it to `--out`."""
import argparse, contextlib, importlib.util, io, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FP32_MATRIX_PEAK = 157.3e12


def cli():
    path = os.path.join(ROOT, "unlearn_saliency_amd", "SD", "eval-scripts", "imageclassify.py")
    spec = importlib.util.spec_from_file_location("sd_cli_imageclassify", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--side", type=int, default=224)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--group", type=int, default=5, help="back-to-back calls per timed window")
    ap.add_argument("--pngs", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imageclassify_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("imageclassify_bench needs a ROCm device: a timing taken anywhere else says nothing")
    from classifier_eval_bench import _event_times, _stats, conv_shapes
    from unlearn_saliency_amd import conv_infer, ops_infer
    from unlearn_saliency_amd.DDPM import pngio
    from unlearn_saliency_amd.SD.resnet50 import InferencePlan50, resnet50, standin_state_dict

    model = resnet50()
    model.load_state_dict(standin_state_dict(0))
    model.eval()
    shapes = conv_shapes(model, a.side)
    torch.manual_seed(0)

    pointwise = []
    for (C, H, W, K, R, stride, pad), count in shapes:
        if R != 1 or stride != 1:
            continue
        xi = torch.randn(a.batch, C, H, W, device="cuda")
        w = torch.randn(K, C, 1, 1, device="cuda") * (2.0 / K) ** 0.5
        scale, shift = torch.rand(K, device="cuda") + 0.5, torch.randn(K, device="cuda") * 0.1
        out = torch.empty(a.batch, K, H, W, device="cuda")
        sv, hv = scale.view(1, -1, 1, 1), shift.view(1, -1, 1, 1)
        run = {"k30": lambda: ops_infer.conv1x1_infer(xi, w, scale, shift, None, True, out),
               "k27": lambda: ops_infer.conv2d_infer(xi, w, scale, shift, None, True, 1, 0, out),
               "library": lambda: F.relu(F.conv2d(xi, w) * sv + hv)}
        same = bool(torch.equal(run["k30"]().clone(), run["k27"]()))
        t = _event_times(run, a.reps, a.group)
        flop = 2.0 * a.batch * K * C * H * W
        rec = {"shape": [a.batch, C, H, W, K], "count": count, "gflop": round(flop / 1e9, 3),
               "k30_route": ops_infer.conv1x1_infer_route(a.batch, C, H * W, K),
               "k27_route": ops_infer.conv2d_infer_route(a.batch, C, H, W, K, 1, 1, 0, H, W), "k30_equals_k27_bits": same}
        for k in run:
            med = statistics.median(t[k])
            rec[k] = dict(_stats(t[k], 1e6, "us"), tflops=round(flop / med / 1e12, 2),
                          of_fp32_matrix_peak=round(flop / med / FP32_MATRIX_PEAK, 3))
        m30, m27 = statistics.median(t["k30"]), statistics.median(t["k27"])
        overlap = max(0.0, min(t["k30"][-1], t["k27"][-1]) - max(t["k30"][0], t["k27"][0]))
        rec["k27_over_k30"] = round(m27 / m30, 3)
        rec["library_over_k30"] = round(statistics.median(t["library"]) / m30, 3)
        rec["k30_wins"] = bool(m27 - m30 > overlap)
        pointwise.append(rec)
        del xi, w, out

    plan, plan27 = InferencePlan50(model, "cuda"), InferencePlan50(model, "cuda", pointwise="k27")
    lib = model.cuda()
    x = torch.randn(a.batch, 3, a.side, a.side, device="cuda")

    def lib_forward():
        with torch.no_grad():
            return lib(x)

    conv_infer.reset_library_infer_calls()
    own, _ = plan.forward(x)
    counts, calls = dict(conv_infer.LIBRARY_INFER_CALLS), dict(plan.kernel_calls)
    ref = lib_forward()
    agree = float((own - ref).abs().max() / ref.abs().max())
    ts = _event_times({"own": lambda: plan.forward(x), "own_all_k27": lambda: plan27.forward(x), "library": lib_forward},
                      a.reps, a.group)
    forward = {"batch": a.batch, "side": a.side, "reps": a.reps, "forwards_per_rep": a.group, "convolutions_by_kernel": calls,
               "own_kernels": _stats(ts["own"]), "own_kernels_pointwise_on_k27": _stats(ts["own_all_k27"]),
               "library_modules": _stats(ts["library"]),
               "library_over_own": round(statistics.median(ts["library"]) / statistics.median(ts["own"]), 4),
               "all_k27_over_own": round(statistics.median(ts["own_all_k27"]) / statistics.median(ts["own"]), 4),
               "LIBRARY_INFER_CALLS": counts, "max_logit_difference_over_max_logit": agree}
    del lib, plan27

    e2e = {}
    m = cli()
    with tempfile.TemporaryDirectory() as d:
        folder = os.path.join(d, "run")
        os.makedirs(folder)
        r = np.random.default_rng(0)
        for i in range(a.pngs):
            pngio.write_png(os.path.join(folder, f"{i % 50}_{i // 50}.png"), r.integers(0, 256, (512, 512, 3)).astype(np.uint8), 1)
        with open(os.path.join(d, "prompts.csv"), "w") as f:
            f.write("case_number,prompt,evaluation_seed\n" + "".join(f"{i},prompt {i},{i}\n" for i in range(50)))
        argv = ["--folder_path", folder, "--prompts_path", os.path.join(d, "prompts.csv"), "--synthetic",
                "--batch_size", str(a.batch)]
        for tag in ("first_run_s", "second_run_s"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                m.main(argv)
            torch.cuda.synchronize()
            e2e[tag] = round(time.perf_counter() - t0, 3)
    e2e["pngs"], e2e["png_side"] = a.pngs, 512
    line = json.dumps({"workload": "resnet50_imageclassify", "pointwise": pointwise, "forward": forward, "end_to_end": e2e})
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
