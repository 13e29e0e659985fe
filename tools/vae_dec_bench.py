"""The Stable-Diffusion first-stage decoder at 512 x 512 on one GPU: the Upsample layers on K27's nearest-2x form, the
whole DecoderPlan beside the same module on library ops, conv_out's share, and the LMS step.

  upsample  the three Upsample shapes of a 512 x 512 decode (512 ch 64 -> 128, 512 ch 128 -> 256, 256 ch 256 -> 512),
            batch 1, three ways: (a) fused = conv_infer.conv_up2_bn_act (one launch, nothing materialised),
            (b) F.interpolate + K27 (conv_infer.conv_bn_act), (c) F.interpolate + the library convolution; alternated
            in ONE process, device events around `--group` back-to-back calls, median and range over `--reps`.
  decoder   seconds per image of DecoderPlan.decode_u8 and of DecoderKLLite.forward under torch.no_grad(), batch 1 and
            `--batch`, alternated.
  conv_out  the final convolution (128 -> 3, stored as 32 channels of which 29 are zero) alone, and its share of the
            plan's time at batch 1.
  lms       one LMS step at [4, 4, 64, 64], guided, order 4: salun_lms_step beside the torch expression.

    python tools/vae_dec_bench.py [--side 512] [--batch 4] [--reps 7] [--group 3] [--out profiles/vae_dec_bench.json]

Weights are seeded random numbers (timing does not depend on them).  Prints one JSON line and writes it to `--out`."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

UP_SHAPES = [(512, 8), (512, 4), (256, 2)]        # (channels, divisor of the image side for the STORED map)


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--group", type=int, default=3, help="back-to-back calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_dec_bench.json"))
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("vae_dec_bench needs a ROCm device: a timing taken anywhere else says nothing")
    from unlearn_saliency_amd import conv_infer, norm, ops_infer, ops_sampler
    from unlearn_saliency_amd.SD import autoencoder
    from unlearn_saliency_amd.SD.autoencoder import DecoderKLLite, DecoderPlan

    torch.manual_seed(0)
    ups = []
    for C, div in UP_SHAPES:
        side = a.side // div
        x = torch.randn(1, C, side, side, device="cuda")
        w = torch.randn(C, C, 3, 3, device="cuda") / (3.0 * C ** 0.5)
        b = torch.randn(C, device="cuda") * 0.1
        y = torch.empty(1, C, 2 * side, 2 * side, device="cuda")
        up = lambda: F.interpolate(x, scale_factor=2.0, mode="nearest")
        run = {"fused": lambda: conv_infer.conv_up2_bn_act(x, w, None, b, out=y),
               "interpolate_k27": lambda: conv_infer.conv_bn_act(up(), w, None, b, pad=1, out=y),
               "interpolate_library": lambda: F.conv2d(up(), w, b, 1, 1),
               "interpolate_alone": up}
        same = torch.equal(conv_infer.conv_up2_bn_act(x, w, None, b), conv_infer.conv_bn_act(up(), w, None, b, pad=1))
        t = _event_times(run, a.reps, a.group)
        flop = 2.0 * C * C * 9 * (2 * side) ** 2
        rec = {"stored": [1, C, side, side], "route": ops_infer.conv2d_infer_up2_route(1, C, side, side, C),
               "bits_equal_materialised": same, "materialised_mb": round(C * (2 * side) ** 2 * 4 / 1e6, 1)}
        for k in run:
            rec[k] = _stats(t[k])
            if k != "interpolate_alone":
                rec[k]["tflops"] = round(flop / statistics.median(t[k]) / 1e12, 1)
        rec["interpolate_k27_over_fused"] = round(statistics.median(t["interpolate_k27"]) / statistics.median(t["fused"]), 3)
        rec["interpolate_library_over_fused"] = round(statistics.median(t["interpolate_library"]) /
                                                      statistics.median(t["fused"]), 3)
        ups.append(rec)
        del x, w, y

    model = DecoderKLLite().cuda()
    plan = DecoderPlan(model)
    dec = []
    for N in (1, a.batch):
        z = torch.randn(N, 4, a.side // 8, a.side // 8, device="cuda")

        def lib():
            with torch.no_grad():
                return model(z * (1.0 / autoencoder.SCALE_FACTOR))

        conv_infer.reset_library_infer_calls()
        norm.reset_library_gn_split_calls()
        for k in autoencoder.ATTENTION_ROUTES:
            autoencoder.ATTENTION_ROUTES[k] = 0
        own = plan.decode(z)
        counts = {"LIBRARY_INFER_CALLS": dict(conv_infer.LIBRARY_INFER_CALLS),
                  "LIBRARY_GN_SPLIT_CALLS": dict(norm.LIBRARY_GN_SPLIT_CALLS),
                  "ATTENTION_ROUTES": dict(autoencoder.ATTENTION_ROUTES)}
        ref = lib()
        agree = float((own - ref).abs().max() / ref.abs().max())
        del own, ref
        t = _event_times({"plan": lambda: plan.decode_u8(z), "library": lib}, a.reps, 1)
        rec = {"batch": N, "side": a.side, "plan_ms_per_image": round(statistics.median(t["plan"]) * 1e3 / N, 3),
               "library_ms_per_image": round(statistics.median(t["library"]) * 1e3 / N, 3),
               "plan": _stats(t["plan"], 1e3, "ms"), "library": _stats(t["library"], 1e3, "ms"),
               "library_over_plan": round(statistics.median(t["library"]) / statistics.median(t["plan"]), 3),
               "max_pixel_difference_over_max_pixel": agree, **counts}
        if N == 1:
            co = model.decoder.conv_out
            h = torch.randn(1, co.in_channels, a.side, a.side, device="cuda")
            tc = _event_times({"conv_out": lambda: plan._conv(co, h)}, a.reps, a.group)
            rec["conv_out"] = dict(_stats(tc["conv_out"]), stored_channels=32, real_channels=co.out_channels,
                                   share_of_plan=round(statistics.median(tc["conv_out"]) / statistics.median(t["plan"]), 4))
            del h
        dec.append(rec)
        del z

    B, shape = 4, (4, 64, 64)
    x = torch.randn((B,) + shape, device="cuda")
    eps = torch.randn((2 * B,) + shape, device="cuda")
    hist = torch.randn((4, B) + shape, device="cuda")
    x_in, out = torch.empty_like(eps), torch.empty_like(x)
    c, den, s = [0.31, -0.22, 0.11, -0.04], 1.7, 7.5
    dent = torch.full((1,), den, device="cuda")

    def torch_step():
        d = eps[:B] + s * (eps[B:] - eps[:B])
        hist[0].copy_(d)
        v = x + c[0] * d + c[1] * hist[3] + c[2] * hist[2] + c[3] * hist[1]
        return v, torch.cat([v / dent] * 2)

    t = _event_times({"fused": lambda: ops_sampler.lms_step(x, eps, s, hist, 0, c, den, out=out, x_in=x_in),
                      "torch": torch_step}, a.reps, 10)
    lms = {"shape": [B] + list(shape), "fused": _stats(t["fused"]), "torch": _stats(t["torch"]),
           "torch_over_fused": round(statistics.median(t["torch"]) / statistics.median(t["fused"]), 2)}

    line = json.dumps({"workload": "sd_vae_decoder", "reps": a.reps, "group": a.group, "upsample": ups, "decoder": dec,
                       "lms_step": lms})
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
