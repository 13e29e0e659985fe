"""CFG-DDPM on STL-10 at 64 x 64 (`stl10_saliency_unlearn.yml`) on one GPU: the masked unlearning step, the kernels of
the 64 x 64 level one by one, and K26 (csrc/salun_resample.hip) beside Pillow.

  step     steps/s of the masked `saliency_unlearn` step (method rl) of the full model at the config's batch size on this
           package's kernels and on the same model with library modules (`--library_conv`), alternated in blocks of
           `--steps` in ONE process; the library convolution calls of one own-kernel step are counted.
  level64  every convolution that runs on 64 x 64 maps, at the step's batch: forward, backward-data and backward-weight
           launched on their own (HIP events around `--group` back-to-back calls, median over `--reps`), with how often
           the step runs each (three passes forward, two of them backward), and from that the share of the step that
           the 3 x 3 backward-weight launches of this level take — they run on the general route, not on the ring
           kernel, which takes W in {4, 8, 16, 32}.  The sum treats the launches as if they ran alone
           and one after the other; inside the step backward-weight runs on a side stream beside other kernels.
  resample K26 on the 13,000 x 96 x 96 x 3 stand-in -> 64 x 64 (events, median over `--reps`), the bytes it has to move
           over that time, and `PIL.Image.resize(..., BILINEAR)` over the same images on one host thread.

    python tools/stl10_bench.py [--steps 3] [--blocks 3] [--reps 7] [--group 5] [--out profiles/stl10_bench.json]

Prints one JSON line and writes it to `--out`."""
import argparse, json, os, statistics, sys, time
from types import SimpleNamespace
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def _events(fn, reps, group):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(group):
            fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e) * 1e-3 / group)
    return statistics.median(ts)


def step_rates(a, cfg):
    import torch
    from unlearn_saliency_amd import conv as sconv
    from unlearn_saliency_amd import ops
    from unlearn_saliency_amd.DDPM.functions import get_optimizer
    from unlearn_saliency_amd.DDPM.runners.diffusion import Diffusion
    from unlearn_saliency_amd.flat import arena_of
    runs, setup = {}, {}
    for name, lib in (("own", False), ("library", True)):
        args = SimpleNamespace(ckpt_folder=None, label_to_forget=0, cond_scale=2.0, mask_path=None, method="rl",
                               alpha=1e-3, synthetic=True, library_conv=lib, seed=1234)
        torch.manual_seed(1234)
        runner = Diffusion(args, cfg)
        if not runs:                      # one data set for both: stand-in -> upload -> K26 -> frozen flip -> split
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loaders = runner._loaders()
            torch.cuda.synchronize()
            setup["data_seconds"] = round(time.perf_counter() - t0, 2)
            batches = next(iter(loaders[0])), next(iter(loaders[1]))
            del loaders
            runner._remain_loader = runner._forget_loader = None
        model = runner._load_model().train()
        arena = arena_of(model)
        opt = get_optimizer(cfg, arena=arena)
        sal = ops.fill_normal(arena.n, 5, 0.0, 1e-3) * (1.0 + ops.fill_uniform(arena.n, 6, 0.0, 0.5))
        opt.set_mask(ops.mask_topk(sal, [int(arena.n * 0.5)], check=True)[0])
        runs[name] = (runner, model, opt)
        setup["parameters"] = arena.n
    rb, fb = batches

    def block(name, steps):
        runner, model, opt = runs[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            runner.unlearn_step(model, opt, rb, fb)
        torch.cuda.synchronize()
        return steps / (time.perf_counter() - t0)

    for name in runs:
        block(name, 2)
    sconv.reset_library_conv_calls()
    block("own", 1)
    counts = dict(sconv.LIBRARY_CONV_CALLS)
    rates = {n: [] for n in runs}
    for _ in range(a.blocks):
        for name in runs:
            rates[name].append(block(name, a.steps))
    fmt = lambda xs: {"steps_per_s_median": round(statistics.median(xs), 4), "steps_per_s_min": round(min(xs), 4),
                      "steps_per_s_max": round(max(xs), 4), "ms_per_step_median": round(1e3 / statistics.median(xs), 1)}
    out = {"batch": int(rb[0].shape[0]), "image": list(rb[0].shape[1:]), "steps_per_block": a.steps, "blocks": a.blocks,
           **setup, "own_kernels": fmt(rates["own"]), "library_modules": fmt(rates["library"]),
           "library_conv_calls_in_one_own_step": counts}
    out["own_over_library"] = round(out["own_kernels"]["steps_per_s_median"] /
                                    out["library_modules"]["steps_per_s_median"], 4)
    model = runs["own"][1]
    for _, _, opt in runs.values():
        if hasattr(opt, "close"):
            opt.close()
    return out, model


def level64(a, model, batch, step_seconds):
    """Every Conv2d of `model` that reads or writes a 64 x 64 map, launched alone."""
    import torch
    from unlearn_saliency_amd import ops
    lv0, up0 = model.down[0], model.up[0]
    convs = [("conv_in", model.conv_in, 64)]
    for i, b in enumerate(lv0.block):
        convs += [(f"down.0.block.{i}.conv1", b.conv1, 64), (f"down.0.block.{i}.conv2", b.conv2, 64)]
    for i, b in enumerate(up0.block):
        convs += [(f"up.0.block.{i}.conv1", b.conv1, 64), (f"up.0.block.{i}.conv2", b.conv2, 64)]
        if b.in_channels != b.out_channels:
            convs.append((f"up.0.block.{i}.nin_shortcut", b.nin_shortcut, 64))
    convs += [("up.1.upsample.conv", model.up[1].upsample.conv, 64), ("conv_out", model.conv_out, 64)]
    rows, wgrad3 = [], 0.0
    for name, m, h in convs:
        K, C, R, _ = m.weight.shape
        stride, pad = m.stride[0], m.padding[0]
        x = torch.randn(batch, C, h, h, device="cuda")   # (the stride-2 downsample reads this level too; it is left out:
        P = h                                            # its low-side padding is a launch of its own, conv.conv2d_lowpad)
        dy = torch.randn(batch, K, P, P, device="cuda")
        w = m.weight.detach()
        rec = {"conv": name, "shape": [batch, C, x.shape[2], x.shape[3], K, R, stride]}
        runs = {"forward": lambda: ops.conv2d_forward(x, w, m.bias.detach(), stride, pad, P, P),
                "backward_data": lambda: ops.conv2d_backward_data(dy, w, x.shape, stride, pad),
                "backward_weight": lambda: ops.conv2d_backward_weight(x, dy, w.shape, stride, pad)}
        for k, fn in runs.items():
            if fn() is None:
                rec[k + "_us"] = None       # outside the kernel's domain: the step would have counted a library call
                continue
            rec[k + "_us"] = round(_events(fn, a.reps, a.group) * 1e6, 1)
        flop = 2.0 * batch * K * C * R * R * P * P
        if rec["forward_us"]:
            rec["forward_tflops"] = round(flop / rec["forward_us"] / 1e6, 2)
        if rec["backward_weight_us"]:
            rec["backward_weight_tflops"] = round(flop / rec["backward_weight_us"] / 1e6, 2)
            if R == 3 and stride == 1:
                wgrad3 += rec["backward_weight_us"] * 1e-6
        rows.append(rec)
        del x, dy
    total = lambda key: sum(r[key] or 0.0 for r in rows) * 1e-6
    return {"batch": batch, "reps": a.reps, "calls_per_rep": a.group, "passes_per_step": {"forward": 3, "backward": 2},
            "convs": rows,
            "seconds_per_step_if_serial": {"forward": round(3 * total("forward_us"), 4),
                                           "backward_data": round(2 * total("backward_data_us"), 4),
                                           "backward_weight": round(2 * total("backward_weight_us"), 4)},
            "wgrad_3x3_w64_seconds_per_step": round(2 * wgrad3, 4),
            "wgrad_3x3_w64_share_of_step": round(2 * wgrad3 / step_seconds, 4)}


def resample(a):
    import numpy as np
    import torch
    from PIL import Image
    from unlearn_saliency_amd import ops_resample
    from unlearn_saliency_amd.DDPM.datasets import stl10
    x, _ = stl10.synthetic_stl10()
    t0 = time.perf_counter()
    xd = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    upload = time.perf_counter() - t0
    t = _events(lambda: ops_resample.resize_u8(xd, (64, 64)), a.reps, a.group)
    got = ops_resample.resize_u8(xd, (64, 64)).cpu().numpy()
    nbytes = x.size + got.size
    t0 = time.perf_counter()
    ref = np.stack([np.asarray(Image.fromarray(img).resize((64, 64), Image.BILINEAR)) for img in x])
    host = time.perf_counter() - t0
    import PIL
    return {"images": int(x.shape[0]), "from": list(x.shape[1:]), "to": [64, 64, 3], "k26_us_median": round(t * 1e6, 1),
            "bytes": int(nbytes), "tb_per_s": round(nbytes / t / 1e12, 3), "of_hbm_peak": round(nbytes / t / HBM_PEAK, 3),
            "lds_bytes": ops_resample.lds_bytes(96, 96, 3, 64, 64), "upload_seconds": round(upload, 3),
            "pillow_seconds_one_thread": round(host, 3), "pillow_version": PIL.__version__,
            "pillow_over_k26": round(host / t, 1), "bytes_differing_from_pillow": int((got != ref).sum())}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=3, help="steps per timed block")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--group", type=int, default=5, help="back-to-back calls per timed window")
    ap.add_argument("--batch", type=int, default=None, help="override the config's batch size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stl10_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("stl10_bench needs a ROCm device: a timing taken anywhere else says nothing")
    from unlearn_saliency_amd.DDPM.functions import load_config
    cfg = load_config(os.path.join(ROOT, "unlearn_saliency_amd", "DDPM", "configs", "stl10_saliency_unlearn.yml"))
    if a.batch:
        cfg.training.batch_size = a.batch
    res = resample(a)
    step, model = step_rates(a, cfg)
    lvl = level64(a, model, step["batch"], 1.0 / step["own_kernels"]["steps_per_s_median"])
    line = json.dumps({"workload": "ddpm_stl10_64_masked_saliency_unlearn_rl", "step": step, "level64": lvl,
                       "resample": res})
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
