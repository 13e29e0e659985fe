"""What K23 (the fused classifier head, csrc/salun_cls_head.hip) saves on a ResNet-18 training step, on one GPU.

  step   steps/s of the pre-training step of Classification/trainer/train.py at batch 256 (forward_loss -> zero_grad ->
         backward -> fused SGD step, meters on the device) with the fused head and with the library head
         (AdaptiveAvgPool2d -> Linear -> CrossEntropyLoss + the three meter updates), the same model and optimizer,
         alternated in blocks of `--steps` in ONE process; a block that passes `--block-seconds` stops early.
  head   the head alone on a [256, 512, 4, 4] activation: forward + backward, HIP events around `--group` back-to-back
         calls, alternated, median and range over `--reps`.

    python tools/cls_train_bench.py [--steps 20] [--blocks 5] [--batch 256] [--block-seconds 30] [--reps 21] [--group 20]

Prints one JSON line (kept under profiles/)."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(batch):
    import torch
    from unlearn_saliency_amd.Classification.models.resnet_cifar import resnet18
    from unlearn_saliency_amd.cls_head import use_fused_head
    from unlearn_saliency_amd.conv import use_salun_convs
    from unlearn_saliency_amd.norm import use_fused_bn
    torch.manual_seed(0)
    model = resnet18(num_classes=10).cuda().train()
    use_salun_convs(model), use_fused_bn(model), use_fused_head(model)
    x = torch.rand(batch, 3, 32, 32, device="cuda")
    y = torch.randint(0, 10, (batch,), device="cuda")
    return model, x, y


def step_rates(a):
    import torch
    from unlearn_saliency_amd.cls_head import HeadMeters, forward_loss
    from unlearn_saliency_amd.flat import arena_of
    from unlearn_saliency_amd.optim import FusedMaskedSGD
    model, x, y = build(a.batch)
    opt = FusedMaskedSGD(arena_of(model), 0.01, momentum=0.9, weight_decay=5e-4)
    meters = HeadMeters(x.device)
    crit = torch.nn.CrossEntropyLoss()

    def block(fused, steps):
        model.fused_head = fused
        torch.cuda.synchronize()
        t0, done = time.perf_counter(), 0
        for _ in range(steps):
            loss, _ = forward_loss(model, x, y, meters, crit)
            opt.zero_grad()
            loss.backward()
            opt.step()
            done += 1
            if time.perf_counter() - t0 > a.block_seconds:
                break
        torch.cuda.synchronize()
        return done / (time.perf_counter() - t0), done

    for fused in (True, False):  # warm-up of both paths: code objects, workspaces, clocks
        block(fused, 5)
    rates = {True: [], False: []}
    short = 0
    for _ in range(a.blocks):
        for fused in (True, False):  # alternated: both see the same clocks and the same neighbours
            r, done = block(fused, a.steps)
            rates[fused].append(r)
            short += done < a.steps
    opt.close()
    fmt = lambda xs: {"steps_per_s_median": round(statistics.median(xs), 3), "steps_per_s_min": round(min(xs), 3),
                      "steps_per_s_max": round(max(xs), 3)}
    out = {"batch": a.batch, "steps_per_block": a.steps, "blocks": a.blocks, "blocks_cut_short": short,
           "fused_head": fmt(rates[True]), "library_head": fmt(rates[False])}
    out["fused_over_library"] = round(out["fused_head"]["steps_per_s_median"] /
                                      out["library_head"]["steps_per_s_median"], 4)
    return out


def head_times(a):
    import torch
    import torch.nn.functional as F
    from unlearn_saliency_amd.cls_head import HeadMeters, fused_cls_head
    torch.manual_seed(0)
    f = torch.randn(a.batch, 512, 4, 4, device="cuda").requires_grad_()
    fc = torch.nn.Linear(512, 10).cuda()
    y = torch.randint(0, 10, (a.batch,), device="cuda")
    meters = HeadMeters(f.device)

    def fused():
        loss, _ = fused_cls_head(f, fc, y, meters)
        loss.backward()

    def library():
        out = fc(torch.flatten(F.adaptive_avg_pool2d(f, 1), 1))
        loss = F.cross_entropy(out, y)
        meters.add_library(loss, out, y)
        loss.backward()

    run = {"fused_head": fused, "library_head": library}
    for fn in run.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in run}
    for _ in range(a.reps):
        for k, fn in run.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.group):
                fn()
            e.record()
            e.synchronize()
            times[k].append(s.elapsed_time(e) * 1e-3 / a.group)
    out = {"shape": [a.batch, 512, 4, 4], "reps": a.reps, "calls_per_rep": a.group}
    for k, ts in times.items():
        ts = sorted(ts)
        out[k] = {"us_median": round(statistics.median(ts) * 1e6, 1), "us_min": round(ts[0] * 1e6, 1),
                  "us_max": round(ts[-1] * 1e6, 1)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=20, help="training steps per timed block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--block-seconds", type=float, default=30.0, help="a block stops early after this long")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--group", type=int, default=20, help="back-to-back head calls per timed window")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cls_train_bench needs a ROCm device: a timing taken anywhere else says nothing")
    print(json.dumps({"workload": "cls_train_resnet18", "train_step": step_rates(a), "head": head_times(a)}))


if __name__ == "__main__":
    main()
