"""The masked RL step on the four datasets (`--dataset cifar10 | svhn | cifar100 | TinyImagenet`), ResNet-18, one GPU.

  step    steps/s of the masked random-label step at batch 256 with the device loader (batch assembly on the device ->
          forward -> cross-entropy on random labels -> zero_grad -> backward -> fused masked SGD step) on this
          package's kernels and on the same model with plain library modules, alternated in blocks of `--steps` in ONE
          process, every dataset in every round; the library convolution calls of one own-kernel step are counted.
          `whole_step_frac_of_fp32_matrix_peak` is bench.py's roofline arithmetic (3.329 GFLOP forward + backward per
          32 x 32 image, x 4 at 64 x 64, over 157.3 TFLOP/s) applied to the WHOLE step's time, loader and
          optimizer included: an end-to-end figure, not a kernel's share of peak.
          Checks: svhn and cifar100 differ from cifar10 in the head alone, so their medians must sit within the spread
          of cifar10's own readings (`within_cifar10_spread`); TinyImagenet must count no library convolution.
  swap    at Tiny-ImageNet size (100,000 x 64 x 64 x 3 bytes resident): what RL's merged branch pays per epoch to change
          the forget labels and start the epoch (new label vector -> first batch), beside a full re-upload of the
          images, which is what a loader keyed on the label vector's identity did.

    python tools/datasets_bench.py [--steps 10] [--blocks 5] [--batch 256] [--images 5120] [--block-seconds 30]
                                   [--out profiles/datasets_bench.json]

Prints one JSON line and writes it to `--out`."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_MATRIX_PEAK_TF = 157.3      # as bench.py
FWD_BWD_GFLOP_PER_IMG_32 = 3.329  # as bench.py (ResNet-18 at 32 x 32); the convolutions scale with the pixel count
NAMES = ("cifar10", "svhn", "cifar100", "TinyImagenet")


def build(name, own):
    import torch
    from unlearn_saliency_amd.Classification.dataset import DATASETS
    from unlearn_saliency_amd.Classification.models import model_dict
    from unlearn_saliency_amd.Classification.models.resnet_cifar import NormalizeByChannelMeanStd
    from unlearn_saliency_amd.conv import use_salun_convs
    from unlearn_saliency_amd.norm import use_fused_bn
    spec = DATASETS[name]
    torch.manual_seed(0)
    model = model_dict["resnet18"](num_classes=spec.classes)
    model.normalize = NormalizeByChannelMeanStd(spec.mean, spec.std)
    model = model.cuda().train()
    if own:
        use_salun_convs(model), use_fused_bn(model)
    return model


def step_rates(a):
    import torch
    import torch.nn.functional as F
    from unlearn_saliency_amd import conv as sconv
    from unlearn_saliency_amd.Classification.dataset import (DATASETS, TRAIN_TRANSFORM, ArrayDataset, BatchLoader,
                                                             synthetic_images)
    from unlearn_saliency_amd.flat import arena_of
    from unlearn_saliency_amd.optim import FusedMaskedSGD
    runs = {}
    for name in NAMES:
        (x, y), _ = synthetic_images(name, a.images, 1)
        # svhn trains without augmentation (the reference's loader has none); the others crop and flip
        ds = ArrayDataset(x, y, "test" if name == "svhn" else TRAIN_TRANSFORM)
        for kind, own in (("own", True), ("library", False)):
            model = build(name, own)
            arena = arena_of(model)
            opt = FusedMaskedSGD(arena, 0.01, momentum=0.9, weight_decay=5e-4)
            opt.set_mask((torch.arange(arena.n, device="cuda") % 2).to(torch.uint8))
            loader = BatchLoader(ds, a.batch, True, device_resident=True, device=torch.device("cuda"))
            runs[name, kind] = dict(model=model, opt=opt, loader=loader, it=None, classes=DATASETS[name].classes)

    def batches(r):
        while True:
            for xb, yb in r["loader"]:
                if xb.shape[0] == a.batch:
                    yield xb, yb

    def block(key, steps):
        r = runs[key]
        r["it"] = r["it"] or batches(r)
        torch.cuda.synchronize()
        t0, done = time.perf_counter(), 0
        for _ in range(steps):
            xb, yb = next(r["it"])
            labels = torch.randint(0, r["classes"], yb.shape, device=yb.device)   # the random labels of an RL step
            loss = F.cross_entropy(r["model"](xb), labels)
            r["opt"].zero_grad()
            loss.backward()
            r["opt"].step()
            done += 1
            if time.perf_counter() - t0 > a.block_seconds:
                break
        torch.cuda.synchronize()
        return done / (time.perf_counter() - t0), done

    counts = {}
    for key in runs:                      # warm-up of every path: code objects, workspaces, library algorithm search
        block(key, 3)
    for name in NAMES:
        sconv.reset_library_conv_calls()
        block((name, "own"), 1)
        counts[name] = sconv.library_conv_calls()
    rates = {key: [] for key in runs}
    short = 0
    for _ in range(a.blocks):
        for key in runs:                  # alternated: every configuration sees the same clocks and neighbours
            r, done = block(key, a.steps)
            rates[key].append(r)
            short += done < a.steps
    for r in runs.values():
        r["opt"].close()
    fmt = lambda xs: {"steps_per_s_median": round(statistics.median(xs), 3), "steps_per_s_min": round(min(xs), 3),
                      "steps_per_s_max": round(max(xs), 3)}
    out = {"batch": a.batch, "steps_per_block": a.steps, "blocks": a.blocks, "blocks_cut_short": short, "datasets": {}}
    c10 = rates["cifar10", "own"]
    for name in NAMES:
        own, lib = fmt(rates[name, "own"]), fmt(rates[name, "library"])
        gflop = FWD_BWD_GFLOP_PER_IMG_32 * (DATASETS[name].image / 32) ** 2 * a.batch
        d = {"own_kernels": own, "library_modules": lib, "library_conv_calls_per_step": counts[name],
             "own_over_library": round(own["steps_per_s_median"] / lib["steps_per_s_median"], 4),
             "gflop_per_step": round(gflop, 1),
             "whole_step_frac_of_fp32_matrix_peak": round(gflop * own["steps_per_s_median"] / 1e3
                                                          / FP32_MATRIX_PEAK_TF, 4)}
        if name in ("svhn", "cifar100"):
            d["within_cifar10_spread"] = bool(min(c10) <= own["steps_per_s_median"] <= max(c10))
        out["datasets"][name] = d
    return out


def swap_times(a):
    import numpy as np
    import torch
    from unlearn_saliency_amd.Classification.dataset import DATASETS, TRAIN_TRANSFORM, ArrayDataset, BatchLoader
    spec = DATASETS["TinyImagenet"]
    n = spec.n_train
    x = np.zeros((n, spec.image, spec.image, 3), np.uint8)   # the upload does not depend on the pixels
    ds = ArrayDataset(x, np.arange(n) % spec.classes, TRAIN_TRANSFORM)
    loader = BatchLoader(ds, a.batch, True, device_resident=True, device=torch.device("cuda"))
    next(iter(loader))
    torch.cuda.synchronize()

    def epoch_start(reupload):
        ds.targets = np.random.randint(0, spec.classes, (n,))
        if reupload:
            loader._dev_data = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        next(iter(loader))
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    swap = sorted(epoch_start(False) for _ in range(a.swap_reps))
    full = sorted(epoch_start(True) for _ in range(a.swap_reps))
    ms = lambda v: {"median": round(statistics.median(v) * 1e3, 3), "min": round(v[0] * 1e3, 3),
                    "max": round(v[-1] * 1e3, 3)}
    return {"resident_bytes": int(x.nbytes), "reps": a.swap_reps, "label_swap_and_epoch_start_ms": ms(swap),
            "full_reupload_and_epoch_start_ms": ms(full), "image_uploads": loader.image_uploads}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--blocks", type=int, default=5)
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--images", type=int, default=5120, help="synthetic training images per dataset")
    p.add_argument("--block-seconds", type=float, default=30.0)
    p.add_argument("--swap-reps", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "datasets_bench.json"))
    a = p.parse_args()
    out = {"tool": "tools/datasets_bench.py", "step": step_rates(a), "swap": swap_times(a)}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
