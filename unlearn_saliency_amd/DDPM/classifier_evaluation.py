"""Unlearning accuracy of generated images: the counterpart of the reference's DDPM/classifier_evaluation.py.

    python -m unlearn_saliency_amd.DDPM.classifier_evaluation --sample_path <run>/class_samples/0 --dataset cifar10

reads the images `sample.py --mode sample_classes` wrote for one class, classifies them with a ResNet-34 at 224 x 224
and prints the mean entropy of the prediction, the mean probability of the forgotten class and the share of images
still classified as that class; the three numbers also go to one row of a CSV that either code base can append to.

Flags and defaults are the reference's four.  Additive: `--classifier_path` (default `{dataset}_resnet34.pth` in the
working directory, where the reference looks), `--synthetic` (seeded stand-in weights when no trained checkpoint is at
hand), `--entropy_zero_safe` (a probability that underflowed to 0 contributes 0 to the entropy instead of the
reference's NaN: SURVEY.md Appendix B) and `--result_csv` (default: the reference's literal path).

The whole pipeline runs on the device (models/resnet34.InferencePlan): the uint8 images are uploaded once, resized by
K26, normalised, pushed through K27's 36 convolutions and folded into four device-side meters by the evaluation head;
the host reads the meters once at the end.  There is no CPU path.
"""
from __future__ import annotations

import argparse
import csv
import math
import os
import pathlib
import sys

import numpy as np
import torch

IMAGE_EXTENSIONS = {"bmp", "jpg", "jpeg", "pgm", "png", "ppm", "tif", "tiff", "webp"}
COLUMNS = ("entropy", "prob of forgotten class", "accuracy of forgotten class")
DEFAULT_CSV = "results/cifar10/forget/result.csv"
IMG_SIZE = 224


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Classifier evaluation (UA, entropy) of generated images")
    p.add_argument("--sample_path", type=str, help="Path to folder containing samples")
    p.add_argument("--dataset", type=str, choices=["cifar10", "stl10"], help="name of the dataset, either cifar10 or stl10")
    p.add_argument("--label_of_forgotten_class", type=int, default=0,
                   help="Class label of forgotten class (for calculating average prob)")
    p.add_argument("-b", "--batch-size", type=int, default=64, help="test batch size for inference")
    p.add_argument("--classifier_path", type=str, default=None, help="checkpoint (default: {dataset}_resnet34.pth)")
    p.add_argument("--synthetic", action="store_true", help="seeded stand-in weights instead of a checkpoint")
    p.add_argument("--entropy_zero_safe", action="store_true", help="0 * log 0 = 0 in the entropy")
    p.add_argument("--result_csv", type=str, default=DEFAULT_CSV)
    return p


def list_images(img_folder: str):
    """The files the reference's ImagePathDataset reads, in its order."""
    path = pathlib.Path(img_folder)
    return sorted([file for ext in IMAGE_EXTENSIONS for file in path.glob("*.{}".format(ext))])


def read_images(files):
    """-> list of uint8 (H, W, 3) arrays: Image.open(path).convert("RGB"), as the reference."""
    from PIL import Image
    return [np.asarray(Image.open(f).convert("RGB"), dtype=np.uint8) for f in files]


def validate_u8(images_u8: torch.Tensor, label: int, plan=None, batch_size: int = 64, zero_safe: bool = False,
                meters=None, finish: bool = True):
    """images_u8: uint8 [n, h, w, 3] on the device.  Runs the plan batch by batch (the last one may be ragged) and
    returns {"entropy", "prob", "accuracy", "n"} — or, with finish=False, only advances `meters`."""
    from .. import ops_infer
    if not images_u8.is_cuda:
        raise RuntimeError("classifier evaluation needs a ROCm device (no CPU fallback)")
    if plan is None:                        # the reference's default: the CIFAR-10 checkpoint in the working directory
        from .models.resnet34 import InferencePlan
        plan = InferencePlan(load_model(argparse.Namespace(synthetic=False, classifier_path=None, dataset="cifar10")),
                             images_u8.device, IMG_SIZE)
    meters = ops_infer.EvalMeters(images_u8.device) if meters is None else meters
    for i in range(0, images_u8.shape[0], batch_size):
        plan.forward_u8(images_u8[i:i + batch_size], label, meters, zero_safe)
    return summarize(meters) if finish else None


def summarize(meters) -> dict:
    m = meters.read()
    n = m["count"]
    return {"entropy": m["entropy_sum"] / n, "prob": m["prob_sum"] / n, "accuracy": m["hits"] / n, "n": n}


def _fmt(v) -> str:
    """A cell as pandas.DataFrame.to_csv writes it: repr of the float, an empty cell for NaN."""
    v = float(v)
    return "" if math.isnan(v) else repr(v)


def update_csv(csv_path: str, name: str, result: dict) -> None:
    """The reference's frame logic without pandas: read the file (index in column 0), overwrite or append row `name`,
    keep every other row and column, write it back in the format pandas.DataFrame.to_csv produces."""
    header, rows = [], []
    if os.path.exists(csv_path):
        with open(csv_path, newline="") as f:
            table = list(csv.reader(f))
        if table:
            header, rows = table[0][1:], [r for r in table[1:] if r]
    for col in COLUMNS:
        if col not in header:
            header.append(col)
    rows = [r + [""] * (1 + len(header) - len(r)) for r in rows]
    row = next((r for r in rows if r[0] == name), None)
    if row is None:
        row = [name] + [""] * len(header)
        rows.append(row)
    for col in COLUMNS:
        row[1 + header.index(col)] = _fmt(result[col])
    os.makedirs(os.path.dirname(csv_path) or ".", exist_ok=True)
    with open(csv_path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow([""] + header)
        w.writerows(rows)


def row_name(sample_path: str) -> str:
    parts = sample_path.split("/")
    return parts[-4] + "/" + parts[-3]


def load_model(args):
    from .models.resnet34 import resnet34, standin_state_dict
    model = resnet34(10)
    if args.synthetic:
        model.load_state_dict(standin_state_dict(0))
    else:
        path = args.classifier_path or f"{args.dataset}_resnet34.pth"
        model.load_state_dict(torch.load(path, map_location="cpu"))
    return model.eval()


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("classifier evaluation needs a ROCm device (no CPU fallback)")
    from .. import conv_infer, ops_infer
    from .models.resnet34 import InferencePlan
    device = torch.device("cuda", torch.cuda.current_device())
    plan = InferencePlan(load_model(args), device, IMG_SIZE)
    files = list_images(args.sample_path)
    if not files:
        raise FileNotFoundError(f"no images under {args.sample_path}")
    images = read_images(files)
    meters = ops_infer.EvalMeters(device)
    by_size: dict = {}
    for im in images:                       # (the sampler writes one size; a mixed folder is run size by size)
        by_size.setdefault(im.shape[:2], []).append(im)
    for group in by_size.values():
        u8 = torch.from_numpy(np.stack(group)).to(device)     # uploaded once
        validate_u8(u8, args.label_of_forgotten_class, plan, args.batch_size, args.entropy_zero_safe, meters, finish=False)
    r = summarize(meters)
    if conv_infer.library_infer_calls():
        print(f"note: {conv_infer.LIBRARY_INFER_CALLS} calls ran on library ops", file=sys.stderr)
    print(f"Average entropy: {r['entropy']}")
    print(f"Average prob of forgotten class: {r['prob']}")
    print(f"Average accuracy of forgotten class: {r['accuracy']}")
    update_csv(args.result_csv, row_name(args.sample_path),
               {COLUMNS[0]: r["entropy"], COLUMNS[1]: r["prob"], COLUMNS[2]: r["accuracy"]})
    return 0


if __name__ == "__main__":
    sys.exit(main())
