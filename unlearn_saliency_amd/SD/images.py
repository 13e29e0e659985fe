"""Image files -> the uint8 NHWC batches the first-stage encoder reads (SD/autoencoder.py), and the manifest of
`encode_images.py`.

The transform is the reference's `get_transform` (SD/train-scripts/dataset.py:23-33) up to ToTensor, on the host with
Pillow: resize the shorter side to `size` (the long side becomes int(size * long / short), torchvision's rule) with
bicubic | bilinear | lanczos, centre crop to size x size, convert("RGB").  ToTensor + Normalize([0.5], [0.5]) run on
the device (conv_infer.u8_to_chw_norm with mean = std = 0.5).  A device resize is out of scope: K26 is bilinear only.
"""
from __future__ import annotations

import csv
import os
from typing import List, NamedTuple, Optional

import numpy as np

INTERPOLATIONS = ("bicubic", "bilinear", "lanczos")
SPLITS = ("forget", "remain")


def _resample(name: str):
    from PIL import Image
    if name not in INTERPOLATIONS:
        raise ValueError(f"interpolation {name!r} is not one of {', '.join(INTERPOLATIONS)}")
    return getattr(getattr(Image, "Resampling", Image), name.upper())


def resized_size(w: int, h: int, size: int):
    """torchvision's Resize(size) for an int: the shorter side becomes `size`, the other int(size * long / short)."""
    if w <= h:
        return size, int(size * h / w)
    return int(size * w / h), size


def crop_box(w: int, h: int, size: int):
    """torchvision's CenterCrop for an image at least `size` on both sides: (left, top, right, bottom)."""
    left, top = int(round((w - size) / 2.0)), int(round((h - size) / 2.0))
    return left, top, left + size, top + size


def transform(image, size: int = 512, interpolation: str = "bicubic") -> np.ndarray:
    """A PIL image -> uint8 [size, size, 3]."""
    w, h = image.size
    nw, nh = resized_size(w, h, size)
    if (nw, nh) != (w, h):
        image = image.resize((nw, nh), _resample(interpolation))
    image = image.crop(crop_box(nw, nh, size)).convert("RGB")
    return np.asarray(image, dtype=np.uint8)


def load(path: str, size: int = 512, interpolation: str = "bicubic") -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return transform(im, size, interpolation)


class Row(NamedTuple):
    split: str
    path: str
    prompt: str
    other_prompt: Optional[str]


def read_manifest(path: str) -> List[Row]:
    """CSV rows `split,path,prompt[,other_prompt]`, split in forget | remain; relative paths are relative to the
    manifest.  Empty lines and lines starting with # are skipped.  A forget row without other_prompt takes ""
    (the empty prompt generate_mask.py pairs with the forget prompt)."""
    rows, base = [], os.path.dirname(os.path.abspath(path))
    with open(path, newline="") as f:
        for ln, rec in enumerate(csv.reader(f), 1):
            if not rec or not "".join(rec).strip() or rec[0].lstrip().startswith("#"):
                continue
            rec = [r.strip() for r in rec]
            if len(rec) not in (3, 4) or rec[0] not in SPLITS:
                raise ValueError(f"{path}:{ln}: expected split,path,prompt[,other_prompt] with split in "
                                 f"{' | '.join(SPLITS)}, got {rec}")
            p = rec[1] if os.path.isabs(rec[1]) else os.path.join(base, rec[1])
            other = rec[3] if len(rec) == 4 else ("" if rec[0] == "forget" else None)
            rows.append(Row(rec[0], p, rec[2], other))
    return rows


def check_prompts(rows: List[Row], contexts: dict) -> None:
    """Every prompt of the manifest must have a context embedding: the first one missing is named."""
    for r in rows:
        for p in (r.prompt, r.other_prompt):
            if p is not None and p not in contexts:
                raise KeyError(f"prompt {p!r} ({r.split}, {r.path}) is missing from the contexts file")
