"""Optimizer factory, YAML -> Namespace config, run-directory layout (reference DDPM/functions/__init__.py)."""
from __future__ import annotations

import argparse
import os
from datetime import datetime

import yaml

from ...flat import FlatArena
from ...optim import FusedMaskedAdam, FusedMaskedSGD


def get_optimizer(config, parameters=None, arena: FlatArena = None):
    """`get_optimizer(config, model.parameters())` in the reference (functions/__init__.py:9-28) returns
    torch.optim.Adam(lr, weight_decay, betas=(beta1, 0.999), amsgrad, eps).  Here the caller passes the
    model's flat arena and gets the fused equivalent; grad clipping (config.optim.grad_clip) is folded in."""
    if arena is None:
        raise ValueError("get_optimizer needs the model's FlatArena (arena=arena_of(model))")
    o = config.optim
    if o.optimizer == "Adam":
        return FusedMaskedAdam(arena, lr=o.lr, betas=(o.beta1, 0.999), eps=o.eps, weight_decay=o.weight_decay,
                               amsgrad=o.amsgrad, grad_clip=getattr(o, "grad_clip", None))
    if o.optimizer == "SGD":
        return FusedMaskedSGD(arena, lr=o.lr, momentum=0.9)
    raise NotImplementedError("Optimizer {} not understood.".format(o.optimizer))


def dict2namespace(config: dict) -> argparse.Namespace:
    ns = argparse.Namespace()
    for key, value in config.items():
        setattr(ns, key, dict2namespace(value) if isinstance(value, dict) else value)
    return ns


def load_config(filename: str) -> argparse.Namespace:
    with open(filename, "r") as fp:
        return dict2namespace(yaml.safe_load(fp))


def _make_run_dirs(config, root):
    config.exp_root_dir = root
    config.log_dir = os.path.join(root, "logs")
    config.ckpt_dir = os.path.join(root, "ckpts")
    os.makedirs(config.log_dir, exist_ok=True)
    os.makedirs(config.ckpt_dir, exist_ok=True)
    with open(os.path.join(config.log_dir, "config.yaml"), "w") as fp:
        yaml.dump(config, fp)
    return config


def mask_tag(mask_path) -> str:
    """Run-dir tag derived from the mask file name (reference functions/__init__.py:58-68).  The
    reference crashes on `None` ("origin" in None); here no mask maps to "full"."""
    if mask_path:
        for tag in ("origin", "inverted", "random", "without"):
            if tag in mask_path:
                return tag
    return "full"


def get_mask_config_and_setup_dirs(args, filename: str):
    """results/<dataset>/forget/<method>/<alpha>_<masktag>/<timestamp>/{logs,ckpts}"""
    config = load_config(filename)
    stamp = datetime.now().strftime("%Y_%m_%d_%H%M%S")
    root = os.path.join("./results", config.data.dataset.lower(), "forget", args.method,
                        f"{args.alpha}_{mask_tag(args.mask_path)}", stamp)
    return _make_run_dirs(config, root)


def get_config_and_setup_dirs(filename: str):
    config = load_config(filename)
    stamp = datetime.now().strftime("%Y_%m_%d_%H%M%S")
    return _make_run_dirs(config, os.path.join("./results", config.data.dataset.lower(), stamp))


def cycle(dl):
    while True:
        for data in dl:
            yield data


def create_class_labels(string: str, n_classes: int = 10):
    """`--classes_to_generate` (reference functions/__init__.py:126-133): a comma list of class ids, or — as soon as
    one entry starts with "x" — every class except the "xN" entries (plain ids next to them are ignored, as there).
    -> (classes, excluded)."""
    entries = string.split(",")
    excluded = [int(e[1:]) for e in entries if e.startswith("x")]
    if excluded:
        return [k for k in range(n_classes) if k not in excluded], excluded
    return [int(e) for e in entries], []


def rank_image_ids(first: int, count: int, rank: int = 0, world_size: int = 1):
    """The image ids of [first, first + count) that `rank` samples: dealt round-robin over the GLOBAL id
    (id % world_size == rank), so every id belongs to exactly one rank whatever the class or round it falls into."""
    if not 0 <= rank < world_size:
        raise ValueError(f"rank {rank} outside a world of {world_size}")
    return [i for i in range(first, first + count) if i % world_size == rank]


def sampling_rounds(ids, batch_size: int):
    """The reference's rounds over `sampling.batch_size` (runners/diffusion.py:690-704): full batches, then the ragged
    tail.  -> list of id lists."""
    ids = list(ids)
    n_rounds = len(ids) // batch_size + (0 if len(ids) % batch_size == 0 else 1)
    out, n_left = [], len(ids)
    for _ in range(n_rounds):
        n = batch_size if n_left >= batch_size else n_left
        done = len(ids) - n_left
        out.append(ids[done:done + n])
        n_left -= n
    return out
