"""`python sample.py --config cifar10_sample.yml --ckpt_folder F --mode sample_classes|sample_fid|visualization
[--n_samples_per_class 500 --classes_to_generate x0 --cond_scale 2.0 --timesteps 1000]`
(`--config stl10_sample.yml`: the same modes at 64 x 64.)

Same flags and defaults as the reference's DDPM/sample.py:16-75.  Writes the folders of PNGs its evaluation reads —
`F/class_samples/<class>/<id>.png`, `F/fid_samples_guidance_<s>[_excluded_class_<a>_<b>]/<id>.png`,
`F/sample-<s>.png` — with the reverse process on the fused step kernel and every draw keyed by (`--seed`, image id):
an image does not depend on `sampling.batch_size` or on the number of ranks.
Multi-GPU: launch with torchrun (one process per GPU); image ids are dealt round-robin over the ranks."""
import argparse
import logging
import os
import sys
import traceback

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import unlearn_saliency_amd.DDPM  # noqa: F401
    __package__ = "unlearn_saliency_amd.DDPM"

import numpy as np
import torch

from .. import dist as sdist
from .functions import load_config
from .runners.diffusion import Diffusion

_HERE = os.path.dirname(os.path.abspath(__file__))

_FLAGS = [
    ("--config", dict(type=str, required=True, help="Path to the config file (relative to configs/)")),
    ("--ckpt_folder", dict(type=str, help="Path to folder with the model to sample (ckpts/ckpt.pth); output root")),
    ("--mode", dict(type=str, choices=["sample_fid", "sample_classes", "visualization"], help="Sampling mode.")),
    ("--n_samples_per_class", dict(type=int, default=5000, help="Number of samples per class to generate.")),
    ("--classes_to_generate", dict(type=str, default="0,1,2,3,4,5,6,7,8,9",
                                   help="Comma-separated class labels to generate, e.g. '0,1,2,3'; or prefix 'x' to "
                                        "drop classes, e.g. 'x0,x1' generates all classes but 0 and 1.")),
    ("--seed", dict(type=int, default=1234, help="Random seed")),
    ("--sample_type", dict(type=str, default="generalized", help="sampling approach (generalized or ddpm_noisy)")),
    ("--skip_type", dict(type=str, default="uniform", help="skip according to (uniform or quad)")),
    ("--timesteps", dict(type=int, default=1000, help="number of steps involved")),
    ("--eta", dict(type=float, default=1.0, help="eta used to control the variances of sigma")),
    ("--cond_scale", dict(type=float, default=2.0, help="classifier-free guidance conditional strength")),
    ("--sequence", dict(action="store_true")),
    # build extensions
    ("--synthetic", dict(action="store_true", help="randomly initialised U-Net when ckpt_folder holds no checkpoint")),
    ("--library_conv", dict(action="store_true", help="use the library (MIOpen) convolutions instead of the MFMA kernels")),
]


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__)
    for flag, kw in _FLAGS:
        parser.add_argument(flag, **kw)
    return parser


def parse_args_and_config(argv=None):
    args = build_parser().parse_args(argv)
    cfg = args.config if os.path.exists(args.config) else os.path.join(_HERE, "configs", args.config)
    config = load_config(cfg)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(args.seed)
    torch.backends.cudnn.benchmark = True
    return args, config


def main(argv=None):
    sdist.init_from_env()
    args, config = parse_args_and_config(argv)
    try:
        runner = Diffusion(args, config)
        if args.ckpt_folder:
            os.makedirs(args.ckpt_folder, exist_ok=True)
        runner.sample()
    except Exception:
        logging.error(traceback.format_exc())
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
