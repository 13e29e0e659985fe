"""Golden values for the DDPM sampling command line, produced by the REFERENCE's own code imported from
/root/reference/DDPM (build container only):

    functions/__init__.py  create_class_labels on plain, excluding and mixed `--classes_to_generate` strings
                           -> ddpm_sample.npz
    sample.py              every flag of its parser with the default a minimal argv gives -> cli_ddpm_sample.json

    python tests/golden/make_golden_sample.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_ddpm import REF, import_reference_ddpm  # noqa: E402

CASES = [("0,1,2,3,4,5,6,7,8,9", 10), ("3", 10), ("7,2,2", 10), ("x0", 10), ("x0,x1", 10), ("x3,x3", 10), ("x9", 10),
         ("1,x3", 10), ("x2,5,x7", 10), ("x0, x1", 10), ("x4", 5), ("0,1", 100)]


def main():
    import_reference_ddpm()
    import functions as RF
    out = {"cases": np.array([s for s, _ in CASES]), "n_classes": np.array([n for _, n in CASES])}
    for k, (s, n) in enumerate(CASES):
        classes, excluded = RF.create_class_labels(s, n_classes=n)
        out[f"classes_{k}"] = np.array(classes, dtype=np.int64)
        out[f"excluded_{k}"] = np.array(excluded, dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "ddpm_sample.npz"), **out)

    argv, cwd = sys.argv, os.getcwd()
    sys.argv = ["sample.py", "--config", "cifar10_sample.yml"]
    os.chdir(REF)
    try:
        import sample as RS
        args, _ = RS.parse_args_and_config()
    finally:
        sys.argv = argv
        os.chdir(cwd)
    table = {k: v for k, v in sorted(vars(args).items()) if k != "config"}
    with open(os.path.join(HERE, "cli_ddpm_sample.json"), "w") as f:
        json.dump({"ddpm_sample_defaults": table}, f, indent=1, sort_keys=True)
    print("ddpm_sample.npz:", len(CASES), "cases; cli_ddpm_sample.json:", len(table), "flags")


if __name__ == "__main__":
    main()
