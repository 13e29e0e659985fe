#!/usr/bin/env python3
"""One SHA-256 per kernel source of its normalised gfx950 device assembly.

    python tools/device_asm_hash.py [--csrc DIR] [--jobs N] [--keep DIR] > listing.txt

Every *.hip under DIR (default: unlearn_saliency_amd/csrc of this tree) is compiled with the Makefile's own CXXFLAGS plus
`--cuda-device-only -S`.  Before hashing, the lines that differ between two builds of the same device code are dropped:
`.file` and `.ident`, comment lines, and every line that names the per-file `__hip_cuid_*` symbol.  Two trees whose
listings are equal emit the same device code; a refactor of host code or of shared headers is checked by diffing the
listing of the parent commit against the one of the head.  The script only hashes text; it looks for nothing in it.
"""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def makefile_var(csrc, name):
    out = subprocess.run(
        ["make", "-s", "-C", csrc, "--no-print-directory", "--eval", f"print-var: ; @echo $({name})", "print-var"],
        check=True, capture_output=True, text=True).stdout
    return out.split()


def normalised(text):
    keep = []
    for line in text.splitlines():
        s = line.strip()
        if s.startswith(".file") or s.startswith(".ident") or s.startswith(";") or "__hip_cuid_" in s:
            continue
        keep.append(line.rstrip())
    return "\n".join(keep) + "\n"


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--csrc", default=os.path.join(here, "..", "unlearn_saliency_amd", "csrc"))
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", default=None, help="also write each normalised listing as DIR/<source>.s")
    a = ap.parse_args()
    csrc = os.path.abspath(a.csrc)
    hipcc = makefile_var(csrc, "HIPCC")
    flags = makefile_var(csrc, "CXXFLAGS")
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    if a.keep:
        os.makedirs(a.keep, exist_ok=True)

    def one(src):
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, src + ".s")
            subprocess.run(hipcc + flags + ["--cuda-device-only", "-S", src, "-o", out], cwd=csrc, check=True)
            with open(out) as f:
                text = normalised(f.read())
        if a.keep:
            with open(os.path.join(a.keep, src + ".s"), "w") as f:
                f.write(text)
        return hashlib.sha256(text.encode()).hexdigest()

    with ThreadPoolExecutor(max_workers=max(1, a.jobs)) as pool:
        for src, digest in zip(srcs, pool.map(one, srcs)):
            print(f"{digest}  {src}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
