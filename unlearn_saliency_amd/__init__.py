"""unlearn_saliency_amd — MI355X-native SalUn hot path (gfx950).

Scope: saliency-mask generation and the masked random-label unlearning
step of OPTML-Group/Unlearn-Saliency, as hand-written HIP kernels behind a C-ABI
(include/salun.h -> libsalun.so), with a Python host side that mirrors the reference's
plugin surface (``Classification/unlearn``, ``DDPM/runners``) so it is a drop-in for
that path and nothing else.

    ops        tensor-level wrappers over the C-ABI (no CPU fallback)
    flat       flat, 16-byte-aligned parameter/gradient arena the kernels stream over
    dist       one-process-per-GPU helpers (RCCL all-reduce of the flat vectors)
    Classification / DDPM   host-side mirrors of the reference entry points
"""
__version__ = "0.1.0"

# HIP maps streams onto a few hardware queues; streams that share a queue run one after the other.  The package
# leaves the queue count to the runtime: streams.py probes each side stream for a queue of its own instead.
