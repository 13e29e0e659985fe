"""The float64 model of K30 (csrc/salun_conv1x1_infer.hip), its cases and the mirror of its plan.  Importable without a
GPU; its premises are asserted by test_conv1x1_ref_cpu.py; used by test_conv1x1_infer_gpu.py.

The model is conv_infer_ref_cpu.forward with R = 1, stride 1, pad 0 - K30 computes what K27 computes for such a layer -
and the inputs are conv_infer_ref_cpu.inputs (exact tier: small integers times powers of two on the axes the reduction
does not run over; bound tier: Gaussians)."""
import conv_infer_ref_cpu as R
from conv_infer_ref_cpu import EPILOGUES, TILES, U, bound_gamma, epilogue, forward, inputs, terms_of  # noqa: F401

# (N, C, H, W, K): the smallest shapes at which K30's indexing can go wrong
SHAPES = [
    (3, 8, 7, 7, 32),          # HW = 49: tiles span images, tail tile, one partial stage, partial channel tile
    (2, 16, 2, 2, 64),
    (5, 64, 1, 1, 64),
    (1, 24, 14, 14, 96),       # 16-byte path, C % 16 = 8
    (1, 64, 56, 56, 256),
    (2, 2048, 7, 7, 512),      # the longest chain, on the 4-byte path
    (1, 256, 14, 14, 1024),
]
CASES = [R.Case(N, C, H, W, K, 1, 1, 0) for N, C, H, W, K in SHAPES]
SKEWED = CASES[3]              # run again with x and y one float off the 16-byte boundary
REFUSED = {"K = 48": dict(K=48), "C = 12": dict(C=12)}


def route(c, tile=0, aligned16=True, w_aligned16=True):
    """The label K30's plan gives (the mirror of plan_pw in csrc/salun_conv1x1_infer.hip), or None where it refuses."""
    N, C, HW, K = c.N, c.C, c.H * c.W, c.K
    if N < 1 or HW < 1 or N * HW > 1 << 40 or C < 8 or C > 65536 or C % 8 or K < 32 or K > 65536 or K % 32:
        return None
    if tile not in (0, 1, 2, 3):
        return None
    pb, kb = (0, 64, 128, 128), (0, 64, 64, 128)
    blocks = lambda t: -(-N * HW // pb[t]) * -(-K // kb[t])
    t = tile
    if t == 0:
        t = 3 if (K % 128 == 0 and blocks(3) >= 256) else 2 if blocks(2) >= 256 else 1
    if blocks(t) > 0x7FFFFFFF:
        return None
    mode = "scalar" if not w_aligned16 else "vec16" if (aligned16 and HW % 4 == 0) else "vec4"
    return f"pw/{pb[t]}x{kb[t]}/{mode}/B{blocks(t)}"
