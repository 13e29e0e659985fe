"""A Python mirror of K28's host arithmetic (csrc/salun_gn_split.hip: the slab plan, the workspace size, the domain) and
the shapes its GPU test runs.  The float64 model and the per-element bounds are norm_ref_cpu.gn_forward /
gn_forward_bound: K28 computes what k_gn_fwd computes, with c1 = C1 roundings on a value's way into the fp32 sums.
Importable without a GPU; checked against brute force by test_gn_split_ref_cpu.py."""
from collections import namedtuple

FLUSH = 16                 # SALUN_GN_SPLIT_FLUSH: float4s a lane adds in fp32 before it folds into its doubles
C1 = 2 + FLUSH             # roundings on a value: the float4 tree (2) and at most FLUSH adds into the accumulator
AUTO_SLAB = 2048           # float4s per slab when slab_vec4 == 0


def ok(N, C, HW, G, slab_vec4=0):
    if N < 1 or C < 1 or G < 1 or C % G or HW < 4 or HW % 4 or slab_vec4 < 0:
        return False
    return C // G * HW < 1 << 31 and N * G * slabs(C, HW, G, slab_vec4, checked=False) < 1 << 31


def slabs(C, HW, G, slab_vec4=0, checked=True):
    """S: a function of cpg * HW and slab_vec4 only.  0 outside the domain."""
    if checked and not ok(1, C, HW, G, slab_vec4):
        return 0
    nvec = C // G * HW // 4
    return -(-nvec // (slab_vec4 or AUTO_SLAB))


def boundaries(C, HW, G, slab_vec4=0):
    """[(lo, hi)] in float4s within a group, one per slab."""
    nvec, slab = C // G * HW // 4, slab_vec4 or AUTO_SLAB
    return [(s * slab, min((s + 1) * slab, nvec)) for s in range(slabs(C, HW, G, slab_vec4))]


def ws_bytes(N, C, HW, G, slab_vec4=0):
    return 16 * N * G * slabs(C, HW, G, slab_vec4) if ok(N, C, HW, G, slab_vec4) else 0


Case = namedtuple("Case", "N C G H W slab why")
CASES = [Case(*s) for s in [
    (2, 8, 2, 4, 4, 0, "S = 1"),
    (2, 8, 2, 4, 4, 3, "S > 1, ragged last slab, boundaries inside a channel"),
    (1, 32, 32, 8, 8, 5, "cpg = 1"),
    (2, 12, 3, 6, 6, 0, "HW = 36, which salun_gn_forward refuses"),
    (2, 12, 3, 6, 6, 7, "HW = 36, a boundary between channels"),
    (1, 8, 2, 512, 512, 0, "L = 2^20, the real split"),
]]
case_id = lambda c: f"{c.N}x{c.C}g{c.G}x{c.H}x{c.W}s{c.slab}"
# the GroupNorm shapes of the v1 encoder at a 512 x 512 image: (C, H = W); G = 32
VAE_SHAPES = [(128, 512), (128, 256), (256, 256), (256, 128), (512, 128), (512, 64)]
CUS = 256
