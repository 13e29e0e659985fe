"""A float64 model of the bf16 convolution (K11: csrc/salun_conv_bf16.hip, and the ring / TN kernels of csrc/salun_gemm.hip
it routes to), the inputs the exact-answer tests feed it, and the shapes they run.  Validated against torch's float64
convolution by test_conv_bf16_ref_cpu.py; used by test_conv_bf16_exact_gpu.py.

The model is conv_ref_cpu's tap-by-tap definition behind layout wrappers: activations NHWC (x[N][H][W][C],
y[N][OH][OW][K]), weights and their gradient OIHW, R in {1, 3}, stride in {1, 2}, symmetric pad in 0..R-1,
OH = (H + 2 pad - R) / stride + 1.  Forward epilogue ((conv + bias[k]) + nbias[n][k]) + addend, the kernels' order;
backward-data + addend; backward-weight gives dw (+ dw0), db[k] = sum of dy (+ db0) and dnb[n][k] = the sum over image n.
Every operation takes `absolute=True`: the same sum over absolute values, the quantity a rounding bound is a multiple of.

Two kinds of input, both seeded, both exactly representable in bf16 (8 significand bits) where the kernel reads bf16:
  integers  small integers times powers of two, conv_ref_cpu's scale scheme: forward and backward-data scale image n by
            2^(-7 (n mod 3)) and output channel k of w by 2^(5 (k mod 3)); backward-weight reduces over the images, so
            there the scales sit on the channels of x and dy.  bias, nbias, dw0 and db0 are fp32, addend is bf16; each
            carries the scale of the element it joins.  Every product and every partial sum, in any order, split or not,
            epilogue terms included, is a whole multiple of the element's unit and below 2^24 units
            (test_conv_bf16_ref_cpu.py asserts it for every case): the fp32 value before the final rounding is EXACT, and
            the one rounding left is fp32 -> bf16, nearest even (none for the fp32 outputs dw, db, dnb).  The integer range
            is picked per case from the shape (int_ranges) so that the condition holds: backward-data reduces over k,
            whose terms span 2^10.
  gaussian  normal draws rounded to bf16 (fp32 for the fp32 operands) times the same scales, for the per-element bound."""
from collections import namedtuple
from types import SimpleNamespace

import torch

import conv_ref_cpu as F

U = F.U                       # unit roundoff of fp32, 2^-24
U16 = 2.0 ** -8               # unit roundoff of bf16: 8 significand bits, round to nearest
IMG_EXP, CH_EXP = F.IMG_EXP, F.CH_EXP
bound_gamma = F.bound_gamma


def out_extent(H, R, stride, pad):
    return (H + 2 * pad - R) // stride + 1


class Case(namedtuple("Case", "N H W C K R stride pad fwd dgrad wgrad")):
    """A shape and the route label each direction is there for (queried workspace, aligned pointers, default switches);
    None: the direction is not run on this shape."""
    __slots__ = ()

    @property
    def shape(self):
        return tuple(self[:8])

    @property
    def OH(self):
        return out_extent(self.H, self.R, self.stride, self.pad)

    @property
    def OW(self):
        return out_extent(self.W, self.R, self.stride, self.pad)

    @property
    def id(self):
        return "x".join(map(str, self.shape))


# ------------------------------------------------------------------------------------------ the model
def nchw(t):
    return None if t is None else t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return None if t is None else t.permute(0, 2, 3, 1).contiguous()


def forward(x, w, stride, pad, bias=None, nbias=None, addend=None, absolute=False):
    """y[n,oh,ow,k] = sum_{r,s,c} x[n,oh*stride-pad+r,ow*stride-pad+s,c] w[k,c,r,s], then ((y + bias[k]) + nbias[n,k]) +
    addend[n,oh,ow,k]."""
    R = w.shape[2]
    OH, OW = out_extent(x.shape[1], R, stride, pad), out_extent(x.shape[2], R, stride, pad)
    return nhwc(F.forward(nchw(x), w, stride, pad, OH, OW, bias, nbias, nchw(addend), absolute))


def backward_data(dy, w, x_shape, stride, pad, addend=None, absolute=False):
    """dx[N][H][W][C] (x_shape = (N, H, W, C)) of dy[N][OH][OW][K]; input pixels no output reads get 0 (+ addend)."""
    N, H, W, C = x_shape
    return nhwc(F.backward_data(nchw(dy), w, (N, C, H, W), stride, pad, nchw(addend), absolute))


def backward_weight(x, dy, R, stride, pad, dw0=None, db0=None, absolute=False):
    """-> (dw[K][C][R][R] (+ dw0), db[K] = sum of dy (+ db0), dnb[N][K] = the sum over image n)."""
    dw = F.backward_weight(nchw(x), nchw(dy), R, stride, pad, dw0, absolute)
    dnb = (dy.abs() if absolute else dy).sum(dim=(1, 2))
    db = dnb.sum(dim=0)
    if db0 is not None:
        db = db + (db0.abs() if absolute else db0)
    return dw, db, dnb


def to_bf16_rne(t64):
    """A float64 tensor rounded to bf16 (8 significand bits), ties to even, as float64.  Normal range only."""
    m, e = torch.frexp(t64)                             # t = m 2^e, 0.5 <= |m| < 1
    return torch.ldexp(torch.round(m * 256.0), e - 8)   # torch.round: halves to even


def is_bf16_tie(t64):
    """Where a value lies exactly half way between two neighbouring bf16 numbers."""
    m, _ = torch.frexp(t64)
    s = m.abs() * 256.0
    return (s - s.floor()) == 0.5


# ------------------------------------------------------------------------------------------ inputs
def _gauss(shape, seed, exp0=0, exp1=0, bf16=True):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(tuple(shape), generator=g, dtype=torch.float32)
    if bf16:
        t = t.bfloat16().float()
    return F._scaled(t.double(), exp0, exp1)


def _sum_scales(n, exp):
    return float(F.scales(n, exp).sum())


def int_ranges(c, direction):
    """(a, p): activations are integers of [-a, a], parameters and epilogue terms of [-p, p]; the widest of the list
    whose worst-case sum of magnitudes, in units of the smallest element's unit, stays below 2^24."""
    RS = c.R * c.R
    pixels = c.N * max(c.OH, 1) * max(c.OW, 1)
    for a, p in ((3, 2), (2, 2), (2, 1), (1, 1)):
        if direction == "fwd":        # bias[k] joins every image: 2^14 units of the smallest
            worst = a * p * c.C * RS + p * 2 ** 14 + 2 * p
        elif direction == "dgrad":    # the terms of one sum carry w's channel scales: 1, 2^5, 2^10
            worst = a * p * RS * _sum_scales(c.K, CH_EXP) + p
        else:
            worst = a * a * pixels + p
        if worst < 2 ** 24:
            return a, p
    raise AssertionError("no integer range keeps %s %s exact" % (c.id, direction))


def inputs(c, direction, kind):
    """The tensors of one case and direction ("fwd", "dgrad", "wgrad"); kind "int" or "gauss".  `unit`: the scale of each
    element of the result, broadcastable to it (wgrad: of dw; `unit_k` of db and dnb)."""
    if kind == "int":
        a, p = int_ranges(c, direction)
        act = lambda shape, seed, e0=0, e1=0: F.integers(shape, -a, a, seed, e0, e1)
        par = lambda shape, seed, e0=0, e1=0: F.integers(shape, -p, p, seed, e0, e1)
        act16 = act
    else:
        act = act16 = lambda shape, seed, e0=0, e1=0: _gauss(shape, seed, e0, e1, True)
        par = lambda shape, seed, e0=0, e1=0: _gauss(shape, seed, e0, e1, False)
    N, H, W, C, K, R, OH, OW = c.N, c.H, c.W, c.C, c.K, c.R, c.OH, c.OW
    sn, sk, sc = F.scales(N, IMG_EXP), F.scales(K, CH_EXP), F.scales(C, IMG_EXP)
    w16 = lambda: (act16 if kind == "gauss" else par)((K, C, R, R), 2, CH_EXP)    # the kernels read a bf16 image of w
    if direction == "fwd":
        return SimpleNamespace(x=nhwc(act((N, C, H, W), 1, IMG_EXP)), w=w16(), bias=par((K,), 3, CH_EXP),
                               nbias=par((N, K), 4, IMG_EXP, CH_EXP),
                               addend=nhwc((act16 if kind == "gauss" else par)((N, K, OH, OW), 5, IMG_EXP, CH_EXP)),
                               unit=sn.view(N, 1, 1, 1) * sk.view(1, 1, 1, K))
    if direction == "dgrad":
        return SimpleNamespace(dy=nhwc(act((N, K, OH, OW), 6, IMG_EXP)), w=w16(),
                               addend=nhwc((act16 if kind == "gauss" else par)((N, C, H, W), 7, IMG_EXP)),
                               unit=sn.view(N, 1, 1, 1))
    assert direction == "wgrad"
    return SimpleNamespace(x=nhwc(act((N, C, H, W), 1, 0, IMG_EXP)), dy=nhwc(act((N, K, OH, OW), 6, 0, CH_EXP)),
                           dw0=par((K, C, R, R), 8, CH_EXP, IMG_EXP), db0=par((K,), 9, CH_EXP),
                           unit=sk.view(K, 1, 1, 1) * sc.view(1, C, 1, 1), unit_k=sk)


def packed(w):
    """The bf16 weight image both data kernels read: wp[K][R*R][C] of w[K][C][R][R]."""
    K, C, R, _ = w.shape
    return w.permute(0, 2, 3, 1).reshape(K, R * R, C).contiguous()


def impulse_points(H, W):
    """A corner, an edge and an interior pixel (the last two fall back on what a tiny extent has)."""
    return list(dict.fromkeys([(0, 0), (H - 1, W - 1), (0, W // 2), (H // 2, W // 3)]))


# ------------------------------------------------------------------------------------------ the shapes
# (N, H, W, C, K, R, stride, pad) and the route each direction is there for, with the queried workspace.  Forward and
# backward-data split their reduction of R*R*Cin/32 stages in s = min(768 / tiles, stages / 6, 16) parts of ceil(stages / s);
# the 128 x 256 tile <2,4,32> takes Kout % 256 == 0.  Backward-weight splits over 8 x 8 chunks of output pixels.
_ = None
CASES = [Case(*s) for s in [
    # M = 35 < one tile, Kout = 96 ends inside a tile; dgrad: 27 stages in 4 splits of 7, 7, 7, 6; one chunk: direct dw
    (1, 5, 7, 32, 96, 3, 1, 1, "igemm<2,2,32>/S1", "igemm<2,2,32,dgrad>/S4", "wgrad_tap<3,1>/S1"),
    # H W = 63 < 128: a pixel tile spans three images (nbias), ragged last tile; forward in the ragged 4 splits; N = 3
    (3, 9, 7, 96, 64, 3, 1, 1, "igemm<2,2,32>/S4", "igemm<2,2,32,dgrad>/S3", "wgrad_tap<3,1>/S6"),
    # 99 stages: the 16-split cap gives 15 splits of 7 (the last holds one stage); 12 chunks over 11 splits of 2: five idle
    (3, 9, 9, 352, 352, 3, 1, 1, "igemm<2,2,32>/S15", "igemm<2,2,32,dgrad>/S15", "wgrad_tap<3,1>/S11"),
    # the 128 x 256 tile, ragged last pixel tile (M = 162), forward and backward-data, split
    (2, 9, 9, 64, 256, 3, 1, 1, "igemm<2,4,32>/S3", "igemm<2,2,32,dgrad>/S12", "wgrad_tap<3,1>/S8"),
    (2, 9, 9, 256, 64, 3, 1, 1, "igemm<2,2,32>/S12", "igemm<2,4,32,dgrad>/S3", "wgrad_tap<3,1>/S8"),
    # ... M = 35 < one tile, unsplit; 1x1; one chunk on the 1x1 tap kernel
    (1, 5, 7, 256, 256, 1, 1, 0, "igemm<2,4,32>/S1", "igemm<2,4,32,dgrad>/S1", "wgrad_tap<1,1>/S1"),
    # a split 1x1: 12 stages in 2
    (2, 8, 8, 384, 64, 1, 1, 0, "igemm<2,2,32>/S2", "igemm<2,2,32,dgrad>/S1", "wgrad_tap<1,1>/S2"),
    # 3x3 at pad 0 and 2, stride 1, H != W
    (2, 9, 6, 32, 64, 3, 1, 0, "igemm<2,2,32>/S1", "igemm<2,2,32,dgrad>/S3", "wgrad_tap<3,1>/S2"),
    (2, 7, 9, 64, 32, 3, 1, 2, "igemm<2,2,32>/S3", "igemm<2,2,32,dgrad>/S1", "wgrad_tap<3,1>/S8"),
    # 3x3 stride 2 at pad 1, 0 and 2, odd and even extents (pad 0, W = 8: the last column is read by no output)
    (2, 9, 8, 64, 64, 3, 2, 1, "igemm<2,2,32>/S3", "igemm<2,2,32,dgrad>/S3", "wgrad_tap<3,2>/S2"),
    (2, 9, 8, 32, 96, 3, 2, 0, "igemm<2,2,32>/S1", "igemm<2,2,32,dgrad>/S4", "wgrad_tap<3,2>/S2"),
    (2, 8, 9, 64, 32, 3, 2, 2, "igemm<2,2,32>/S3", "igemm<2,2,32,dgrad>/S1", "wgrad_tap<3,2>/S2"),
    # 1x1 stride 2: backward-data writes zero (+ addend) at the three quarters of the input no output reads
    (3, 9, 8, 64, 96, 1, 2, 0, "igemm<2,2,32>/S1", "igemm<2,2,32,dgrad>/S1", "wgrad_tap<1,2>/S3"),
    # a 1x1-pixel image with pad 1; extents smaller than the filter at pad 1, pad 2 and stride 2
    (3, 1, 1, 64, 64, 3, 1, 1, "igemm<2,2,32>/S3", "igemm<2,2,32,dgrad>/S3", "wgrad_tap<3,1>/S3"),
    (2, 2, 1, 32, 32, 3, 1, 1, "igemm<2,2,32>/S1", "igemm<2,2,32,dgrad>/S1", "wgrad_tap<3,1>/S2"),
    (1, 1, 2, 32, 32, 3, 1, 2, "igemm<2,2,32>/S1", "igemm<2,2,32,dgrad>/S1", "wgrad_tap<3,1>/S1"),
    (2, 1, 2, 32, 32, 3, 2, 1, "igemm<2,2,32>/S1", "igemm<2,2,32,dgrad>/S1", "wgrad_tap<3,2>/S2"),
    # one chunk, N = 1: the stride-2 tap kernels add straight into dw
    (1, 9, 7, 64, 32, 3, 2, 1, "igemm<2,2,32>/S3", "igemm<2,2,32,dgrad>/S1", "wgrad_tap<3,2>/S1"),
    (1, 9, 8, 32, 64, 1, 2, 0, "igemm<2,2,32>/S1", "igemm<2,2,32,dgrad>/S1", "wgrad_tap<1,2>/S1"),
    # N = 1, OH = 10 and OW = 17 no multiples of 8: 2 x 3 ragged chunks
    (1, 10, 17, 32, 32, 3, 1, 1, "igemm<2,2,32>/S1", "igemm<2,2,32,dgrad>/S1", "wgrad_tap<3,1>/S6"),
    # the TN GEMM takes 1x1 stride-1 weight gradients from 1024 pixels on: with a split, and (256 tiles) without
    (1, 32, 32, 64, 64, 1, 1, 0, "igemm<2,2,32>/S1", "igemm<2,2,32,dgrad>/S1", "wgrad_tn<v2>/S4"),
    (1, 32, 32, 2048, 2048, 1, 1, 0, _, _, "wgrad_tn<v2>/S1"),
    # the ring forms of the default switch (1x1 only), C = 32, the fewest pixels ring_tile's thresholds admit
    # (ceil(M / 256) * K / 128 >= 128; ... * K / 64 >= 128 for K % 128 != 0; ceil(M / 128) * K / 128 >= 128), ragged last tile
    (3, 105, 104, 32, 128, 1, 1, 0, "ring<4,2,3>", _, _),
    (2, 74, 73, 32, 192, 1, 1, 0, "ring<4,1,3>", _, _),
    (1, 127, 129, 32, 128, 1, 1, 0, "ring<2,2,4>", _, _),
]]

# the same forms on 3x3 shapes (one with stride 2): reached only in a process started with SALUN_CONV_RING=3
RING3_CASES = [Case(*s) for s in [
    (3, 105, 104, 32, 128, 3, 1, 1, "ring<4,2,3>", _, _),
    (2, 74, 73, 32, 192, 3, 1, 1, "ring<4,1,3>", _, _),
    (1, 253, 257, 32, 128, 3, 2, 1, "ring<2,2,4>", _, _),
]]

# outside the domain, every direction: H < R - 2 pad (OH = 0 and OH < 0), pad = R, C or K = 16 or 48, R = 5, stride 3, N = 0
REFUSED = [(2, 2, 5, 32, 32, 3, 1, 0), (1, 1, 1, 32, 32, 3, 1, 0), (2, 8, 8, 32, 32, 3, 1, 3), (2, 8, 8, 32, 32, 1, 1, 1),
           (2, 8, 8, 16, 32, 3, 1, 1), (2, 8, 8, 48, 32, 3, 1, 1), (2, 8, 8, 32, 16, 1, 1, 0), (2, 8, 8, 32, 48, 3, 2, 1),
           (2, 8, 8, 64, 64, 5, 1, 2), (2, 8, 8, 32, 32, 3, 3, 1), (0, 8, 8, 32, 32, 3, 1, 1)]
# a backward-weight workspace one byte short is SALUN_ENOSPC: on the tap route and on the TN route
SHORT_WS = [(3, 9, 7, 96, 64, 3, 1, 1), (1, 32, 32, 64, 64, 1, 1, 0)]


# ------------------------------------------------------------------------------------------ the variants of a call
def data_ws_modes(shape, direction):
    """[(what, bytes the route query is asked about)] of a forward ("fwd") / backward-data ("dgrad") call: the queried
    workspace (the larger of the two directions' needs), NULL, and one byte short of what this direction's split needs (the
    last two only disable the split); where the direction does not split there is only the queried one and NULL."""
    import bf16_routes as M
    N, H, W, C, K, R, stride, pad = shape
    dws = M.data_workspace_bytes(shape)
    if direction == "fwd":
        need = M._igemm_split(N * out_extent(H, R, stride, pad) * out_extent(W, R, stride, pad), C, K, R)[2]
    else:
        need = M._igemm_split(N * H * W, K, C, R)[2]
    return [("queried", dws), ("null", 0)] + ([("short", need - 1)] if need else [])


FWD_TERMS = ((), ("bias",), ("nbias",), ("addend",), ("bias", "nbias", "addend"))
DGRAD_ADDEND = (None, "apart", "inplace")
# (accumulate, db, dnb, dw one float off a 16-byte boundary)
WGRAD_VARIANTS = [(False, False, False, False), (True, False, False, False), (False, True, False, False),
                  (True, True, False, False), (False, False, True, False), (False, True, True, False),
                  (True, True, True, False), (False, True, False, True), (True, False, True, True)]
