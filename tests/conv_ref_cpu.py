"""A float64 model of the fp32 convolution family (K8 / K8r: csrc/salun_conv.hip, csrc/salun_conv_ring.hip), the inputs
the exact-answer tests feed it, and the shapes they run.  Validated against torch's float64 convolution by
test_conv_ref_cpu.py; used by test_conv_exact_gpu.py.

The model is the definition, written out: a sum over the R x R taps of shifted, strided slices of the zero-padded
input, one matmul per tap.  NCHW activations, OIHW weights, R in {1, 3}, stride in {1, 2}; `pad` is the low-side
(top / left) padding and P, Q are given by the caller, as in the C-ABI, so the DDPM downsample (pad 0, P = H / 2, one
row and column of zeros on the high side) is expressible.  Every operation takes `absolute=True` to compute the same
sum over the absolute values of its inputs and epilogue terms: the quantity a rounding-error bound is a multiple of.

Two kinds of input, both seeded, both exactly representable in fp32:
  integers  small integers times powers of two.  Every product and every partial sum is then an integer multiple of
            one power of two and below 2^24 of them (test_conv_ref_cpu.py asserts that for every case), so fp32
            arithmetic is EXACT in every summation order, fused or not, split or not: the kernel's answer must equal
            the model's bit for bit, and a dropped, doubled or misplaced term cannot hide in a tolerance.
  gaussian  fp32 normal draws times the same powers of two, for the per-element bound gamma_(2n+e) * abs_sum.
The powers of two sit on the axes a reduction does NOT run over, so that every element of a result has one scale of
its own and the elements of one tensor span 2^24 between them: an error in a small-amplitude image or channel is as
visible as one in a large.  Forward and backward-data: image n of x / dy times 2^(-7 (n mod 3)), output channel k of w
times 2^(5 (k mod 3)) (backward-data reduces over k; its terms then span 2^10 and the cap is checked with that).
Backward-weight reduces over the images, so there the scales go on the channels: channel c of x times 2^(-7 (c mod 3)),
channel k of dy times 2^(5 (k mod 3)).  Epilogue terms carry the scale of the element they join (bias[k], shared by
all images, the scale of the largest: it is a whole multiple of the others)."""
from collections import namedtuple
from types import SimpleNamespace

import torch

U = 2.0 ** -24
IMG_EXP, CH_EXP = -7, 5


def bound_gamma(m):
    """Higham's gamma_m for fp32: the relative error bound of m roundings in a row."""
    return m * U / (1.0 - m * U)


class Case(namedtuple("Case", "N C H W K R stride pad")):
    __slots__ = ()

    @property
    def P(self):
        return self.H // 2 if (self.stride == 2 and self.pad == 0) else (self.H + 2 * self.pad - self.R) // self.stride + 1

    @property
    def Q(self):
        return self.W // 2 if (self.stride == 2 and self.pad == 0) else (self.W + 2 * self.pad - self.R) // self.stride + 1

    @property
    def id(self):
        return "x".join(map(str, self))


# ------------------------------------------------------------------------------------------ the model
def _a(t, absolute):
    return None if t is None else (t.abs() if absolute else t)


def _padded_shape(H, W, R, stride, pad, P, Q):
    return max(pad + H, (P - 1) * stride + R), max(pad + W, (Q - 1) * stride + R)


def _taps(R, stride, P, Q):
    for r in range(R):
        for s in range(R):
            yield r, s, slice(r, r + (P - 1) * stride + 1, stride), slice(s, s + (Q - 1) * stride + 1, stride)


def _pad(x, R, stride, pad, P, Q):
    N, C, H, W = x.shape
    xp = x.new_zeros((N, C) + _padded_shape(H, W, R, stride, pad, P, Q))
    xp[:, :, pad:pad + H, pad:pad + W] = x
    return xp


def epilogue(y, bias=None, nbias=None, addend=None):
    """((y + bias[k]) + nbias[n, k]) + addend, each term optional."""
    if bias is not None:
        y = y + bias[None, :, None, None]
    if nbias is not None:
        y = y + nbias[:, :, None, None]
    if addend is not None:
        y = y + addend
    return y


def forward(x, w, stride, pad, P, Q, bias=None, nbias=None, addend=None, absolute=False):
    """y[n,k,p,q] = sum_{c,r,s} x[n,c,p*stride-pad+r,q*stride-pad+s] w[k,c,r,s], then ((y + bias[k]) + nbias[n,k]) +
    addend[n,k,p,q] (the order of the reference's separate adds)."""
    x, w, bias, nbias, addend = (_a(t, absolute) for t in (x, w, bias, nbias, addend))
    N, K, R = x.shape[0], w.shape[0], w.shape[2]
    xp = _pad(x, R, stride, pad, P, Q)
    y = x.new_zeros((N, K, P * Q))
    for r, s, rows, cols in _taps(R, stride, P, Q):
        y += torch.matmul(w[:, :, r, s], xp[:, :, rows, cols].reshape(N, -1, P * Q))
    return epilogue(y.view(N, K, P, Q), bias, nbias, addend)


def backward_data(dy, w, x_shape, stride, pad, addend=None, absolute=False):
    """dx[n,c,h,w] = sum over the (k, r, s, p, q) whose forward term read x[n,c,h,w] of dy[n,k,p,q] w[k,c,r,s] (+ addend)."""
    dy, w, addend = (_a(t, absolute) for t in (dy, w, addend))
    N, C, H, W = x_shape
    K, R, P, Q = w.shape[0], w.shape[2], dy.shape[2], dy.shape[3]
    dxp = dy.new_zeros((N, C) + _padded_shape(H, W, R, stride, pad, P, Q))
    flat = dy.reshape(N, K, P * Q)
    for r, s, rows, cols in _taps(R, stride, P, Q):
        dxp[:, :, rows, cols] += torch.matmul(w[:, :, r, s].t(), flat).view(N, C, P, Q)
    dx = dxp[:, :, pad:pad + H, pad:pad + W].contiguous()
    return dx if addend is None else dx + addend


def backward_weight(x, dy, R, stride, pad, dw0=None, absolute=False):
    """dw[k,c,r,s] = sum_{n,p,q} dy[n,k,p,q] x[n,c,p*stride-pad+r,q*stride-pad+s] (+ dw0: `accumulate`)."""
    x, dy, dw0 = (_a(t, absolute) for t in (x, dy, dw0))
    N, C = x.shape[:2]
    K, P, Q = dy.shape[1:]
    xp = _pad(x, R, stride, pad, P, Q)
    dw = x.new_zeros((K, C, R, R))
    flat = dy.permute(1, 0, 2, 3).reshape(K, N * P * Q)
    for r, s, rows, cols in _taps(R, stride, P, Q):
        dw[:, :, r, s] = flat @ xp[:, :, rows, cols].permute(0, 2, 3, 1).reshape(N * P * Q, C)
    return dw if dw0 is None else dw + dw0


# ------------------------------------------------------------------------------------------ inputs
def scales(n, exp):
    return 2.0 ** (exp * (torch.arange(n) % 3)).double()


def _scaled(t, exp0, exp1):
    if exp0:
        t = t * scales(t.shape[0], exp0).view(-1, *[1] * (t.dim() - 1))
    if exp1:
        t = t * scales(t.shape[1], exp1).view(1, -1, *[1] * (t.dim() - 2))
    return t


def integers(shape, lo, hi, seed, exp0=0, exp1=0):
    """Integers of [lo, hi] as float64; entry i of axis 0 times 2^(exp0 (i mod 3)), entry j of axis 1 times 2^(exp1 (j mod 3))."""
    g = torch.Generator().manual_seed(seed)
    return _scaled(torch.randint(lo, hi + 1, tuple(shape), generator=g).double(), exp0, exp1)


def gaussian(shape, seed, exp0=0, exp1=0):
    """fp32 normal draws (held in float64) with the same power-of-two scales: exactly representable in fp32."""
    g = torch.Generator().manual_seed(seed)
    return _scaled(torch.randn(tuple(shape), generator=g, dtype=torch.float32).double(), exp0, exp1)


def inputs(c, direction, kind):
    """The tensors of one case and direction ("fwd", "dgrad", "wgrad"); kind "int" or "gauss".  `unit` is the scale of
    each element of the result (broadcastable to it): on integer inputs the exact answer is an integer times unit."""
    if kind == "int":
        act = lambda shape, seed, e0=0, e1=0: integers(shape, -3, 3, seed, e0, e1)
        par = lambda shape, seed, e0=0, e1=0: integers(shape, -2, 2, seed, e0, e1)
    else:
        act = par = lambda shape, seed, e0=0, e1=0: gaussian(shape, seed, e0, e1)
    N, C, H, W, K, R, P, Q = c.N, c.C, c.H, c.W, c.K, c.R, c.P, c.Q
    sn, sk, sc = scales(N, IMG_EXP), scales(K, CH_EXP), scales(C, IMG_EXP)
    if direction == "fwd":
        return SimpleNamespace(x=act((N, C, H, W), 1, IMG_EXP), w=par((K, C, R, R), 2, CH_EXP), bias=par((K,), 3, CH_EXP),
                               nbias=par((N, K), 4, IMG_EXP, CH_EXP), addend=par((N, K, P, Q), 5, IMG_EXP, CH_EXP),
                               unit=sn.view(N, 1, 1, 1) * sk.view(1, K, 1, 1))
    if direction == "dgrad":
        return SimpleNamespace(dy=act((N, K, P, Q), 6, IMG_EXP), w=par((K, C, R, R), 2, CH_EXP),
                               addend=par((N, C, H, W), 7, IMG_EXP), unit=sn.view(N, 1, 1, 1))
    assert direction == "wgrad"
    return SimpleNamespace(x=act((N, C, H, W), 1, 0, IMG_EXP), dy=act((N, K, P, Q), 6, 0, CH_EXP),
                           dw0=par((K, C, R, R), 8, CH_EXP, IMG_EXP), unit=sk.view(K, 1, 1, 1) * sc.view(1, C, 1, 1))


def impulses(shape):
    """Five tensors of `shape` [N, C, H, W], each a single 1 in the last image's last channel: at the four corners and
    at one interior point."""
    N, C, H, W = shape
    out = []
    for h, w in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 3)):
        t = torch.zeros(shape, dtype=torch.float64)
        t[N - 1, C - 1, h, w] = 1.0
        out.append(t)
    return out


# ------------------------------------------------------------------------------------------ the shapes
# (N, C, H, W, K, R, stride, pad); the route each was chosen for (conv_routes.py names what it actually gets; every
# case runs forward, backward-data and backward-weight wherever the library takes the shape)
CASES = [Case(*s) for s in [
    # plan_data: 64-pixel tile, unsplit, H != W
    (3, 8, 8, 16, 16, 3, 1, 1), (3, 8, 16, 8, 16, 3, 1, 1), (2, 8, 4, 32, 16, 3, 1, 1), (2, 8, 2, 64, 16, 3, 1, 1),
    # several images per tile, ragged N
    (5, 8, 2, 2, 8, 3, 1, 1), (5, 64, 4, 4, 64, 3, 1, 1), (3, 64, 8, 4, 16, 3, 1, 1),
    # reduction split S = 2 and S = 8; declined for HW % 4 != 0
    (2, 64, 8, 8, 64, 3, 1, 1), (2, 256, 4, 4, 16, 3, 1, 1), (5, 64, 2, 1, 16, 1, 1, 0),
    # slow staging: ragged reduction chunk, ragged / masked channel tile
    (8, 3, 32, 32, 64, 3, 1, 1), (2, 40, 16, 16, 72, 3, 1, 1), (5, 1, 16, 16, 40, 3, 1, 1), (4, 8, 32, 32, 3, 3, 1, 1),
    # 128-pixel tiles KT4 / KT2 / KT1, the 256-pixel PT = 2 form (and its ragged channel tile), 64-pixel KT2 WK2
    (24, 8, 32, 32, 130, 3, 1, 1), (48, 8, 32, 32, 40, 3, 1, 1), (48, 8, 32, 32, 24, 3, 1, 1),
    (128, 8, 32, 32, 64, 3, 1, 1), (128, 8, 32, 32, 40, 3, 1, 1), (12, 8, 32, 32, 130, 3, 1, 1), (64, 8, 3, 64, 130, 3, 1, 1),
    # 1x1: fast (chunk 32), 128-pixel tile, slow
    (3, 32, 8, 16, 40, 1, 1, 0), (24, 32, 32, 32, 130, 1, 1, 0), (3, 16, 8, 16, 40, 1, 1, 0),
    # stride-2 forward: 3x3 pad 1, 3x3 pad 0 with P = H / 2, 1x1, 128-pixel tile
    (3, 8, 16, 32, 24, 3, 2, 1), (3, 8, 16, 16, 24, 3, 2, 0), (3, 8, 16, 32, 24, 1, 2, 0), (24, 16, 64, 64, 130, 3, 2, 1),
    # stride-2 backward-data, merged kernel: 64-pixel KT1 at pad 1 and 0, 128-pixel KT2 and KT1, 64-pixel KT2 WK2, R = 1
    (4, 64, 16, 32, 16, 3, 2, 1), (4, 64, 16, 32, 16, 3, 2, 0), (32, 64, 64, 64, 8, 3, 2, 1), (32, 32, 64, 64, 8, 3, 2, 1),
    (86, 128, 12, 64, 8, 3, 2, 1), (4, 64, 16, 16, 16, 1, 2, 0),
    # ... per parity class: all four tap kernels at pad 1 and 0, the C = 3 stem, R = 1 (three classes empty), PSZ > 256
    (3, 24, 8, 16, 12, 3, 2, 1), (3, 24, 8, 16, 12, 3, 2, 0), (8, 3, 32, 32, 64, 3, 2, 1), (3, 24, 8, 16, 12, 1, 2, 0),
    (1, 8, 2, 256, 8, 3, 2, 1),
    # backward-weight: 1x1 stride 2, generic C < 32 at stride 2, small-C R = 3 and R = 1
    (3, 32, 16, 16, 40, 1, 2, 0), (3, 16, 16, 16, 40, 1, 2, 0), (3, 3, 8, 16, 40, 3, 1, 1), (3, 4, 8, 16, 40, 1, 1, 0),
    (3, 4, 16, 16, 40, 1, 2, 0),
    # ... the ring kernel at W = 4, 8, 16, 32 (flagged SALUN_WGRAD_SHARED: conv_wgrad_v<1, 6 / 5 / 6 / 8>), H != W
    (5, 64, 4, 4, 96, 3, 1, 1), (3, 64, 8, 8, 32, 3, 1, 1), (2, 64, 16, 16, 32, 3, 1, 1), (1, 64, 32, 32, 32, 3, 1, 1),
    (3, 64, 8, 16, 40, 3, 1, 1),
    # ... conv_wgrad_v<2, 9 / 10>, the generic kernel with full and ragged channel tiles
    (4, 64, 16, 16, 40, 3, 2, 1), (4, 64, 8, 8, 40, 3, 2, 1), (2, 64, 32, 32, 40, 3, 2, 1), (2, 64, 2, 64, 16, 3, 1, 1),
    (2, 40, 16, 16, 72, 3, 2, 1),
]]

# the ring kernels, 3x3 / stride 1 / pad 1: (N, Cred, H, W, Kout), each at every tile cfg 1..5 whose domain holds it
RING_CASES = [
    (5, 8, 4, 4, 8), (9, 8, 8, 4, 40), (3, 16, 16, 4, 40), (2, 8, 64, 4, 64),   # W = 4: up to 16 images per tile, ragged
    (3, 8, 1, 32, 8), (3, 64, 8, 8, 64), (5, 8, 4, 8, 40), (2, 16, 16, 8, 72), (2, 8, 32, 8, 8),
    (2, 40, 16, 16, 72), (3, 8, 8, 16, 64), (5, 16, 4, 16, 40), (3, 8, 1, 16, 8),
    (2, 8, 32, 32, 40), (3, 16, 8, 32, 64), (5, 8, 2, 32, 8), (3, 8, 4, 32, 130),
    (64, 8, 32, 32, 64),                                            # more tiles than the persistent grid at cfg 3
]
