"""A float64 model of the normalisation kernels (csrc/salun_norm.hip: fused BatchNorm (+residual) (+ReLU) and fp32
GroupNorm (+SiLU) with the fused backward; csrc/salun_norm_bf16.hip, K12: GroupNorm on bf16 NHWC), the inputs the
exact-answer tests feed them, the per-element error bounds, the shapes, and a Python mirror of the host logic that picks
a route.  Validated against torch's float64 ops by test_norm_ref_cpu.py; used by test_norm_exact_gpu.py.

THE MODEL is the definition, written out.  Every backward is a function of what the backward kernel is given (dy, the
saved y, x, the saved statistics), so each entry point is compared on its own inputs.  `absolute=True` returns, field
for field, the sums of the absolute values of the terms: what a rounding bound is a multiple of.

EXACT INPUTS (seeded, all fp32 numbers).  Within one reduction set (BN: a channel over N*HW; GN: an (image, group)) the
deviations from a centre m are built from blocks of sum 0 and equal mean square 4 s^2: {-2s, +2s}, and where the set's
size is a multiple of 8 also {-4s, 0 x 6, +4s}, shuffled over the set.  s is a power of two and m a small integer times
s; both differ from one set to the next, so a statistic taken from a neighbouring slice or group is another number.
Then mean = m and var = 4 s^2 in every summation order; with eps = 0, var + eps is a power of four and invstd = 1/(2s).
The "eps" family has s = 1/4 everywhere and eps = 0.75 (var + eps = 1): a dropped eps gives invstd = 2.  A set of odd
size (K12 only: cpg * HW = 105, 27) takes three-point blocks {2s, 2s, -4s}, mean square 8 s^2, with s = 1/4 and
eps = 0.5.  gamma, beta, dy, the residual and the addend are small integers times per-channel powers of two.  With
these mean, var, invstd, xhat in {0, +-1, +-2}, a = invstd * gamma, b = beta - mean * a and y are exact in fp32, fused
or not; the backward sums are exact, and dx is exact where the divisor (N*HW; cpg*HW) is a power of two.  For other
divisors there is the "vanishing" family: dy is +v / -v on pairs of positions of one channel with the same xhat and the
same ReLU branch, so sum dz = sum dz * xhat = 0 per set and dx = gamma * invstd * dz.  The premise (every partial sum
below 2^24 units) is asserted case by case in test_norm_ref_cpu.py.

GAUSSIAN INPUTS: fp32 normal draws with the amplitudes 2^(5 (c mod 3)) per channel and 2^(-7 (n mod 3)) per image, each
only on an axis the statistic does not run over: BN reduces over the images, so its x, dy, residual carry the channel
amplitude only; GN (fp32 and K12) reduces over the channels of a group, so x, dz, addend carry the image amplitude and
an amplitude 2^(5 (g mod 3)) per group.  A centre offset mu / sigma in {0, 2^4, 2^8} is added before scaling; at 2^8
the forward bound reaches a few per cent of sigma (kappa u), so the ReLU variants run at 0 and 2^4 (RELU_OFFSETS) and
2^8 runs without ReLU: the offset is there for the statistics.  SiLU is not homogeneous: the SiLU cases keep gamma and beta of order one (|y| < 80, asserted).

PER-ELEMENT BOUNDS, from the rounding points of the kernels as written (u = 2^-24, gamma_k = k u / (1 - k u); the
kernels are compiled without contraction, and a fused multiply-add only removes a rounding).
  statistics.  A lane adds the four values of a float4 as a tree (2 roundings) into an fp32 accumulator that is folded
  into fp64 every 8 (BN) or 16 (GN re-read mode) items, or after all ITEMS (GN cached): a value passes through at most
  c1 = 2 + 8 (BN) / 2 + max(ITEMS, 16 for re-read) (GN) roundings, its square through one more.  K12: ceil(rows / 8)
  adds per pixel lane plus 7 for the eight lanes.  The fp64 folds, the division and the subtraction add F64 = (M + 16)
  2^-53 relative to the absolute sums.  So with A1 = sum |x|, A2 = sum x^2:
      d_mu  = (gamma_c1 + F64) A1 / M                                  (then one rounding of mean to fp32: + u |mu|)
      d_var = (gamma_(c1+1) + F64) A2 / M + (2 |mu| + d_mu) d_mu       (A2 / M = mu^2 + sigma^2: this carries kappa)
      d_is  = d_var / (2 (max(var - d_var, 0) + eps)^1.5) + u (invstd + that)
  (clamping a negative computed variance to 0 moves it towards the truth).
  forward element.  a = fl(invstd * gamma), b = fl(beta - fl(mean * a)), y = fl(fl(x * a) + b), then fl(y + res): the
  term mean * a passes through 5 roundings, x * a through 4.  With A = |gamma| (invstd + d_is), MU = |mu| + d_mu + u |mu|:
      bound(y) = |gamma| (|x - mu| d_is + (invstd + d_is) (d_mu + u |mu|))           statistics part
               + gamma_5 (|x| A + MU A + |beta| + |res|)                             rounding part
  ReLU is 1-Lipschitz and adds nothing.  SiLU: z = y / (1 + E) or y * (1 / (1 + E)) with E = exp(-y) of relative error
  EXP_ULP u (see the constants): relative (EXP_ULP + 3) u on silu(y^), and |silu'| <= 1.1 carries bound(y) through.
  K12 rounds the result to bf16: + U16 (|value| + bound).
  backward, given the saved fp32 statistics: xhat^ = fl(fl(x - mean) * invstd) (2 roundings), a product dz * xhat one
  more, then the same chains, then one rounding to fp32: d_dbeta = (gamma_(c1+1) + F64) sum |dz|,
  d_dgamma = (gamma_(c1+4) + F64) sum |dz xhat|.  BN: inv_m = fl(1 / M), kb = fl(dbeta * inv_m), kg likewise (2
  roundings each), dx = fl(gi * fl(dz - fl(kb + fl(xhat^ * kg)))) with gi = fl(gamma * invstd):
      bound(dx) = |gamma invstd| (d_kb + |xhat| d_kg + gamma_3 |xhat| KG + gamma_4 (|dz| + KB + (1 + gamma_3) |xhat| KG))
  with d_kb = (d_dbeta + gamma_2 (|dbeta| + d_dbeta)) / M, KB = |dbeta| / M + d_kb, and the same for kg.  Eval mode:
  gamma_2 |gamma invstd dz|.  dres = dz exactly.  `acc += v`: d_v + u (|acc| + |v| + d_v).
  GN backward: per-(image, channel) sums in fp32 over a float4 tree (2), a butterfly over r lanes (log2 r) and the
  fold of the channel's segments (segs_per_ch): cs = 2 + log2 r + segs_per_ch roundings; the fold over the images runs
  in fp64.  The group means ma, mb: one product by gamma, cpg sequential adds by one lane, one division by L.  dx =
  fl(rstd * fl(fl(fl(dy * gamma) - ma) - fl(xhat^ * mb))) (+ addend): at most 6 roundings on a term.  nk = sum_hw dx:
  the elements' own bounds plus gamma_cs on their magnitudes; csum folds nk in fp64.  With SiLU, dy = dz * f(y^),
  f = s (1 + y (1 - s)): |f| <= 1.1, |f'| <= 0.5, and counting the roundings of s, 1 - s, the two products and the sum
  gives |f^ - f(y^)| <= (2 EXP_ULP + 8) (1 + |y|) u.
No constant is fitted to what the kernels produce, there is no absolute slack and nothing is scaled by a tensor's
maximum.

RELU EDGE.  An element whose pre-activation lies within its own forward bound of 0 may take either branch in the
forward; both satisfy the forward bound.  The backward kernels read the branch from the saved y, so the backward model
is evaluated on the y the forward wrote: the gradient of such an element is not masked, it is checked against the
model of the branch taken, and the branch taken must be the model's everywhere else.  relu_edge_share() is capped at 1 %.
"""
import math
from collections import namedtuple
from types import SimpleNamespace as NS

import torch

from attn_ref_cpu import bf16_round  # noqa: F401  (re-exported: one RNE rounding of a float64 value to bf16)

F64 = torch.float64
U = 2.0 ** -24
U16 = 2.0 ** -8            # unit roundoff of bf16 (8 significant bits)
MOMENTUM = 0.25
IMG_EXP, CH_EXP = -7, 5
# Relative error of exp, in units of u (1 ulp <= 2 u).  expf (k_gn_fwd / k_gn_bwd) is OCML's __ocml_exp_f32: 1 ulp
# (HIP math API reference, "Single precision mathematical functions": expf, maximum ULP error 1).  __expf (K12) is the
# native path v_exp_f32(fl(x * log2 e)): the instruction is good to 1 ulp (CDNA ISA guide, V_EXP_F32) and the rounded
# argument adds 2 u |x log2 e| ln 2 = 2 u |x|; with |y| < 80 asserted for the SiLU cases that is 2 + 160.
EXP_ULP = {"expf": 2.0, "__expf": 162.0}
SILU_SLOPE, SILU_CURV = 1.1, 0.5            # max |silu'| = 1.0998, max |silu''| = 0.5


def gam(k):
    return k * U / (1.0 - k * U)


def f64_term(M):
    return (M + 16) * 2.0 ** -53


# ================================================================================================ the model
def _relu_mask(y):
    return (y > 0).to(F64)


def bn_forward(x, gamma, beta, res=None, relu=False, train=True, running_mean=None, running_var=None, nbt=None,
               momentum=MOMENTUM, eps=0.0, absolute=False):
    """torch.nn.BatchNorm2d (+ res) (+ ReLU).  -> y, pre (before the ReLU), mean, invstd (the saved statistics), var,
    and in train mode the updated running_mean / running_var (unbiased) / nbt (None where not given).
    absolute: mean = sum |x| / M, var = sum x^2 / M, y = |a x| + |mean a| + |beta| + |res|."""
    N, C, H, W = x.shape
    M = N * H * W
    v = lambda t: t.view(1, C, 1, 1)
    o = NS(running_mean=running_mean, running_var=running_var, nbt=nbt)
    if train:
        mean = x.mean((0, 2, 3))
        var = (x - v(mean)).pow(2).mean((0, 2, 3))
        if running_mean is not None:
            o.running_mean = (1 - momentum) * running_mean + momentum * mean
            o.running_var = (1 - momentum) * running_var + momentum * (var * M / (M - 1) if M > 1 else var)
        if nbt is not None:
            o.nbt = nbt + 1
    else:
        mean, var = running_mean, running_var
    invstd = 1.0 / torch.sqrt(var + eps)
    a = invstd * gamma
    if absolute:
        o.mean, o.var = x.abs().mean((0, 2, 3)), x.pow(2).mean((0, 2, 3))
        o.y = x.abs() * v(a.abs()) + v((mean * a).abs() + beta.abs()) + (0 if res is None else res.abs())
        return o
    pre = x * v(a) + v(beta - mean * a)
    if res is not None:
        pre = pre + res
    o.pre, o.y, o.mean, o.var, o.invstd = pre, (pre.clamp_min(0) if relu else pre), mean, var, invstd
    return o


def bn_backward(dy, y, x, gamma, mean, invstd, train=True, relu=False, dres=False, gacc=None, bacc=None, absolute=False):
    """dz = dy [y > 0]; dbeta = sum dz; dgamma = sum dz xhat; dx = gamma invstd (dz - (dbeta + xhat dgamma) / M) in
    train mode, gamma invstd dz in eval mode; dres = dz; gacc / bacc += dgamma / dbeta."""
    N, C, H, W = x.shape
    M = N * H * W
    v = lambda t: t.view(1, C, 1, 1)
    dz = dy * _relu_mask(y) if relu else dy
    xh = (x - v(mean)) * v(invstd)
    if absolute:
        dz, xh = dz.abs(), xh.abs()
    dbeta, dgamma = dz.sum((0, 2, 3)), (dz * xh).sum((0, 2, 3))
    gi = gamma * invstd
    if absolute:
        dx = v(gi.abs()) * (dz + (v(dbeta) + xh * v(dgamma)) / M) if train else v(gi.abs()) * dz
    else:
        dx = v(gi) * (dz - (v(dbeta) + xh * v(dgamma)) / M) if train else v(gi) * dz
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    return NS(dx=dx, dres=dz if dres else None, dgamma=dgamma, dbeta=dbeta, dz=dz, xh=xh,
              gacc=None if gacc is None else f(gacc) + dgamma, bacc=None if bacc is None else f(bacc) + dbeta)


def sigmoid(y):
    return torch.sigmoid(y)


def _grp(t, G):
    N, C = t.shape[:2]
    return t.reshape(N, G, -1)


def gn_forward(x, gamma, beta, G, eps=0.0, silu=False, absolute=False):
    """GroupNorm over (C / G) * HW per (image, group) (biased variance), affine, optional SiLU.  -> y, pre, mean, rstd,
    var ([N, G]).  absolute: mean = sum |x| / L, var = sum x^2 / L, y = |a x| + |mean a| + |beta|."""
    N, C, H, W = x.shape
    cpg = C // G
    xg = _grp(x, G)
    mean = xg.mean(2)
    var = (xg - mean[:, :, None]).pow(2).mean(2)
    rstd = 1.0 / torch.sqrt(var + eps)
    ch = lambda t: t.repeat_interleave(cpg, 1).view(N, C, 1, 1)          # [N, G] -> per channel
    a = ch(rstd) * gamma.view(1, C, 1, 1)
    if absolute:
        return NS(mean=xg.abs().mean(2), var=xg.pow(2).mean(2),
                  y=x.abs() * a.abs() + (ch(mean) * a).abs() + beta.abs().view(1, C, 1, 1))
    pre = x * a + (beta.view(1, C, 1, 1) - ch(mean) * a)
    return NS(pre=pre, y=pre * sigmoid(pre) if silu else pre, mean=mean, var=var, rstd=rstd)


def silu_grad(y):
    s = sigmoid(y)
    return s * (1 + y * (1 - s))


def gn_backward(dz, x, gamma, beta, mean, rstd, G, silu=False, addend=None, csum_acc=None, gacc=None, bacc=None,
                absolute=False):
    """Given the saved mean / rstd [N, G]: dy = dz silu'(y) (y recomputed); dgamma = sum_{n,hw} dy xhat, dbeta = sum dy;
    dx = rstd (dy gamma - ma - xhat mb) (+ addend), ma / mb the group means of dy gamma and dy gamma xhat;
    nk[n, c] = sum_hw dx; csum = sum_n nk; *_acc += .  Also dy, xh, ma, mb for the bounds."""
    N, C, H, W = x.shape
    cpg, L = C // G, (C // G) * H * W
    ch = lambda t: t.repeat_interleave(cpg, 1).view(N, C, 1, 1)
    gv = gamma.view(1, C, 1, 1)
    xh = (x - ch(mean)) * ch(rstd)
    dy = dz * silu_grad(xh * gv + beta.view(1, C, 1, 1)) if silu else dz
    if absolute:
        dy, xh, gv = dy.abs(), xh.abs(), gv.abs()
    ma, mb = _grp(dy * gv, G).sum(2) / L, _grp(dy * gv * xh, G).sum(2) / L
    if absolute:
        dx = ch(rstd) * (dy * gv + ch(ma) + xh * ch(mb)) + (0 if addend is None else addend.abs())
    else:
        dx = ch(rstd) * (dy * gv - ch(ma) - xh * ch(mb)) + (0 if addend is None else addend)
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    dgamma, dbeta, nk = (dy * xh).sum((0, 2, 3)), dy.sum((0, 2, 3)), dx.sum((2, 3))
    return NS(dx=dx, dgamma=dgamma, dbeta=dbeta, nk=nk, csum=nk.sum(0), dy=dy, xh=xh, ma=ma, mb=mb,
              csum_acc=None if csum_acc is None else f(csum_acc) + nk.sum(0),
              gacc=None if gacc is None else f(gacc) + dgamma, bacc=None if bacc is None else f(bacc) + dbeta)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def gn16_forward(x, gamma, beta, G, eps=0.0, silu=False):
    """K12 on the logical NCHW tensor x (bf16-exact values): mr [N, G, 2] = (mean, rstd), ab [N, C, 2] = (gamma rstd,
    beta - mean gamma rstd), y64 the float64 answer and y = one RNE rounding of it to bf16."""
    N, C = x.shape[:2]
    o = gn_forward(x, gamma, beta, G, eps, silu)
    a = o.rstd.repeat_interleave(C // G, 1) * gamma
    o.mr = torch.stack((o.mean, o.rstd), 2)
    o.ab = torch.stack((a, beta - o.mean.repeat_interleave(C // G, 1) * a), 2)
    o.y64, o.y = o.y, bf16_round(o.y)
    return o


def gn16_backward(dy, x, gamma, mr, ab, G, silu=False, dgamma0=None, dbeta0=None):
    """K12 backward given the forward's mr / ab; z for SiLU is ab[..., 0] x + ab[..., 1].  dgamma0 / dbeta0: `accumulate`."""
    N, C = x.shape[:2]
    z = ab[:, :, 0].view(N, C, 1, 1) * x + ab[:, :, 1].view(N, C, 1, 1)
    d = dy * silu_grad(z) if silu else dy
    o = gn_backward(d, x, gamma, gamma * 0, mr[:, :, 0], mr[:, :, 1], G)
    o.z, o.dx64, o.dx = z, o.dx, bf16_round(o.dx)
    if dgamma0 is not None:
        o.dgamma, o.dbeta = o.dgamma + dgamma0, o.dbeta + dbeta0
    return o


# ================================================================================================ mirror of the host logic
BN_MAX_SPLIT, GN_ITEMS, GN_MAX_SEG, GN_CHUNKS_MAX = 64, 16, 1024, 64


def bn_nsplit(N, C):
    return max(1, min((1024 + C - 1) // C, N, BN_MAX_SPLIT))


def bn_ok(N, C, HW):
    return N >= 1 and C >= 1 and HW >= 4 and HW % 4 == 0


def bn_ws_bytes(C):
    return 8 * 2 * max(C, 0) * BN_MAX_SPLIT


def bn_slices(N, C):
    ns = bn_nsplit(N, C)
    return [(N * s // ns, N * (s + 1) // ns) for s in range(ns)]


def bn_walk(N, C, H, W):
    """BnWalk as the kernels run it, over the largest batch slice: -> (wraps, wraps with i + di == hw4 exactly, wraps
    after dn = 0) counted over every lane's `next()` whose result an iteration uses."""
    hw4 = H * W // 4
    work = max(hi - lo for lo, hi in bn_slices(N, C)) * hw4
    dn = 256 // hw4
    di = 256 - dn * hw4
    wraps = equal = 0
    for t in range(min(256, work)):
        n, i, e = t // hw4, t % hw4, t
        while e + 256 < work:                  # the loop's `e += 256, wk.next()` before an iteration that runs
            e, n, i = e + 256, n + dn, i + di
            if i >= hw4:
                wraps, equal, i, n = wraps + 1, equal + (i == hw4), i - hw4, n + 1
            assert (n, i) == (e // hw4, e % hw4)
    return wraps, equal, wraps if dn == 0 else 0


def bn_routes(N, C, H, W):
    hw4, ns = H * W // 4, bn_nsplit(N, C)
    sizes = [hi - lo for lo, hi in bn_slices(N, C)]
    r = set()
    wraps, equal, wraps0 = bn_walk(N, C, H, W)
    if wraps and hw4 < 256:
        r.add("walk wraps, di != 0, hw4 < 256")
    if equal:
        r.add("walk wraps with i + di == hw4")
    if wraps0:
        r.add("walk wraps, dn = 0")
    r.add("hw4=1" if hw4 == 1 else "hw4=256" if hw4 == 256 else "hw4>256,%256!=0" if hw4 > 256 and hw4 % 256 else
          "hw4<256,npo2" if hw4 < 256 and hw4 & (hw4 - 1) else "hw4 other")
    if H != W:
        r.add("H!=W")
    if ns == 1:
        r.add("nsplit=1")
    if ns == N < 64 and max(sizes) * hw4 < 256:
        r.add("nsplit=N<64,work<256")
    if ns == 64 and len(set(sizes)) > 1:
        r.add("nsplit=64,uneven")
    if N > 64 and ns == 64:
        r.add("N>64")
    if (max(sizes) * hw4 + 255) // 256 >= 8:
        r.add("fp64 flush")
    return r


def gn_items(C, HW, G):
    nvec = (C // G) * HW // 4
    for it in (1, 2, 4, 8, 16):
        if nvec <= it * 256:
            return it
    return 0


def gn_r(HW):
    return min(HW // 4, 64)


def gn_shape_ok(N, C, HW, G):
    if N < 1 or C < 1 or G < 1 or C % G or HW < 4 or HW & (HW - 1):
        return False
    cpg = C // G
    return cpg <= 256 and cpg * (HW // 4) // gn_r(HW) <= GN_MAX_SEG and cpg * HW < 1 << 30


def gn_ws_bytes(N, C):
    return 4 * 2 * max(N, 0) * max(C, 0)


def gn_routes(N, C, H, W, G):
    HW, cpg = H * W, C // G
    nvec, r = cpg * HW // 4, gn_r(HW)
    out = {f"ITEMS={gn_items(C, HW, G)}@G{'=32' if G == 32 else '!=32'}", f"r={r}", f"hw4={HW // 4}"}
    if cpg == 256:
        out.add("cpg=256")
    if cpg in (1, 3, 10, 60):
        out.add(f"cpg={cpg}")
    if HW // 4 // r > 1:
        out.add("segs_per_ch>1")
    if nvec % 256:
        out.add("padding round")
    if cpg & (cpg - 1) and HW // 4 < 64:
        out.add("cpg npo2, small hw4")
    return out


def gn16_ok(N, C, HW, G):
    return N >= 1 and HW >= 1 and G >= 1 and C % 8 == 0 and C % G == 0 and C >= 8


def gn_chunks(HW):
    return max(1, min((HW + 31) // 32, GN_CHUNKS_MAX))


def rows_per_chunk(HW):
    return -(-HW // gn_chunks(HW))


def gn16_ws_bytes(N, C, HW, G):
    return (N * gn_chunks(HW) * C * 2 + N * G * 2) * 4 if gn16_ok(N, C, HW, G) else 0


def gn16_routes(N, C, H, W, G):
    HW, cpg = H * W, C // G
    ch, rpc = gn_chunks(HW), rows_per_chunk(HW)
    out = set()
    if HW % rpc:
        out.add("ragged chunk")
    if (ch - 1) * rpc >= HW:
        out.add("empty trailing chunk")
    if HW == 1:
        out.add("HW=1")
    if ch == 64 and HW == 64 * rpc:
        out.add("64 full chunks")
    if (C // 8) % 32:
        out.add("C/8 % 32 != 0")
    if C // 8 > 32:
        out.add("two channel blocks")
    if 8 % cpg and cpg % 8:
        out.add(f"group straddles an octet, cpg={cpg}")
    if (cpg * HW) & (cpg * HW - 1):
        out.add("divisor npo2")
    return out


# ================================================================================================ the shapes
BnCase = namedtuple("BnCase", "N C H W why")
GnCase = namedtuple("GnCase", "N C H W G why")
_cid = lambda c: "x".join(map(str, c[:-1]))

BN_CASES = [BnCase(*s) for s in [
    (3, 8, 2, 2, "hw4 = 1"),
    (5, 16, 6, 6, "hw4 = 9"), (2, 32, 14, 14, "hw4 = 49"), (3, 8, 6, 10, "hw4 = 15, H != W"),
    (2, 8, 32, 32, "hw4 = 256: dn = 1, di = 0"),
    (2, 8, 34, 32, "hw4 = 272 > 256: dn = 0"),
    (4, 1024, 2, 2, "nsplit = 1"),
    (7, 64, 2, 2, "nsplit = N < 64, fewer than 256 items"),
    (65, 8, 2, 2, "nsplit = 64, slices of 1 and 2 images"), (100, 16, 2, 2, "nsplit = 64, slices of 1 and 2 images"),
    (32, 1024, 6, 6, "hw4 = 9, 288 items: lanes take a second iteration, di = 4, the walk wraps, i + di == hw4 included"),
    (4, 512, 34, 32, "hw4 = 272, two images per slice: dn = 0 and the walk wraps, i + 256 == hw4 included"),
]]
BN_BIG = BnCase(8, 1024, 32, 32, "8 iterations per lane: the fp64 flush inside the loop")
BN_REQUIRED = ["hw4=1", "hw4<256,npo2", "hw4=256", "hw4>256,%256!=0", "H!=W", "nsplit=1", "nsplit=N<64,work<256",
               "nsplit=64,uneven", "N>64", "fp64 flush", "walk wraps, di != 0, hw4 < 256", "walk wraps with i + di == hw4",
               "walk wraps, dn = 0"]
BN_OUTSIDE = (2, 8, 7, 7)                     # HW = 49

GN_CASES = [GnCase(*s) for s in [
    (2, 64, 2, 2, 32, "ITEMS 1, hw4 = 1, r = 1, nvec = 2"),
    (2, 64, 16, 32, 32, "ITEMS 1 full: nvec = 256"),
    (2, 128, 16, 16, 32, "ITEMS 1, hw4 = 64, cpg = 4"),
    (2, 128, 16, 32, 32, "ITEMS 2, hw4 = 128, segs_per_ch = 2"),
    (2, 256, 16, 32, 32, "ITEMS 4"),
    (1, 256, 32, 32, 32, "ITEMS 8, hw4 = 256"),
    (1, 512, 32, 32, 32, "ITEMS 16"),
    (1, 256, 64, 64, 32, "re-read mode at G = 32, hw4 = 1024"),
    (2, 8, 64, 64, 1, "re-read mode at its smallest"),
    (3, 24, 4, 8, 8, "ITEMS 1 at G = 8, cpg = 3, hw4 = 8: cpg npo2 with r = 8, padding"),
    (2, 20, 32, 32, 2, "ITEMS 16 at G = 2, cpg = 10, hw4 = 256: padding rounds"),
    (2, 12, 16, 32, 4, "ITEMS 2 at G = 4, cpg = 3: 384 float4, second round half empty"),
    (2, 24, 16, 32, 4, "ITEMS 4 at G = 4, cpg = 6"),
    (2, 12, 32, 32, 2, "ITEMS 8 at G = 2, cpg = 6, hw4 = 256"),
    (2, 256, 2, 2, 1, "cpg = 256: every lane owns a channel"), (2, 512, 4, 4, 2, "cpg = 256, hw4 = 4"),
    (3, 5, 2, 4, 5, "cpg = 1, hw4 = 2, r = 2"),
    (2, 120, 4, 4, 2, "cpg = 60, hw4 = 4"),
    (2, 30, 8, 4, 3, "cpg = 10, hw4 = 8"),
    (2, 6, 8, 8, 2, "cpg = 3, hw4 = 16"), (2, 6, 8, 16, 2, "cpg = 3, hw4 = 32"),
]]
GN_REQUIRED = [f"ITEMS={i}@G{g}" for i in (1, 2, 4, 8, 16, 0) for g in ("=32", "!=32")] + \
              ["cpg=256", "cpg=1", "cpg=3", "cpg=10", "cpg=60", "segs_per_ch>1", "padding round", "cpg npo2, small hw4"] + \
              [f"hw4={h}" for h in (1, 2, 8, 64, 256, 1024)] + [f"r={r}" for r in (1, 2, 4, 8, 16, 32, 64)]
GN_EXTRA = [("addend",), ("nk",), ("addend", "nk"), ("nk", "csum"), ("nk", "csum_acc"), ("addend", "nk", "csum", "csum_acc")]
GN_OUTSIDE = [(2, 8, 6, 6, 2, "HW = 36"), (1, 257, 2, 2, 1, "cpg = 257")]

GN16_CASES = [GnCase(*s) for s in [
    (2, 64, 1, 1, 32, "HW = 1"), (3, 96, 5, 7, 32, "cpg = 3, HW = 35: ragged chunk, odd set"),
    (1, 24, 3, 3, 8, "cpg = 3, HW = 9, odd set"), (2, 320, 4, 4, 32, "cpg = 10, two channel blocks"),
    (1, 8, 1, 2113, 1, "64 chunks of 34 rows: the last starts past the end"),
    (1, 8, 32, 64, 1, "HW = 2048: 64 full chunks"), (1, 264, 4, 4, 33, "C / 8 = 33"),
    (2, 40, 2, 4, 2, "cpg = 20"),
]]
GN16_REQUIRED = ["ragged chunk", "empty trailing chunk", "HW=1", "64 full chunks", "C/8 % 32 != 0", "two channel blocks",
                 "group straddles an octet, cpg=3", "group straddles an octet, cpg=10", "group straddles an octet, cpg=20",
                 "divisor npo2"]


# ================================================================================================ inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, lo, hi, seed, nonzero=False):
    t = torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).double()
    return torch.where(t == 0, torch.ones_like(t), t) if nonzero else t


def set_scale(S, family):
    """(s, m) of S reduction sets: s cycles through 1/4, 1/2, 1 (1/4 everywhere in the eps families), m in -3 s .. 3 s."""
    i = torch.arange(S)
    s = 2.0 ** ((i % 3) - 2).double() if family == "eps0" else torch.full((S,), 0.25, dtype=F64)
    return s, (((i * 5 + 1) % 7) - 3).double() * s


def block_sets(S, L, seed):
    """[S, L] deviations in units of s: blocks of sum 0 and equal mean square, shuffled within each set."""
    if L % 2:
        assert L % 3 == 0
        base = torch.tensor([2.0, 2.0, -4.0], dtype=F64).repeat(L // 3)
    else:
        base = torch.tensor([-2.0, 2.0], dtype=F64).repeat(L // 2)
        if L % 8 == 0:
            k = L // 16 * 8                                     # half of the octets take the eight-point block
            base[:k] = torch.tensor([-4.0, 0, 0, 0, 0, 0, 0, 4.0], dtype=F64).repeat(k // 8)
    perm = torch.rand(S, L, generator=_gen(seed)).argsort(1)
    return base[perm]


def eps_of(family, L):
    return 0.0 if family == "eps0" else 0.5 if L % 2 else 0.75


def exact_x(kind, N, C, H, W, G=None, family="eps0", seed=1):
    """x [N, C, H, W] (float64 holding fp32 numbers) with exactly known statistics; kind "bn" or "gn"."""
    HW = H * W
    if kind == "bn":
        s, m = set_scale(C, family)
        d = block_sets(C, N * HW, seed).view(C, N, HW).permute(1, 0, 2)
        return ((d + (m / s).view(1, C, 1)) * s.view(1, C, 1)).reshape(N, C, H, W).contiguous()
    L = C // G * HW
    s, m = set_scale(N * G, family)
    d = block_sets(N * G, L, seed)
    return ((d + (m / s)[:, None]) * s[:, None]).view(N, C, H, W)


def ch_pow(C, lo=-1):
    return 2.0 ** ((torch.arange(C) % 3) + lo).double()


def exact_params(C, seed=2):
    """gamma (never 0), beta: small integers times 2^((c mod 3) - 1)."""
    return _ints((C,), -2, 3, seed, nonzero=True) * ch_pow(C), _ints((C,), -3, 3, seed + 1) * ch_pow(C)


def exact_like(shape, seed, lo=-1):
    """Integers of [-3, 3] times a per-channel power of two (axis 1): a residual, a dy, an addend."""
    return _ints(shape, -3, 3, seed) * ch_pow(shape[1], lo).view(1, -1, 1, 1)


def vanishing_dy(keys, seed, scale):
    """keys [S, L] (integers): +v / -v on pairs of positions of one set with equal key, 0 on what is left over, so that
    every sum of dy over a key class vanishes.  scale [S] or [S, L]."""
    S, L = keys.shape
    order = keys.argsort(dim=1, stable=True)
    ks = keys.gather(1, order)
    v = torch.randint(1, 4, (S, L), generator=_gen(seed)).double()
    j = torch.arange(L)
    first = (j % 2 == 0) & (j + 1 < L)
    pair_ok = torch.zeros(S, L, dtype=torch.bool)
    pair_ok[:, :-1] = first[:-1] & (ks[:, :-1] == ks[:, 1:])
    vals = torch.zeros(S, L, dtype=F64)
    vals[pair_ok] = v[pair_ok]
    second = torch.zeros_like(pair_ok)
    second[:, 1:] = pair_ok[:, :-1]
    vals[second] = -v[:, :-1][pair_ok[:, :-1]]
    out = torch.zeros(S, L, dtype=F64)
    out.scatter_(1, order, vals)
    return out * (scale if scale.dim() == 2 else scale[:, None])


def bn_vanishing_dy(x, y, mean, invstd, relu, seed=9):
    N, C, H, W = x.shape
    xh = (2 * (x - mean.view(1, C, 1, 1)) * invstd.view(1, C, 1, 1)).round().long() + 8
    keys = xh * 2 + ((y > 0).long() if relu else 0)
    keys = keys.permute(1, 0, 2, 3).reshape(C, -1)
    dy = vanishing_dy(keys, seed, ch_pow(C, -1))
    return dy.view(C, N, H, W).permute(1, 0, 2, 3).contiguous()


def gn_vanishing_dz(x, mean, rstd, G, seed=9):
    """Per (image, channel): pairs with equal xhat, so sum dz = sum dz xhat = 0 per channel and per group."""
    N, C, H, W = x.shape
    cpg = C // G
    ch = lambda t: t.repeat_interleave(cpg, 1).view(N, C, 1, 1)
    keys = ((2 * (x - ch(mean)) * ch(rstd)).round().long() + 8).view(N * C, H * W)
    return vanishing_dy(keys, seed, ch_pow(C, -1).repeat(N)).view(N, C, H, W)


def scales(n, exp):
    return 2.0 ** (exp * (torch.arange(n) % 3)).double()


def gauss(shape, seed, offset=0.0):
    """fp32 normal draws + offset (rounded to fp32), held in float64."""
    return (torch.randn(tuple(shape), generator=_gen(seed), dtype=torch.float32) + offset).double()


def gauss_bn(N, C, H, W, seed, offset=0.0):
    """BN reduces over the images: the channel amplitude only."""
    return gauss((N, C, H, W), seed, offset) * scales(C, CH_EXP).view(1, C, 1, 1)


def gauss_gn(N, C, H, W, G, seed, offset=0.0):
    """GN reduces over a group's channels: image and group amplitudes."""
    amp = scales(N, IMG_EXP).view(N, 1) * scales(G, CH_EXP).view(1, G)
    return gauss((N, C, H, W), seed, offset) * amp.repeat_interleave(C // G, 1).view(N, C, 1, 1)


def f32(t):
    """The fp32 rounding of a float64 tensor, as float64."""
    return t.float().double()


def is_f32(t):
    return torch.equal(t.float().double(), t)


# ================================================================================================ bounds
def stats_bound(A1, A2, mu, var, eps, M, c1):
    """-> d_mu (of the fp32 mean), d_is (of the fp32 invstd), invstd; all arguments per set, A1 = sum |x| / M, A2 = sum x^2 / M."""
    d_mu64 = (gam(c1) + f64_term(M)) * A1
    d_var = (gam(c1 + 1) + f64_term(M)) * A2 + (2 * mu.abs() + d_mu64) * d_mu64
    lo = (var - d_var).clamp_min(0) + eps
    inv = 1.0 / torch.sqrt(var + eps)
    d_is = d_var / (2 * lo.pow(1.5))
    return d_mu64 + U * (mu.abs() + d_mu64), d_is + (U + 2.0 ** -50) * (inv + d_is), inv


def affine_bound(x, mu, inv, g, beta, res, d_mu, d_is):
    """Forward element bound; every per-set / per-channel argument already broadcast to x."""
    A = g.abs() * (inv + d_is)
    stat = g.abs() * ((x - mu).abs() * d_is + (inv + d_is) * d_mu)
    return stat + gam(5) * (x.abs() * A + (mu.abs() + d_mu) * A + beta.abs() + (0 if res is None else res.abs()))


def silu_bound(y, by, fn):
    """|z^ - silu(y)| given |y^ - y| <= by."""
    return (EXP_ULP[fn] + 3) * U * 1.001 * ((y * sigmoid(y)).abs() + SILU_SLOPE * by) + SILU_SLOPE * by


def silu_grad_bound(y, by, fn):
    """|f^ - f(y)|, f = silu'."""
    return (2 * EXP_ULP[fn] + 8) * (1 + y.abs() + by) * U * 1.001 + SILU_CURV * by


def bn_forward_bound(x, gamma, beta, res, train, eps, running_mean=None, running_var=None):
    N, C, H, W = x.shape
    M = N * H * W
    v = lambda t: t.view(1, C, 1, 1)
    if train:
        o = bn_forward(x, gamma, beta, eps=eps)
        ab = bn_forward(x, gamma, beta, eps=eps, absolute=True)
        d_mu, d_is, inv = stats_bound(ab.mean, ab.var, o.mean, o.var, eps, M, 2 + 8)
        mu = o.mean
    else:                                     # invstd = fl(1 / fl(sqrt(fl(var + eps)))): three roundings
        mu, inv = running_mean, 1.0 / torch.sqrt(running_var + eps)
        d_mu, d_is = torch.zeros_like(mu), gam(3) * inv
    return NS(y=affine_bound(x, v(mu), v(inv), v(gamma), v(beta), res, v(d_mu), v(d_is)), mean=d_mu, invstd=d_is)


def sum_bounds(dz_abs_sum, dzx_abs_sum, M, c1):
    return (gam(c1 + 1) + f64_term(M)) * dz_abs_sum, (gam(c1 + 4) + f64_term(M)) * dzx_abs_sum


def bn_backward_bound(dy, y, x, gamma, mean, invstd, train, relu, gacc=None, bacc=None):
    N, C, H, W = x.shape
    M = N * H * W
    v = lambda t: t.view(1, C, 1, 1)
    o = bn_backward(dy, y, x, gamma, mean, invstd, train, relu)
    a = bn_backward(dy, y, x, gamma, mean, invstd, train, relu, absolute=True)
    d_db, d_dg = sum_bounds(a.dbeta, a.dgamma, M, 2 + 8)
    gi = (gamma * invstd).abs()
    if train:
        d_kb = (d_db + gam(2) * (o.dbeta.abs() + d_db)) / M
        d_kg = (d_dg + gam(2) * (o.dgamma.abs() + d_dg)) / M
        KB, KG = o.dbeta.abs() / M + d_kb, o.dgamma.abs() / M + d_kg
        dx = v(gi) * (v(d_kb) + a.xh * v(d_kg) + gam(3) * a.xh * v(KG)
                      + gam(4) * (a.dz + v(KB) + (1 + gam(3)) * a.xh * v(KG)))
    else:
        dx = gam(2) * v(gi) * a.dz
    acc = lambda d, val, acc0: None if acc0 is None else d + U * (acc0.abs() + val.abs() + d)
    return NS(dx=dx, dbeta=d_db, dgamma=d_dg, gacc=acc(d_dg, o.dgamma, gacc), bacc=acc(d_db, o.dbeta, bacc))


def gn_c1(C, HW, G):
    return 2 + (gn_items(C, HW, G) or 16)


def gn_forward_bound(x, gamma, beta, G, eps, silu, c1=None, fn="expf"):
    N, C, H, W = x.shape
    cpg = C // G
    ch = lambda t: t.repeat_interleave(cpg, 1).view(N, C, 1, 1)
    o = gn_forward(x, gamma, beta, G, eps)
    ab = gn_forward(x, gamma, beta, G, eps, absolute=True)
    d_mu, d_is, inv = stats_bound(ab.mean, ab.var, o.mean, o.var, eps, cpg * H * W, c1 or gn_c1(C, H * W, G))
    by = affine_bound(x, ch(o.mean), ch(inv), gamma.view(1, C, 1, 1), beta.view(1, C, 1, 1), None, ch(d_mu), ch(d_is))
    return NS(y=silu_bound(o.pre, by, fn) if silu else by, pre=by, mean=d_mu, rstd=d_is)


def gn_backward_bound(dz, x, gamma, beta, mean, rstd, G, silu, addend=None, csum_acc=None, gacc=None, bacc=None):
    N, C, H, W = x.shape
    HW, cpg = H * W, C // G
    L = cpg * HW
    r = gn_r(HW)
    cs = 2 + int(math.log2(r)) + HW // 4 // r
    ch = lambda t: t.repeat_interleave(cpg, 1).view(N, C, 1, 1)
    gv = gamma.abs().view(1, C, 1, 1)
    o = gn_backward(dz, x, gamma, beta, mean, rstd, G, silu, addend)
    a = gn_backward(dz, x, gamma, beta, mean, rstd, G, silu, addend, absolute=True)
    if silu:                                  # y^ = fl(fl(xhat^ * gamma) + beta): 4 roundings on the first term
        yv = o.xh * gamma.view(1, C, 1, 1) + beta.view(1, C, 1, 1)
        by = gam(4) * (a.xh * gv + beta.abs().view(1, C, 1, 1))
        e_dy = dz.abs() * (silu_grad_bound(yv, by, "expf") + U * SILU_SLOPE)
    else:
        e_dy = torch.zeros_like(dz)
    # per (image, channel) sums in fp32, folded over the images in fp64, rounded once
    d_db = e_dy.sum((0, 2, 3)) + (gam(cs + 1) + f64_term(N)) * (a.dy + e_dy).sum((0, 2, 3))
    d_dg = (e_dy * a.xh).sum((0, 2, 3)) + (gam(cs + 4) + f64_term(N)) * ((a.dy + e_dy) * a.xh).sum((0, 2, 3))
    # group means: + one product by gamma, cpg sequential adds, one division
    kg = cs + 2 + cpg
    d_ma = _grp(e_dy * gv, G).sum(2) / L + gam(kg) * _grp((a.dy + e_dy) * gv, G).sum(2) / L
    d_mb = _grp(e_dy * gv * a.xh, G).sum(2) / L + gam(kg + 3) * _grp((a.dy + e_dy) * gv * a.xh, G).sum(2) / L
    MA, MB = o.ma.abs() + d_ma, o.mb.abs() + d_mb
    rs = ch(rstd)
    terms = rs * ((a.dy + e_dy) * gv + ch(MA) + a.xh * ch(MB)) + (0 if addend is None else addend.abs())
    dx = rs * (e_dy * gv + ch(d_ma) + a.xh * ch(d_mb)) + gam(6) * terms
    d_nk = dx.sum((2, 3)) + gam(cs) * (o.dx.abs() + dx).sum((2, 3))
    d_cs = d_nk.sum(0) + (U + f64_term(N)) * (o.nk.abs() + d_nk).sum(0)
    acc = lambda d, val, acc0: None if acc0 is None else d + U * (acc0.abs() + val.abs() + d)
    return NS(dx=dx, dbeta=d_db, dgamma=d_dg, nk=d_nk, csum=d_cs, csum_acc=acc(d_cs, o.csum, csum_acc),
              gacc=acc(d_dg, o.dgamma, gacc), bacc=acc(d_db, o.dbeta, bacc))


def gn16_c1(HW):
    return -(-rows_per_chunk(HW) // 8) + 7


def gn16_forward_bound(x, gamma, beta, G, eps, silu):
    """K12: mr, ab in fp32; y rounded once more to bf16."""
    N, C, H, W = x.shape
    cpg = C // G
    b = gn_forward_bound(x, gamma, beta, G, eps, silu, c1=gn16_c1(H * W), fn="__expf")
    o = gn16_forward(x, gamma, beta, G, eps, silu)
    rep = lambda t: t.repeat_interleave(cpg, 1)
    d_a = gamma.abs() * rep(b.rstd) + U * (o.ab[:, :, 0].abs() + gamma.abs() * rep(b.rstd))
    A = o.ab[:, :, 0].abs() + d_a
    d_b = rep(o.mean).abs() * d_a + A * rep(b.mean) + gam(2) * ((rep(o.mean).abs() + rep(b.mean)) * A + beta.abs())
    return NS(y=b.y + U16 * (o.y64.abs() + b.y), mr=torch.stack((b.mean, b.rstd), 2), ab=torch.stack((d_a, d_b), 2))


def gn16_backward_bound(dy, x, gamma, mr, ab, G, silu, dgamma0=None, dbeta0=None):
    """K12 backward: per-channel chunk sums in fp32 (gn16_c1 adds), everything after them in fp64 until one rounding;
    dx = fl(rstd * fl(fl(dz * gamma) - fl(fl(s1 + fl(xhat^ * s2)) * inv_m))) with inv_m = fl(1 / fl(HW * cpg)): at most 8 roundings on a term; then bf16."""
    N, C, H, W = x.shape
    HW, cpg = H * W, C // G
    L = cpg * HW
    c1 = gn16_c1(HW)
    ch = lambda t: t.repeat_interleave(cpg, 1).view(N, C, 1, 1)
    gv = gamma.abs().view(1, C, 1, 1)
    o = gn16_backward(dy, x, gamma, mr, ab, G, silu)
    xh, rs = o.xh.abs(), ch(mr[:, :, 1])
    if silu:                                  # z^ = fl(fl(a * x) + b)
        bz = gam(2) * ((ab[:, :, 0].view(N, C, 1, 1) * x).abs() + ab[:, :, 1].abs().view(N, C, 1, 1))
        e_d = dy.abs() * (silu_grad_bound(o.z, bz, "__expf") + U * SILU_SLOPE)
    else:
        e_d = torch.zeros_like(dy)
    d = o.dy.abs() + e_d
    d_db = e_d.sum((0, 2, 3)) + (gam(c1 + 1) + f64_term(N * HW)) * d.sum((0, 2, 3))
    d_dg = (e_d * xh).sum((0, 2, 3)) + (gam(c1 + 4) + f64_term(N * HW)) * (d * xh).sum((0, 2, 3))
    d_s1 = _grp(e_d * gv, G).sum(2) + (gam(c1 + 1) + f64_term(L)) * _grp(d * gv, G).sum(2)
    d_s2 = _grp(e_d * gv * xh, G).sum(2) + (gam(c1 + 4) + f64_term(L)) * _grp(d * gv * xh, G).sum(2)
    S1, S2 = (o.ma.abs() * L + d_s1), (o.mb.abs() * L + d_s2)
    terms = rs * (d * gv + (ch(S1) + xh * ch(S2)) / L)
    dx = rs * (e_d * gv + (ch(d_s1) + xh * ch(d_s2)) / L) + gam(8) * terms
    dx = dx + U16 * (o.dx64.abs() + dx)
    acc = lambda b, val, a0: b if a0 is None else b + U * (a0.abs() + val.abs() + b)
    return NS(dx=dx, dgamma=acc(d_dg, o.dgamma, dgamma0), dbeta=acc(d_db, o.dbeta, dbeta0))


def relu_edge_share(pre, bound):
    """Share of elements whose pre-activation lies within its own forward bound of 0."""
    return float((pre.abs() <= bound).double().mean())


def kappa(mean, var, eps):
    return (mean.pow(2) + var) / (var + eps)


# ================================================================================================ the tensors of a case
EPS_BN, EPS_GN = float(torch.tensor(1e-5, dtype=torch.float32)), float(torch.tensor(1e-6, dtype=torch.float32))
OFFSETS = (0.0, 16.0, 256.0)
RELU_OFFSETS = (0.0, 16.0)


def bn_inputs(c, kind, family="eps0", offset=0.0):
    """x, gamma, beta, res, dy, running statistics, eps of a BN case; kind "exact" or "gauss"."""
    N, C, H, W = c[:4]
    if kind == "exact":
        s, _ = set_scale(C, family)
        g, b = exact_params(C)
        return NS(x=exact_x("bn", N, C, H, W, family=family), gamma=g, beta=b, res=exact_like((N, C, H, W), 4),
                  dy=exact_like((N, C, H, W), 5, lo=-2), rm=_ints((C,), -2, 2, 6) * 4 * s, rv=_ints((C,), 1, 3, 7),
                  gacc=_ints((C,), -3, 3, 8), bacc=_ints((C,), -3, 3, 9), eps=eps_of(family, N * H * W))
    amp = scales(C, CH_EXP)
    return NS(x=gauss_bn(N, C, H, W, 1, offset), gamma=gauss((C,), 2) * amp, beta=gauss((C,), 3) * amp,
              res=gauss_bn(N, C, H, W, 4), dy=gauss((N, C, H, W), 5) * scales(C, IMG_EXP).view(1, C, 1, 1),
              rm=gauss((C,), 6, offset) * amp, rv=f32(gauss((C,), 7).abs() + 0.5) * amp * amp,
              gacc=gauss((C,), 8), bacc=gauss((C,), 9), eps=EPS_BN)


def gn_inputs(c, kind, family="eps0", offset=0.0, bf16=False):
    """x, gamma, beta, dz, addend, accumulators, eps of a GN case (fp32 kernels, or K12 with bf16: bf16-exact x, dz)."""
    N, C, H, W, G = c[:5]
    L = C // G * H * W
    if kind == "exact":
        g, b = exact_params(C)
        x = exact_x("gn", N, C, H, W, G, family)
        s, _ = set_scale(N * G, family)
        rs = (1.0 / (2 * s) if family == "eps0" else torch.ones_like(s)).view(N, G)
        add = exact_like((N, C, H, W), 5, lo=-2) * rs.repeat_interleave(C // G, 1).view(N, C, 1, 1)
        return NS(x=x, gamma=g, beta=b, dz=exact_like((N, C, H, W), 4, lo=-1), addend=add, gacc=_ints((C,), -3, 3, 8),
                  bacc=_ints((C,), -3, 3, 9), cacc=_ints((C,), -3, 3, 10), eps=eps_of(family, L))
    rnd = bf16_round if bf16 else (lambda t: t)
    return NS(x=rnd(gauss_gn(N, C, H, W, G, 1, offset)), gamma=gauss((C,), 2), beta=gauss((C,), 3),
              dz=rnd(gauss_gn(N, C, H, W, G, 4)), addend=gauss((N, C, H, W), 5), gacc=gauss((C,), 8), bacc=gauss((C,), 9),
              cacc=gauss((C,), 10), eps=EPS_GN)


def exact_dx(c, vanishing):
    """Is dx of the exact GN case c exact in fp32?  Always in the vanishing family; else where cpg * HW is a power of two
    (the group means are whole multiples of a unit L times finer than dy gamma: up to L = 2^14 that fits 24 bits)."""
    L = c.C // c.G * c.H * c.W
    return vanishing or (L & (L - 1) == 0 and L <= 1 << 14)


def exact_nk(c, vanishing):
    """nk sums HW values of dx, whole multiples of a unit L times finer than their size: exact while L * HW is small."""
    L = c.C // c.G * c.H * c.W
    return vanishing or (L & (L - 1) == 0 and L * c.H * c.W <= 4096)
