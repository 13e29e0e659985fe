"""A float64 model of K14 (csrc/salun_tok_bf16.hip: LayerNorm forward / backward and GEGLU forward / backward on bf16
tokens), the inputs the exact-answer tests feed it, the per-element error bounds, the shapes, and a Python mirror of the
host logic.  Validated against torch's float64 ops by test_tok_bf16_ref_cpu.py; used by test_tok_bf16_exact_gpu.py.
The number formats, the zero-sum blocks, the parameter draws and gamma_k come from norm_ref_cpu / attn_ref_cpu.

THE MODEL is the definition, written out.  Every backward is a function of what the backward kernel is handed: the
LayerNorm backward takes the saved (mean, rstd) as an input, it does not recompute them.  `absolute=True` returns, field
for field, the sums of the absolute values of the terms.  GELU is evaluated as 0.5 b erfc(-b / sqrt 2): in float64
1 + erf(b / sqrt 2) is 0 at b = -16 and has lost half its digits at b = -5.

EXACT INPUTS (seeded, all bf16 numbers).  LayerNorm: row r is a centre m = k s plus the zero-sum blocks of norm_ref_cpu
({-2s, +2s}; {-4s, 0 x 6, +4s}) shuffled along the row; s a power of two, k and s change from row to row.  Then
mean = m and var = 4 s^2 in every summation order, at power-of-two and 5 * 2^k widths alike.  Family "eps0": eps = 0,
rstd = 1 / (2s).  Family "eps": s = 1/4, eps = 0.75, rstd = 1; a dropped eps gives 2.  xhat is in {0, +-1/2, +-1, +-2}.
gamma = (a non-zero integer of [-2, 3]) * p_c, p_c = 2^((c mod 3) - 1); beta = (an ODD integer of [-5, 7]) * p_c / 4.
xhat * gamma is a whole multiple of p_c / 2, so y is never a cancellation: y = beta where xhat = 0, else
|y| >= p_c / 4 >= 2^-6 (|xhat gamma| + |beta|) (asserted), and a last-place difference in rstd cannot carry y over a
bf16 rounding boundary.  dy: integers of [-3, 3] times p_c (the general family; dx is exact in fp32, and compared
after ONE rounding to bf16, where C is a power of two), or the vanishing family: +-6 v / gamma_c on pairs of positions
of a row with equal xhat, so g = dy * gamma = +-6 v, sum g = sum g xhat = 0 per row and dx = rstd * g, a bf16 number.
GEGLU: gates from {0, +-16, +-32}, values and dy integers of [-3, 3] times a power of two per column.  There
gelu(b) rounds to 0, b, -0 and gelu'(b) to 1/2, 1, -0 in bf16 and in the fp32 formula alike.  +-8 is NOT in the set:
gelu(-8) = -4.9e-15 is a bf16 number, while the fp32 formula returns -0.

GAUSSIAN INPUTS: bf16-rounded normal draws; amplitude 2^(-7 (r mod 3)) per row on x and dy (the row is the axis the
statistic does not run over), 2^(5 (c mod 3)) per channel on gamma, beta and dy; row offset mu / sigma in {0, 2^4} (bf16
leaves no deviation bits beyond that).  GEGLU gates are unit draws shifted by 0 or by -4 (GEGLU_SHIFTS), so that
b in [-6, -3] is populated; |b| < 12 is asserted, which keeps exp(-b^2 / 2) a normal fp32 number.

PER-ELEMENT BOUNDS, from the rounding points of the kernels as written (u = 2^-24, gamma_k = k u / (1 - k u), U16 = 2^-8;
a fused multiply-add only removes a rounding).
  lane sum.  A lane adds the 8 values of each of its ceil((C / 8) / 64) octets one after the other, then 6 butterfly
  steps: a value passes through at most c1 = 8 ceil((C / 8) / 64) + 6 roundings.
  mean = fl(sum / (float) C):                          d_mu = gamma_(c1+1) sum |x| / C
  variance, two-pass: d = fl(x - mean^), fl(d d), the same chain, the division, + eps.  With mean^ = mu + dm the exact
  two-pass value is var + dm^2; the terms pass through 3 + c1 + 1 roundings and the sum with eps through one more:
      d_v  = d_mu^2 + gamma_(c1+5) (var + d_mu^2 + eps)          (of fl(var^ + eps) against var + eps)
  rstd = rsqrtf(.):  d_rs = d_v / (2 max(var + eps - d_v, 0)^1.5) + RSQRT_ULP u (rstd + that)
  y = bf16(fl(fl(fl(fl(x - mean^) rstd^) gamma) + beta)): four operations, one bf16 rounding.  With
  T = (|x - mu| + d_mu) (rstd + d_rs) |gamma|:
      b32(y)   = |gamma| (|x - mu| d_rs + (rstd + d_rs) d_mu) + gamma_4 (T + |beta|)
      bound(y) = b32 + U16 (|y| + b32)
  backward, given the saved fp32 (mean, rstd): xhat^ = fl(fl(x - mean) rstd) (2 roundings), g^ = fl(dy gamma) (1).
  m1 = fl(sum g^ / C): 1 + c1 + 1 roundings; m2 = fl(sum fl(g^ xhat^) / C): 4 + c1 + 1.
  dx = bf16(fl(rstd fl(fl(g^ - m1) - fl(xhat^ m2)))): at most 5 roundings on a term.  With M1 = |m1| + d_m1, M2 likewise:
      d_m1 = gamma_(c1+2) sum |g| / C,  d_m2 = gamma_(c1+5) sum |g xhat| / C
      b32(dx)   = rstd (d_m1 + |xhat| d_m2) + gamma_5 rstd (|g| + M1 + |xhat| M2)
      bound(dx) = b32 + U16 (|dx| + b32)
  dgamma / dbeta: each of the four waves of a workgroup adds the rows it walks, at most ceil(rows_per_wg / 4), in fp32 per
  lane and channel; 3 more adds through LDS; the workgroups' partials are folded in fp64 (f64_term(parts)) and rounded
  once: with na = ceil(rows_per_wg / 4) + 3, a term dy xhat^ passes through 3 + na + 1 roundings, a term dy through na + 1:
      d_dgamma = (gamma_(na+4) + f64) sum |dy xhat|,  d_dbeta = (gamma_(na+1) + f64) sum |dy|
  `acc += v`: d_v + u (|acc| + |v| + d_v).
  GEGLU.  t^ = fl(b c^), c^ = fl(1 / sqrt 2): two roundings of the argument, and |erf'(t)| = 2 / sqrt(pi) exp(-t^2):
      d_E    = ERF_ULP u |erf t| + 1.001 gamma_2 |t| 2 / sqrt(pi) exp(-t^2)          (of erff(t^) against erf t)
      d_S    = d_E + u (|1 + erf t| + d_E)                                           (of fl(1 + E^))
      d_gelu = |b| / 2 (d_S + u (|1 + erf t| + d_S))                                 (0.5 b is exact, one product)
      out    = bf16(fl(a gelu^)):  b32 = |a| d_gelu + u |a| (|gelu| + d_gelu),  bound = b32 + U16 (|out| + b32)
  dh[:, :F] = bf16(fl(dy gelu^)): the same with dy for a.  In the tail b < -3, 1 + erf t cancels: the ABSOLUTE error
  ERF_ULP u of erff is an error 0.5 |a b| ERF_ULP u of the output, however small the output; this is the term the bound
  must carry there, and elsewhere it is 2^-16 of the bf16 rounding term.
  gelu'^ = fl(0.5 S^ + fl(fl(b k^) Ex^)), k^ = fl(1 / sqrt(2 pi)), Ex^ = __expf(fl((-0.5 b) b)): the native path
  v_exp_f32(fl(x log2 e)) as in norm_ref_cpu's EXP_ULP["__expf"], with |arg| = b^2 / 2 in place of 80, and u |arg| more
  for the rounding of the argument itself: relative (2 + 3 b^2 / 2) u.  The product b k^ has two roundings, the product
  by Ex^ one:
      d_phi = 1.001 (5 + 3 b^2 / 2) u |b phi(b)|
      d_gg  = 0.5 d_S + d_phi + u (|gelu'| + 0.5 d_S + d_phi)
      dh[:, F:] = bf16(fl(fl(dy a) gelu'^)):  b32 = |dy a| d_gg + gamma_2 |dy a| (|gelu'| + d_gg),  then U16 as above.
No constant is fitted to what the kernels produce, there is no absolute slack and nothing is scaled by a tensor's
maximum.

THE TWO LIBRARY CONSTANTS.  ERF_ULP and RSQRT_ULP are the maximum errors of erff and rsqrtf in units of u (1 ulp <= 2 u),
as EXP_ULP is for expf.  The table norm_ref_cpu cites for expf (HIP math API reference, "Single precision mathematical
functions") was not at hand when this was written: 4 ulp for erff and 2 ulp for rsqrtf are ASSUMED here.  The assumption
carries little weight: outside the tail b < -3 these terms are 2^-16 of the bf16 rounding term.
"""
import math
from collections import namedtuple
from types import SimpleNamespace as NS

import torch

from norm_ref_cpu import (CH_EXP, EXP_ULP, F64, IMG_EXP, U, U16, _ints, bf16_round, block_sets, ch_pow,  # noqa: F401
                          exact_params, f32, f64_term, gam, gauss, is_f32, scales, set_scale, vanishing_dy)

ERF_ULP = 8.0            # erff: 4 ulp, assumed (see the docstring)
RSQRT_ULP = 4.0          # rsqrtf: 2 ulp, assumed
V_EXP_U = EXP_ULP["__expf"] - 2 * 80.0       # what EXP_ULP["__expf"] holds for the instruction itself: 1 ulp = 2 u
SQRT1_2 = 0.7071067811865476
INV_SQRT_2PI = 0.3989422804014327
LN_MAXO, LN_PARTS_MAX, GEGLU_MAX_GRID = 4, 1024, 2048
EPS_LN = float(torch.tensor(1e-5, dtype=torch.float32))
LN_OFFSETS = (0.0, 16.0)
GEGLU_SHIFTS = (0.0, -4.0)
TAIL = (-6.0, -3.0)


# ================================================================================================ the model
def ln16_forward(x, gamma, beta, eps, absolute=False):
    """LayerNorm over the last axis of x [rows, C] (biased variance).  -> y (ONE rounding of y64 to bf16), y64, mean,
    rstd, var, xh, stats [rows, 2].  absolute: mean = sum |x| / C, var = sum x^2 / C, y = |xhat gamma| + |beta|."""
    mean = x.mean(1)
    d = x - mean[:, None]
    var = d.pow(2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = d * rstd[:, None]
    if absolute:
        return NS(mean=x.abs().mean(1), var=x.pow(2).mean(1), y=(xh * gamma).abs() + beta.abs())
    y64 = xh * gamma + beta
    return NS(y=bf16_round(y64), y64=y64, mean=mean, rstd=rstd, var=var, xh=xh, stats=torch.stack((mean, rstd), 1))


def ln16_backward(dy, x, gamma, mean, rstd, dgamma0=None, dbeta0=None, absolute=False):
    """Given the saved mean / rstd [rows]: g = dy gamma; dx = rstd (g - mean_c(g) - xhat mean_c(g xhat));
    dgamma = sum_rows dy xhat (+ dgamma0), dbeta = sum_rows dy (+ dbeta0).  Also dx64, g, xh, m1, m2."""
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    dyv, xh, g = f(dy), f(xh), f(g)
    m1, m2 = g.mean(1), (g * xh).mean(1)
    if absolute:
        dx64 = rstd.abs()[:, None] * (g + m1[:, None] + xh * m2[:, None])
    else:
        dx64 = rstd[:, None] * (g - m1[:, None] - xh * m2[:, None])
    dgamma, dbeta = (dyv * xh).sum(0), dyv.sum(0)
    if dgamma0 is not None:
        dgamma, dbeta = dgamma + f(dgamma0), dbeta + f(dbeta0)
    return NS(dx=bf16_round(dx64), dx64=dx64, dgamma=dgamma, dbeta=dbeta, g=g, xh=xh, m1=m1, m2=m2)


def norm_cdf(b):
    """Phi(b) = 0.5 erfc(-b / sqrt 2): no cancellation on the negative side."""
    return 0.5 * torch.special.erfc(-b * SQRT1_2)


def norm_pdf(b):
    return torch.exp(-0.5 * b * b) * INV_SQRT_2PI


def gelu(b):
    return b * norm_cdf(b)


def gelu_grad(b):
    return norm_cdf(b) + b * norm_pdf(b)


def geglu16_forward(h):
    """h [rows, 2F] -> out = h[:, :F] gelu(h[:, F:]) (one rounding to bf16), out64."""
    F = h.shape[1] // 2
    out64 = h[:, :F] * gelu(h[:, F:])
    return NS(out=bf16_round(out64), out64=out64)


def geglu16_backward(h, dy, absolute=False):
    """dh[:, :F] = dy gelu(b), dh[:, F:] = dy a gelu'(b).  absolute: |dy a| (Phi(b) + |b phi(b)|) for the second."""
    F = h.shape[1] // 2
    a, b = h[:, :F], h[:, F:]
    if absolute:
        return NS(dh64=torch.cat(((dy * gelu(b)).abs(), (dy * a).abs() * (norm_cdf(b) + (b * norm_pdf(b)).abs())), 1))
    dh64 = torch.cat((dy * gelu(b), dy * a * gelu_grad(b)), 1)
    return NS(dh=bf16_round(dh64), dh64=dh64)


# ================================================================================================ mirror of the host logic
def ln_ok(rows, C):
    return rows >= 1 and C >= 8 and C % 8 == 0 and C <= 8 * 64 * LN_MAXO


def ln_parts(rows):
    return max(1, min((rows + 63) // 64, LN_PARTS_MAX))


def rows_per_wg(rows):
    return -(-rows // ln_parts(rows))


def ln_ws_bytes(rows, C):
    return ln_parts(rows) * C * 2 * 4 if ln_ok(rows, C) else 0


def ln_lds_bytes(C):
    return 8 * 3 * C


def octets_per_lane(C):
    """How many of the octets lane, lane + 64, ... (< C / 8) each of the 64 lanes owns."""
    return [len(range(lane, C // 8, 64)) for lane in range(64)]


def wg_rows(rows):
    """The number of rows each workgroup of the backward walks (0: it only writes zero partials)."""
    rpw = rows_per_wg(rows)
    return [max(0, min(rows, (w + 1) * rpw) - w * rpw) for w in range(ln_parts(rows))]


def empty_wgs(rows):
    return [w for w, n in enumerate(wg_rows(rows)) if n == 0]


def geglu_ok(rows, F):
    return rows >= 1 and F >= 8 and F % 8 == 0


def geglu_grid(rows, F):
    return max(1, min(-(-(rows * (F // 8)) // 256), GEGLU_MAX_GRID))


def geglu_trips(rows, F):
    """-> (the most grid-stride trips a thread takes, how many threads take a second one)"""
    total, threads = rows * (F // 8), geglu_grid(rows, F) * 256
    return -(-total // threads), max(0, min(total - threads, threads))


def ln_routes(rows, C):
    no, parts, rpw, per = C // 8, ln_parts(rows), rows_per_wg(rows), wg_rows(rows)
    own = octets_per_lane(C)
    out = {f"parts={parts}" if parts in (1, 2, 3, 4, 65) else "parts capped" if parts == LN_PARTS_MAX else "parts other"}
    if rows == 1 and no == 1:
        out.add("one lane, one row")
    if rows < 4:
        out.add("rows<4")
    if rows % 4 == 1:
        out.add("rows%4=1")
    if no == 64:
        out.add("C/8=64")
    if no == 65 and own[0] == 2 and set(own[1:]) == {1}:
        out.add("C/8=65: lane 0 alone owns a second octet")
    if 128 < no < 192:
        out.add("third slot partial")
    if no == 256:
        out.add("four full slots")
    if ln_lds_bytes(C) == 48 * 1024:
        out.add("LDS 48 KiB")
    if C in (320, 640, 1280):
        out.add(f"SD width {C}")
    if C & (C - 1):
        out.add("C npo2")
    if any(n % 4 for n in per):
        out.add("unequal waves")
    if rpw % 4:
        out.add("rows_per_wg%4!=0")
    if rpw > 64:
        out.add("rows_per_wg>64")
    if empty_wgs(rows):
        out.add("empty workgroups")
    if 0 < per[-1 - len(empty_wgs(rows))] < rpw:
        out.add("ragged last workgroup")
    return out


def geglu_routes(rows, F):
    fo = F // 8
    out = {"one octet" if fo == 1 else f"fo={fo}" if fo in (2, 3) else "fo other"}
    if rows > 1 and fo > 1:
        out.add("i / fo across rows")
    if fo & (fo - 1):
        out.add("fo npo2")
    if F == 5120:
        out.add("SD feed-forward width")
    if geglu_trips(rows, F)[0] == 2:
        out.add("second trip")
    if geglu_grid(rows, F) > 1:
        out.add("more than one block")
    return out


# ================================================================================================ the shapes
LnCase = namedtuple("LnCase", "rows C why")
GegluCase = namedtuple("GegluCase", "rows F why")
_cid = lambda c: "x".join(map(str, c[:-1]))

LN_CASES = [LnCase(*s) for s in [
    (1, 8, "one lane, one row, one workgroup"),
    (3, 24, "rows < 4"),
    (9, 512, "C / 8 = 64: every lane holds exactly one octet; rows % 4 = 1"),
    (6, 520, "C / 8 = 65: lane 0 alone owns a second octet"),
    (5, 1032, "the third slot is partial"),
    (3, 2048, "all four slots full; the backward's dynamic LDS is exactly 48 KiB"),
    (67, 320, "SD width, parts = 2, rows_per_wg = 34"),
    (130, 640, "SD width, parts = 3, the last workgroup walks 42 rows"),
    (193, 1280, "SD width, parts = 4, rows_per_wg = 49"),
    (4097, 16, "parts = 65"),
    (65541, 8, "parts capped at 1024, rows_per_wg = 65, workgroup 1008 holds 21 rows, 1009..1023 are empty"),
]]
LN_REQUIRED = ["one lane, one row", "rows<4", "rows%4=1", "C/8=64", "C/8=65: lane 0 alone owns a second octet",
               "third slot partial", "four full slots", "LDS 48 KiB", "SD width 320", "SD width 640", "SD width 1280",
               "C npo2", "parts=1", "parts=2", "parts=3", "parts=4", "parts=65", "parts capped", "unequal waves",
               "rows_per_wg%4!=0", "rows_per_wg>64", "empty workgroups", "ragged last workgroup"]
LN_BIG = LN_CASES[-1]
LN_ARENA = [LN_CASES[i] for i in (0, 2, 3, 4, 5, 8, 10)]   # one lane; C/8 = 64, 65; slot 3 partial; four slots; parts 4; the cap

GEGLU_CASES = [GegluCase(*s) for s in [
    (1, 8, "one octet"), (3, 16, "two octets per row: i / fo across rows"), (5, 24, "three octets per row"),
    (7, 1280, "160 octets per row, five blocks"),
    (2, 5120, "the SD feed-forward width at 1280"),
    (2049, 2048, "524,544 octets against 524,288 threads: the first 256 threads take a second trip"),
]]
GEGLU_REQUIRED = ["one octet", "fo=2", "fo=3", "i / fo across rows", "fo npo2", "SD feed-forward width", "second trip",
                  "more than one block"]
GEGLU_BIG = GEGLU_CASES[-1]
GEGLU_ARENA = [GEGLU_CASES[i] for i in (0, 2, 5)]

LN_OUTSIDE_C = (0, 4, 12, 2056)
GEGLU_OUTSIDE_F = (0, 4, 12)


# ================================================================================================ inputs
def pow2(n):
    return n & (n - 1) == 0


def ln_families():
    return ("eps0", "eps")


def ln_exact_inputs(c, family, seed=1):
    """x, gamma, beta, dy (general family), integer accumulators, eps; the row scales s and centres m."""
    rows, C = c[:2]
    s, m = set_scale(rows, family)
    x = (block_sets(rows, C, seed) + (m / s)[:, None]) * s[:, None]
    gamma, _ = exact_params(C)
    beta = (2 * _ints((C,), -3, 3, 3) + 1) * ch_pow(C) / 4
    return NS(x=x, gamma=gamma, beta=beta, dy=_ints((rows, C), -3, 3, 5) * ch_pow(C)[None, :], s=s, m=m,
              rstd=1.0 / (2 * s) if family == "eps0" else torch.ones_like(s), gacc=_ints((C,), -3, 3, 8),
              bacc=_ints((C,), -3, 3, 9), eps=0.0 if family == "eps0" else 0.75)


def ln_vanishing_dy(x, gamma, mean, rstd, seed=9):
    """+-6 v / gamma_c (v in 1..3) on pairs of positions of a row with equal xhat, 0 on what is left over: g = +-6 v, and
    sum g = sum g xhat = 0 per row."""
    keys = (2 * (x - mean[:, None]) * rstd[:, None]).round().long() + 8
    return 6 * vanishing_dy(keys, seed, torch.ones(x.shape[0], dtype=F64)) / gamma


def ln_exact_dx(c, vanishing):
    """Is dx of the exact case exact in fp32 (and so equal to the model after one rounding to bf16)?"""
    return vanishing or pow2(c.C)


def ln_gauss_inputs(c, offset=0.0):
    rows, C = c[:2]
    ra, ca = scales(rows, IMG_EXP)[:, None], scales(C, CH_EXP)
    return NS(x=bf16_round(gauss((rows, C), 1, offset) * ra), gamma=gauss((C,), 2) * ca, beta=gauss((C,), 3) * ca,
              dy=bf16_round(gauss((rows, C), 4) * ra * ca[None, :]), gacc=gauss((C,), 8), bacc=gauss((C,), 9), eps=EPS_LN)


GATES = (0.0, 16.0, -16.0, 32.0, -32.0)


def geglu_exact_inputs(c, seed=1):
    rows, F = c[:2]
    gate = torch.tensor(GATES, dtype=F64)[torch.randint(0, len(GATES), (rows, F), generator=torch.Generator().manual_seed(seed))]
    a = _ints((rows, F), -3, 3, seed + 1) * ch_pow(F)[None, :]
    return NS(h=torch.cat((a, gate), 1).contiguous(), dy=_ints((rows, F), -3, 3, seed + 2) * ch_pow(F, -2)[None, :])


def geglu_gauss_inputs(c, shift=0.0):
    rows, F = c[:2]
    ra, ca = scales(rows, IMG_EXP)[:, None], scales(F, CH_EXP)[None, :]
    a = bf16_round(gauss((rows, F), 1) * ra)
    b = bf16_round(gauss((rows, F), 2, shift))
    return NS(h=torch.cat((a, b), 1).contiguous(), dy=bf16_round(gauss((rows, F), 3) * ra * ca))


def in_tail(h):
    b = h[:, h.shape[1] // 2:]
    return (b >= TAIL[0]) & (b <= TAIL[1])


# ================================================================================================ bounds
def ln_c1(C):
    return 8 * -(-(C // 8) // 64) + 6


def ln16_forward_bound(x, gamma, beta, eps):
    """-> y, mean, rstd: the per-element / per-row bounds of the docstring."""
    C = x.shape[1]
    c1 = ln_c1(C)
    o = ln16_forward(x, gamma, beta, eps)
    d_mu = gam(c1 + 1) * x.abs().mean(1)
    d_v = d_mu ** 2 + gam(c1 + 5) * (o.var + d_mu ** 2 + eps)
    lo = (o.var + eps - d_v).clamp_min(0)
    d_rs = d_v / (2 * lo.pow(1.5))
    d_rs = d_rs + RSQRT_ULP * U * (o.rstd + d_rs)
    dev, rs, g = (x - o.mean[:, None]).abs(), (o.rstd + d_rs)[:, None], gamma.abs()[None, :]
    b32 = g * (dev * d_rs[:, None] + rs * d_mu[:, None]) + gam(4) * ((dev + d_mu[:, None]) * rs * g + beta.abs()[None, :])
    return NS(y=b32 + U16 * (o.y64.abs() + b32), mean=d_mu, rstd=d_rs)


def ln_na(rows):
    return -(-rows_per_wg(rows) // 4) + 3


def ln16_backward_bound(dy, x, gamma, mean, rstd, dgamma0=None, dbeta0=None):
    rows, C = x.shape
    c1, na = ln_c1(C), ln_na(rows)
    o = ln16_backward(dy, x, gamma, mean, rstd)
    a = ln16_backward(dy, x, gamma, mean, rstd, absolute=True)
    d_m1, d_m2 = gam(c1 + 2) * a.m1, gam(c1 + 5) * a.m2
    M1, M2 = (o.m1.abs() + d_m1)[:, None], (o.m2.abs() + d_m2)[:, None]
    rs = rstd.abs()[:, None]
    b32 = rs * (d_m1[:, None] + a.xh * d_m2[:, None]) + gam(5) * rs * (a.g + M1 + a.xh * M2)
    f64 = f64_term(ln_parts(rows))
    d_dg, d_db = (gam(na + 4) + f64) * a.dgamma, (gam(na + 1) + f64) * a.dbeta
    acc = lambda b, val, a0: b if a0 is None else b + U * (a0.abs() + val.abs() + b)
    return NS(dx=b32 + U16 * (o.dx64.abs() + b32), dgamma=acc(d_dg, o.dgamma, dgamma0), dbeta=acc(d_db, o.dbeta, dbeta0))


def gelu_bound(b):
    """-> d_gelu, d_S, |1 + erf t| of the docstring, per element of the gate."""
    t = b * SQRT1_2
    s = torch.special.erfc(-t)                                   # 1 + erf t >= 0
    d_e = ERF_ULP * U * torch.erf(t).abs() + 1.001 * gam(2) * t.abs() * (2 / math.sqrt(math.pi)) * torch.exp(-t * t)
    d_s = d_e + U * (s + d_e)
    return 0.5 * b.abs() * (d_s + U * (s + d_s)), d_s, s


def _to_bf16(exact64, b32):
    return b32 + U16 * (exact64.abs() + b32)


def geglu16_forward_bound(h):
    F = h.shape[1] // 2
    a, b = h[:, :F].abs(), h[:, F:]
    d_gelu, _, _ = gelu_bound(b)
    out64 = geglu16_forward(h).out64
    return NS(out=_to_bf16(out64, a * d_gelu + U * a * (gelu(b).abs() + d_gelu)))


def geglu16_backward_bound(h, dy):
    F = h.shape[1] // 2
    a, b, d = h[:, :F].abs(), h[:, F:], dy.abs()
    o = geglu16_backward(h, dy)
    d_gelu, d_s, _ = gelu_bound(b)
    da = d * d_gelu + U * d * (gelu(b).abs() + d_gelu)
    d_phi = 1.001 * (V_EXP_U + 3 + 3 * 0.5 * b * b) * U * (b * norm_pdf(b)).abs()
    gg = gelu_grad(b).abs()
    d_gg = 0.5 * d_s + d_phi + U * (gg + 0.5 * d_s + d_phi)
    db = d * a * d_gg + gam(2) * d * a * (gg + d_gg)
    return NS(dh=_to_bf16(o.dh64, torch.cat((da, db), 1)))


# ================================================================================================ fp32 emulations
def _b16(t):
    return t.to(torch.bfloat16).double()


def emulate_ln(t, wrong=None):
    """The kernels' formulas in torch fp32 (its own summation order), rounded to bf16 where the kernels round.
    wrong="gamma shifted": gamma of the neighbouring channel.  -> y, stats, dx (on those stats), dgamma, dbeta."""
    x, dy, g, b = t.x.float(), t.dy.float(), t.gamma.float(), t.beta.float()
    if wrong == "gamma shifted":
        g = torch.roll(g, 1)
    C = x.shape[1]
    mean = x.sum(1) / C
    d = x - mean[:, None]
    rstd = torch.rsqrt((d * d).sum(1) / C + torch.tensor(t.eps, dtype=torch.float32))
    y = (d * rstd[:, None]) * g + b
    xh, gg = (x - mean[:, None]) * rstd[:, None], dy * g
    m1, m2 = gg.sum(1) / C, (gg * xh).sum(1) / C
    dx = rstd[:, None] * ((gg - m1[:, None]) - xh * m2[:, None])
    return NS(y=_b16(y), mean=mean.double(), rstd=rstd.double(), dx=_b16(dx), dgamma=(dy * xh).sum(0).double(),
              dbeta=dy.sum(0).double())


def emulate_geglu(t, wrong=None):
    """wrong="tanh": the tanh form of GELU (and its derivative)."""
    h, dy = t.h.float(), t.dy.float()
    F = h.shape[1] // 2
    a, b = h[:, :F], h[:, F:]
    if wrong == "tanh":
        k = math.sqrt(2 / math.pi)
        th = torch.tanh(k * (b + 0.044715 * b ** 3))
        ge, gr = 0.5 * b * (1 + th), 0.5 * (1 + th) + 0.5 * b * (1 - th * th) * k * (1 + 3 * 0.044715 * b * b)
    else:
        s = 1 + torch.erf(b * torch.tensor(SQRT1_2, dtype=torch.float32))
        ge = (0.5 * b) * s
        gr = 0.5 * s + (b * torch.tensor(INV_SQRT_2PI, dtype=torch.float32)) * torch.exp((-0.5 * b) * b)
    return NS(out=_b16(a * ge), dh=_b16(torch.cat((dy * ge, (dy * a) * gr), 1)))
