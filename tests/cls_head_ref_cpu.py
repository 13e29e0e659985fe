"""float64 model of K23 (csrc/salun_cls_head.hip) on the CPU, a numpy-float32 restatement in the kernel's summation
order, and the per-element bounds of |kernel - model| derived from the kernel's rounding points.  Test infrastructure
only (same discipline as norm_ref_cpu.py): nothing here is fitted to what the kernels produce, there is no absolute
slack and nothing is scaled by a tensor's maximum.

The kernel (x [B, C, HW], w [K, C], bias [K], labels [B], g the incoming scalar gradient):

  pooled[b, c]  chain over the plane (HW % 4 == 0 and x 16-byte aligned: acc += (x0 + x1) + (x2 + x3) per float4; else
                acc += x per element), then ONE division by (float)HW
  logit[b, k]   lane l's fmaf chain over c = l, l + 64, ...; the 64-lane shfl_down tree (32, 16, ..., 1); + bias[k]
  m = max_k logit (lowest index on ties -> hit);  t_k = logit_k - m;  e_k = expf(t_k)
  S             thread t's chain over k = t, t + 256, ...; the tree; the four wave sums as (w0 + w1) + (w2 + w3)
  p_k = e_k / S;   loss = logf(S) - t_y
  scale = g / (float)B;   dlogit_k = (p_k - [k == y]) * scale
  dx[b, c, :]   (fmaf chain over k = 0 .. K-1 of dlogit_k w[k, c]) / (float)HW
  dW[k, c]      wave v's fmaf chain over b = v, v + 4, ...; (v0 + v1) + (v2 + v3)          [accumulate: old + that]
  db[k]         thread t's chain over b = t, t + 256, ...; the tree; (w0 + w1) + (w2 + w3)  [accumulate: old + that]
  loss_sum += float64 sum of the fp32 losses;  hits += #hits;  count += B;  loss_mean = (float)(that sum / B)

Bounds.  u = 2^-24, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1: a
value that passed through n roundings carries a factor within 1 +- gamma_n).  Per output, with |.| element-wise, the
model's values unmarked and E_* the bound of the quantity the kernel feeds forward:

  E_pool  = gamma_{HW+1} mean_hw|x|                       a term passes at most max(HW - 1, 2 + HW / 4) additions, + the
                                                          division: at most HW + 1 roundings for every HW >= 1
  E_logit = gamma_{nl} (sum_c (|pool| + E_pool)|w| + |bias|) + sum_c E_pool |w|,   nl = ceil(C / 64) + 7
                                                          (fmaf chain, 6 tree levels, the bias addition)
  E_t[k]  = E_logit[k] (1 + u) + u ((m - logit_k) + max_k E_logit)          t_k against logit_k - m^ (m^ the kernel's
                                                          maximum: a softmax does not depend on the shift, and m^ is
                                                          within max_k E_logit of m)
  rho_k   = exp(E_t[k]) (1 + EXP_U u) - 1                 relative error of e_k
  rho_S   = sum_k p_k ((1 + rho_k)(1 + gamma_{nS}) - 1),  nS = ceil(K / 256) + 8        (positive terms: the relative
                                                          error of the sum is the p-weighted mean of its terms')
  E_p[k]  = p_k ((1 + rho_k)(1 + u) / (1 - rho_S) - 1)
  E_loss  = (E_log + E_t[y]) (1 + u) + u |loss|,   E_log = r + LOG_U u ((lse - m) + max_k E_logit + r),
                                                          r = -log(1 - rho_S)
  E_q[k]  = E_p[k] (1 + u) + u |p_k - onehot|             the subtraction
  E_d[k]  = |g| / B (E_q[k] (1 + gamma_2) + gamma_2 |p_k - onehot|)          the rounding of scale and of the product
  E_dx    = (gamma_{K+1} sum_k (|d_k| + E_d[k]) |w_kc| + sum_k E_d[k] |w_kc|) / HW
  E_dW    = gamma_{nw} sum_b (|d| + E_d)(|pool| + E_pool) + sum_b (E_d (|pool| + E_pool) + |d| E_pool),
                                                          nw = ceil(B / 4) + 2
  E_db    = gamma_{nb} sum_b (|d| + E_d) + sum_b E_d,     nb = ceil(B / 256) + 8
  accumulate adds fl(old + new): u (|old| + |new| + E) more.

EXP_U, LOG_U: relative error of expf / logf in units of u.  Both are OCML's (__ocml_exp_f32, __ocml_log_f32), 1 ulp
each (HIP math API reference, "Single precision mathematical functions": expf and logf, maximum ULP error 1);
1 ulp <= 2 u.
"""
import math
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
EXP_U = 2.0
LOG_U = 2.0
F32, F64 = np.float32, np.float64


def gamma(n):
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------------------ the float64 model
def model(x, w, bias, labels, g=1.0):
    """Everything K23 computes, in float64.  x [B, C, HW].  A label outside [0, K): NaN loss, NaN dlogits / dx rows,
    hit 0 (and NaN in every sum it enters)."""
    x, w, bias = (np.asarray(t, F64) for t in (x, w, bias))
    labels = np.asarray(labels, np.int64)
    B, C, HW = x.shape
    K = w.shape[0]
    pooled = x.mean(-1)
    logits = pooled @ w.T + bias
    m = logits.max(-1, keepdims=True)
    e = np.exp(logits - m)
    S = e.sum(-1, keepdims=True)
    p = e / S
    lse = (m + np.log(S))[:, 0]
    ok = (labels >= 0) & (labels < K)
    safe = np.where(ok, labels, 0)
    rows = np.arange(B)
    loss = np.where(ok, lse - logits[rows, safe], np.nan)
    hit = ok & (logits.argmax(-1) == labels)          # numpy's argmax returns the lowest index of the maximum
    onehot = np.zeros((B, K))
    onehot[rows, safe] = 1.0
    d = (p - onehot) * (g / B)
    d[~ok] = np.nan
    dx = np.repeat(((d @ w) / HW)[:, :, None], HW, -1)
    return SimpleNamespace(pooled=pooled, logits=logits, p=p, loss=loss, hit=hit, onehot=onehot, ok=ok, lse=lse, m=m[:, 0],
                           dlogits=d, dx=dx, dw=d.T @ pooled, db=d.sum(0), loss_sum=loss.sum(), hits=int(hit.sum()),
                           count=B, loss_mean=loss.sum() / B)


def bounds(ex, x, w, bias, g=1.0, any_order=False):
    """Per-element bounds of |kernel - model| for every output (the derivation in the module docstring).  Rows of a
    bad label are NaN in the model and are compared as NaN, not through a bound.
    any_order: the same derivation for an fp32 head whose summation orders are unknown (the library head): a sum of n
    terms passes a term through at most n - 1 additions in ANY order, so the chain lengths become nl = C + 1 (C - 1
    additions, the product, the bias), nS = K, nw = B + 1 and nb = B."""
    x, w, bias = (np.abs(np.asarray(t, F64)) for t in (x, w, bias))
    B, C, HW = x.shape
    K = w.shape[0]
    e_pool = gamma(HW + 1) * x.mean(-1)
    apool = np.abs(ex.pooled) + e_pool
    nl = C + 1 if any_order else math.ceil(C / 64) + 7
    e_logit = gamma(nl) * (apool @ w.T + bias) + e_pool @ w.T
    emax = e_logit.max(-1, keepdims=True)
    e_t = e_logit * (1 + U) + U * ((ex.m[:, None] - ex.logits) + emax)
    rho = np.exp(e_t) * (1 + EXP_U * U) - 1
    ns = K if any_order else math.ceil(K / 256) + 8
    rho_s = (ex.p * ((1 + rho) * (1 + gamma(ns)) - 1)).sum(-1, keepdims=True)
    e_p = ex.p * ((1 + rho) * (1 + U) / (1 - rho_s) - 1)
    r = -np.log1p(-rho_s[:, 0])
    e_log = r + LOG_U * U * ((ex.lse - ex.m) + emax[:, 0] + r)
    rows = np.arange(B)
    safe = np.where(ex.ok, np.argmax(ex.onehot, -1), 0)
    e_loss = (e_log + e_t[rows, safe]) * (1 + U) + U * np.abs(np.nan_to_num(ex.loss))
    q = np.abs(ex.p - ex.onehot)
    e_q = e_p * (1 + U) + U * q
    e_d = abs(g) / B * (e_q * (1 + gamma(2)) + gamma(2) * q)
    ad = np.abs(np.nan_to_num(ex.dlogits)) + e_d
    e_dx = (gamma(K + 1) * (ad @ w) + e_d @ w) / HW
    nw = B + 1 if any_order else math.ceil(B / 4) + 2
    e_dw = gamma(nw) * (ad.T @ apool) + e_d.T @ apool + np.abs(np.nan_to_num(ex.dlogits)).T @ e_pool
    nb = B if any_order else math.ceil(B / 256) + 8
    e_db = gamma(nb) * ad.sum(0) + e_d.sum(0)
    # loss_sum: the float64 sum of the fp32 losses (B roundings at 2^-53) ; loss_mean: that / B rounded to fp32
    e_sum = e_loss.sum() + gamma(B + 1) * 2.0 ** -29 * (np.abs(np.nan_to_num(ex.loss)) + e_loss).sum()
    e_mean = e_sum / B * (1 + U) + U * abs(np.nan_to_num(ex.loss_mean))
    return SimpleNamespace(pooled=e_pool, logits=e_logit, p=e_p, loss=e_loss, dlogits=e_d,
                           dx=np.repeat(e_dx[:, :, None], HW, -1), dw=e_dw, db=e_db, loss_sum=e_sum, loss_mean=e_mean)


# ------------------------------------------------------------------------ fp32 restatement in the kernel's order
def _fma(a, b, c):
    """fl32(a * b + c): the product of two fp32 values is exact in float64; the float64 addition rounds once more before
    the fp32 rounding (a double rounding that can differ from a true fmaf by one fp32 ulp in rare ties; this is a
    noise model, not a bit-exact oracle)."""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def _tree(v):
    """The 64-lane shfl_down tree over the last axis (length 64): lane 0's value."""
    v = v.copy()
    for off in (32, 16, 8, 4, 2, 1):
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
    return v[..., 0]


def _block_sum(per_thread):
    """[..., 256] fp32 per-thread values -> tree per wave, then (w0 + w1) + (w2 + w3)."""
    wv = _tree(per_thread.reshape(per_thread.shape[:-1] + (4, 64)))
    return (wv[..., 0] + wv[..., 1]) + (wv[..., 2] + wv[..., 3])


def _strided(v, n):
    """Chain over i = t, t + n, ... of the last axis for t in [0, n): [..., n] (acc starts at 0)."""
    L = v.shape[-1]
    acc = np.zeros(v.shape[:-1] + (n,), F32)
    for i0 in range(0, L, n):
        blk = v[..., i0:i0 + n]
        acc[..., :blk.shape[-1]] = acc[..., :blk.shape[-1]] + blk
    return acc


def emulate32(x, w, bias, labels, g=1.0, vec=None):
    """K23 in numpy float32, operation by operation in the kernel's order (np.exp / np.log stand in for expf / logf)."""
    x, w, bias = (np.asarray(t, F32) for t in (x, w, bias))
    labels = np.asarray(labels, np.int64)
    B, C, HW = x.shape
    K = w.shape[0]
    vec = (HW % 4 == 0) if vec is None else vec
    acc = np.zeros((B, C), F32)
    if vec:
        for j in range(0, HW, 4):
            acc = acc + ((x[..., j] + x[..., j + 1]) + (x[..., j + 2] + x[..., j + 3]))
    else:
        for j in range(HW):
            acc = acc + x[..., j]
    pooled = acc / F32(HW)
    lanes = np.zeros((B, K, 64), F32)
    for c0 in range(0, C, 64):
        n = min(64, C - c0)
        lanes[..., :n] = _fma(pooled[:, None, c0:c0 + n], w[None, :, c0:c0 + n], lanes[..., :n])
    logits = _tree(lanes) + bias[None, :]
    m = logits.max(-1, keepdims=True)
    e = np.exp(logits - m).astype(F32)
    S = _block_sum(_strided(e, 256))[:, None]
    p = e / S
    ok = (labels >= 0) & (labels < K)
    safe = np.where(ok, labels, 0)
    rows = np.arange(B)
    loss = np.where(ok, np.log(S[:, 0]).astype(F32) - (logits - m)[rows, safe], F32(np.nan)).astype(F32)
    hit = ok & (logits.argmax(-1) == labels)
    scale = F32(g) / F32(B)
    q = p.copy()
    q[rows, safe] = np.where(ok, p[rows, safe] - F32(1.0), p[rows, safe])
    d = (q * scale).astype(F32)
    d[~ok] = np.nan
    acc = np.zeros((B, C), F32)
    for k in range(K):
        acc = _fma(d[:, k:k + 1], w[k:k + 1, :], acc)
    dx = np.repeat((acc / F32(HW))[:, :, None], HW, -1)
    part = np.zeros((4, K, C), F32)
    for b in range(B):
        part[b % 4] = _fma(d[b, :, None], pooled[b, None, :], part[b % 4])
    dw = (part[0] + part[1]) + (part[2] + part[3])
    db = _block_sum(_strided(np.ascontiguousarray(d.T), 256))
    tot = loss.astype(F64).sum()
    return SimpleNamespace(pooled=pooled, logits=logits, p=p, loss=loss, hit=hit, dlogits=d, dx=dx, dw=dw, db=db,
                           loss_sum=tot, hits=int(hit.sum()), count=B, loss_mean=F32(tot / B))


# ------------------------------------------------------------------------------------------------- inputs
SHAPES = [(B, C, HW, K) for B, C, HW, K in
          [(1, 24, 1, 2), (5, 24, 16, 10), (64, 512, 16, 10), (257, 24, 64, 100), (5, 512, 64, 2), (64, 24, 1, 100),
           (257, 512, 16, 10), (1, 512, 64, 100), (5, 24, 64, 100), (64, 512, 1, 2), (257, 24, 16, 2), (1, 24, 16, 10)]]
"""Every B in {1, 5, 64, 257}, C in {24, 512}, HW in {1, 16, 64} and K in {2, 10, 100} occurs, every pair of values of
two different dimensions at least once where twelve cases allow: B = 257 takes the second trip of the grid-stride-free
batch loops (b = tid + 256) and a ragged wave split of dW; C = 24 leaves lanes idle in the logit chains and C = 512
gives them 8 steps; HW = 1 is the scalar route, 16 and 64 the float4 route; K = 2 leaves three waves without a class."""


ALL_SHAPES = [(B, C, HW, K) for B in (1, 5, 64, 257) for C in (24, 512) for HW in (1, 16, 64) for K in (2, 10, 100)]
"""The whole grid (the GPU test runs it; the CPU tests keep to SHAPES, whose float32 restatement loops in Python)."""


def gaussian(shape, seed=0, amp=1.0):
    """x ~ N(0, 1), w ~ N(0, amp^2 / C) (logits of spread ~ amp / sqrt(HW)... times sqrt(HW) restored below), bias
    ~ N(0, 0.1^2), labels uniform; fp32 values."""
    B, C, HW, K = shape
    r = np.random.default_rng(1000 * B + 100 * HW + 10 * K + C + seed)
    x = r.standard_normal((B, C, HW)).astype(F32)
    w = (r.standard_normal((K, C)) * (amp * math.sqrt(HW / C))).astype(F32)   # pooled ~ N(0, 1/HW): logits ~ N(0, amp^2)
    bias = (r.standard_normal(K) * 0.1).astype(F32)
    labels = r.integers(0, K, B).astype(np.int64)
    return x, w, bias, labels


def uniform_logits(shape):
    """w = 0 and bias = 3: every logit is 3, t = 0, e = 1, S = K, and with K a power of two p = 1 / K exactly; with B a
    power of two and g = +-2^j, dlogits = (1 / K - onehot) g / B exactly, dx = 0, dW = dlogits^T pooled.  x is Gaussian.
    Premise (asserted in test_cls_head_ref_cpu.py): K and B are powers of two."""
    B, C, HW, K = shape
    r = np.random.default_rng(B + C + HW + K)
    x = r.standard_normal((B, C, HW)).astype(F32)
    labels = r.integers(0, K, B).astype(np.int64)
    return x, np.zeros((K, C), F32), np.full(K, 3.0, F32), labels


def dyadic(shape, shift=0.0):
    """Inputs on which pooled, logits, dlogits' linear images dW / db / dx are exact in fp32 whatever the order:
    x = integers in [-8, 8] (plane sums are integers below 2^10; HW a power of two makes the mean exact), w = integers
    in [-4, 4] / 8, bias = integers in [-4, 4] / 8 (+ shift).  |pooled| <= 8 in steps of 1 / HW, |logit - bias| <=
    C * 8 * 0.5 in steps of 1 / (8 HW): below 2^24 steps for C <= 512, HW <= 64.  dW / db / dx are exact only for an
    exact dlogits, which the caller supplies (see `dyadic_dlogits`).  Premise: HW is a power of two."""
    B, C, HW, K = shape
    r = np.random.default_rng(7 * B + C + 3 * HW + K)
    x = r.integers(-8, 9, (B, C, HW)).astype(F32)
    w = (r.integers(-4, 5, (K, C)) / 8.0).astype(F32)
    bias = (r.integers(-4, 5, K) / 8.0 + shift).astype(F32)
    labels = r.integers(0, K, B).astype(np.int64)
    return x, w, bias, labels


def dyadic_p(shape):
    """A p whose backward is exact: p[b, k] = integers in [0, 16] / 16 (it need not sum to one: the backward kernels
    take p as data).  With g = 1 and B a power of two, dlogits = (p - onehot) / B is exact (multiples of 1 / (16 B)),
    and against the dyadic pooled (multiples of 1 / HW, |.| <= 8) and w (multiples of 1 / 8, |.| <= 0.5):
    dW = sum_b dlogits pooled has steps 1 / (16 B HW) and magnitude <= 8: below 2^24 steps for B HW <= 2^13;
    dx = (sum_k dlogits w) / HW and db likewise.  Premise: B and HW powers of two, B * HW <= 8192."""
    B, C, HW, K = shape
    r = np.random.default_rng(11 * B + C + HW + 5 * K)
    return (r.integers(0, 17, (B, K)) / 16.0).astype(F32)


def rel_size(bound, ref):
    """bound / |ref| over the elements with ref != 0 (how many times its own value an element may move)."""
    ref = np.abs(np.asarray(ref, F64)).reshape(-1)
    b = np.asarray(bound, F64).reshape(-1)
    keep = ref > 0
    return b[keep] / ref[keep]


# The non-vacuity number of test_cls_head_ref_cpu.py.  The leading term of every bound is the pooling error carried
# through a sum over the channels: E_pool ~ (HW + 1) u mean|x| per channel, against |pooled| ~ mean|x| sqrt(pi / 2) /
# sqrt(HW) (a mean of HW zero-mean terms), so a pooled element may move by about (HW + 1) sqrt(HW) u of its own size;
# a logit sums C such terms whose signed values cancel like sqrt(C) while the bound adds their magnitudes: another
# factor sqrt(C).  At the largest shapes tested (HW = 64, C = 512) that is 65 * sqrt(64 * 512) u = 7.0e-4; the factor 2
# covers the remaining first-order terms (gamma_nl, the exp / division roundings), all of which are O(10 u).
MEDIAN_REL_LIMIT = 2 * 65 * math.sqrt(64 * 512) * U
