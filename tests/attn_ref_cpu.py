"""torch-float64 restatement of K13 (csrc/salun_attn.hip) on the CPU (test infrastructure only, like esd_ref_cpu.py):
the exact softmax(scale * q k^T) v with its gradients, the first-order per-element error bound of the rounding points the
kernel header declares, a kernel-faithful model of the tiled online softmax, and the two input constructions with known
answers.  Everything works on [B, H, N, D] tensors holding bf16-representable values.

Rounding points (salun_attn.hip header): P and dS go to bf16 for the second GEMMs; O, dQ, dK, dV are stored as bf16; the
backward's D_q = sum_d dO*O is formed from the bf16 O.  Scores, softmax and all accumulation are fp32.
"""
import math
from types import SimpleNamespace

import torch

U = 2.0 ** -8            # bf16 unit roundoff (round to nearest even, 8 significand bits)
KT = 64                  # keys per tile of the forward's online softmax
LOG2E = 1.4426950408889634
F64 = torch.float64


# ------------------------------------------------------------------------------------------ number formats
def bf16_round(x):
    """Round to the nearest bf16 value (ties to even), result in x's dtype.  float64 is rounded in ONE step on its bit
    pattern (through float32 it would round twice); magnitudes under 2^-120 take the float32 route, which flushes what
    bf16 cannot hold."""
    if x.dtype != F64:
        return x.to(torch.bfloat16).to(x.dtype)
    bits = x.contiguous().view(torch.int64)
    bits = (bits + ((bits >> 45) & 1) + ((1 << 44) - 1)) & ~((1 << 45) - 1)
    tiny = x.abs() < 2.0 ** -120
    return torch.where(tiny, x.float().to(torch.bfloat16).to(F64), bits.view(F64))


def fp32_round(x):
    return x.float().to(x.dtype)


def ulp_bf16(x):
    """2^(floor(log2|x|) - 7): the spacing of bf16 values at |x|; 0 at 0."""
    _, e = torch.frexp(x.to(F64).abs())              # |x| = m * 2^e with m in [0.5, 1): floor(log2|x|) = e - 1
    return torch.where(x == 0, torch.zeros((), dtype=F64), torch.ldexp(torch.ones((), dtype=F64), e - 8))


def is_bf16(x):
    return bool(torch.equal(bf16_round(x.to(F64)), x.to(F64)))


# ------------------------------------------------------------------------------------------ exact answer
def exact(q, k, v, d_o, scale):
    """float64 o, lse2 (log2 units: what the kernel stores), dq, dk, dv of softmax(scale * q k^T) v, plus P,
    dS = P * (dP - Dq) * scale and Dq = sum_d dO * O."""
    q, k, v, d_o = (t.to(F64) for t in (q, k, v, d_o))
    s = q @ k.transpose(-1, -2) * scale
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    o = P @ v
    dP = d_o @ v.transpose(-1, -2)
    Dq = (d_o * o).sum(-1)
    dS = P * (dP - Dq[..., None]) * scale
    return SimpleNamespace(o=o, lse2=lse / math.log(2.0), dq=dS @ k, dk=dS.transpose(-1, -2) @ q,
                           dv=P.transpose(-1, -2) @ d_o, P=P, dS=dS, Dq=Dq, s=s)


def bounds(ex, q, k, v, d_o, scale):
    """First-order per-element bound B1 of |kernel - exact| for o, dq, dk, dv, from exactly the rounding points above."""
    q, k, v, d_o = (t.to(F64).abs() for t in (q, k, v, d_o))
    P, Pt = ex.P, ex.P.transpose(-1, -2)
    b_o = U * (P @ v) + U * ex.o.abs()
    b_dv = U * (Pt @ d_o) + U * ex.dv.abs()
    d_Dq = (d_o * b_o).sum(-1)
    b_dS = U * ex.dS.abs() + scale * P * d_Dq[..., None]
    b_dq = b_dS @ k + U * ex.dq.abs()
    b_dk = b_dS.transpose(-1, -2) @ q + U * ex.dk.abs()
    return SimpleNamespace(o=b_o, dq=b_dq, dk=b_dk, dv=b_dv)


# ------------------------------------------------------------------------------------------ kernel-faithful model
def emulate_forward(q, k, v, scale, dtype=F64):
    """The forward as the kernel runs it, accumulating in `dtype`: keys in tiles of 64, a running per-query maximum
    m_new = max(m, max_tile(s) * c) with c = scale * log2(e), p = exp2(s*c - m_new), l = l*alpha + sum(p) on the
    unrounded p, acc = acc*alpha + bf16(p) @ v_tile; o = bf16(acc / l), lse2 = fp32(m + log2 l)."""
    q, k, v = (t.to(dtype) for t in (q, k, v))
    Nk = k.shape[-2]
    c = (torch.tensor(scale, dtype=dtype) * torch.tensor(LOG2E, dtype=dtype))
    m = torch.full(q.shape[:-1], -math.inf, dtype=dtype)
    l = torch.zeros(q.shape[:-1], dtype=dtype)
    acc = torch.zeros(q.shape[:-1] + (v.shape[-1],), dtype=dtype)
    for j0 in range(0, Nk, KT):
        s = q @ k[..., j0:j0 + KT, :].transpose(-1, -2)
        m_new = torch.maximum(m, s.max(-1).values * c)
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(s * c - m_new[..., None])
        l = l * alpha + p.sum(-1)
        acc = acc * alpha[..., None] + bf16_round(p) @ v[..., j0:j0 + KT, :]
        m = m_new
    return bf16_round(acc / l[..., None]), fp32_round(m + torch.log2(l))


def emulate_backward(q, k, v, o, d_o, lse2, scale, dtype=F64):
    """The backward as the kernels run it, from a given bf16 o and fp32 lse2: P = exp2(s*c - lse2), Dq = sum dO*o,
    dS = bf16(P*(dP - Dq)*scale), dv = bf16(bf16(P)^T @ dO), dq = bf16(dS @ k), dk = bf16(dS^T @ q)."""
    q, k, v, o, d_o, lse2 = (t.to(dtype) for t in (q, k, v, o, d_o, lse2))
    c = (torch.tensor(scale, dtype=dtype) * torch.tensor(LOG2E, dtype=dtype))
    s = q @ k.transpose(-1, -2)
    P = torch.exp2(s * c - lse2[..., None])
    Dq = (d_o * o).sum(-1)
    dP = d_o @ v.transpose(-1, -2)
    dS = bf16_round(P * (dP - Dq[..., None]) * torch.tensor(scale, dtype=dtype))
    dv = bf16_round(bf16_round(P).transpose(-1, -2) @ d_o)
    return bf16_round(dS @ k), bf16_round(dS.transpose(-1, -2) @ q), dv


def emulate(q, k, v, d_o, scale, dtype=F64):
    """-> o, lse2, dq, dk, dv (float64 tensors holding the model's values).  dtype=float64 is the reference; float32 is a
    noise model of a correct fp32 implementation."""
    o, lse2 = emulate_forward(q, k, v, scale, dtype)
    dq, dk, dv = emulate_backward(q, k, v, o, d_o, lse2, scale, dtype)
    return SimpleNamespace(o=o.to(F64), lse2=lse2.to(F64), dq=dq.to(F64), dk=dk.to(F64), dv=dv.to(F64))


# ------------------------------------------------------------------------------------------ inputs
# (B, H, Nq, Nk, D): the smallest shapes at which each boundary exists — 128 queries per workgroup and 32 per wave,
# 64-key tiles in forward and dQ, 32-query tiles and 128 keys per workgroup in dK/dV — and every supported D.
SHAPES = [(2, 3, 33, 65, 8), (2, 3, 16, 7, 16), (2, 3, 1, 1, 32), (2, 3, 130, 77, 40), (2, 3, 31, 64, 40),
          (2, 3, 129, 129, 64), (2, 3, 65, 127, 80), (2, 3, 128, 128, 80), (1, 2, 40, 129, 160), (2, 2, 33, 77, 160),
          (1, 3, 127, 193, 32)]


def gaussian(shape, amp, order=None):
    """bf16-valued Gaussian q, k (times `amp`), v, dO (at 1).  order = "asc" / "desc" sorts every (b, h) slice's keys (k and
    v together) by mean_q(q) . k: ascending makes the running maximum grow tile after tile (the rescale branch runs every
    time), descending settles it in the first tile (the branch never runs again) — as far as one order can serve every
    query: with zero-mean q the mean query says little about any single one.  order = "grow" / "settle" (amplitude 1)
    force the two regimes for EVERY query: channel 0 of q is 4 and channel 0 of k is step * (tile index) — counted from
    the last tile for "settle" —, step the power of two with 4 * step * scale >= 10, more than the Gaussian part of the
    scaled scores spans (test_attn_ref_cpu.py asserts that)."""
    B, H, Nq, Nk, D = shape
    g = torch.Generator().manual_seed(1000 * Nq + 10 * Nk + D)
    rn = lambda n, a: bf16_round(torch.randn(B, H, n, D, generator=g, dtype=F64) * a)
    q, k, v, d_o = rn(Nq, amp), rn(Nk, amp), rn(Nk, 1.0), rn(Nq, 1.0)
    if order in ("grow", "settle"):
        step = 2.0 ** math.ceil(math.log2(2.5 * D ** 0.5))
        tile = torch.arange(Nk, dtype=F64) // KT
        q[..., 0] = 4.0
        k[..., 0] = step * (tile if order == "grow" else (Nk - 1) // KT - tile)
    elif order is not None:
        key = (q.mean(-2, keepdim=True) * k).sum(-1)
        idx = torch.argsort(key, -1, descending=(order == "desc"))[..., None].expand(-1, -1, -1, D)
        k, v = torch.gather(k, 2, idx), torch.gather(v, 2, idx)
    return q, k, v, d_o, D ** -0.5


def onehot_capacity(D):
    h = D // 2 if D <= 32 else 8
    return h * (D - h)


def onehot_code(shape):
    """Key j and the query that selects it carry A*(e_{j mod h} + e_{h + j div h}), h = D/2 for D <= 32 and 8 otherwise:
    the selected key scores 2A^2, every other at most A^2.  A is the smallest power of two with
    A^2 * scale * log2(e) >= 200, so every other key's p is 0 in fp32 and the softmax is one-hot exactly.  v and dO are
    integers in [-4, 4].  Query i selects key (g*i + 3) mod Nk, g the smallest integer >= 7 coprime with Nk (7 itself
    unless 7 | Nk), so the queries walk through every key.  -> q, k, v, d_o, scale, sel [Nq], A."""
    B, H, Nq, Nk, D = shape
    assert Nk <= onehot_capacity(D)
    scale = D ** -0.5
    h = D // 2 if D <= 32 else 8
    A = 1.0
    while A * A * scale * LOG2E < 200:
        A *= 2
    j = torch.arange(Nk)
    code = torch.zeros(Nk, D, dtype=F64)
    code[j, j % h] = A
    code[j, h + j // h] = A
    step = next(s for s in range(7, 7 + Nk + 1) if math.gcd(s, Nk) == 1)
    sel = (step * torch.arange(Nq) + 3) % Nk
    g = torch.Generator().manual_seed(77 * Nq + Nk + D)
    ints = lambda n: torch.randint(-4, 5, (B, H, n, D), generator=g).to(F64)
    k = code.expand(B, H, Nk, D).clone()
    q = code[sel].expand(B, H, Nq, D).clone()
    return q, k, ints(Nk), ints(Nq), scale, sel, A


def uniform_counts(shape):
    """q = 0 and v[j, d] = (j mod D == d): every p is 1, so o[i, d] = count_d / Nk with count_d = #{j < Nk: j mod D == d}
    and lse2 = log2 Nk; a dropped or an extra key changes count_d or Nk.  k and dO are Gaussian (the backward's
    dk = dS^T @ q is 0 whatever they are).  -> q, k, v, d_o, scale, count [D]."""
    B, H, Nq, Nk, D = shape
    g = torch.Generator().manual_seed(13 * Nq + Nk + D)
    rn = lambda n: bf16_round(torch.randn(B, H, n, D, generator=g, dtype=F64))
    j = torch.arange(Nk)
    v1 = torch.zeros(Nk, D, dtype=F64)
    v1[j, j % D] = 1.0
    count = v1.sum(0)
    return torch.zeros(B, H, Nq, D, dtype=F64), rn(Nk), v1.expand(B, H, Nk, D).clone(), rn(Nq), D ** -0.5, count
