"""K13 (csrc/salun_attn.hip) against the float64 model of attn_ref_cpu.py (validated by test_attn_ref_cpu.py):

(a) per-element bounds on Gaussian inputs at amplitudes 1 and 2.5 (peaked softmax, scores of tens), the latter also with
    the keys sorted by the mean query's score, and two constructions in which every query's running maximum grows on
    every tile / never after the first.  Hard tier: every element of
    o, dq, dk, dv within 1.25 * B1 of the exact answer (B1 = the first-order bound of the declared rounding points; 1.25
    covers the (1+u) cross terms and the fp32 accumulation; no absolute slack).  Sharp tier: against the kernel-faithful
    float64 model, at most 1 % of a tensor beyond ulp_bf16 + B1/8 (a dominant p on a bf16 tie may flip) and nothing
    beyond ulp_bf16 + 2*B1.  lse within 2^-16 + 2^-21*|lse2| (argument error |s*c| * 2^-24 at |s*c| <= 128 plus one ulp
    each of v_exp / v_log).
(b) constructions with known answers: a one-hot softmax (o = the selected v row, dv = integer sums, dq = dk = 0, all bit
    for bit) and a uniform one (o = count_d / Nk).
(c) invariances, bit for bit: (b, h) slices computed alone, NaN in every row and column the views do not own, strided
    outputs behind sentinels, the backward on column slices of a fused projection.

Forward and backward are judged separately: the backward is given the MODEL's bf16 o and fp32 lse, so a one-ulp flip in
the kernel's forward cannot leak into the backward's verdict.  Layouts as in test_attn_gpu.py: [B, tokens, H*D] storage
viewed as [B, tokens, H, D].
"""
import math
import os
from ctypes import c_double, c_longlong, c_void_p
from functools import lru_cache
from types import SimpleNamespace

import pytest
import torch

import attn_ref_cpu as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = 0x7FA5          # a bf16 NaN pattern no result holds

# (shape, amplitude of q and k, key order)
CASES = [(s, a, o) for s in R.SHAPES for a, o in ((1.0, None), (2.5, None), (2.5, "asc"), (2.5, "desc"))]
# the running maximum growing on every tile / on none after the first, for every query (shapes with more than one tile)
CASES += [(s, 1.0, o) for s in R.SHAPES if s[3] > R.KT for o in ("grow", "settle")]
ONEHOT_SHAPES = [s for s in R.SHAPES if s[3] <= R.onehot_capacity(s[4])]


def _sid(shape):
    return "x".join(map(str, shape))


def _cid(case):
    return f"{_sid(case[0])}-a{case[1]}-{case[2] or 'drawn'}"


# ------------------------------------------------------------------------------------------ host <-> device
def dev(t):
    """[B, H, N, D] float64 holding bf16 values -> [B, N, H, D] bf16 view of contiguous [B, N, H*D] device storage."""
    return t.permute(0, 2, 1, 3).contiguous().to(torch.bfloat16).cuda()


def dev_lse(lse2):
    return lse2.float().reshape(-1, lse2.shape[-1]).contiguous().cuda()


def host(t):
    """[B, N, H, D] bf16 device tensor -> [B, H, N, D] float64."""
    return t.float().cpu().double().permute(0, 2, 1, 3)


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def log(line):
    print(line)
    d = os.environ.get("SALUN_MEASURED_DIR")      # where a recording run keeps its figures (profiles/ has the last ones)
    if d and os.path.isdir(d):
        with open(os.path.join(d, "attn_bounds_measured.txt"), "a") as f:
            f.write(line + "\n")


# ------------------------------------------------------------------------------------------ shared references
@lru_cache(maxsize=None)
def case(shape, amp, order):
    q, k, v, d_o, scale = R.gaussian(shape, amp, order)
    ex = R.exact(q, k, v, d_o, scale)
    assert float(ex.s.abs().max()) <= 60.0          # the lse bound below is derived for |s*scale| <= 60
    return SimpleNamespace(q=q, k=k, v=v, d_o=d_o, scale=scale, ex=ex, b1=R.bounds(ex, q, k, v, d_o, scale),
                           em=R.emulate(q, k, v, d_o, scale), shape=shape)


def lse_bound(lse2):
    return 2.0 ** -16 + 2.0 ** -21 * lse2.abs()


def tiers(tag, name, got, ex, em, b1):
    """Both tiers for one tensor; the measured figures are printed (and logged) before anything is asserted."""
    err_x, err_m, ulp = (got - ex).abs(), (got - em).abs(), R.ulp_bf16(em)
    pos = b1 > 0
    hard = torch.where(pos, err_x / b1.clamp_min(1e-300), torch.where(err_x > 0, math.inf, 0.0).to(torch.float64))
    sharp = torch.where(pos, (err_m - ulp) / b1.clamp_min(1e-300),
                        torch.where(err_m > ulp, math.inf, 0.0).to(torch.float64)).clamp_min(0.0)
    share = float((err_m > ulp + b1 / 8).double().mean())
    log(f"{tag} {name}: hard {float(hard.max()):.3f} B1, sharp share {share:.5f} worst ulp + {float(sharp.max()):.3f} B1")
    assert (err_x <= 1.25 * b1).all(), f"{name}: {float(hard.max()):.3f} B1 from the exact answer"
    assert share <= 0.01, f"{name}: {share:.4f} of the elements beyond ulp + B1/8 of the model"
    assert (err_m <= ulp + 2 * b1).all(), f"{name}: ulp + {float(sharp.max()):.3f} B1 from the model"


# ------------------------------------------------------------------------------------------ (a) per-element bounds
@pytest.mark.parametrize("cs", CASES, ids=_cid)
def test_forward_within_per_element_bounds(cs):
    from unlearn_saliency_amd import ops
    c = case(*cs)
    B, H, Nq, Nk, D = c.shape
    o, lse = ops.attn_forward(dev(c.q), dev(c.k), dev(c.v), c.scale)
    assert o.shape == (B, Nq, H, D) and o.dtype == torch.bfloat16 and lse.shape == (B * H, Nq)
    lse = lse.cpu().double().view(B, H, Nq)
    e_lse = (lse - c.ex.lse2).abs()
    log(f"{_cid(cs)} lse: {float((e_lse / lse_bound(c.ex.lse2)).max()):.3f} of its bound, |lse2| <= "
        f"{float(c.ex.lse2.abs().max()):.1f}")
    tiers(_cid(cs), "o", host(o), c.ex.o, c.em.o, c.b1.o)
    assert (e_lse <= lse_bound(c.ex.lse2)).all()


@pytest.mark.parametrize("cs", CASES, ids=_cid)
def test_backward_within_per_element_bounds(cs):
    from unlearn_saliency_amd import ops
    c = case(*cs)
    dq, dk, dv = ops.attn_backward(dev(c.q), dev(c.k), dev(c.v), dev(c.em.o), dev(c.d_o), dev_lse(c.em.lse2), c.scale)
    for name, got in (("dq", dq), ("dk", dk), ("dv", dv)):
        tiers(_cid(cs), name, host(got), getattr(c.ex, name), getattr(c.em, name), getattr(c.b1, name))


# ------------------------------------------------------------------------------------------ (b) exact answers
@pytest.mark.parametrize("shape", ONEHOT_SHAPES, ids=_sid)
def test_onehot_softmax_is_exact(shape):
    """Any slip in the P.V operand pairing, in a mask, or in a head / batch stride changes these answers by whole
    integers; every loser's p is 2^-200 or less, i.e. 0 in fp32."""
    from unlearn_saliency_amd import ops
    B, H, Nq, Nk, D = shape
    q, k, v, d_o, scale, sel, A = R.onehot_code(shape)
    o, lse = ops.attn_forward(dev(q), dev(k), dev(v), scale)
    assert same_bits(o, dev(v[:, :, sel]))
    # the winner's score is 2A^2 exactly; c is the kernel's fp32 scale * log2(e)
    want = torch.tensor(2 * A * A, dtype=torch.float32) * (torch.tensor(scale, dtype=torch.float32) *
                                                           torch.tensor(R.LOG2E, dtype=torch.float32))
    ulp32 = 2.0 ** (math.floor(math.log2(float(want))) - 23)
    assert float((lse.cpu().double() - want.double()).abs().max()) <= ulp32
    em_o, em_lse = R.emulate_forward(q, k, v, scale)
    dq, dk, dv = ops.attn_backward(dev(q), dev(k), dev(v), dev(em_o), dev(d_o), dev_lse(em_lse), scale)
    assert same_bits(dv, dev(torch.zeros_like(v).index_add_(2, sel, d_o)))
    assert not bits(dq).any() and not bits(dk).any()      # dP = Dq exactly for the winner, p = 0 for everyone else


@pytest.mark.parametrize("shape", R.SHAPES, ids=_sid)
def test_uniform_softmax_counts_the_keys(shape):
    from unlearn_saliency_amd import ops
    B, H, Nq, Nk, D = shape
    q, k, v, d_o, scale, count = R.uniform_counts(shape)
    o, lse = ops.attn_forward(dev(q), dev(k), dev(v), scale)
    want = (count.float() * (torch.tensor(1.0) / torch.tensor(float(Nk)))).to(torch.bfloat16)     # fp32 product, one rounding
    want = want.expand(B, Nq, H, D)
    if Nk in (64, 128):
        assert same_bits(o.cpu(), want)
    else:
        assert ((o.cpu().double() - want.double()).abs() <= R.ulp_bf16(want.double())).all()
    lse2 = torch.full((B * H, Nq), math.log2(Nk), dtype=torch.float64)
    assert ((lse.cpu().double() - lse2).abs() <= lse_bound(lse2)).all()
    em_o, em_lse = R.emulate_forward(q, k, v, scale)
    _, dk, _ = ops.attn_backward(dev(q), dev(k), dev(v), dev(em_o), dev(d_o), dev_lse(em_lse), scale)
    assert not bits(dk).any()                              # dk = dS^T @ q with q = 0


# ------------------------------------------------------------------------------------------ (c) invariances
def _device_case(shape):
    c = case(shape, 2.5, None)
    return SimpleNamespace(q=dev(c.q), k=dev(c.k), v=dev(c.v), o=dev(c.em.o), d_o=dev(c.d_o), lse=dev_lse(c.em.lse2),
                           scale=c.scale)


@pytest.mark.parametrize("shape", R.SHAPES, ids=_sid)
def test_every_slice_alone_equals_its_part_of_the_batched_call(shape):
    from unlearn_saliency_amd import ops
    B, H, Nq, Nk, D = shape
    t = _device_case(shape)
    o, lse = ops.attn_forward(t.q, t.k, t.v, t.scale)
    dq, dk, dv = ops.attn_backward(t.q, t.k, t.v, t.o, t.d_o, t.lse, t.scale)
    for b in range(B):
        for h in range(H):
            cut = lambda x: x[b:b + 1, :, h:h + 1].contiguous()
            o1, lse1 = ops.attn_forward(cut(t.q), cut(t.k), cut(t.v), t.scale)
            assert same_bits(o1, cut(o)) and torch.equal(lse1, lse[b * H + h:b * H + h + 1])
            got = ops.attn_backward(cut(t.q), cut(t.k), cut(t.v), cut(t.o), cut(t.d_o),
                                    t.lse[b * H + h:b * H + h + 1].contiguous(), t.scale)
            for g1, g in zip(got, (dq, dk, dv)):
                assert same_bits(g1, cut(g))


def _in_nan_padding(x):
    """The [B, N, H, D] tensor as a view of a NaN-filled buffer with 5 more token rows per batch and 8 more columns
    behind H*D in every token row."""
    B, N, H, D = x.shape
    buf = torch.full((B, N + 5, H * D + 8), NAN, dtype=torch.bfloat16, device=x.device)
    buf[:, :N, :H * D] = x.reshape(B, N, H * D)
    return buf[:, :N, :H * D].unflatten(-1, (H, D))


@pytest.mark.parametrize("shape", R.SHAPES, ids=_sid)
def test_rows_and_columns_past_the_end_are_never_read(shape):
    from unlearn_saliency_amd import ops
    t = _device_case(shape)
    p = SimpleNamespace(**{n: _in_nan_padding(getattr(t, n)) for n in ("q", "k", "v", "o", "d_o")})
    assert all(same_bits(getattr(p, n), getattr(t, n)) and not getattr(p, n).is_contiguous() for n in ("q", "k", "v"))
    o, lse = ops.attn_forward(t.q, t.k, t.v, t.scale)
    o_p, lse_p = ops.attn_forward(p.q, p.k, p.v, t.scale)
    assert same_bits(o_p, o) and torch.equal(lse_p, lse)
    assert not o_p.isnan().any() and not lse_p.isnan().any()
    grads = ops.attn_backward(t.q, t.k, t.v, t.o, t.d_o, t.lse, t.scale)
    grads_p = ops.attn_backward(p.q, p.k, p.v, p.o, p.d_o, t.lse, t.scale)
    for g_p, g in zip(grads_p, grads):
        assert same_bits(g_p, g) and not g_p.isnan().any()


@pytest.mark.parametrize("shape", R.SHAPES, ids=_sid)
def test_strided_output_is_written_only_where_it_is_owned(shape):
    """The forward through the C-ABI with o at token pitch H*D + 8 and 3 spare rows per batch: every byte outside the
    [B, Nq, H, D] view keeps its sentinel, the view holds the contiguous call's result."""
    from unlearn_saliency_amd import _lib, ops
    from unlearn_saliency_amd.streams import _stream
    B, H, Nq, Nk, D = shape
    t = _device_case(shape)
    o, lse = ops.attn_forward(t.q, t.k, t.v, t.scale)
    HD, pitch, rows = H * D, H * D + 8, Nq + 3
    buf = torch.full((B, rows, pitch), SENTINEL, dtype=torch.int16, device="cuda")
    lse_s = torch.empty_like(lse)
    ptr = lambda x: c_void_p(x.data_ptr())
    rc = _lib.lib().salun_attn_forward(ptr(t.q), ptr(t.k), ptr(t.v), ptr(buf), ptr(lse_s), B, H, Nq, Nk, D,
                                       c_longlong(Nq * HD), HD, c_longlong(Nk * HD), HD, c_longlong(Nk * HD), HD,
                                       c_longlong(rows * pitch), pitch, c_double(t.scale), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[:, :Nq, :HD], bits(o).view(B, Nq, HD)) and torch.equal(lse_s, lse)
    outside = buf.clone()
    outside[:, :Nq, :HD] = SENTINEL
    assert bool((outside == SENTINEL).all())


@pytest.mark.parametrize("shape", [(2, 3, 97, 97, 40), (2, 2, 33, 33, 160), (1, 3, 130, 130, 16)], ids=_sid)
def test_backward_on_strided_views_of_a_fused_projection(shape):
    """q / k / v as column slices of one [B, N, 3*H*D] projection and dO as a slice of a wider tensor: read in place,
    bit for bit what the contiguous copies give (the backward twin of test_attn_gpu's forward test)."""
    from unlearn_saliency_amd import ops
    B, H, N, _, D = shape
    HD = H * D
    g = torch.Generator().manual_seed(5 + N)
    qkv = torch.randn(B, N, 3 * HD, generator=g).to(torch.bfloat16).cuda()
    wide = torch.randn(B, N, 2 * HD + 8, generator=g).to(torch.bfloat16).cuda()
    q, k, v = (qkv[..., i * HD:(i + 1) * HD].unflatten(-1, (H, D)) for i in range(3))
    d_o = wide[..., 8:8 + HD].unflatten(-1, (H, D))
    scale = D ** -0.5
    o, lse = ops.attn_forward(q, k, v, scale)
    got = ops.attn_backward(q, k, v, o, d_o, lse, scale)
    want = ops.attn_backward(q.contiguous(), k.contiguous(), v.contiguous(), o, d_o.contiguous(), lse, scale)
    for a, b in zip(got, want):
        assert same_bits(a, b) and not a.isnan().any()
