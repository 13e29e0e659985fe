"""The normalisation kernels (csrc/salun_norm.hip: fused BatchNorm and fp32 GroupNorm; csrc/salun_norm_bf16.hip: K12)
against the float64 model of norm_ref_cpu.py (validated by test_norm_ref_cpu.py), on every route of the host logic
(norm_ref_cpu.BN_CASES / GN_CASES / GN16_CASES):

(a) exact tier: inputs whose statistics, affine coefficients, outputs and backward sums are exact in fp32 in every
    summation order (the premise is asserted in test_norm_ref_cpu.py), so every output of every entry point must EQUAL
    the float64 answer: y, the saved statistics, the running mean, the counter, dx, dres, dgamma, dbeta, the `*_acc`
    targets pre-filled with integers, nk, csum, csum_acc, K12's mr / ab / y / dx / dgamma / dbeta.  running_var (M / (M - 1))
    within 2 fp32 ulp.  Where the backward divisor is not a power of two dx is exact in the vanishing family and within
    the bound in the other.  One case per family also goes through the C-ABI with every output and the workspace carved
    out of a sentinel-filled arena: nothing outside the outputs may change, no output element may stay unwritten.
(b) bound tier: Gaussian inputs; every element within the bound derived in norm_ref_cpu's docstring.  The worst
    |got - exact| / bound and the worst error in units of u * abs are printed and logged (SALUN_MEASURED_DIR;
    profiles/norm_bounds_measured.txt has the last recording); the bound is asserted, the ratio is recorded.
(c) conditioning: mu / sigma in {0, 2^4, 2^8}; beside the kernel's error that of torch's fp32 op on the same input.
(d) invariances, bit for bit; (e) degenerate sets; (f) the edges of the domain: refusals, and inputs and gradients off
    the 16-byte grid through fused_bn_act / fused_gn_act (a spy on the fused node says which path ran)."""
import itertools
import math
import os
from ctypes import c_size_t, c_void_p

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import norm_ref_cpu as R

pytestmark = pytest.mark.gpu

GUARD = 4096
NAN_BITS, SENTINEL = 0x7FC00000, 0x7FA5A5A5
EINVAL = -22
_id = R._cid
BF = torch.bfloat16


def L():
    from unlearn_saliency_amd import _lib
    return _lib.lib()


def stream():
    from unlearn_saliency_amd.streams import _stream
    return _stream()


def ops():
    from unlearn_saliency_amd import ops as o
    return o


def log(line):
    print(line)
    d = os.environ.get("SALUN_MEASURED_DIR")
    if d and os.path.isdir(d):
        with open(os.path.join(d, "norm_bounds_measured.txt"), "a") as f:
            f.write(line + "\n")


def dev(t, dtype=torch.float32):
    return None if t is None else t.to(dtype).cuda()


def host(t):
    return t.detach().float().cpu()


def same(got, want64):
    """Bit-for-bit equality with a float64 answer that fp32 holds exactly (+0 and -0 alike), nothing non-finite."""
    got = host(got).reshape(want64.shape)
    assert R.is_f32(want64), "the expected answer is not an fp32 number"
    return bool(torch.isfinite(got).all()) and torch.equal(got, want64.float())


def within_ulps(got, want64, n):
    got = host(got).double().reshape(want64.shape)
    ulp = 2.0 ** (torch.floor(torch.log2(want64.abs().clamp_min(2.0 ** -126))) - 23)
    return bool(((got - want64).abs() <= n * ulp).all())


def within(tag, got, exact, bound, absolute=None):
    """Every element within its bound; the measured ratios are logged first."""
    got = host(got).double().reshape(exact.shape)
    err = (got - exact).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    line = f"{tag}: worst |got - exact| / bound = {float(ratio.max()):.4f}"
    if absolute is not None:
        a = absolute.expand_as(exact) if absolute.shape != exact.shape else absolute
        line += f", worst |got - exact| = {float((err / (R.U * a.clamp_min(1e-300)))[a > 0].max()) if bool((a > 0).any()) else 0.0:.2f} u * abs"
    log(line)
    assert bool(torch.isfinite(got).all()), tag + ": non-finite"
    assert bool((err <= bound).all()), tag
    return float(ratio.max())


def pow2(n):
    return n & (n - 1) == 0


def families(Lset):
    return ("eps",) if Lset % 2 else ("eps0", "eps")


def heavy(c):
    """Over 2^20 elements: the case is there for its walk, not for the template variants; it runs two of each."""
    return c.N * c.C * c.H * c.W > 1 << 20


BOTH = [(True, True), (False, False)]


# ------------------------------------------------------------------------------------------ (a) exact tier: BatchNorm
@pytest.mark.parametrize("c", R.BN_CASES + [R.BN_BIG], ids=_id)
def test_bn_equals_the_exact_answer(c):
    N, C, H, W = c[:4]
    M, big = N * H * W, c is R.BN_BIG
    for family in (("eps0",) if big else families(M)):
        t = R.bn_inputs(c, "exact", family)
        x, g, b, r = dev(t.x), dev(t.gamma), dev(t.beta), dev(t.res)
        for relu, res in ([(True, True)] if big else BOTH if heavy(c) else itertools.product((False, True), repeat=2)):
            tag = (c[:4], family, relu, res)
            m = R.bn_forward(t.x, t.gamma, t.beta, t.res if res else None, relu, True, t.rm, t.rv, torch.tensor(5),
                             R.MOMENTUM, t.eps)
            rm, rv, nbt = dev(t.rm), dev(t.rv), torch.tensor(5, device="cuda")
            y, mean, invstd = ops().bn_forward(x, r if res else None, g, b, rm, rv, True, R.MOMENTUM, t.eps, relu, nbt)
            assert same(y, m.y) and same(mean, m.mean) and same(invstd, m.invstd), tag
            assert same(rm, m.running_mean) and within_ulps(rv, m.running_var, 2) and int(nbt) == 6, tag
            y0, mean0, _ = ops().bn_forward(x, r if res else None, g, b, None, None, True, R.MOMENTUM, t.eps, relu, None)
            assert torch.equal(y0, y) and torch.equal(mean0, mean), tag          # running_* null in train mode
            # eval mode on running statistics preset to the batch statistics: the bits of train mode
            ye, me, ie = ops().bn_forward(x, r if res else None, g, b, dev(m.mean), dev(m.var), False, R.MOMENTUM, t.eps,
                                          relu, None)
            assert torch.equal(ye, y) and torch.equal(me, mean) and torch.equal(ie, invstd), tag
            for train, dres in ([(True, True)] if big else BOTH if heavy(c) else itertools.product((False, True), repeat=2)):
                dys = [("plain", t.dy)]
                if train and not pow2(M):
                    dys.append(("vanishing", R.bn_vanishing_dy(t.x, m.y, m.mean, m.invstd, relu)))
                for name, dy in dys:
                    acc = dres                                   # the accumulators ride with one half of the variants
                    k = R.bn_backward(dy, m.y, t.x, t.gamma, m.mean, m.invstd, train, relu, dres,
                                      t.gacc if acc else None, t.bacc if acc else None)
                    ga, ba = (dev(t.gacc), dev(t.bacc)) if acc else (None, None)
                    dx, dr, dg, db = ops().bn_backward(dev(dy), y if relu else None, x, g, mean, invstd, train, relu, dres,
                                                       ga, ba)
                    assert same(dg, k.dgamma) and same(db, k.dbeta), tag + (train, dres, name)
                    if acc:
                        assert same(ga, k.gacc) and same(ba, k.bacc), tag + (train, dres, name)
                    if dres:
                        assert same(dr, k.dres), tag + (train, dres, name)
                    if not train or pow2(M) or name == "vanishing":
                        assert same(dx, k.dx), tag + (train, dres, name)
                    else:
                        bd = R.bn_backward_bound(dy, m.y, t.x, t.gamma, m.mean, m.invstd, train, relu)
                        within(f"bn dx exact-input {_id(c)} {family} relu={int(relu)} res={int(res)} dres={int(dres)}", dx, k.dx, bd.dx)


# ------------------------------------------------------------------------------------------ (a) exact tier: GroupNorm fp32
def gn_backward_call(t, c, dz, mean, rstd, silu, extra, acc):
    ga, ba = (dev(t.gacc), dev(t.bacc)) if acc else (None, None)
    ca = dev(t.cacc) if "csum_acc" in extra else None
    out = ops().gn_backward(dev(dz), dev(t.x), dev(t.gamma), dev(t.beta), mean, rstd, c.G, silu, ga, ba,
                            addend=dev(t.addend) if "addend" in extra else None, nk_sum="nk" in extra,
                            csum="csum" in extra, csum_acc=ca)
    return out + (None, None) * (len(out) == 3) + (ga, ba, ca)


@pytest.mark.parametrize("c", R.GN_CASES, ids=_id)
def test_gn_equals_the_exact_answer(c):
    N, C, H, W, G = c[:5]
    for family in families(C // G * H * W):
        t = R.gn_inputs(c, "exact", family)
        m = R.gn_forward(t.x, t.gamma, t.beta, G, t.eps)
        z, mean, rstd = ops().gn_forward(dev(t.x), dev(t.gamma), dev(t.beta), G, t.eps, False)
        assert same(z, m.y) and same(mean, m.mean) and same(rstd, m.rstd), (c[:5], family)
        for vanishing in (False, True):
            dz = R.gn_vanishing_dz(t.x, m.mean, m.rstd, G) if vanishing else t.dz
            ks = {a: R.gn_backward(dz, t.x, t.gamma, t.beta, m.mean, m.rstd, G, False, t.addend if a else None, t.cacc,
                                   t.gacc, t.bacc) for a in (False, True)}
            bd = None
            for extra in [()] + R.GN_EXTRA:
                tag = (c[:5], family, vanishing, extra)
                k, acc = ks["addend" in extra], len(extra) != 1
                dx, dg, db, nk, cs, ga, ba, ca = gn_backward_call(t, c, dz, mean, rstd, False, extra, acc)
                assert same(dg, k.dgamma) and same(db, k.dbeta), tag
                if acc:
                    assert same(ga, k.gacc) and same(ba, k.bacc), tag
                if R.exact_dx(c, vanishing):
                    assert same(dx, k.dx), tag
                elif extra in ((), ("addend", "nk")):
                    bd = R.gn_backward_bound(dz, t.x, t.gamma, t.beta, m.mean, m.rstd, G, False, t.addend if extra else None)
                    within(f"gn dx exact-input {_id(c)} {family} {'+'.join(extra) or 'plain'}", dx, k.dx, bd.dx)
                    if extra:
                        within(f"gn nk exact-input {_id(c)} {family}", nk, k.nk, bd.nk)
                if "nk" in extra and R.exact_nk(c, vanishing):
                    assert same(nk, k.nk), tag
                    if "csum" in extra:
                        assert same(cs, k.csum), tag
                    if "csum_acc" in extra:
                        assert same(ca, k.csum_acc), tag


# ------------------------------------------------------------------------------------------ (a) exact tier: K12
def k12_forward(t, c, silu):
    xn = dev(R.nhwc(t.x), BF)
    y, mr, ab = ops().gn_bf16_forward(xn, dev(t.gamma), dev(t.beta), c.G, t.eps, silu)
    return xn, y.permute(0, 3, 1, 2), mr, ab


def k12_backward(t, c, xn, dz, mr, ab, silu, accumulate):
    nan = lambda: torch.full((c.C,), float("nan"), device="cuda")
    gw, gb = (dev(t.gacc), dev(t.bacc)) if accumulate else (nan(), nan())
    dx = ops().gn_bf16_backward(dev(R.nhwc(dz), BF), xn, dev(t.gamma), mr, ab, c.G, silu, gw, gb, accumulate)
    return dx.permute(0, 3, 1, 2), gw, gb


@pytest.mark.parametrize("c", R.GN16_CASES, ids=_id)
def test_k12_equals_the_exact_answer(c):
    N, C, H, W, G = c[:5]
    for family in families(C // G * H * W):
        t = R.gn_inputs(c, "exact", family)
        m = R.gn16_forward(t.x, t.gamma, t.beta, G, t.eps)
        xn, y, mr, ab = k12_forward(t, c, False)
        assert same(y, m.y) and same(mr, m.mr) and same(ab, m.ab), (c[:5], family)
        for vanishing, accumulate in itertools.product((False, True), repeat=2):
            tag = (c[:5], family, vanishing, accumulate)
            dz = R.gn_vanishing_dz(t.x, m.mean, m.rstd, G) if vanishing else t.dz
            k = R.gn16_backward(dz, t.x, t.gamma, m.mr, m.ab, G, False, *((t.gacc, t.bacc) if accumulate else (None, None)))
            dx, gw, gb = k12_backward(t, c, xn, dz, mr, ab, False, accumulate)
            assert same(gw, k.dgamma) and same(gb, k.dbeta), tag
            if R.exact_dx(c, vanishing):
                assert same(dx, k.dx), tag
            else:
                bd = R.gn16_backward_bound(dz, t.x, t.gamma, m.mr, m.ab, G, False)
                within(f"k12 dx exact-input {_id(c)} {family} acc={int(accumulate)}", dx, k.dx64, bd.dx)


# ------------------------------------------------------------------------------------------ (a) through the C-ABI, in an arena
class Arena:
    """The tensors of one call as 32-bit words inside one flat device allocation, each between GUARD words: NaN around
    the inputs, a sentinel around and inside the outputs."""

    def __init__(self):
        self.parts, self.fills, self.n = {}, [], 0

    def put(self, name, data=None, dtype=torch.float32, words=None, out=False):
        w = None if data is None else data.to(dtype).contiguous().view(-1).view(torch.int32)
        words = w.numel() if w is not None else words
        start = self.n + GUARD
        end = (start + words + 3) // 4 * 4
        self.fills.append((self.n, end + GUARD, SENTINEL if out else NAN_BITS, start, w))
        self.parts[name] = (start, words, out)
        self.n = end + GUARD
        return self

    def upload(self):
        hostbuf = torch.empty(self.n, dtype=torch.int32)
        for lo, hi, bits, start, w in self.fills:
            hostbuf[lo:hi] = bits
            if w is not None:
                hostbuf[start:start + w.numel()] = w
        self.host, self.dev = hostbuf, hostbuf.cuda()
        return self

    def ptr(self, name):
        return c_void_p(self.dev.data_ptr() + 4 * self.parts[name][0]) if name in self.parts else c_void_p(None)

    def nbytes(self, name):
        return c_size_t(4 * self.parts[name][1])

    def check(self):
        torch.cuda.synchronize()
        self.after = self.dev.cpu()
        lo = 0
        for start, words, out in sorted(self.parts.values()) + [(self.n, 0, True)]:
            if out:
                assert torch.equal(self.after[lo:start], self.host[lo:start]), "a guard or an input was written"
                lo = start + words
        return self

    def result(self, name, dtype=torch.float32):
        start, words, _ = self.parts[name]
        return self.after[start:start + words].view(dtype)

    def untouched(self, *names):
        return all(bool((self.result(n, torch.int32) == SENTINEL).all()) for n in names)


def bn_arena(c, t, relu, res, dy):
    C, n = c.C, c.N * c.C * c.H * c.W
    a = Arena().put("x", t.x).put("gamma", t.gamma).put("beta", t.beta).put("dy", dy)
    if res:
        a.put("res", t.res)
    a.put("rm", t.rm, out=True).put("rv", t.rv, out=True).put("nbt", torch.tensor([5]), torch.int64, out=True)
    for name, words in (("y", n), ("mean", C), ("invstd", C), ("dx", n), ("dres", n), ("dgamma", C), ("dbeta", C)):
        a.put(name, words=words, out=True)
    a.put("gacc", t.gacc, out=True).put("bacc", t.bacc, out=True)
    return a.put("ws", words=R.bn_ws_bytes(C) // 4, out=True).upload()


def test_bn_through_the_c_abi_writes_its_outputs_and_nothing_else():
    c, relu, res = R.BN_CASES[3], True, True                         # (3, 8, 6, 10): M = 180
    t = R.bn_inputs(c, "exact", "eps0")
    m = R.bn_forward(t.x, t.gamma, t.beta, t.res, relu, True, t.rm, t.rv, torch.tensor(5), R.MOMENTUM, t.eps)
    dy = R.bn_vanishing_dy(t.x, m.y, m.mean, m.invstd, relu)
    k = R.bn_backward(dy, m.y, t.x, t.gamma, m.mean, m.invstd, True, relu, True, t.gacc, t.bacc)
    a = bn_arena(c, t, relu, res, dy)
    p, HW = a.ptr, c.H * c.W
    assert L().salun_bn_forward(p("x"), p("res"), p("y"), p("gamma"), p("beta"), p("rm"), p("rv"), p("nbt"), p("mean"),
                                p("invstd"), c.N, c.C, HW, 1, R.MOMENTUM, t.eps, 1, p("ws"), a.nbytes("ws"), stream()) == 0
    assert L().salun_bn_backward(p("dy"), p("y"), p("x"), p("gamma"), p("mean"), p("invstd"), p("dx"), p("dres"),
                                 p("dgamma"), p("dbeta"), p("gacc"), p("bacc"), c.N, c.C, HW, 1, 1, p("ws"),
                                 a.nbytes("ws"), stream()) == 0
    a.check()
    for name, want in (("y", m.y), ("mean", m.mean), ("invstd", m.invstd), ("rm", m.running_mean), ("dx", k.dx),
                       ("dres", k.dres), ("dgamma", k.dgamma), ("dbeta", k.dbeta), ("gacc", k.gacc), ("bacc", k.bacc)):
        assert same(a.result(name), want), name
    assert within_ulps(a.result("rv"), m.running_var, 2) and int(a.result("nbt", torch.int64)) == 6
    # outside the domain (HW = 49) and a missing running statistic in eval mode: refused, nothing written
    for args in ((c.N, c.C, 49, 1), (c.N, c.C, HW, 0)):
        a = bn_arena(c, t, relu, res, dy)
        p = a.ptr
        rc = L().salun_bn_forward(p("x"), p("res"), p("y"), p("gamma"), p("beta"), None if args[3] == 0 else p("rm"),
                                  p("rv"), p("nbt"), p("mean"), p("invstd"), *args[:3], args[3], R.MOMENTUM, t.eps, 1,
                                  p("ws"), a.nbytes("ws"), stream())
        assert rc == EINVAL and a.check().untouched("y", "mean", "invstd", "ws")
    assert L().salun_bn_backward(p("dy"), p("y"), p("x"), p("gamma"), p("mean"), p("invstd"), p("dx"), p("dres"), p("dgamma"),
                                 p("dbeta"), None, None, c.N, c.C, 49, 1, 1, p("ws"), a.nbytes("ws"), stream()) == EINVAL
    assert a.check().untouched("dx", "dres", "dgamma", "dbeta", "ws")


def gn_arena(c, t, dz):
    N, C, G, n = c.N, c.C, c.G, c.N * c.C * c.H * c.W
    a = Arena().put("x", t.x).put("gamma", t.gamma).put("beta", t.beta).put("dz", dz).put("addend", t.addend)
    for name, words in (("y", n), ("mean", N * G), ("rstd", N * G), ("dx", n), ("dgamma", C), ("dbeta", C), ("nk", N * C),
                        ("csum", C)):
        a.put(name, words=words, out=True)
    a.put("gacc", t.gacc, out=True).put("bacc", t.bacc, out=True).put("cacc", t.cacc, out=True)
    return a.put("ws", words=max(R.gn_ws_bytes(N, C) // 4, 4), out=True).upload()


def gn_fused_call(a, shape, dx="dx", addend="addend", nk="nk", csum="csum"):
    p = a.ptr
    return L().salun_gn_backward_fused(p("dz"), p("x"), p("gamma"), p("beta"), p("mean"), p("rstd"), p(addend), p(dx),
                                       p("dgamma"), p("dbeta"), p("gacc"), p("bacc"), p(nk), p(csum), p("cacc"), *shape, 0,
                                       p("ws"), a.nbytes("ws"), stream())


def test_gn_through_the_c_abi_writes_its_outputs_and_nothing_else():
    c = R.GnCase(3, 24, 4, 8, 8, "")                                 # cpg = 3: padding round, r = 8
    assert c[:5] in [k[:5] for k in R.GN_CASES]
    t = R.gn_inputs(c, "exact", "eps0")
    m = R.gn_forward(t.x, t.gamma, t.beta, c.G, t.eps)
    dz = R.gn_vanishing_dz(t.x, m.mean, m.rstd, c.G)
    k = R.gn_backward(dz, t.x, t.gamma, t.beta, m.mean, m.rstd, c.G, False, t.addend, t.cacc, t.gacc, t.bacc)
    a = gn_arena(c, t, dz)
    p, shape = a.ptr, (c.N, c.C, c.H * c.W, c.G)
    assert L().salun_gn_forward(p("x"), p("y"), p("gamma"), p("beta"), p("mean"), p("rstd"), *shape, t.eps, 0, stream()) == 0
    assert gn_fused_call(a, shape) == 0
    a.check()
    for name, want in (("y", m.y), ("mean", m.mean), ("rstd", m.rstd), ("dx", k.dx), ("dgamma", k.dgamma), ("dbeta", k.dbeta),
                       ("nk", k.nk), ("csum", k.csum), ("cacc", k.csum_acc), ("gacc", k.gacc), ("bacc", k.bacc)):
        assert same(a.result(name), want), name


def test_gn_refusals_return_einval_and_write_nothing():
    c = R.GnCase(3, 24, 4, 8, 8, "")
    t = R.gn_inputs(c, "exact", "eps0")
    outs = ("y", "mean", "rstd", "dx", "dgamma", "dbeta", "nk", "csum", "ws")
    for N, C, H, W, G, why in R.GN_OUTSIDE:                           # HW = 36, cpg = 257: within the arena's sizes
        assert N * C * H * W <= t.x.numel() and not R.gn_shape_ok(N, C, H * W, G)
        a = gn_arena(c, t, t.dz)
        p = a.ptr
        rc = L().salun_gn_forward(p("x"), p("y"), p("gamma"), p("beta"), p("mean"), p("rstd"), N, C, H * W, G, t.eps, 0, stream())
        assert rc == EINVAL and gn_fused_call(a, (N, C, H * W, G)) == EINVAL, why
        assert a.check().untouched(*outs), why
    shape = (c.N, c.C, c.H * c.W, c.G)
    a = gn_arena(c, t, t.dz)
    assert gn_fused_call(a, shape, addend="dx") == EINVAL            # addend == dx
    assert gn_fused_call(a, shape, nk="none") == EINVAL              # csum without nk_sum
    assert a.check().untouched(*outs)
    t36 = R.gn_inputs(R.GnCase(2, 8, 6, 6, 2, ""), "gauss")
    assert ops().gn_forward(dev(t36.x), dev(t36.gamma), dev(t36.beta), 2, t36.eps, True) is None


def test_k12_through_the_c_abi_writes_its_outputs_and_nothing_else():
    c = R.GN16_CASES[1]                                              # (3, 96, 5, 7, 32): ragged chunk, cpg = 3
    N, C, H, W, G = c[:5]
    n, HW = N * C * H * W, H * W
    t = R.gn_inputs(c, "exact", "eps")
    m = R.gn16_forward(t.x, t.gamma, t.beta, G, t.eps)
    dz = R.gn_vanishing_dz(t.x, m.mean, m.rstd, G)
    k = R.gn16_backward(dz, t.x, t.gamma, m.mr, m.ab, G, False, t.gacc, t.bacc)
    a = Arena().put("x", R.nhwc(t.x), BF).put("dy", R.nhwc(dz), BF).put("gamma", t.gamma).put("beta", t.beta)
    a.put("y", words=n // 2, out=True).put("mr", words=N * G * 2, out=True).put("ab", words=N * C * 2, out=True)
    a.put("dx", words=n // 2, out=True).put("dgamma", t.gacc, out=True).put("dbeta", t.bacc, out=True)
    a.put("ws", words=R.gn16_ws_bytes(N, C, HW, G) // 4, out=True).upload()
    p = a.ptr
    assert L().salun_gn_bf16_forward(p("x"), p("gamma"), p("beta"), p("y"), p("mr"), p("ab"), N, C, HW, G, t.eps, 0, p("ws"),
                                     a.nbytes("ws"), stream()) == 0
    assert L().salun_gn_bf16_backward(p("dy"), p("x"), p("gamma"), p("mr"), p("ab"), p("dx"), p("dgamma"), p("dbeta"), N, C,
                                      HW, G, 0, 1, p("ws"), a.nbytes("ws"), stream()) == 0
    a.check()
    assert same(a.result("y", BF), R.nhwc(m.y)) and same(a.result("dx", BF), R.nhwc(k.dx))
    assert same(a.result("mr"), m.mr) and same(a.result("ab"), m.ab)
    assert same(a.result("dgamma"), k.dgamma) and same(a.result("dbeta"), k.dbeta)


# ------------------------------------------------------------------------------------------ (b) bound tier
def bn_bound_case(c, offset, relu, res, train, label="bn"):
    """Forward, then backward on what the forward wrote (its y and statistics are the backward kernel's inputs)."""
    N, C, H, W = c[:4]
    t = R.bn_inputs(c, "gauss", offset=offset)
    rs = t.res if res else None
    tag = f"{label} {_id(c)} mu/sigma={offset:g} relu={int(relu)} res={int(res)} train={int(train)}"
    m = R.bn_forward(t.x, t.gamma, t.beta, rs, relu, train, t.rm, t.rv, None, R.MOMENTUM, t.eps)
    ab = R.bn_forward(t.x, t.gamma, t.beta, rs, relu, train, t.rm, t.rv, eps=t.eps, absolute=True)
    bf = R.bn_forward_bound(t.x, t.gamma, t.beta, rs, train, t.eps, t.rm, t.rv)
    x, g = dev(t.x), dev(t.gamma)
    rm, rv = dev(t.rm), dev(t.rv)
    y, mean, invstd = ops().bn_forward(x, dev(rs), g, dev(t.beta), rm, rv, train, R.MOMENTUM, t.eps, relu, None)
    within(tag + " y", y, m.y, bf.y, ab.y)
    within(tag + " mean", mean, m.mean, bf.mean + 0 * m.mean)
    within(tag + " invstd", invstd, m.invstd, bf.invstd + 0 * m.invstd)
    if train:                                  # 0.75 r + 0.25 v: the statistic's error and two roundings
        within(tag + " running_mean", rm, m.running_mean, R.MOMENTUM * bf.mean + R.gam(2) * m.running_mean.abs() + R.U * t.rm.abs())
    yk, mk, ik = host(y).double(), host(mean).double(), host(invstd).double()
    if relu:
        edge = m.pre.abs() <= bf.y
        share = float(edge.double().mean())
        log(tag + f" ReLU-edge share = {share:.5f}")
        assert share <= 0.01 and torch.equal((yk > 0)[~edge], (m.pre > 0)[~edge]), tag
    k = R.bn_backward(t.dy, yk, t.x, t.gamma, mk, ik, train, relu, res, t.gacc, t.bacc)
    ka = R.bn_backward(t.dy, yk, t.x, t.gamma, mk, ik, train, relu, absolute=True)
    bb = R.bn_backward_bound(t.dy, yk, t.x, t.gamma, mk, ik, train, relu, t.gacc, t.bacc)
    ga, ba = dev(t.gacc), dev(t.bacc)
    dx, dr, dg, db = ops().bn_backward(dev(t.dy), y if relu else None, x, g, mean, invstd, train, relu, res, ga, ba)
    within(tag + " dx", dx, k.dx, bb.dx, ka.dx)
    within(tag + " dgamma", dg, k.dgamma, bb.dgamma, ka.dgamma)
    within(tag + " dbeta", db, k.dbeta, bb.dbeta, ka.dbeta)
    within(tag + " gamma.grad +=", ga, k.gacc, bb.gacc)
    within(tag + " beta.grad +=", ba, k.bacc, bb.bacc)
    if res:
        assert torch.equal(host(dr).double(), k.dres), tag + " dres"
    return t, m, bf, y


@pytest.mark.parametrize("c", R.BN_CASES + [R.BN_BIG], ids=_id)
def test_bn_within_the_per_element_bound(c):
    if c is R.BN_BIG:
        bn_bound_case(c, 0.0, True, True, True)
        return
    if heavy(c):
        bn_bound_case(c, 0.0, True, True, True)
        bn_bound_case(c, 16.0, False, False, True)
        return
    for offset in R.OFFSETS:
        for relu, res, train in ([(False, False, True), (False, True, False)] if offset not in R.RELU_OFFSETS else
                                 [(True, True, True), (True, False, False), (False, False, True), (True, False, True)]):
            bn_bound_case(c, offset, relu, res, train)


def gn_bound_case(c, offset, silu, extra):
    N, C, H, W, G = c[:5]
    t = R.gn_inputs(c, "gauss", offset=offset)
    tag = f"gn {_id(c)} mu/sigma={offset:g} silu={int(silu)}"
    m = R.gn_forward(t.x, t.gamma, t.beta, G, t.eps, silu)
    ab = R.gn_forward(t.x, t.gamma, t.beta, G, t.eps, absolute=True)
    bf = R.gn_forward_bound(t.x, t.gamma, t.beta, G, t.eps, silu)
    z, mean, rstd = ops().gn_forward(dev(t.x), dev(t.gamma), dev(t.beta), G, t.eps, silu)
    within(tag + " y", z, m.y, bf.y, ab.y)
    within(tag + " mean", mean, m.mean, bf.mean)
    within(tag + " rstd", rstd, m.rstd, bf.rstd)
    mk, rk = host(mean).double().view(N, G), host(rstd).double().view(N, G)
    ad = t.addend if "addend" in extra else None
    k = R.gn_backward(t.dz, t.x, t.gamma, t.beta, mk, rk, G, silu, ad, t.cacc, t.gacc, t.bacc)
    ka = R.gn_backward(t.dz, t.x, t.gamma, t.beta, mk, rk, G, silu, ad, absolute=True)
    bb = R.gn_backward_bound(t.dz, t.x, t.gamma, t.beta, mk, rk, G, silu, ad, t.cacc, t.gacc, t.bacc)
    dx, dg, db, nk, cs, ga, ba, ca = gn_backward_call(t, c, t.dz, mean, rstd, silu, extra, True)
    tag += " " + "+".join(extra)
    within(tag + " dx", dx, k.dx, bb.dx, ka.dx)
    within(tag + " dgamma", dg, k.dgamma, bb.dgamma, ka.dgamma)
    within(tag + " dbeta", db, k.dbeta, bb.dbeta, ka.dbeta)
    within(tag + " gamma.grad +=", ga, k.gacc, bb.gacc)
    within(tag + " beta.grad +=", ba, k.bacc, bb.bacc)
    if "nk" in extra:
        within(tag + " nk", nk, k.nk, bb.nk, ka.nk)
        within(tag + " csum", cs, k.csum, bb.csum, ka.csum)
        within(tag + " csum_acc +=", ca, k.csum_acc, bb.csum_acc)


@pytest.mark.parametrize("c", R.GN_CASES, ids=_id)
def test_gn_within_the_per_element_bound(c):
    full = ("addend", "nk", "csum", "csum_acc")
    small = c.C * c.H * c.W <= 1 << 16
    for offset in (R.OFFSETS if small else (0.0,)):
        gn_bound_case(c, offset, True, full)
        if offset == 0.0 or small:
            gn_bound_case(c, offset, False, () if offset else full)


@pytest.mark.parametrize("c", R.GN16_CASES, ids=_id)
def test_k12_within_the_per_element_bound(c):
    N, C, H, W, G = c[:5]
    for offset, silu in itertools.product(R.OFFSETS if H * W < 2048 else (0.0,), (False, True)):
        t = R.gn_inputs(c, "gauss", offset=offset, bf16=True)
        tag = f"k12 {_id(c)} mu/sigma={offset:g} silu={int(silu)}"
        m = R.gn16_forward(t.x, t.gamma, t.beta, G, t.eps, silu)
        bf = R.gn16_forward_bound(t.x, t.gamma, t.beta, G, t.eps, silu)
        xn, y, mr, ab = k12_forward(t, c, silu)
        within(tag + " y", y, m.y64, bf.y)
        within(tag + " mr", mr, m.mr, bf.mr)
        within(tag + " ab", ab, m.ab, bf.ab)
        mrk, abk = host(mr).double(), host(ab).double()
        for accumulate in (False, True):
            acc = (t.gacc, t.bacc) if accumulate else (None, None)
            k = R.gn16_backward(t.dz, t.x, t.gamma, mrk, abk, G, silu, *acc)
            bb = R.gn16_backward_bound(t.dz, t.x, t.gamma, mrk, abk, G, silu, *acc)
            dx, gw, gb = k12_backward(t, c, xn, t.dz, mr, ab, silu, accumulate)
            within(tag + f" acc={int(accumulate)} dx", dx, k.dx64, bb.dx)
            within(tag + f" acc={int(accumulate)} dgamma", gw, k.dgamma, bb.dgamma)
            within(tag + f" acc={int(accumulate)} dbeta", gb, k.dbeta, bb.dbeta)


# ------------------------------------------------------------------------------------------ (c) conditioning
def _worst(got, exact, bound):
    err = (host(got).double().reshape(exact.shape) - exact).abs()
    return float((err / bound.clamp_min(1e-300)).max())


def test_conditioning_table_kernel_and_library_against_float64():
    """mu / sigma in {0, 2^4, 2^8}: kappa = (mu^2 + sigma^2) / (sigma^2 + eps).  Both the kernel's y and the fp32 library
    op's y are measured in units of the kernel's per-element bound (which carries kappa); the kernel's is asserted."""
    for offset in R.OFFSETS:
        c = R.BnCase(2, 32, 14, 14, "")
        t = R.bn_inputs(c, "gauss", offset=offset)
        m = R.bn_forward(t.x, t.gamma, t.beta, eps=t.eps)
        bf = R.bn_forward_bound(t.x, t.gamma, t.beta, None, True, t.eps)
        y, _, _ = ops().bn_forward(dev(t.x), None, dev(t.gamma), dev(t.beta), None, None, True, R.MOMENTUM, t.eps, False, None)
        lib = F.batch_norm(dev(t.x), None, None, dev(t.gamma), dev(t.beta), True, 0.0, t.eps)
        kap = float(R.kappa(m.mean, m.var, t.eps).max())
        kw, lw = _worst(y, m.y, bf.y), _worst(lib, m.y, bf.y)
        log(f"cond bn {_id(c)} mu/sigma={offset:g} kappa={kap:.3g}: kernel {kw:.4f} of the bound, library {lw:.4f}")
        assert kw <= 1.0
        g = R.GnCase(2, 64, 16, 16, 32, "")
        t = R.gn_inputs(g, "gauss", offset=offset)
        m = R.gn_forward(t.x, t.gamma, t.beta, g.G, t.eps)
        bf = R.gn_forward_bound(t.x, t.gamma, t.beta, g.G, t.eps, False)
        z, _, _ = ops().gn_forward(dev(t.x), dev(t.gamma), dev(t.beta), g.G, t.eps, False)
        lib = F.group_norm(dev(t.x), g.G, dev(t.gamma), dev(t.beta), t.eps)
        kap = float(R.kappa(m.mean, m.var, t.eps).max())
        kw, lw = _worst(z, m.y, bf.y), _worst(lib, m.y, bf.y)
        log(f"cond gn {_id(g)} mu/sigma={offset:g} kappa={kap:.3g}: kernel {kw:.4f} of the bound, library {lw:.4f}")
        assert kw <= 1.0
        t = R.gn_inputs(g, "gauss", offset=offset, bf16=True)
        m = R.gn16_forward(t.x, t.gamma, t.beta, g.G, t.eps)
        bf = R.gn16_forward_bound(t.x, t.gamma, t.beta, g.G, t.eps, False)
        _, y, _, _ = k12_forward(t, g, False)
        lib = F.group_norm(dev(t.x), g.G, dev(t.gamma), dev(t.beta), t.eps).to(BF)
        kap = float(R.kappa(m.mean, m.var, t.eps).max())
        kw, lw = _worst(y, m.y64, bf.y), _worst(lib, m.y64, bf.y)
        log(f"cond k12 {_id(g)} mu/sigma={offset:g} kappa={kap:.3g}: kernel {kw:.4f} of the bound, library {lw:.4f}")
        assert kw <= 1.0


# ------------------------------------------------------------------------------------------ (d) invariances, bit for bit
def test_bn_of_a_channel_does_not_depend_on_the_other_channels_and_repeats():
    for c in (R.BN_CASES[1], R.BN_CASES[8]):
        t = R.bn_inputs(c, "gauss")
        args = lambda x: (dev(x), dev(t.res), dev(t.gamma), dev(t.beta), None, None, True, R.MOMENTUM, t.eps, True, None)
        y, mean, invstd = ops().bn_forward(*args(t.x))
        y2, mean2, _ = ops().bn_forward(*args(t.x))
        assert torch.equal(y, y2) and torch.equal(mean, mean2)
        x1 = t.x.clone()
        x1[:, 1] = R.gauss(x1[:, 1].shape, 77, 3.0)
        y1, mean1, invstd1 = ops().bn_forward(*args(x1))
        keep = [i for i in range(c.C) if i != 1]
        assert torch.equal(y1[:, keep], y[:, keep]) and torch.equal(mean1[keep], mean[keep]) and not torch.equal(y1[:, 1], y[:, 1])
        b = [ops().bn_backward(dev(t.dy), yy, dev(xx), dev(t.gamma), mm, ii, True, True, True)
             for yy, xx, mm, ii in ((y, t.x, mean, invstd), (y, t.x, mean, invstd), (y1, x1, mean1, invstd1))]
        assert all(torch.equal(p, q) for p, q in zip(b[0], b[1]))
        assert torch.equal(b[2][0][:, keep], b[0][0][:, keep]) and torch.equal(b[2][2][keep], b[0][2][keep])


def test_gn_of_an_image_alone_and_in_the_batch_and_fused_against_plain_backward():
    for c, silu in ((R.GN_CASES[9], True), (R.GN_CASES[3], False), (R.GN_CASES[11], True)):
        t = R.gn_inputs(c, "gauss")
        g, b = dev(t.gamma), dev(t.beta)
        z, mean, rstd = ops().gn_forward(dev(t.x), g, b, c.G, t.eps, silu)
        z2, _, _ = ops().gn_forward(dev(t.x), g, b, c.G, t.eps, silu)
        assert torch.equal(z, z2)
        n = c.N - 1
        z1, mean1, rstd1 = ops().gn_forward(dev(t.x[n:n + 1]), g, b, c.G, t.eps, silu)
        assert torch.equal(z1[0], z[n]) and torch.equal(mean1, mean.view(c.N, c.G)[n])
        dx0, dg0, db0 = ops().gn_backward(dev(t.dz), dev(t.x), g, b, mean, rstd, c.G, silu)
        dx1, dg1, db1, nk, cs = ops().gn_backward(dev(t.dz), dev(t.x), g, b, mean, rstd, c.G, silu, addend=dev(t.addend),
                                                  nk_sum=True, csum=True)
        assert torch.equal(dg0, dg1) and torch.equal(db0, db1) and torch.equal(dx1, dx0 + dev(t.addend))
        dxa, _, _ = ops().gn_backward(dev(t.dz[n:n + 1]), dev(t.x[n:n + 1]), g, b, mean1, rstd1, c.G, silu)
        assert torch.equal(dxa[0], dx0[n])
    c = R.GN16_CASES[1]
    t = R.gn_inputs(c, "gauss", bf16=True)
    a, b2 = k12_forward(t, c, True), k12_forward(t, c, True)
    assert torch.equal(a[1], b2[1]) and torch.equal(a[2], b2[2])
    d1, d2 = (k12_backward(t, c, a[0], t.dz, a[2], a[3], True, False) for _ in range(2))
    assert all(torch.equal(p, q) for p, q in zip(d1, d2))


# ------------------------------------------------------------------------------------------ (e) degenerate sets
def _degenerate(x_sets):
    """x_sets [S, L]: set 0 all zero, set 1 constant 3, set 2 one outlier of 2^20 among unit draws."""
    x_sets[0] = 0
    x_sets[1] = 3.0
    x_sets[2, 5] = 2.0 ** 20
    return x_sets


def test_degenerate_channels_and_groups():
    c = R.BnCase(4, 8, 4, 4, "")
    t = R.bn_inputs(c, "gauss")
    t.x = _degenerate(t.x.permute(1, 0, 2, 3).reshape(c.C, -1).clone()).view(c.C, c.N, 4, 4).permute(1, 0, 2, 3).contiguous()
    for relu in (False, True):
        m = R.bn_forward(t.x, t.gamma, t.beta, None, relu, True, eps=t.eps)
        bf = R.bn_forward_bound(t.x, t.gamma, t.beta, None, True, t.eps)
        y, mean, invstd = ops().bn_forward(dev(t.x), None, dev(t.gamma), dev(t.beta), None, None, True, R.MOMENTUM, t.eps, relu, None)
        within(f"bn degenerate relu={int(relu)} y", y, m.y, bf.y)
        within(f"bn degenerate relu={int(relu)} invstd", invstd, m.invstd, bf.invstd)
        assert float(host(invstd)[0]) == float(torch.tensor(1.0 / math.sqrt(t.eps)).float()) and float(host(mean)[0]) == 0.0
        assert torch.equal(host(y)[:, 0].double(), (t.beta[0].clamp_min(0) if relu else t.beta[0]).expand(c.N, 4, 4))
        yk, mk, ik = host(y).double(), host(mean).double(), host(invstd).double()
        k = R.bn_backward(t.dy, yk, t.x, t.gamma, mk, ik, True, relu)
        bb = R.bn_backward_bound(t.dy, yk, t.x, t.gamma, mk, ik, True, relu)
        dx, _, dg, db = ops().bn_backward(dev(t.dy), y if relu else None, dev(t.x), dev(t.gamma), mean, invstd, True, relu, False)
        within(f"bn degenerate relu={int(relu)} dx", dx, k.dx, bb.dx)
        within(f"bn degenerate relu={int(relu)} dgamma", dg, k.dgamma, bb.dgamma)
        within(f"bn degenerate relu={int(relu)} dbeta", db, k.dbeta, bb.dbeta)
    g = R.GnCase(1, 24, 4, 4, 6, "")
    for silu in (False, True):
        t = R.gn_inputs(g, "gauss")
        t.x = _degenerate(t.x.reshape(g.G, -1).clone()).view(1, g.C, 4, 4)
        m = R.gn_forward(t.x, t.gamma, t.beta, g.G, t.eps, silu)
        bf = R.gn_forward_bound(t.x, t.gamma, t.beta, g.G, t.eps, silu)
        z, mean, rstd = ops().gn_forward(dev(t.x), dev(t.gamma), dev(t.beta), g.G, t.eps, silu)
        within(f"gn degenerate silu={int(silu)} y", z, m.y, bf.y)          # the all-zero group: silu(beta) through the bound
        assert float(host(mean)[0]) == 0.0 and float(host(rstd)[0]) == float(torch.tensor(1.0 / math.sqrt(t.eps)).float())
        mk, rk = host(mean).double().view(1, g.G), host(rstd).double().view(1, g.G)
        k = R.gn_backward(t.dz, t.x, t.gamma, t.beta, mk, rk, g.G, silu)
        bb = R.gn_backward_bound(t.dz, t.x, t.gamma, t.beta, mk, rk, g.G, silu)
        dx, dg, db = ops().gn_backward(dev(t.dz), dev(t.x), dev(t.gamma), dev(t.beta), mean, rstd, g.G, silu)
        within(f"gn degenerate silu={int(silu)} dx", dx, k.dx, bb.dx)
        within(f"gn degenerate silu={int(silu)} dgamma", dg, k.dgamma, bb.dgamma)
        within(f"gn degenerate silu={int(silu)} dbeta", db, k.dbeta, bb.dbeta)
        tb = R.gn_inputs(g, "gauss", bf16=True)
        tb.x = R.bf16_round(t.x)
        m = R.gn16_forward(tb.x, tb.gamma, tb.beta, g.G, tb.eps, silu)
        bf = R.gn16_forward_bound(tb.x, tb.gamma, tb.beta, g.G, tb.eps, silu)
        xn, y, mr, ab = k12_forward(tb, g, silu)
        within(f"k12 degenerate silu={int(silu)} y", y, m.y64, bf.y)
        k = R.gn16_backward(tb.dz, tb.x, tb.gamma, host(mr).double(), host(ab).double(), g.G, silu)
        bb = R.gn16_backward_bound(tb.dz, tb.x, tb.gamma, host(mr).double(), host(ab).double(), g.G, silu)
        dx, gw, gb = k12_backward(tb, g, xn, tb.dz, mr, ab, silu, False)
        within(f"k12 degenerate silu={int(silu)} dx", dx, k.dx64, bb.dx)
        within(f"k12 degenerate silu={int(silu)} dgamma", gw, k.dgamma, bb.dgamma)


# ------------------------------------------------------------------------------------------ (f) the edges of the domain
def _off_grid(t):
    """A contiguous fp32 device copy of t whose base lies one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device="cuda")
    k = 1 + (-(buf.data_ptr() // 4)) % 4
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _bn_pair(C, eps):
    a, b = nn.BatchNorm2d(C, eps=eps, momentum=R.MOMENTUM).cuda(), nn.BatchNorm2d(C, eps=eps, momentum=R.MOMENTUM).cuda()
    with torch.no_grad():
        a.weight.uniform_(0.5, 1.5)
        a.bias.normal_()
    b.load_state_dict(a.state_dict())
    return a, b


def _spy(cls):
    """Count the calls of an autograd Function's `apply` (the fused node) while the block runs."""
    from unittest import mock
    return mock.patch.object(cls, "apply", wraps=cls.apply)


@pytest.mark.parametrize("what", ["HW=49", "x off the grid", "residual off the grid", "dy off the grid", "aligned"])
def test_fused_bn_act_outside_the_kernel_domain_equals_the_library(what):
    from unlearn_saliency_amd import norm
    torch.manual_seed(0)
    shape = (2, 8, 7, 7) if what == "HW=49" else (3, 8, 6, 10)
    x, r = torch.randn(shape, device="cuda"), torch.randn(shape, device="cuda")
    if what == "x off the grid":
        x = _off_grid(x)
    if what == "residual off the grid":
        r = _off_grid(r)
    bn, ref = _bn_pair(shape[1], 1e-5)
    x1, r1 = x.detach().requires_grad_(True), r.detach().requires_grad_(True)
    x2, r2 = x.detach().requires_grad_(True), r.detach().requires_grad_(True)
    with _spy(norm._FusedBN) as spy:
        y = norm.fused_bn_act(x1, bn, residual=r1, relu=True)
    fused = what in ("aligned", "dy off the grid")
    assert spy.call_count == int(fused)        # inside the domain the fused node runs, outside it the library ops
    y2 = F.relu(ref(x2) + r2)
    dy = torch.randn_like(y)
    if what == "dy off the grid":              # the backward kernels take an aligned copy of such a gradient
        dy_al, dy = dy, _off_grid(dy)
        ya = norm.fused_bn_act(x2, ref, residual=r2, relu=True)
        y.backward(dy)
        ya.backward(dy_al)
        assert torch.equal(y, ya) and torch.equal(x1.grad, x2.grad) and torch.equal(r1.grad, r2.grad)
        assert torch.equal(bn.weight.grad, ref.weight.grad) and torch.equal(bn.bias.grad, ref.bias.grad)
        return
    y.backward(dy)
    y2.backward(dy)
    if fused:
        assert int(bn.num_batches_tracked) == 1 and bool(torch.isfinite(x1.grad).all())
        return
    assert torch.equal(y, y2) and torch.equal(x1.grad, x2.grad) and torch.equal(r1.grad, r2.grad)
    assert torch.equal(bn.weight.grad, ref.weight.grad) and torch.equal(bn.running_var, ref.running_var)
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == 1


@pytest.mark.parametrize("what", ["HW=36", "x off the grid", "dz off the grid", "aligned"])
def test_fused_gn_act_outside_the_kernel_domain_equals_the_library(what):
    from unlearn_saliency_amd import norm
    torch.manual_seed(0)
    shape = (2, 8, 6, 6) if what == "HW=36" else (2, 8, 4, 8)
    x = torch.randn(shape, device="cuda")
    if what == "x off the grid":
        x = _off_grid(x)
    gn, ref = nn.GroupNorm(2, 8).cuda(), nn.GroupNorm(2, 8).cuda()
    with torch.no_grad():
        gn.weight.uniform_(0.5, 1.5)
        gn.bias.normal_()
    ref.load_state_dict(gn.state_dict())
    x1, x2 = x.detach().requires_grad_(True), x.detach().requires_grad_(True)
    with _spy(norm._FusedGN) as spy:
        z = norm.fused_gn_act(x1, gn, silu=True)
    fused = what in ("aligned", "dz off the grid")
    assert spy.call_count == int(fused)
    dz = torch.randn_like(z)
    if fused:
        za = norm.fused_gn_act(x2, ref, silu=True)
        z.backward(_off_grid(dz) if what == "dz off the grid" else dz)
        za.backward(dz)
        assert torch.equal(z, za) and torch.equal(x1.grad, x2.grad) and torch.equal(gn.weight.grad, ref.weight.grad)
        return
    y2 = ref(x2)
    z2 = y2 * torch.sigmoid(y2)
    z.backward(dz)
    z2.backward(dz)
    assert torch.equal(z, z2) and torch.equal(x1.grad, x2.grad) and torch.equal(gn.weight.grad, ref.weight.grad)
