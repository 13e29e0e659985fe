"""K28 (csrc/salun_gn_split.hip) against the float64 model of norm_ref_cpu.py, called through the C-ABI on views inside
guarded_arena.Arena (NaN guards around inputs, sentinels around and inside y, save_mean, save_rstd and the workspace;
everything outside the outputs must be unchanged after every call).

Per element:  |y - model| <= norm_ref_cpu.gn_forward_bound(..., c1 = 2 + SALUN_GN_SPLIT_FLUSH).y, and mean / rstd within
the bounds of the same call.  The largest error / bound ratio per case is logged (profiles/gn_split_bounds_measured.txt)
and not asserted beyond <= 1."""
import ctypes
import os

import pytest
import torch

import gn_split_ref_cpu as S
import norm_ref_cpu as R
from guarded_arena import SENTINEL, Arena

pytestmark = pytest.mark.gpu

EINVAL = -22
_cache = {}


def L():
    from unlearn_saliency_amd import _lib
    return _lib.lib()


def stream():
    from unlearn_saliency_amd.streams import _stream
    return _stream()


def log(line):
    print(line)
    d = os.environ.get("SALUN_MEASURED_DIR")
    if d and os.path.isdir(d):
        with open(os.path.join(d, "gn_split_bounds_measured.txt"), "a") as f:
            f.write(line + "\n")


def gn_case(c):
    return R.GnCase(c.N, c.C, c.H, c.W, c.G, c.why)


def inputs(c, kind, family="eps0", offset=0.0):
    key = (c[:5], kind, family, offset)
    if key not in _cache:
        _cache[key] = R.gn_inputs(gn_case(c), kind, family, offset)
    return _cache[key]


def call(c, t, silu, slab=None, x=None, inplace=False, ws_words=None, skew=None, null=(), shape=None):
    """One salun_gn_split_forward call inside a fresh arena.  -> (rc, arena)."""
    x = t.x if x is None else x
    N = x.shape[0]
    slab = c.slab if slab is None else slab
    nbytes = int(L().salun_gn_split_workspace_bytes(N, c.C, ctypes.c_int64(c.H * c.W), c.G, slab))
    words = max(nbytes // 4, 4) if ws_words is None else ws_words
    a = Arena()
    if inplace:
        a.put("y", x, out=True)
    else:
        a.put("x", x, skew=1 if skew == "x" else 0).put("y", shape=tuple(x.shape), out=True, skew=1 if skew == "y" else 0)
    a.put("gamma", t.gamma).put("beta", t.beta).put("mean", shape=(N, c.G), out=True).put("rstd", shape=(N, c.G), out=True)
    a.put("ws", shape=(words,), out=True).upload()
    p = lambda n: ctypes.c_void_p(None) if n in null else a.ptr("y" if (inplace and n == "x") else n)
    Nn, C, HW, G = shape or (N, c.C, c.H * c.W, c.G)
    rc = L().salun_gn_split_forward(p("x"), p("y"), p("gamma"), p("beta"), p("mean"), p("rstd"), Nn, C, ctypes.c_int64(HW), G,
                                    ctypes.c_double(t.eps), int(silu), slab, p("ws"), ctypes.c_size_t(4 * words), stream())
    return rc, a


def outputs(a):
    after = a.download()                      # asserts that no guard and no input changed
    return a.part(after, "y"), a.part(after, "mean"), a.part(after, "rstd")


def same(got, want64):
    want = want64.float()
    assert torch.equal(want.double(), want64), "the expected answer is not an fp32 number"
    return torch.equal(got.reshape(want.shape), want)


def worst(got, want, bound):
    err = (got.double().reshape(want.shape) - want).abs()
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


def bound_case(c, silu, offset=0.0):
    t = inputs(c, "gauss", offset=offset)
    m = R.gn_forward(t.x, t.gamma, t.beta, c.G, t.eps, silu)
    b = R.gn_forward_bound(t.x, t.gamma, t.beta, c.G, t.eps, silu, c1=S.C1)
    rc, a = call(c, t, silu)
    assert rc == 0
    y, mean, rstd = outputs(a)
    ry, rm, rr = worst(y, m.y, b.y), worst(mean, m.mean, b.mean), worst(rstd, m.rstd, b.rstd)
    log(f"gn_split {S.case_id(c)} S={S.slabs(c.C, c.H * c.W, c.G, c.slab)} silu={int(silu)} mu/sigma={offset:g}: "
        f"err/bound y {ry:.4f} mean {rm:.4f} rstd {rr:.4f}")


# ------------------------------------------------------------------------------------------ the bound
@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_within_the_per_element_bound(c, silu):
    assert S.C1 == 2 + 16
    bound_case(c, silu)


@pytest.mark.parametrize("offset", R.OFFSETS)
def test_large_means(offset):
    for c in (S.CASES[1], S.CASES[4]):
        for silu in (False, True):
            if silu:
                t = inputs(c, "gauss", offset=offset)
                assert float(R.gn_forward(t.x, t.gamma, t.beta, c.G, t.eps).pre.abs().max()) < 80
            bound_case(c, silu, offset)


# ------------------------------------------------------------------------------------------ exact answers
@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_equals_the_exact_answer(c):
    for family in ("eps0", "eps"):
        t = inputs(c, "exact", family)
        m = R.gn_forward(t.x, t.gamma, t.beta, c.G, t.eps)
        rc, a = call(c, t, False)
        assert rc == 0
        y, mean, rstd = outputs(a)
        assert same(mean, m.mean) and same(rstd, m.rstd) and same(y, m.y), (S.case_id(c), family)


# ------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("c", [c for c in S.CASES if c.N > 1], ids=S.case_id)
def test_same_bits_again_and_alone(c):
    t = inputs(c, "gauss")
    bits = lambda v: v.view(torch.int32)
    rc, a = call(c, t, True)
    y, mean, rstd = outputs(a)
    rc2, a2 = call(c, t, True)
    y2, mean2, rstd2 = outputs(a2)
    assert rc == 0 and rc2 == 0
    assert torch.equal(bits(y), bits(y2)) and torch.equal(bits(mean), bits(mean2)) and torch.equal(bits(rstd), bits(rstd2))
    rc, b = call(c, t, True, x=t.x[1:2])
    y1, mean1, rstd1 = outputs(b)
    assert rc == 0 and torch.equal(bits(y1[0]), bits(y[1]))
    assert torch.equal(bits(mean1[0]), bits(mean[1])) and torch.equal(bits(rstd1[0]), bits(rstd[1]))


@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_in_place_gives_the_out_of_place_bits(c):
    t = inputs(c, "gauss")
    for silu in (False, True):
        rc, a = call(c, t, silu)
        rc2, b = call(c, t, silu, inplace=True)
        assert rc == 0 and rc2 == 0
        for u, v in zip(outputs(a), outputs(b)):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32))


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_return_einval_and_write_nothing():
    c = S.CASES[1]
    t = inputs(c, "gauss")

    def refused(why, **kw):
        rc, a = call(c, t, True, **kw)
        assert rc == EINVAL, why
        after = a.download()
        for name in ("y", "mean", "rstd", "ws"):
            if not (kw.get("inplace") and name == "y"):
                assert bool((a.part(after, name).view(torch.int32) == SENTINEL).all()), (why, name)

    assert c.N * c.C * c.H * c.W >= 2 * 8 * 6
    refused("HW = 6", shape=(2, 8, 6, 2))
    refused("HW = 2", shape=(c.N, c.C * 8, 2, c.G))
    refused("C % G != 0", shape=(c.N, c.C, c.H * c.W, 3))
    refused("N = 0", shape=(0, c.C, c.H * c.W, c.G))
    refused("G = 0", shape=(c.N, c.C, c.H * c.W, 0))
    refused("slab_vec4 < 0", slab=-1, ws_words=4096)
    refused("x off 16 bytes", skew="x")
    refused("y off 16 bytes", skew="y")
    full = int(L().salun_gn_split_workspace_bytes(c.N, c.C, ctypes.c_int64(c.H * c.W), c.G, c.slab)) // 4
    assert full >= 8
    refused("short workspace", ws_words=full - 4)
    for name in ("x", "y", "gamma", "beta", "mean", "rstd", "ws"):
        refused("NULL " + name, null=(name,))


# ------------------------------------------------------------------------------------------ the route query
@pytest.mark.parametrize("c", S.CASES, ids=S.case_id)
def test_the_slab_query_agrees_with_the_workspace_and_what_ran(c):
    HW = ctypes.c_int64(c.H * c.W)
    s = L().salun_gn_split_slabs(c.C, HW, c.G, c.slab)
    assert s == S.slabs(c.C, c.H * c.W, c.G, c.slab) > 0
    nbytes = L().salun_gn_split_workspace_bytes(c.N, c.C, HW, c.G, c.slab)
    assert nbytes == 16 * c.N * c.G * s == S.ws_bytes(c.N, c.C, c.H * c.W, c.G, c.slab)
    # the call fills exactly that many bytes of the workspace: every pair is a number, the word after stays a sentinel
    t = inputs(c, "gauss")
    rc, a = call(c, t, False, ws_words=nbytes // 4 + 4)
    assert rc == 0
    ws = a.part(a.download(), "ws").view(torch.int32)
    assert bool((ws[nbytes // 4:] == SENTINEL).all())
    pairs = ws[:nbytes // 4].view(torch.float64).view(c.N * c.G, s, 2)
    g = R._grp(t.x, c.G).reshape(c.N * c.G, -1)
    want, size = torch.stack([g.sum(1), g.pow(2).sum(1)], 1), torch.stack([g.abs().sum(1), g.pow(2).sum(1)], 1)
    assert bool(((pairs.sum(1) - want).abs() <= R.gam(S.C1 + 1) * 2 * size).all())


def test_python_wrapper_routes_and_counts():
    """norm.gn_split_act: K28 inside the domain (nothing counted), the library outside it, counted by reason."""
    import torch.nn as nn
    from unlearn_saliency_amd import norm
    norm.reset_library_gn_split_calls()
    gn = nn.GroupNorm(3, 12, eps=1e-6).cuda()
    with torch.no_grad():
        gn.weight.normal_()
        gn.bias.normal_()
    x = torch.randn(2, 12, 6, 6, device="cuda")
    with torch.no_grad():
        want = gn(x)
        y = norm.gn_split_act(x, gn, silu=False)
        assert all(v == 0 for v in norm.LIBRARY_GN_SPLIT_CALLS.values())
        assert torch.allclose(y, want, rtol=1e-4, atol=1e-5)
        norm.gn_split_act(x.half(), gn.half(), silu=True)
        gn.float()
        norm.gn_split_act(torch.randn(2, 12, 3, 3, device="cuda"), gn, silu=True)
    norm.gn_split_act(x, gn, silu=True)                       # parameters require grad under grad mode
    assert norm.LIBRARY_GN_SPLIT_CALLS == {"dtype_or_autocast": 1, "requires_grad": 1, "shape": 1}
    norm.reset_library_gn_split_calls()
