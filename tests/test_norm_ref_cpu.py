"""The float64 normalisation model of norm_ref_cpu.py against torch's float64 ops and autograd, the premise of the exact
tier (every partial sum of every exact case below 2^24 units, every intermediate an fp32 number), the ReLU-edge cap of
the bound tier, the mirror of the host logic against the library's queries, and the coverage of the routes.  No GPU."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import norm_ref_cpu as R

_id = R._cid
ODD_BN = [R.BnCase(2, 3, 3, 5, ""), R.BnCase(1, 4, 2, 2, ""), R.BnCase(5, 2, 6, 6, "")]
ODD_GN = [R.GnCase(2, 6, 3, 5, 2, ""), R.GnCase(3, 8, 2, 2, 8, ""), R.GnCase(1, 12, 4, 4, 1, "")]


def close(got, want, tol=1e-12):
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= tol * max(float(want.abs().max()), 1e-300)


# ------------------------------------------------------------------------------------------ model against torch
@pytest.mark.parametrize("relu,res,train", list(itertools.product((False, True), repeat=3)))
@pytest.mark.parametrize("c", R.BN_CASES[:4] + ODD_BN, ids=_id)
def test_bn_model_agrees_with_torch_float64(c, relu, res, train):
    t = R.bn_inputs(c, "gauss", offset=16.0)
    x = t.x.clone().requires_grad_(True)
    r = t.res.clone().requires_grad_(True)
    g, b = t.gamma.clone().requires_grad_(True), t.beta.clone().requires_grad_(True)
    rm, rv = t.rm.clone(), t.rv.clone()
    y = F.batch_norm(x, rm, rv, g, b, train, R.MOMENTUM, t.eps)
    if res:
        y = y + r
    if relu:
        y = F.relu(y)
    y.backward(t.dy)
    o = R.bn_forward(t.x, t.gamma, t.beta, t.res if res else None, relu, train, t.rm, t.rv, torch.tensor(3), R.MOMENTUM, t.eps)
    close(o.y, y.detach())
    close(o.running_mean, rm)
    close(o.running_var, rv)
    assert int(o.nbt) == (4 if train else 3)
    k = R.bn_backward(t.dy, o.y, t.x, t.gamma, o.mean, o.invstd, train, relu, res, t.gacc, t.bacc)
    close(k.dx, x.grad, 1e-10)
    close(k.dgamma, g.grad, 1e-10)
    close(k.dbeta, b.grad, 1e-10)
    close(k.gacc, t.gacc + g.grad, 1e-10)
    close(k.bacc, t.bacc + b.grad, 1e-10)
    if res:
        close(k.dres, r.grad)
    a = R.bn_backward(t.dy, o.y, t.x, t.gamma, o.mean, o.invstd, train, relu, absolute=True)
    assert (a.dx >= k.dx.abs() * (1 - 1e-12)).all() and (a.dgamma >= k.dgamma.abs() * (1 - 1e-12)).all()
    assert (R.bn_forward(t.x, t.gamma, t.beta, t.res if res else None, relu, train, t.rm, t.rv, eps=t.eps, absolute=True).y
            >= o.pre.abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("c", [c for c in R.GN_CASES if c.C * c.H * c.W <= 1 << 16] + ODD_GN, ids=_id)
def test_gn_model_agrees_with_torch_float64(c, silu):
    t = R.gn_inputs(c, "gauss", offset=16.0)
    x, g, b = (v.clone().requires_grad_(True) for v in (t.x, t.gamma, t.beta))
    y = F.group_norm(x, c.G, g, b, t.eps)
    z = y * torch.sigmoid(y) if silu else y
    z.backward(t.dz)
    o = R.gn_forward(t.x, t.gamma, t.beta, c.G, t.eps, silu)
    close(o.y, z.detach())
    k = R.gn_backward(t.dz, t.x, t.gamma, t.beta, o.mean, o.rstd, c.G, silu, t.addend, t.cacc, t.gacc, t.bacc)
    close(k.dx, x.grad + t.addend, 1e-10)
    close(k.dgamma, g.grad, 1e-10)
    close(k.dbeta, b.grad, 1e-10)
    close(k.nk, (x.grad + t.addend).sum((2, 3)), 1e-10)
    close(k.csum, (x.grad + t.addend).sum((0, 2, 3)), 1e-10)
    close(k.csum_acc, t.cacc + k.csum)
    close(k.gacc, t.gacc + k.dgamma)
    a = R.gn_backward(t.dz, t.x, t.gamma, t.beta, o.mean, o.rstd, c.G, silu, t.addend, absolute=True)
    assert (a.dx >= k.dx.abs() * (1 - 1e-12)).all() and (a.nk >= k.nk.abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("c", [c for c in R.GN16_CASES if c.H * c.W < 2048], ids=_id)
def test_k12_model_agrees_with_torch_float64(c, silu):
    t = R.gn_inputs(c, "gauss", bf16=True)
    assert torch.equal(R.bf16_round(t.x), t.x) and torch.equal(t.x.bfloat16().double(), t.x)
    x, g, b = (v.clone().requires_grad_(True) for v in (t.x, t.gamma, t.beta))
    y = F.group_norm(x, c.G, g, b, t.eps)
    z = y * torch.sigmoid(y) if silu else y
    z.backward(t.dz)
    o = R.gn16_forward(t.x, t.gamma, t.beta, c.G, t.eps, silu)
    close(o.y64, z.detach())
    assert torch.equal(o.y, R.bf16_round(z.detach())) or float((o.y - z.detach()).abs().max()) <= 2 ** -8 * float(z.abs().max())
    k = R.gn16_backward(t.dz, t.x, t.gamma, o.mr, o.ab, c.G, silu, t.gacc, t.bacc)
    close(k.dx64, x.grad, 1e-10)
    close(k.dgamma, g.grad + t.gacc, 1e-10)
    close(k.dbeta, b.grad + t.bacc, 1e-10)
    assert torch.equal(k.dx, R.bf16_round(k.dx64))


def test_bf16_round_ties_to_even_in_one_step():
    f = lambda v: float(R.bf16_round(torch.tensor([v], dtype=torch.float64)))
    assert f(1 + 2.0 ** -8) == 1.0 and f(1 + 3 * 2.0 ** -8) == 1 + 2.0 ** -6      # ties: to the even neighbour
    assert f(1 + 2.0 ** -8 + 2.0 ** -40) == 1 + 2.0 ** -7                          # above a tie; through fp32 it is a tie
    assert f(-1 - 2.0 ** -8) == -1.0 and f(3.0) == 3.0 and f(0.0) == 0.0
    assert R.U16 == 2.0 ** -8 and f(1 + 2.0 ** -9) == 1.0


# ------------------------------------------------------------------------------------------ the premise of the exact tier
def unit_of(*ts):
    """The largest power of two that every element of every tensor is a whole multiple of."""
    k = 0
    while not all(torch.equal(t * 2.0 ** k, (t * 2.0 ** k).round()) for t in ts):
        k += 1
        assert k < 80
    return 2.0 ** -k


def capped(terms, dims):
    """Every partial sum of `terms` over `dims`, in any order, is exact in fp32."""
    q = unit_of(terms)
    return float(terms.abs().sum(dims).max()) / q < 2 ** 24


def fp32_all(*ts):
    return all(R.is_f32(t) for t in ts)


def families(L):
    return ("eps",) if L % 2 else ("eps0", "eps")


@pytest.mark.parametrize("c", R.BN_CASES + [R.BN_BIG], ids=_id)
def test_bn_exact_cases_keep_every_partial_sum_below_2_to_24_units(c):
    N, C, H, W = c[:4]
    M = N * H * W
    big = c is R.BN_BIG                        # the GPU test runs the large cases in fewer variants
    heavy = N * C * H * W > 1 << 20
    for family in (("eps0",) if big else families(M)):
        t = R.bn_inputs(c, "exact", family)
        assert fp32_all(t.x, t.gamma, t.beta, t.res, t.dy, t.rm, t.rv)
        assert capped(t.x, (0, 2, 3)) and capped(t.x * t.x, (0, 2, 3))
        for relu, res in ([(True, True)] if big else [(True, True), (False, False)] if heavy else
                          itertools.product((False, True), repeat=2)):
            o = R.bn_forward(t.x, t.gamma, t.beta, t.res if res else None, relu, True, t.rm, t.rv, None, R.MOMENTUM, t.eps)
            s, m = R.set_scale(C, family)
            assert torch.equal(o.mean, m) and torch.equal(o.var + t.eps, (o.var + t.eps).float().double())
            assert torch.equal(o.invstd, 1 / (2 * s) if family == "eps0" else torch.ones_like(s))
            a = o.invstd * t.gamma
            assert fp32_all(a, o.mean * a, t.beta - o.mean * a, t.x * a.view(1, C, 1, 1), o.pre, o.running_mean)
            for dy in (t.dy, R.bn_vanishing_dy(t.x, o.y, o.mean, o.invstd, relu)):
                k = R.bn_backward(dy, o.y, t.x, t.gamma, o.mean, o.invstd, True, relu, True, t.gacc, t.bacc)
                assert capped(k.dz, (0, 2, 3)) and capped(k.dz * k.xh, (0, 2, 3)) and fp32_all(k.xh, k.dz * k.xh)
                assert fp32_all(k.dgamma, k.dbeta, k.gacc, k.bacc)
                if dy is not t.dy:
                    assert not k.dgamma.any() and not k.dbeta.any() and fp32_all(k.dx) and float(k.dx.abs().max()) > 0
                elif M & (M - 1) == 0:
                    v = lambda q: q.view(1, C, 1, 1)
                    assert fp32_all(k.dx, k.dbeta / M, k.dgamma / M, k.xh * v(k.dgamma / M),
                                    v(k.dbeta / M) + k.xh * v(k.dgamma / M), k.dz - (v(k.dbeta / M) + k.xh * v(k.dgamma / M)))


@pytest.mark.parametrize("c", R.GN_CASES + R.GN16_CASES, ids=_id)
def test_gn_exact_cases_keep_every_partial_sum_below_2_to_24_units(c):
    N, C, H, W, G = c[:5]
    cpg, L = C // G, C // G * H * W
    ch = lambda q: q.repeat_interleave(cpg, 1).view(N, C, 1, 1)
    gv = lambda q: q.view(1, C, 1, 1)
    for family in families(L):
        t = R.gn_inputs(c, "exact", family)
        assert fp32_all(t.x, t.gamma, t.beta, t.dz, t.addend)
        if c in R.GN16_CASES:
            assert torch.equal(t.x.bfloat16().double(), t.x) and torch.equal(t.dz.bfloat16().double(), t.dz)
        xg = t.x.view(N, G, L)
        assert capped(xg, 2) and capped(xg * xg, 2)
        o = R.gn_forward(t.x, t.gamma, t.beta, G, t.eps)
        s, m = R.set_scale(N * G, family)
        assert torch.equal(o.mean.reshape(-1), m) and float(o.rstd.min()) > 0
        assert torch.equal(torch.log2(o.rstd), torch.log2(o.rstd).round())
        a = ch(o.rstd) * gv(t.gamma)
        assert fp32_all(a, ch(o.mean) * a, gv(t.beta) - ch(o.mean) * a, t.x * a, o.pre)
        for dz in (t.dz, R.gn_vanishing_dz(t.x, o.mean, o.rstd, G)):
            k = R.gn_backward(dz, t.x, t.gamma, t.beta, o.mean, o.rstd, G, False, t.addend, t.cacc, t.gacc, t.bacc)
            assert capped(dz.view(N, C, -1), 2) and capped((dz * k.xh).view(N, C, -1), 2)
            assert capped((dz * gv(t.gamma)).view(N, G, L), 2) and capped((dz * gv(t.gamma) * k.xh).view(N, G, L), 2)
            assert fp32_all(k.xh, dz * k.xh, k.dgamma, k.dbeta, k.gacc, k.bacc)
            if dz is not t.dz:
                assert not k.dgamma.any() and not k.ma.any() and not k.mb.any() and float(dz.abs().max()) > 0 or H * W < 2
            if R.exact_dx(c, dz is not t.dz):
                p = dz * gv(t.gamma)
                assert fp32_all(k.ma, k.mb, p, p - ch(k.ma), k.xh * ch(k.mb), p - ch(k.ma) - k.xh * ch(k.mb), k.dx,
                                k.dx - t.addend)
            if R.exact_nk(c, dz is not t.dz):
                assert capped(k.dx.view(N, C, -1), 2) and fp32_all(k.nk, k.csum, k.csum_acc)


# ------------------------------------------------------------------------------------------ the ReLU-edge cap
@pytest.mark.parametrize("offset", R.RELU_OFFSETS)
@pytest.mark.parametrize("c", R.BN_CASES + [R.BN_BIG], ids=_id)
def test_relu_edge_share_of_the_bound_cases_is_below_one_percent(c, offset):
    if c is R.BN_BIG and offset:
        return                                 # the bound tier runs the large case at offset 0, residual, train mode
    t = R.bn_inputs(c, "gauss", offset=offset)
    for res, train in ([(True, True)] if c is R.BN_BIG else itertools.product((False, True), repeat=2)):
        o = R.bn_forward(t.x, t.gamma, t.beta, t.res if res else None, True, train, t.rm, t.rv, None, R.MOMENTUM, t.eps)
        b = R.bn_forward_bound(t.x, t.gamma, t.beta, t.res if res else None, train, t.eps, t.rm, t.rv)
        assert bool(torch.isfinite(b.y).all())
        assert R.relu_edge_share(o.pre, b.y) <= 0.01, (res, train)


@pytest.mark.parametrize("c", R.BN_CASES[:10], ids=_id)
def test_at_mu_over_sigma_2_to_8_the_relu_edge_share_exceeds_the_cap(c):
    """Why the ReLU variants of the bound tier stop at 2^4: at 2^8 the forward bound (kappa u) is a few per cent of
    sigma, and more than 1 % of the pre-activations lie within it of 0."""
    t = R.bn_inputs(c, "gauss", offset=256.0)
    o = R.bn_forward(t.x, t.gamma, t.beta, None, True, True, eps=t.eps)
    b = R.bn_forward_bound(t.x, t.gamma, t.beta, None, True, t.eps)
    share = R.relu_edge_share(o.pre, b.y)
    assert 0.01 < share < 0.2, share


def test_silu_cases_stay_inside_the_domain_of_the_exp_constant():
    for c in R.GN_CASES + R.GN16_CASES:
        for offset in ((0.0,) if c.C * c.H * c.W > 1 << 16 else R.OFFSETS):
            t = R.gn_inputs(c, "gauss", offset=offset, bf16=c in R.GN16_CASES)
            assert float(R.gn_forward(t.x, t.gamma, t.beta, c.G, t.eps).pre.abs().max()) < 80


# ------------------------------------------------------------------------------------------ the mirror
def _lib():
    from unlearn_saliency_amd import _lib
    _lib.build()
    return _lib.lib()


def test_mirror_agrees_with_the_library_queries():
    L = _lib()
    for c in R.BN_CASES + [R.BN_BIG]:
        assert L.salun_bn_workspace_bytes(c.C) == R.bn_ws_bytes(c.C) >= 16 * c.C * R.bn_nsplit(c.N, c.C)
        assert R.bn_ok(c.N, c.C, c.H * c.W)
        sl = R.bn_slices(c.N, c.C)
        assert sl[0][0] == 0 and sl[-1][1] == c.N and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
        assert all(hi > lo for lo, hi in sl)
    assert not R.bn_ok(*R.BN_OUTSIDE[:2], R.BN_OUTSIDE[2] * R.BN_OUTSIDE[3])
    for c in R.GN_CASES:
        assert L.salun_gn_workspace_bytes(c.N, c.C) == R.gn_ws_bytes(c.N, c.C)
        assert R.gn_shape_ok(c.N, c.C, c.H * c.W, c.G)
    for N, C, H, W, G, _ in R.GN_OUTSIDE:
        assert not R.gn_shape_ok(N, C, H * W, G)
    n = 0
    for N, C, HW, G in itertools.product((1, 2, 3), (8, 24, 64, 264, 320, 12, 0), (1, 9, 31, 32, 33, 35, 2047, 2048, 2113, 4096),
                                         (1, 2, 8, 32, 33, 5)):
        assert L.salun_gn_bf16_workspace_bytes(N, C, HW, G) == R.gn16_ws_bytes(N, C, HW, G), (N, C, HW, G)
        n += 1
    assert n > 100
    for c in R.GN16_CASES:
        assert R.gn16_ws_bytes(c.N, c.C, c.H * c.W, c.G) > 0
        assert R.gn_chunks(c.H * c.W) * R.rows_per_chunk(c.H * c.W) >= c.H * c.W
    assert R.gn_chunks(2113) == 64 and R.rows_per_chunk(2113) == 34 and 63 * 34 > 2113


def test_cases_reach_every_route():
    seen = set().union(*(R.bn_routes(*c[:4]) for c in R.BN_CASES + [R.BN_BIG]))
    assert not [r for r in R.BN_REQUIRED if r not in seen]
    sizes = [hi - lo for lo, hi in R.bn_slices(65, 8)]
    assert set(sizes) == {1, 2} and len(sizes) == 64
    seen = set().union(*(R.gn_routes(*c[:5]) for c in R.GN_CASES))
    assert not [r for r in R.GN_REQUIRED if r not in seen]
    assert any(c[:5] == (2, 8, 64, 64, 1) and R.gn_items(c.C, c.H * c.W, c.G) == 0 for c in R.GN_CASES)
    assert {R.gn_items(c.C, c.H * c.W, c.G) for c in R.GN_CASES if c.C // c.G == 256} == {1, 4}
    seen = set().union(*(R.gn16_routes(*c[:5]) for c in R.GN16_CASES))
    assert not [r for r in R.GN16_REQUIRED if r not in seen]
    assert len(R.GN_EXTRA) == 6 and len({c.why for c in R.BN_CASES}) >= 8
