"""The float64 GEMM / softmax / column-sum models of gemm_ref_cpu.py against torch float64 (matmul, softmax, autograd), the
premise of the exact tier (every partial sum of every integer case below 2^24 units), and the Python mirror of the
host-side plan held to `salun_gemm_f32_route` - the plan `salun_gemm_f32` launches from - field for field, on the cases
and on a sweep.  The coverage test reads from that query, not from comments, that gemm_ref_cpu.CASES enters every route
of the fp32 GEMM family.  No GPU: the library is loaded, no kernel is launched."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

import gemm_ref_cpu as R

F64 = torch.float64
EINVAL = -22
FIELDS_JOB = ("nchunks", "per", "empty_shares", "tile0", "fast_tiles")
FIELDS_SEG = ("amode", "bmode", "chunk0")
_id = lambda c: c.id
FAKE_WS = 1 << 30                                 # a workspace address the query reads for null-ness and alignment only


def _lib():
    from unlearn_saliency_amd import _lib
    _lib.build()
    return _lib.lib()


def fake_addresses(c, aligned=None):
    """name -> an address with the alignment the arena of the GPU tests gives the buffer (16 bytes plus its skew)."""
    out, at = {}, 1 << 20
    for name, (n, skew) in sorted(R.layout(c).items()):
        off = skew if aligned is None else (0 if aligned[name] else 1)
        out[name] = at + 4 * off
        at += (n + 8 + 3) // 4 * 16
    return out


def lib_route(L, c, aligned=None, ws_bytes=None, ws=-1):
    """salun_gemm_f32_route -> dict of the fields (None for SALUN_EINVAL), and the workspace size the library asks for.
    ws: the workspace address passed (None: NULL; default: by c.ws)."""
    from unlearn_saliency_amd._lib import GemmRoute
    J, S, st = R.tables(c, fake_addresses(c, aligned))
    need = L.salun_gemm_f32_workspace_bytes(J, len(J), S, len(S), c.batch[0], c.batch[1])
    if ws_bytes is None:
        ws_bytes = R.WS_BYTES[c.ws](need)
    if ws == -1:
        ws = FAKE_WS if R.WS_POINTER[c.ws] else None
    r = GemmRoute()
    rc = L.salun_gemm_f32_route(J, len(J), S, len(S), c.batch[0], c.batch[1], st, ws, ws_bytes, ctypes.byref(r))
    assert rc in (0, EINVAL), rc
    if rc:
        return None, need
    d = {k: getattr(r, k) for k in ("tile", "nsplit", "nsplit_wanted", "njobs", "nsegs", "tiles")}
    d.update({k: list(getattr(r, k))[:r.njobs] for k in FIELDS_JOB})
    d.update({k: list(getattr(r, k))[:r.nsegs] for k in FIELDS_SEG})
    d["ws_need"] = need
    return d, need


# ------------------------------------------------------------------------------------------ the models
def _close(got, want, exact):
    assert got.shape == want.shape
    if exact:
        assert torch.equal(got, want)
    else:
        assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-300)


def torch_gemm(c, t, alpha, bias, accumulate, absolute=False):
    """The same call through strided torch views and matmul, job by job."""
    f = (lambda x: x.abs()) if absolute else (lambda x: x)
    st = R.case_strides(c) or (0,) * 6
    outs = []
    first = {}
    for ji, j, si, s in R.seg_rows(c):
        first.setdefault(ji, si)
    for ji, j in enumerate(c.jobs):
        acc = torch.zeros(c.batch + (j.M, j.N), dtype=F64)
        for k, s in enumerate(j.segs):
            si = first[ji] + k
            ar, ak, _ = R.op_strides(s.a, j.M, s.K)
            br, bk, _ = R.op_strides(s.b, j.N, s.K)
            for o, i in itertools.product(range(c.batch[0]), range(c.batch[1])):
                A = torch.as_strided(t[f"a{si}"], (j.M, s.K), (ar, ak), o * st[0] + i * st[1])
                B = torch.as_strided(t[f"b{si}"], (j.N, s.K), (br, bk), o * st[2] + i * st[3])
                acc[o, i] += torch.matmul(f(A), f(B).t())
        acc = acc * (abs(alpha) if absolute else alpha)
        use_bias, accu = R.job_flags(j, bias, accumulate)
        if use_bias:
            acc = acc + f(t[f"bias{ji}"])[None, None, None, :]
        if accu:
            for o, i in itertools.product(range(c.batch[0]), range(c.batch[1])):
                acc[o, i] += f(torch.as_strided(t[f"c{ji}"], (j.M, j.N), (j.ldc, 1), o * st[4] + i * st[5]))
        outs.append(acc)
    return outs


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("c", R.CASES, ids=_id)
def test_gemm_model_agrees_with_torch_float64_and_abs_sum_is_the_sum_of_absolute_terms(c, kind):
    t = R.inputs(c, kind)
    for alpha, bias, acc in ((1.0, False, False), (-2.0, True, True)):
        got = R.gemm_model(c, t, alpha, bias, acc)
        for g, want, wabs, j in zip(got, torch_gemm(c, t, alpha, bias, acc), torch_gemm(c, t, alpha, bias, acc, True), c.jobs):
            _close(g.exact, want, kind == "int")
            _close(g.abs_sum, wabs, kind == "int")
            assert g.n == sum(s.K for s in j.segs) and bool((g.abs_sum >= g.exact.abs()).all())
    assert R.bound_gamma(1) == 2.0 ** -24 / (1 - 2.0 ** -24) and R.bound_gamma(2123) < 2123 * 2.0 ** -24 * 1.001


def test_softmax_colsum_and_composed_models_agree_with_torch_float64():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(5, 77, generator=g, dtype=F64) * 4
    P, b = R.softmax_model(x)
    _close(P, torch.softmax(x, -1), False)
    assert bool((b > 0).all()) and float((b / P).max()) < 400 * R.U
    dP = torch.randn(5, 77, generator=g, dtype=F64)
    xs = x.clone().requires_grad_(True)
    torch.softmax(0.125 * xs, -1).backward(dP)
    dS, bb = R.softmax_backward_model(torch.softmax(0.125 * x, -1), dP, 0.125)
    _close(dS, xs.grad, False)
    assert bool((bb >= 0).all())
    m = torch.randn(17, 6, generator=g, dtype=F64)
    e, a = R.colsum_model(m, m[0])
    _close(e, m.sum(0) + m[0], False), _close(a, m.abs().sum(0) + m[0].abs(), False)
    # linear
    xl, w, bias, dy = (torch.randn(*s, generator=g, dtype=F64) for s in ((2, 3, 8), (5, 8), (5,), (2, 3, 5)))
    xr, wr, br = (t.clone().requires_grad_(True) for t in (xl, w, bias))
    F.linear(xr, wr, br).backward(dy)
    lm = R.linear_model(xl, w, bias, dy)
    _close(lm.y[0], F.linear(xl, w, bias).reshape(-1, 5), False)
    _close(lm.dx[0], xr.grad.reshape(-1, 8), False), _close(lm.dw[0], wr.grad, False), _close(lm.db[0], br.grad, False)
    assert lm.y[2] == 8 and lm.dx[2] == 5 and lm.dw[2] == 6
    # attention
    q, k, v, do = (torch.randn(2, 3, T, 4, generator=g, dtype=F64) for T in (5, 7, 7, 5))
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = torch.softmax(0.5 * (qr @ kr.transpose(-1, -2)), -1) @ vr
    o.backward(do)
    am = R.attention_model(q, k, v, do, 0.5)
    for got, want in ((am.o, o.detach()), (am.dq, qr.grad), (am.dk, kr.grad), (am.dv, vr.grad)):
        _close(got, want, False)
    ab = R.attention_bounds(q, k, v, do, 0.5)
    assert all(bool((getattr(ab, n) > 0).all()) and float(getattr(ab, n).max()) < 1e-4 for n in ("o", "dq", "dk", "dv"))


# ------------------------------------------------------------------------------------------ the exact tier's premise
@pytest.mark.parametrize("c", R.CASES, ids=_id)
def test_exact_tier_premise_every_partial_sum_below_2_to_24_units(c):
    """A condition, not a measurement: every term a whole multiple of the unit and the sum of their magnitudes below 2^24
    units - then every fp32 partial sum is exact in every order and under every split, and so are the alpha multiply
    (a power of two), the bias add and the accumulate add."""
    t = R.inputs(c, "int")
    for name, (n, _) in R.layout(c).items():
        nz = t[name][t[name] != 0].abs()
        lg = torch.log2(nz.min()) if len(nz) else torch.zeros(())
        assert abs(float(lg)) <= 20
    for alpha in R.ALPHAS:
        unit = R.unit_of(c, alpha)
        assert abs(torch.log2(torch.tensor(unit)).item()) <= 20 and 2.0 ** round(torch.log2(torch.tensor(unit)).item()) == unit
        for g in R.gemm_model(c, t, alpha, True, True):
            units = g.abs_sum / unit
            assert torch.equal(units, units.round()), "a term is not a whole multiple of the unit"
            assert float(units.max()) < 2 ** 24
            ex = g.exact / unit
            assert torch.equal(ex, ex.round())


@pytest.mark.parametrize("M,N,ld", R.COLSUM_SHAPES)
def test_exact_tier_premise_of_the_column_sums(M, N, ld):
    x, old = R.colsum_inputs(M, N, ld, "int")
    e, a = R.colsum_model(x.view(M, ld)[:, :N], old)
    units = a / 0.25
    assert torch.equal(units, units.round()) and float(units.max()) < 2 ** 24
    assert R.colsum_slabs(M, N) * -(-M // R.colsum_slabs(M, N)) >= M


def test_impulse_inputs_name_their_element():
    c = R.BY_ID["segs_mixed"]
    for job, row, seg, k in R.impulses(c):
        t, want = R.impulse_inputs(c, job, row, seg, k)
        got = R.gemm_model(c, t, 1.0, False, False)
        assert torch.equal(got[job].exact, want[job]) and int((want[job] != 0).sum()) == c.jobs[job].N


# ------------------------------------------------------------------------------------------ mirror against the library
def assert_same_route(L, c, aligned=None, ws_bytes=None, ws=-1):
    got, need = lib_route(L, c, aligned, ws_bytes, ws)
    want = R.mirror(c, aligned, ws_bytes, None if ws == -1 else (ws is not None and ws % 4 == 0))
    assert got == want, (c.id, aligned, ws_bytes, ws, got, want)
    return got


def test_mirror_equals_the_library_route_on_the_cases():
    L = _lib()
    for c in R.CASES:
        r = assert_same_route(L, c)
        assert r is not None, c.id
        assert_same_route(L, c, ws_bytes=0)
        assert_same_route(L, c, aligned={name: False for name in R.layout(c)})
        # the workspace pointer is judged as the call judges it: NULL or off the 4-byte grid is no workspace, whatever
        # its size; the query never reads through it
        for ws in (None, FAKE_WS + 2, FAKE_WS + 4):
            got = assert_same_route(L, c, ws_bytes=1 << 40, ws=ws)
            assert got["nsplit"] == (got["nsplit_wanted"] if ws == FAKE_WS + 4 else 1), (c.id, ws)


def sweep_cases():
    one = lambda M, N, K, a, b, batch, strides=None: R.Case("sweep", (R.JobSpec(M, N, N, (R.SegSpec(K, a, b),)),), batch, strides)
    up4 = lambda n: (n + 3) // 4 * 4
    for M, N in itertools.product((1, 3, 63, 64, 65, 127, 128, 129, 130, 256, 2944), repeat=2):
        for K, batch in itertools.product((1, 15, 16, 17, 64, 656, 1060), ((1, 1), (3, 2), (16, 8), (32, 16))):
            pats = [(R.Op("k"), R.Op("k")), (R.Op("k", up4(K)), R.Op("r", up4(N))), (R.Op("r", up4(M)), R.Op("k", up4(K))),
                    (R.Op("k", up4(K), 1), R.Op("s2")), (R.Op("r"), R.Op("r"))]
            for a, b in pats:
                yield one(M, N, K, a, b, batch)
            if batch != (1, 1):                   # a batch stride off the float4 grid
                base = R.case_strides(one(M, N, K, pats[1][0], pats[1][1], batch))
                yield one(M, N, K, pats[1][0], pats[1][1], batch, (base[0], base[1] + 1, base[2] + 2, base[3], base[4], base[5]))


def test_mirror_equals_the_library_route_on_a_sweep():
    L = _lib()
    n = 0
    for c in sweep_cases():
        for ws in (None, 0):
            assert_same_route(L, c, ws_bytes=ws)
            n += 1
    assert n > 30000


def test_workspace_query_sizes_the_split_the_plan_wants():
    L = _lib()
    for c in R.CASES:
        r, need = lib_route(L, c)
        batch = c.batch[0] * c.batch[1]
        want = 4 * r["nsplit_wanted"] * sum(j.M * j.N for j in c.jobs) * batch if r["nsplit_wanted"] > 1 else 0
        assert need == want, c.id


# ------------------------------------------------------------------------------------------ coverage, from the query
def test_cases_enter_every_route():
    L = _lib()
    routes = {c.id: lib_route(L, c)[0] for c in R.CASES}
    by = lambda pred: [i for i, r in routes.items() if pred(r, R.BY_ID[i])]
    assert {r["tile"] for r in routes.values()} == {64, 128}
    pairs64 = {(a, b) for r in routes.values() if r["tile"] == 64 for a, b in zip(r["amode"], r["bmode"])}
    assert pairs64 == set(itertools.product(range(3), repeat=2))
    assert {(a, b) for r in routes.values() if r["tile"] == 128 for a, b in zip(r["amode"], r["bmode"])} >= {(1, 1), (1, 2), (2, 1)}
    for tile in (64, 128):
        arms = set()
        for i, r in routes.items():
            if r["tile"] == tile:
                arms |= R.tail_arms(R.BY_ID[i], r)
        assert arms >= ({(m, l) for m in (1, 2) for l in (1, 2, 3)} if tile == 64 else {(1, 2), (2, 2)}), (tile, arms)
    for tile in (64, 128):
        # FAST and guarded tiles in one launch; a launch that is all guarded although every mode is a vector mode
        assert by(lambda r, c: r["tile"] == tile and 0 < sum(r["fast_tiles"]) <= r["tiles"]), tile
    assert by(lambda r, c: 0 < sum(r["fast_tiles"]) < r["tiles"])
    assert by(lambda r, c: sum(r["fast_tiles"]) == 0 and min(r["amode"] + r["bmode"]) > 0 and
              all(j.M >= r["tile"] and j.N >= r["tile"] for j in c.jobs))          # K % 16 != 0 on an interior tile
    assert by(lambda r, c: r["nsplit"] == 1 and r["nsplit_wanted"] == 1)
    assert {r["nsplit"] for r in routes.values()} >= {1, 2, 3, 8, 10, 16}
    assert by(lambda r, c: r["nsplit"] > 1 and max(r["empty_shares"]) == 2)
    assert by(lambda r, c: r["nsplit"] > 1 and max(r["empty_shares"]) == 1 and r["nchunks"][0] % r["per"][0] == 1)
    assert by(lambda r, c: r["nsplit"] > 1 and c.jobs[0].segs[-1].K % 16 == 1)     # ends on a one-element chunk
    declined = by(lambda r, c: r["nsplit"] == 1 and r["nsplit_wanted"] == 16)
    assert {R.BY_ID[i].ws for i in declined} == {"none", "short", "null_sized"}
    # more than one segment, a mode change at every boundary, a one-chunk segment, K % 16 != 0, a share starting inside
    seg = routes["segs_mixed"]
    modes = list(zip(seg["amode"], seg["bmode"]))
    assert seg["nsegs"] == 5 and all(modes[i] != modes[i + 1] for i in range(4)) and seg["nsplit"] == 2
    assert seg["per"][0] in seg["chunk0"][1:] or any(c0 < seg["per"][0] for c0 in seg["chunk0"][1:])
    assert 0 < seg["per"][0] < seg["nchunks"][0] and seg["chunk0"] == [0, 1, 2, 5, 9]
    s32 = routes["segs_32x1"]
    assert s32["nsegs"] == 32 and s32["chunk0"] == list(range(32)) and s32["nsplit"] == 8
    assert by(lambda r, c: r["njobs"] > 1 and r["nsplit"] > 1 and len(set(r["nchunks"])) > 1)
    assert by(lambda r, c: r["njobs"] == 32)
    assert by(lambda r, c: r["njobs"] > 1 and r["tile"] == 128 and r["tile0"][1] > 0)
    assert by(lambda r, c: r["njobs"] == 3 and r["nsplit"] == 1)
    assert by(lambda r, c: c.batch != (1, 1) and r["nsplit"] > 1 and min(r["amode"] + r["bmode"]) > 0)
    assert by(lambda r, c: c.batch != (1, 1) and r["nsplit"] > 1 and max(r["amode"] + r["bmode"]) == 0)
    assert by(lambda r, c: r["tile"] == 128 and c.batch == (1, 1) and r["tiles"] == 512)
    assert by(lambda r, c: any(j.ldc > j.N for j in c.jobs) and r["nsplit"] > 1)
    assert by(lambda r, c: any(j.ldc > j.N for j in c.jobs) and r["tile"] == 128)
    assert routes["one"]["tile"] == 64 and routes["one"]["nsplit"] == 1 and routes["one"]["amode"] == [0]


# ------------------------------------------------------------------------------------------ refusals
def refused_calls():
    """name -> arguments of a call outside the library's domain (R.REFUSALS over a valid table at fake addresses)."""
    base = R.BY_ID[R.REFUSAL_BASE]
    out = {}
    for name, mut in R.REFUSALS.items():
        J, S, _ = R.tables(base, fake_addresses(base))
        out[name] = dict(J=J, nj=len(J), S=S, ns=len(S), bo=1, bi=1)
        mut(out[name])
    return out


def test_calls_outside_the_domain_are_refused_by_the_query():
    from unlearn_saliency_amd._lib import GemmRoute
    L = _lib()
    zeros = (ctypes.c_int64 * 6)()
    for name, a in refused_calls().items():
        r = GemmRoute()
        rc = L.salun_gemm_f32_route(a["J"], a["nj"], a["S"], a["ns"], a["bo"], a["bi"], zeros, FAKE_WS, 1 << 30, ctypes.byref(r))
        assert rc == EINVAL, name
        assert L.salun_gemm_f32_workspace_bytes(a["J"], a["nj"], a["S"], a["ns"], a["bo"], a["bi"]) == 0, name
    base = R.BY_ID[R.REFUSAL_BASE]
    assert R.mirror(base._replace(batch=(256, 256), strides=(0,) * 6)) is None
    assert R.mirror(base._replace(jobs=base.jobs * 17)) is None
