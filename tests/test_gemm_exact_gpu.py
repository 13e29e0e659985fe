"""K15 (csrc/salun_gemm.hip lines 1-540; gemm.py) against the float64 models of gemm_ref_cpu.py (validated by
test_gemm_ref_cpu.py), on every route the host-side plan can take (gemm_ref_cpu.CASES; test_gemm_ref_cpu.py reads from
`salun_gemm_f32_route` that they are entered):

(a) exact tier: integers in [-8, 8] times a power of two per tensor, integer bias and old C.  Every fp32 partial sum is
    exact in every order and under every split (the cap asserted in test_gemm_ref_cpu.py), so C must EQUAL the float64
    answer: writing and accumulating, with and without bias, at alpha 1, 0.5 and -2 (all twelve combinations); a second
    call of the last combination (alpha -2, bias, accumulating) gives the same bits - that one only, not each of the
    twelve; without a workspace (NULL with or without a size, or one a byte short) the unsplit launch gives the bits of
    the split one.  Impulse inputs name
    the (row, column, k, segment) of a wrong element.
(b) bound tier: Gaussian operands; every element within gamma_(2n+3) * abs_sum of the exact answer (n = reduction
    length; 2n: product and add rounded separately, so the bound holds for every summation tree and split; +3: alpha,
    bias, accumulate).  No absolute slack, nothing scaled by a tensor's maximum.  The worst ratio is printed and logged
    (profiles/gemm_bounds_measured.txt) but not asserted: nothing here is taken from what the kernels do today.
(c) refusals: SALUN_EINVAL and every output sentinel still in place.
(d) salun_colsum_f32, (e) salun_softmax_rows / _backward: exact inputs and derived bounds (gemm_ref_cpu's docstring).
(f) gemm.py (linear, grouped_linear, attention_f32) on the composed models.

The kernels are called through the C-ABI on views the test owns (guarded_arena.py): one flat allocation, 4096 floats of
NaN around every input, a sentinel NaN pattern around and inside every output - between the rows of a C with ldc > N and
in the workspace too; everything that is not an output must be bit-identical afterwards."""
import os
from ctypes import c_double, c_int64, c_size_t, c_void_p
from types import SimpleNamespace

import pytest
import torch

import gemm_ref_cpu as R
from guarded_arena import NAN_BITS, SENTINEL, Arena

pytestmark = pytest.mark.gpu

F64 = torch.float64
I32 = torch.int32
EINVAL, ENOSPC = -22, -28
CASES = R.CASES
_id = lambda c: c.id
VARIANTS = [(alpha, bias, acc) for acc in (False, True) for bias in (False, True) for alpha in R.ALPHAS]


def L():
    from unlearn_saliency_amd import _lib
    return _lib.lib()


def stream():
    from unlearn_saliency_amd.streams import _stream
    return _stream()


def log(line):
    print(line)
    d = os.environ.get("SALUN_MEASURED_DIR")      # where a recording run keeps its figures (profiles/ has the last ones)
    if d and os.path.isdir(d):
        with open(os.path.join(d, "gemm_bounds_measured.txt"), "a") as f:
            f.write(line + "\n")


def bits_of(x):
    return x.float().contiguous().view(I32)


def same(got, want64):
    """Bit-for-bit equality with a float64 answer that fp32 holds exactly (+0 and -0 alike)."""
    want = want64.float()
    assert torch.equal(want.double(), want64), "the expected answer is not an fp32 number"
    return got.shape == want.shape and torch.equal(got, want)


def first_wrong(got, want64):
    bad = (got.double() != want64).nonzero()
    if len(bad) == 0:
        return "shape"
    i = tuple(int(v) for v in bad[0])
    return f"{len(bad)} wrong, first at {i}: got {float(got[i])!r}, want {float(want64[i])!r}"


# ------------------------------------------------------------------------------------------ one salun_gemm_f32 call
class Call:
    """The buffers of a case in a guarded arena; run() launches one variant and returns C per job after checking that
    nothing but the logical elements of the outputs changed."""

    def __init__(self, c, t):
        self.c, self.t, self.st = c, t, R.case_strides(c) or (0,) * 6
        self.need = R.mirror(c)["ws_need"]
        a = Arena()
        for name, (n, skew) in sorted(R.layout(c).items()):
            if name[0] == "c":
                a.put(name, shape=(n,), out=True)
            else:
                a.put(name, t[name], skew=skew)
        if self.need and c.ws == "full":
            a.put("ws", shape=(self.need // 4,), out=True)
        elif self.need and c.ws == "short":        # offered a byte short: must not be touched
            a.put("ws", torch.full((self.need // 4,), NAN_BITS, dtype=I32))
        self.a = a.upload()
        self.inside = {}
        for ji, j in enumerate(c.jobs):
            m = torch.zeros(R.layout(c)[f"c{ji}"][0], dtype=torch.bool)
            R.c_view(m, j, self.st, c.batch)[:] = True
            self.inside[ji] = m

    def c_start(self, ji, accumulate):
        """The bit pattern C starts from: the sentinel, with the old values at the logical elements of an accumulating job."""
        j = self.c.jobs[ji]
        b = torch.full((R.layout(self.c)[f"c{ji}"][0],), SENTINEL, dtype=I32)
        if accumulate:
            R.c_view(b, j, self.st, self.c.batch)[:] = R.c_view(bits_of(self.t[f"c{ji}"]), j, self.st, self.c.batch)
        return b

    def run(self, alpha=1.0, bias=False, accumulate=False):
        c, a = self.c, self.a
        a.restore(**{f"c{ji}": self.c_start(ji, R.job_flags(j, bias, accumulate)[1]) for ji, j in enumerate(c.jobs)})
        addr = {name: a.ptr(name).value for name in R.layout(c)}
        J, S, st = R.tables(c, addr, bias, accumulate)
        assert L().salun_gemm_f32_workspace_bytes(J, len(J), S, len(S), c.batch[0], c.batch[1]) == self.need
        ws_bytes = R.WS_BYTES[c.ws](self.need)
        rc = L().salun_gemm_f32(J, len(J), S, len(S), c.batch[0], c.batch[1], st, c_double(alpha),
                                a.ptr("ws") if R.WS_POINTER[c.ws] else c_void_p(None), c_size_t(ws_bytes), stream())
        assert rc == 0, (c.id, rc)
        after = a.download()
        outs = []
        for ji, j in enumerate(c.jobs):
            raw = a.part(after, f"c{ji}")
            assert bool((raw.view(I32)[~self.inside[ji]] == SENTINEL).all()), \
                f"{c.id}: job {ji} wrote between the rows of C (ldc {j.ldc} > N {j.N}) or between its batch instances"
            outs.append(R.c_view(raw, j, self.st, c.batch))
        return outs


# ------------------------------------------------------------------------------------------ (a) exact tier
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_gemm_equals_the_exact_answer(c):
    """All twelve (alpha, bias, accumulate) combinations; the last one is then called a second time."""
    t = R.inputs(c, "int")
    call = Call(c, t)
    for alpha, bias, acc in VARIANTS:
        got = call.run(alpha, bias, acc)
        for ji, (g, m) in enumerate(zip(got, R.gemm_model(c, t, alpha, bias, acc))):
            assert same(g, m.exact), (c.id, alpha, bias, acc, f"job {ji}", first_wrong(g, m.exact))
    again = call.run(alpha, bias, acc)
    assert all(torch.equal(x.contiguous().view(I32), y.contiguous().view(I32)) for x, y in zip(got, again)), "second call"


@pytest.mark.parametrize("ws", ["null", "short", "null_sized"])
def test_without_a_workspace_the_unsplit_launch_gives_the_bits_of_the_split_one(ws):
    split, unsplit = R.BY_ID["split16"], R.BY_ID[f"split_no_ws_{ws}"]
    assert R.mirror(split)["nsplit"] == 16 and R.mirror(unsplit)["nsplit"] == 1 and R.layout(split) == R.layout(unsplit)
    t = R.inputs(split, "int")
    for alpha, bias, acc in ((1.0, False, False), (-2.0, True, True)):
        x, y = Call(split, t).run(alpha, bias, acc)[0], Call(unsplit, t).run(alpha, bias, acc)[0]
        assert torch.equal(x.contiguous().view(I32), y.contiguous().view(I32))
        assert same(x, R.gemm_model(split, t, alpha, bias, acc)[0].exact)


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_impulses_give_the_column_of_b_where_it_belongs(c):
    """A single 1 in A at (row, k) of one segment against B(col, k) = a distinct integer: C[row, :] is that column of B,
    every other element of every job is 0."""
    for job, row, seg, k in R.impulses(c):
        t, want = R.impulse_inputs(c, job, row, seg, k)
        got = Call(c, t).run()
        for ji, (g, w) in enumerate(zip(got, want)):
            if not same(g, w):
                bad = (g.double() != w).nonzero()[0].tolist()
                ktot = sum(s.K for s in c.jobs[ji].segs)
                v = float(g[tuple(bad)])
                src = f"holds B(col {int(v - 1) // ktot}, k {int(v - 1) % ktot})" if v == v and v == int(v) and v >= 1 else "no element of B"
                raise AssertionError(f"{c.id}: impulse at job {job} row {row} segment {seg} k {k}: job {ji} element "
                                     f"(batch {bad[:2]}, row {bad[2]}, col {bad[3]}) is {v!r}, want {float(w[tuple(bad)])!r} ({src})")


# ------------------------------------------------------------------------------------------ (b) bound tier
def within_bound(tag, got, exact, abs_sum, k):
    """|got - exact| <= gamma_k * abs_sum for every element; the measured ratio to u * abs_sum is logged first."""
    err = (got.double() - exact).abs()
    ratio = torch.where(abs_sum > 0, err / (R.U * abs_sum.clamp_min(1e-300)), torch.where(err > 0, float("inf"), 0.0).double())
    log(f"{tag}: worst |got - exact| = {float(ratio.max()):.3f} u * abs_sum (bound {R.bound_gamma(k) / R.U:.1f})")
    assert bool((err <= R.bound_gamma(k) * abs_sum).all()), tag


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_gemm_within_the_per_element_bound(c):
    t = R.inputs(c, "gauss")
    call = Call(c, t)
    r = R.mirror(c)
    for alpha, bias, acc in ((1.0, False, False), (-2.0, True, True)):
        got = call.run(alpha, bias, acc)
        for ji, (g, m) in enumerate(zip(got, R.gemm_model(c, t, alpha, bias, acc))):
            if ji in (0, len(got) - 1) or len(got) <= 3:
                within_bound(f"gemm {c.id} job {ji} tile {r['tile']} split {r['nsplit']} alpha {alpha} bias {int(bias)} "
                             f"acc {int(acc)} n {m.n}", g, m.exact, m.abs_sum, 2 * m.n + 3)
            else:
                assert bool(((g.double() - m.exact).abs() <= R.bound_gamma(2 * m.n + 3) * m.abs_sum).all()), (c.id, ji)


# ------------------------------------------------------------------------------------------ (c) refusals
def test_calls_outside_the_domain_are_refused_and_nothing_is_written():
    c = R.BY_ID[R.REFUSAL_BASE]
    zeros = (c_int64 * 6)()
    for name, mut in R.REFUSALS.items():
        call = Call(c, R.inputs(c, "int"))
        a = call.a
        J, S, _ = R.tables(c, {n: a.ptr(n).value for n in R.layout(c)})
        args = dict(J=J, nj=len(J), S=S, ns=len(S), bo=1, bi=1)
        mut(args)
        rc = L().salun_gemm_f32(args["J"], args["nj"], args["S"], args["ns"], args["bo"], args["bi"], zeros, c_double(1.0),
                                a.ptr("ws"), c_size_t(call.need), stream())
        assert rc == EINVAL, name
        after = a.download()
        for out in ("c0", "c1", "ws"):
            assert bool((a.part(after, out).view(I32) == SENTINEL).all()), (name, out)


# ------------------------------------------------------------------------------------------ (d) column sums
def call_colsum(M, N, ld, x, old, accumulate, short=False):
    wsb = L().salun_colsum_f32_workspace_bytes(c_int64(M), N)
    assert wsb == 4 * R.colsum_slabs(M, N) * N
    a = Arena().put("x", x).put("out", data=old if accumulate else None, shape=(N,), out=True)
    a.put("ws", shape=(wsb // 4,), out=True).upload()
    rc = L().salun_colsum_f32(a.ptr("x"), a.ptr("out"), c_int64(M), N, c_int64(ld), int(accumulate), a.ptr("ws"),
                              c_size_t(wsb - 1 if short else wsb), stream())
    return rc, a


@pytest.mark.parametrize("M,N,ld", R.COLSUM_SHAPES)
def test_colsum_exact_and_within_its_bound(M, N, ld):
    """(8197, 3, 8): 512 slabs of 17 rows, the last ones start past M.  Bound: M - 1 additions inside the sum and one to
    accumulate: gamma_M * (sum |x| + |old|)."""
    for accumulate in (False, True):
        x, old = R.colsum_inputs(M, N, ld, "int")
        rc, a = call_colsum(M, N, ld, x, old, accumulate)
        exact, _ = R.colsum_model(x.view(M, ld)[:, :N], old if accumulate else None)
        got = a.result("out")
        assert rc == 0 and same(got, exact), (accumulate, first_wrong(got, exact))
        x, old = R.colsum_inputs(M, N, ld, "gauss")
        rc, a = call_colsum(M, N, ld, x, old, accumulate)
        exact, abs_sum = R.colsum_model(x.view(M, ld)[:, :N], old if accumulate else None)
        assert rc == 0
        within_bound(f"colsum {M}x{N} ld {ld} slabs {R.colsum_slabs(M, N)} acc {int(accumulate)}", a.result("out"), exact,
                     abs_sum, M)
    rc, a = call_colsum(M, N, ld, x, old, True, short=True)
    after = a.download()
    assert rc == ENOSPC and torch.equal(a.part(after, "out").view(I32), bits_of(old))
    assert bool((a.part(after, "ws").view(I32) == SENTINEL).all())


# ------------------------------------------------------------------------------------------ (e) row softmax
def padded_bits(x, ld, fill):
    """rows x n values as the bit pattern of rows x ld floats, `fill` in the ld - n columns behind every row."""
    rows, n = x.shape
    b = torch.full((rows, ld), fill, dtype=I32)
    b[:, :n] = bits_of(x)
    return b


def run_softmax(x, ld):
    rows, n = x.shape
    a = Arena().put("s", data=padded_bits(x, ld, SENTINEL), out=True).upload()
    assert L().salun_softmax_rows(a.ptr("s"), c_int64(rows), n, ld, stream()) == 0
    got = a.result("s")
    assert bool((got.view(I32)[:, n:] == SENTINEL).all()), "wrote behind a row"
    return got[:, :n]


def run_softmax_backward(p, dp, ld, scale):
    rows, n = p.shape
    a = Arena().put("p", data=padded_bits(p, ld, NAN_BITS)).put("dp", data=padded_bits(dp, ld, SENTINEL), out=True).upload()
    assert L().salun_softmax_rows_backward(a.ptr("p"), a.ptr("dp"), c_int64(rows), n, ld, c_double(scale), stream()) == 0
    got = a.result("dp")
    assert bool((got.view(I32)[:, n:] == SENTINEL).all()), "wrote behind a row"
    return got[:, :n]


def one_hot_rows(rows, n, g):
    """One 0 per row, every other entry <= -200: the hot column in the first 64, at a multiple of 64, last."""
    spots = sorted({min(5, n - 1), (n - 1) // 64 * 64, n - 1, 0})
    hot = torch.tensor([spots[r % len(spots)] for r in range(rows)])
    x = -200.0 - torch.randint(0, 50, (rows, n), generator=g).to(F64)
    x[torch.arange(rows), hot] = 0.0
    return x, hot


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("n", R.SOFTMAX_N)
def test_softmax_rows_exact_and_within_their_bound(n, pad):
    ld = n + pad
    for rows in R.SOFTMAX_ROWS:                   # 8197 rows: past the 2048-block grid of 4 rows each
        g = torch.Generator().manual_seed(rows * 1000 + n)
        tag = f"softmax rows {rows} n {n} ld {ld}"
        x, hot = one_hot_rows(rows, n, g)
        want = torch.zeros(rows, n, dtype=F64)
        want[torch.arange(rows), hot] = 1.0
        got = run_softmax(x, ld)
        assert same(got, want), (tag, "one-hot", first_wrong(got, want))
        dP = torch.randint(-8, 9, (rows, n), generator=g).to(F64)
        exact_P = [want, torch.randint(0, 5, (rows, n), generator=g).to(F64) / 64]
        if n & (n - 1) == 0:                      # constant rows, n a power of two: exactly 1 / n
            x = (torch.arange(rows, dtype=F64) % 7 - 3)[:, None].expand(rows, n).contiguous()
            want = torch.full((rows, n), 1.0 / n, dtype=F64)
            got = run_softmax(x, ld)
            assert same(got, want), (tag, "constant", first_wrong(got, want))
            exact_P.append(want)
        for P in exact_P:
            dS, _ = R.softmax_backward_model(P, dP, 0.125)
            got = run_softmax_backward(P, dP, ld, 0.125)
            assert same(got, dS), (tag, "backward", first_wrong(got, dS))
        for std in (1.0, 4.0):
            x = (torch.randn(rows, n, generator=g, dtype=F64) * std).float().to(F64)
            assert float((x - x.max(-1, keepdim=True).values).abs().max()) <= 60
            P, bound = R.softmax_model(x)
            got = run_softmax(x, ld)
            err = (got.double() - P).abs()
            log(f"{tag} std {std}: worst |got - exact| = {float((err / bound).max()):.3f} of the bound "
                f"({float((err / (R.U * P)).max()):.2f} u relative)")
            assert bool((err <= bound).all()), tag
            dP = torch.randn(rows, n, generator=g, dtype=F64).float().to(F64)
            Pf = got.double()                     # the backward's input is the fp32 P the forward produced
            dS, bound = R.softmax_backward_model(Pf, dP, 0.125)
            err = (run_softmax_backward(Pf, dP, ld, 0.125).double() - dS).abs()
            ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), (err > 0).double() * float("inf")).nan_to_num(0.0)
            log(f"{tag} std {std} backward: worst |got - exact| = {float(ratio.max()):.3f} of the bound")
            assert bool((err <= bound).all()), tag


# ------------------------------------------------------------------------------------------ (f) gemm.py
def ints(shape, g, lim=8):
    return torch.randint(-lim, lim + 1, shape, generator=g).to(F64)


def gauss(shape, g):
    return torch.randn(shape, generator=g, dtype=F64).float().to(F64)


def dev(x):
    return x.float().cuda()


def check(tag, got, exact, bound, exact_tier):
    got = got.detach().cpu()
    exact = exact.reshape(got.shape)
    if exact_tier:
        assert same(got, exact), (tag, first_wrong(got, exact))
    else:
        bound = bound.reshape(got.shape)
        err = (got.double() - exact).abs()
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), (err > 0).double() * float("inf")).nan_to_num(0.0)
        log(f"{tag}: worst |got - exact| = {float(ratio.max()):.3f} of the bound")
        assert bool((err <= bound).all()), tag


def pb(e_s_n):
    """gamma_(2n+3) * abs_sum of a gemm_ref_cpu.product."""
    return R.bound_gamma(2 * e_s_n[2] + 3) * e_s_n[1]


@pytest.mark.parametrize("tier", ["exact", "bound"])
@pytest.mark.parametrize("form", ["3d", "strided", "sink_twice"])
def test_linear_on_the_model(form, tier):
    from unlearn_saliency_amd import gemm
    from unlearn_saliency_amd.flat import arena_of
    ex = tier == "exact"
    g = torch.Generator().manual_seed(len(form) + 10 * ex)
    mk = ints if ex else gauss
    K, N = 13, 6
    x64, w, b, dy = mk((3, 5, 2 * K if form == "strided" else K), g), mk((N, K), g), mk((N,), g), mk((3, 5, N), g)
    lin = torch.nn.Linear(K, N).cuda()
    with torch.no_grad():
        lin.weight.copy_(dev(w)), lin.bias.copy_(dev(b))
    assert gemm.use_salun_linears(lin) == 1
    arena = arena_of(lin) if form == "sink_twice" else None
    xd = dev(x64).requires_grad_(True)
    xin, x64 = (xd[..., ::2], x64[..., ::2]) if form == "strided" else (xd, x64)
    assert (xin.stride(-1) != 1) == (form == "strided")
    m = R.linear_model(x64, w, b, dy)
    passes = 2 if form == "sink_twice" else 1
    for _ in range(passes):
        y = lin(xin)
        y.backward(dev(dy))
    check(f"linear {form} y", y, m.y[0], pb(m.y), ex)
    dxb = pb(m.dx)
    dx = xd.grad[..., ::2] if form == "strided" else xd.grad
    # autograd adds the passes' dx: one more rounding of the sum
    check(f"linear {form} dx", dx, passes * m.dx[0], passes * dxb + (passes - 1) * R.U * (passes * m.dx[0].abs() + 2 * dxb), ex)
    if form == "sink_twice":
        assert lin.weight.grad.data_ptr() == arena.grads.data_ptr()
        b1 = pb(m.dw)
        b2 = R.bound_gamma(2 * m.dw[2] + 3) * (m.dw[1] + m.dw[0].abs() + b1) + b1
        check("linear sink_twice dW", lin.weight.grad, 2 * m.dw[0], b2, ex)
        c1 = R.bound_gamma(m.rows) * m.db[1]
        check("linear sink_twice db", lin.bias.grad, 2 * m.db[0], R.bound_gamma(m.rows) * (m.db[1] + m.db[0].abs() + c1) + c1, ex)
    else:
        check(f"linear {form} dW", lin.weight.grad, m.dw[0], pb(m.dw), ex)
        check(f"linear {form} db", lin.bias.grad, m.db[0], R.bound_gamma(m.rows) * m.db[1], ex)


@pytest.mark.parametrize("tier", ["exact", "bound"])
@pytest.mark.parametrize("dead", [None, 17])
def test_grouped_linear_of_34_layers_on_the_model(dead, tier):
    """34 Linear(8 -> 3) on one input: two forward launches (32 + 2 jobs), two weight-gradient launches, and an input
    gradient of two launches (32 + 2 segments, or 32 + 1 with one gradient None) whose second accumulates."""
    from unlearn_saliency_amd import gemm
    ex = tier == "exact"
    variant = "34 live" if dead is None else f"33 live, [{dead}] None"
    g = torch.Generator().manual_seed(34 + ex)
    mk = ints if ex else gauss
    G, M, K, N = 34, 5, 8, 3
    x64 = mk((M, K), g)
    ws, bs, dys = [mk((N, K), g) for _ in range(G)], [mk((N,), g) for _ in range(G)], [mk((M, N), g) for _ in range(G)]
    layers = [torch.nn.Linear(K, N).cuda() for _ in range(G)]
    with torch.no_grad():
        for l, w, b in zip(layers, ws, bs):
            l.weight.copy_(dev(w)), l.bias.copy_(dev(b))
    x = dev(x64).requires_grad_(True)
    outs = gemm.grouped_linear(x, layers)
    live = [i for i in range(G) if i != dead]
    torch.autograd.backward([outs[i] for i in live], [dev(dys[i]) for i in live])
    for i in range(G):
        y = R.product(x64, ws[i], bias=bs[i])
        check(f"grouped {variant} y[{i}]", outs[i], y[0], pb(y), ex)
        if i == dead:
            assert layers[i].weight.grad is None or float(layers[i].weight.grad.abs().max()) == 0
            continue
        dw = R.product(dys[i].t(), x64.t())
        check(f"grouped {variant} dW[{i}]", layers[i].weight.grad, dw[0], pb(dw), ex)
        db = R.colsum_model(dys[i])
        check(f"grouped {variant} db[{i}]", layers[i].bias.grad, db[0], R.bound_gamma(M) * db[1], ex)
    first, rest = live[:32], live[32:]
    cat = lambda idx: (torch.cat([dys[i] for i in idx], 1), torch.cat([ws[i] for i in idx], 0).t())
    d1 = R.product(*cat(first))
    b1 = pb(d1)
    d2 = R.product(*cat(rest), old=d1[0])
    check(f"grouped {variant} dx", x.grad, d2[0], R.bound_gamma(2 * d2[2] + 3) * (d2[1] + b1) + b1, ex)


def one_hot_attention(B, H, Tq, Tk, D, g):
    """Integer q, k with one key per query ahead of every other by >= 512 in the scaled score: P is one-hot exactly
    (exp2 of less than -700 is 0 in fp32), so o = v[selected] and dv = P^T dO exactly, dq = dk = 0."""
    if D == 1:
        codes = torch.arange(1, Tk + 1, dtype=F64)[:, None]
        u = torch.tensor([[1.0 if i % 2 == 0 else -1.0] for i in range(Tq)], dtype=F64)
    else:
        assert D == 3 and Tk <= 7
        codes = torch.tensor([(1, 2, 2), (2, 1, 2), (2, 2, 1), (-1, 2, 2), (2, -1, 2), (2, 2, -1), (1, -2, 2)], dtype=F64)[:Tk]
        u = codes[(3 * torch.arange(Tq) + 1) % Tk]
    s = u @ codes.t()
    top = s.topk(2, -1).values if Tk > 1 else None
    assert Tk == 1 or float((top[:, 0] - top[:, 1]).min()) >= 1
    q = (32 * u).expand(B, H, Tq, D).clone()
    k = (32 * codes).expand(B, H, Tk, D).clone()
    return q, k, ints((B, H, Tk, D), g), ints((B, H, Tq, D), g), 0.5


def in_layout(x64, layout):
    """[B, H, T, D] values as a device view in the DDPM's channel-major memory ([B, D, T], H = 1), the SD projections'
    ([B, T, H * D]), or with an arbitrary stride on every size-1 dimension."""
    B, H, T, D = x64.shape
    if layout == "ddpm":
        assert H == 1
        return dev(x64).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    if layout == "sd":
        return dev(x64).permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    t = dev(x64).contiguous()
    strides = [st if sz > 1 else 12345 + 2 * i for i, (st, sz) in enumerate(zip(t.stride(), t.shape))]
    if D == 1:
        strides[2] = 1
    return t.as_strided(t.shape, strides)


@pytest.mark.parametrize("tier", ["exact", "bound"])
@pytest.mark.parametrize("layout,B,H,Tq,Tk,D", [("ddpm", 3, 1, 5, 7, 3), ("sd", 1, 3, 5, 7, 3), ("odd", 1, 3, 1, 7, 3),
                                                ("odd", 3, 1, 5, 7, 1)])
def test_attention_f32_on_the_model(layout, B, H, Tq, Tk, D, tier):
    from unlearn_saliency_amd import gemm
    ex = tier == "exact"
    g = torch.Generator().manual_seed(B * 100 + Tq * 10 + D + ex)
    if ex:
        q64, k64, v64, do64, scale = one_hot_attention(B, H, Tq, Tk, D, g)
    else:
        q64, k64, v64, do64 = gauss((B, H, Tq, D), g), gauss((B, H, Tk, D), g), gauss((B, H, Tk, D), g), gauss((B, H, Tq, D), g)
        scale = float(torch.tensor(D ** -0.5).float())       # the fp32 number the kernels multiply by
    q, k, v = (in_layout(t, layout).requires_grad_(True) for t in (q64, k64, v64))
    assert all(t.stride(2) == 1 or t.stride(3) == 1 for t in (q, k, v))
    o = gemm.attention_f32(q, k, v, scale)
    o.backward(in_layout(do64, layout))
    m = R.attention_model(q64, k64, v64, do64, scale)
    b = None if ex else R.attention_bounds(q64, k64, v64, do64, scale)
    if ex:
        # in float64 the other keys keep exp(-512) of weight; in fp32 they keep none: the answer is the one-hot one
        P = torch.zeros_like(m.P).scatter_(-1, m.s.argmax(-1, keepdim=True), 1.0)
        assert float((m.P - P).abs().max()) < 1e-200 and float((m.s.max(-1, keepdim=True).values - m.s)[P == 0].min()) >= 512
        zero = lambda t: torch.zeros_like(t)
        m = SimpleNamespace(o=P @ v64, dv=P.transpose(-1, -2) @ do64, dq=zero(q64), dk=zero(k64))
    for name, got in (("o", o), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        check(f"attention {layout} B{B} H{H} {Tq}x{Tk} d{D} {name}", got, getattr(m, name), None if ex else getattr(b, name), ex)
