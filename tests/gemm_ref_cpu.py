"""torch-float64 restatement of K15 (csrc/salun_gemm.hip lines 1-540, gemm.py) on the CPU (test infrastructure only, like
conv_ref_cpu.py): the exact answer of one `salun_gemm_f32` call over a job / segment table of strided views with a
two-level batch, with the per-element quantities its error bound needs; the row softmax, its backward and the column
sum with the bounds that follow from the rounding points those kernels have; the input makers of the exact, impulse and
bound tiers; a pure Python mirror of the host-side plan (`gemm_plan`); and CASES, one named table per route.

Error bound of a GEMM element: gamma_(2n+3) * abs_sum with abs_sum = |alpha| * sum |a||b| + |bias| + |c_old| and n the
total reduction length (2n: product and add rounded separately, so it holds fused or not, for every summation tree and
every split; +3: the alpha multiply, the bias add, the accumulate add).

Rounding points of k_softmax_rows (fp32 throughout), for one row x with maximum m (found exactly):
  t_j  = (x_j - m) * log2(e)   three roundings: the subtraction, the fp32 constant, the product -> |dt| <= ((1+u)^3 - 1)|t|
  e_j  = exp2(t_j)             the hardware exp2 (`__expf` is exp2 of the scaled argument): one ulp, 2^-23 relative;
                               the argument error |t| * 2^-24 per rounding above moves e_j by 2^dt
  sum  = sum_j e_j             n - 1 additions in some tree: gamma_(n-1)
  inv  = 1.0f / sum            csrc/Makefile passes neither -ffast-math nor -fno-hip-fp32-correctly-rounded-divide-sqrt, so
                               hipcc's default holds: the division is correctly rounded, one rounding u
  p_j  = e_j * inv             one rounding u
|x_j - m| <= 60 keeps every e_j a normal number (e^-60 > 2^-87), so nothing is flushed.
k_softmax_rows_bwd: dot = sum_j P_j dP_j (n products, n - 1 additions: gamma_n on sum |P dP|), then a subtraction and two
products, each rounded once."""
import math
from collections import namedtuple
from types import SimpleNamespace

import torch

F64 = torch.float64
U = 2.0 ** -24
BK = 16
MAXJ = MAXS = 32
ALPHAS = (1.0, 0.5, -2.0)


def bound_gamma(k):
    return k * U / (1 - k * U)


# ------------------------------------------------------------------------------------------ tables
# An operand of a segment: how the logical [rows, K] matrix lies in its buffer.
#   kind "k": rows of `width` floats, k contiguous         (row stride width, k stride 1)
#        "r": k-major, `width` floats per k, rows contiguous (row stride 1, k stride width) - a `.t()` view
#        "s2": every second column of a [rows, 2K] matrix    (row stride 2K, k stride 2)
#   skew: floats the base pointer lies off the 16-byte grid
Op = namedtuple("Op", "kind width skew", defaults=(None, 0))
SegSpec = namedtuple("SegSpec", "K a b")
# bias / accumulate: None follows the variant a test runs, True / False pins the flag for this job
JobSpec = namedtuple("JobSpec", "M N ldc segs bias accumulate", defaults=(None, None))
# strides: (a_bo, a_bi, b_bo, b_bi, c_bo, c_bi) or None for tight ones; ws: "full", "none" (NULL, 0 bytes), "short" (one
# byte short) or "null_sized" (NULL with the full byte count)
Case = namedtuple("Case", "id jobs batch strides ws", defaults=((1, 1), None, "full"))


def op_strides(op, rows, K):
    """-> (row stride, k stride, floats of one batch instance)"""
    if op.kind == "k":
        w = op.width or K
        assert w >= K
        return w, 1, rows * w
    if op.kind == "r":
        w = op.width or rows
        assert w >= rows
        return 1, w, K * w
    assert op.kind == "s2"
    return 2 * K, 2, rows * 2 * K


def _up4(n):
    return (n + 3) // 4 * 4


def case_strides(c):
    """The six batch strides of the call (None for a single instance)."""
    bo, bi = c.batch
    if bo * bi == 1:
        return None
    if c.strides is not None:
        return tuple(c.strides)
    a = max(op_strides(s.a, j.M, s.K)[2] for j in c.jobs for s in j.segs)
    b = max(op_strides(s.b, j.N, s.K)[2] for j in c.jobs for s in j.segs)
    cc = max(j.M * j.ldc for j in c.jobs)
    a, b, cc = _up4(a), _up4(b), _up4(cc)
    return (a * bi, a, b * bi, b, cc * bi, cc)


def buffer_len(inst, s_o, s_i, batch):
    return (batch[0] - 1) * s_o + (batch[1] - 1) * s_i + inst


def layout(c):
    """Every buffer of the call: name -> (floats, skew).  Operands "a<seg>", "b<seg>" (segments numbered through the
    call), outputs "c<job>", biases "bias<job>"."""
    st = case_strides(c) or (0,) * 6
    out, si = {}, 0
    for ji, j in enumerate(c.jobs):
        out[f"c{ji}"] = (buffer_len(j.M * j.ldc, st[4], st[5], c.batch), 0)
        out[f"bias{ji}"] = (j.N, 0)
        for s in j.segs:
            out[f"a{si}"] = (buffer_len(op_strides(s.a, j.M, s.K)[2], st[0], st[1], c.batch), s.a.skew)
            out[f"b{si}"] = (buffer_len(op_strides(s.b, j.N, s.K)[2], st[2], st[3], c.batch), s.b.skew)
            si += 1
    return out


def view(buf, rows, K, s_row, s_k, s_o, s_i, batch):
    return torch.as_strided(buf, (batch[0], batch[1], rows, K), (s_o, s_i, s_row, s_k))


def c_view(buf, j, st, batch):
    return torch.as_strided(buf, (batch[0], batch[1], j.M, j.N), (st[4], st[5], j.ldc, 1))


def seg_rows(c):
    """(job index, job, global segment index, segment) for every segment of the call, in table order."""
    si = 0
    for ji, j in enumerate(c.jobs):
        for s in j.segs:
            yield ji, j, si, s
            si += 1


def job_flags(j, bias, accumulate):
    return (j.bias if j.bias is not None else bias), (j.accumulate if j.accumulate is not None else accumulate)


def tables(c, addr, bias=False, accumulate=False):
    """The ctypes job / segment tables of the call over buffers at `addr` (name -> address) -> (J, S, strides or None)."""
    import ctypes
    from unlearn_saliency_amd._lib import GemmJob, GemmSeg
    nseg = sum(len(j.segs) for j in c.jobs)
    J, S = (GemmJob * len(c.jobs))(), (GemmSeg * nseg)()
    seg0 = 0
    for ji, j in enumerate(c.jobs):
        use_bias, acc = job_flags(j, bias, accumulate)
        J[ji].C, J[ji].bias = addr[f"c{ji}"], (addr[f"bias{ji}"] if use_bias else None)
        J[ji].M, J[ji].N, J[ji].ldc, J[ji].seg0, J[ji].nseg, J[ji].accumulate = j.M, j.N, j.ldc, seg0, len(j.segs), int(acc)
        seg0 += len(j.segs)
    for ji, j, si, s in seg_rows(c):
        S[si].A, S[si].B, S[si].K = addr[f"a{si}"], addr[f"b{si}"], s.K
        S[si].a_i, S[si].a_k, _ = op_strides(s.a, j.M, s.K)
        S[si].b_j, S[si].b_k, _ = op_strides(s.b, j.N, s.K)
    st = case_strides(c)
    return J, S, ((ctypes.c_int64 * 6)(*st) if st is not None else None)


# ------------------------------------------------------------------------------------------ the model
def gemm_model(c, t, alpha, bias, accumulate):
    """-> per job a SimpleNamespace(exact, abs_sum [both batch x M x N float64], n).  t: name -> float64 buffer, with
    "c<job>" holding the old contents of C (read where the job accumulates)."""
    st = case_strides(c) or (0,) * 6
    res, si = [], 0
    for ji, j in enumerate(c.jobs):
        use_bias, acc = job_flags(j, bias, accumulate)
        exact = torch.zeros(c.batch + (j.M, j.N), dtype=F64)
        absolute = torch.zeros_like(exact)
        n = 0
        for s in j.segs:
            ar, ak, _ = op_strides(s.a, j.M, s.K)
            br, bk, _ = op_strides(s.b, j.N, s.K)
            A = view(t[f"a{si}"], j.M, s.K, ar, ak, st[0], st[1], c.batch)
            B = view(t[f"b{si}"], j.N, s.K, br, bk, st[2], st[3], c.batch)
            exact += A @ B.transpose(-1, -2)
            absolute += A.abs() @ B.abs().transpose(-1, -2)
            n += s.K
            si += 1
        exact, absolute = exact * alpha, absolute * abs(alpha)
        if use_bias:
            exact = exact + t[f"bias{ji}"]
            absolute = absolute + t[f"bias{ji}"].abs()
        if acc:
            old = c_view(t[f"c{ji}"], j, st, c.batch)
            exact = exact + old
            absolute = absolute + old.abs()
        res.append(SimpleNamespace(exact=exact, abs_sum=absolute, n=n))
    return res


def softmax_model(x, slack=0.0):
    """Rows of x (float64, last dimension) -> (P, bound) from the rounding points in the module docstring.  slack: added to
    every |x_j - m| (a caller whose x is itself off by that much)."""
    x = x.to(F64)
    n = x.shape[-1]
    d = x - x.max(-1, keepdim=True).values
    P = torch.softmax(x, -1)
    t = (d.abs() + slack) * math.log2(math.e)
    E = torch.exp2(t * ((1 + U) ** 3 - 1)) * (1 + 2 * U) - 1          # relative error of e_j
    W = (P * E).sum(-1, keepdim=True)                                  # relative error the e_j leave in the sum
    rel = (1 + E) * (1 + U) ** 2 / ((1 - W) * (1 - bound_gamma(max(n - 1, 0)))) - 1
    return P, P * rel


def softmax_backward_model(P, dP, scale):
    """dS = scale * P * (dP - sum_j dP_j P_j) for a given P (taken as exact input) -> (dS, bound)."""
    P, dP = P.to(F64), dP.to(F64)
    n = P.shape[-1]
    dot = (P * dP).sum(-1, keepdim=True)
    d_dot = bound_gamma(n) * (P * dP).abs().sum(-1, keepdim=True)
    dS = scale * P * (dP - dot)
    bound = abs(scale) * P.abs() * (((dP - dot).abs() + d_dot) * ((1 + U) ** 3 - 1) + d_dot)
    return dS, bound


def colsum_model(x, old=None):
    """out[j] = sum_i x[i, j] (+ old[j]) -> (exact, abs_sum)."""
    x = x.to(F64)
    e, a = x.sum(0), x.abs().sum(0)
    if old is not None:
        e, a = e + old.to(F64), a + old.to(F64).abs()
    return e, a


# compositions (gemm.py): every product as a tuple (exact, abs_sum, n), so a bound can follow it
def product(a, b, alpha=1.0, bias=None, old=None):
    """alpha * a @ b^T (+ bias) (+ old) over the last two dimensions -> (exact, abs_sum, n)."""
    a, b = a.to(F64), b.to(F64)
    e = alpha * (a @ b.transpose(-1, -2))
    s = abs(alpha) * (a.abs() @ b.abs().transpose(-1, -2))
    if bias is not None:
        e, s = e + bias.to(F64), s + bias.to(F64).abs()
    if old is not None:
        e, s = e + old.to(F64), s + old.to(F64).abs()
    return e, s, a.shape[-1]


def product_bound(a, b, da, db, alpha=1.0, bias=None, old=None, d_old=None):
    """Bound of a computed product whose operands carry the absolute errors da, db (float64 tensors or 0):
    the rounding of this product, gamma_(2n+3) * abs_sum on the perturbed magnitudes, plus what the operand errors
    propagate: |alpha| (da |b| + |a| db + da db)."""
    a, b = a.to(F64).abs(), b.to(F64).abs()
    da = torch.zeros_like(a) if isinstance(da, (int, float)) else da
    db = torch.zeros_like(b) if isinstance(db, (int, float)) else db
    bt, dbt = b.transpose(-1, -2), db.transpose(-1, -2)
    prop = abs(alpha) * (da @ bt + a @ dbt + da @ dbt)
    s = abs(alpha) * ((a + da) @ (bt + dbt))
    if bias is not None:
        s = s + bias.to(F64).abs()
    if old is not None:
        s = s + old.to(F64).abs() + (d_old if d_old is not None else 0)
        prop = prop + (d_old if d_old is not None else 0)
    return bound_gamma(2 * a.shape[-1] + 3) * s + prop


def linear_model(x, w, b, dy):
    """nn.Linear forward and backward in float64: y, dx, dw, db with abs sums and reduction lengths."""
    x2, dy2 = x.to(F64).reshape(-1, x.shape[-1]), dy.to(F64).reshape(-1, dy.shape[-1])
    y = product(x2, w, bias=b)
    dx = product(dy2, w.to(F64).t())
    dw = product(dy2.t(), x2.t())
    db = colsum_model(dy2)
    return SimpleNamespace(y=y, dx=dx, dw=dw, db=db, rows=x2.shape[0])


def attention_model(q, k, v, d_o, scale):
    """softmax(scale q k^T) v with its gradients, float64, over [B, H, T, D]."""
    q, k, v, d_o = (t.to(F64) for t in (q, k, v, d_o))
    s = scale * (q @ k.transpose(-1, -2))
    P = torch.softmax(s, -1)
    o = P @ v
    dP = d_o @ v.transpose(-1, -2)
    dS = scale * P * (dP - (dP * P).sum(-1, keepdim=True))
    return SimpleNamespace(s=s, P=P, o=o, dP=dP, dS=dS, dv=P.transpose(-1, -2) @ d_o, dq=dS @ k,
                           dk=dS.transpose(-1, -2) @ q)


def attention_bounds(q, k, v, d_o, scale):
    """Per-element bounds of o, dq, dk, dv of gemm.attention_f32: each product's own rounding (product_bound) plus the
    errors of its operands carried through.  Scores off by d_s move the softmax by at most P * (exp(2 max_row d_s) - 1);
    the softmax kernel's own bound is taken at arguments that much larger.  dS = f(P, dP) is the backward kernel's
    rounding on the perturbed P, dP plus |f(P + d_P, dP + d_dP) - f(P, dP)|, term by term."""
    q, k, v, d_o = (t.to(F64) for t in (q, k, v, d_o))
    m = attention_model(q, k, v, d_o, scale)
    n = m.P.shape[-1]
    c3 = (1 + U) ** 3 - 1
    d_s = product_bound(q, k, 0, 0, alpha=scale).max(-1, keepdim=True).values
    shift = torch.exp(2 * d_s) - 1
    _, b_soft = softmax_model(m.s, slack=2 * d_s)
    d_P = b_soft * (1 + shift) + m.P * shift
    b_o = product_bound(m.P, v.transpose(-1, -2), d_P, 0)
    b_dv = product_bound(m.P.transpose(-1, -2), d_o.transpose(-1, -2), d_P.transpose(-1, -2), 0)
    d_dP = product_bound(d_o, v, 0, 0)
    Pp, dPa = m.P + d_P, m.dP.abs() + d_dP
    d_dot = (d_P * m.dP.abs() + m.P * d_dP + d_P * d_dP).sum(-1, keepdim=True)
    r_dot = bound_gamma(n) * (Pp * dPa).sum(-1, keepdim=True)
    diff = (m.dP - (m.dP * m.P).sum(-1, keepdim=True)).abs()
    rounding = abs(scale) * Pp * ((diff + d_dP + d_dot + r_dot) * c3 + r_dot)
    carried = abs(scale) * (d_P * diff + Pp * (d_dP + d_dot))
    d_dS = rounding + carried
    b_dq = product_bound(m.dS, k.transpose(-1, -2), d_dS, 0)
    b_dk = product_bound(m.dS.transpose(-1, -2), q.transpose(-1, -2), d_dS.transpose(-1, -2), 0)
    return SimpleNamespace(o=b_o, dq=b_dq, dk=b_dk, dv=b_dv)


# ------------------------------------------------------------------------------------------ inputs
def _gen(c, salt):
    return torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id)) * 7 + salt)


def tensor_scale(i, name):
    """The power of two of the i-th buffer of sorted(layout): 2^-1, 1 or 2 for operands, 1 for bias and C."""
    return 2.0 ** ((i * 5 + len(name)) % 3 - 1) if (name[0] in "ab" and not name.startswith("bias")) else 1.0


def inputs(c, kind):
    """name -> float64 buffer for every buffer of layout(c), padding included (what lies between the rows of a view is
    data too: a kernel that reads it gets a wrong answer, not a zero).
    kind "int": integers in [-8, 8] times one power of two per tensor (tensor_scale); integer bias and old C, |.| <= 2^10.
    kind "gauss": fp32-valued standard normals times the same scales; bias and old C normal at 8."""
    g = _gen(c, 1 if kind == "int" else 2)
    t = {}
    for i, (name, (n, _)) in enumerate(sorted(layout(c).items())):
        operand = name[0] in "ab" and not name.startswith("bias")
        if kind == "int":
            lim = 8 if operand else 1024
            t[name] = torch.randint(-lim, lim + 1, (n,), generator=g).to(F64) * tensor_scale(i, name)
        else:
            t[name] = (torch.randn(n, generator=g, dtype=F64) * (tensor_scale(i, name) if operand else 8.0)).float().to(F64)
    return t


def unit_of(c, alpha):
    """The smallest power of two every term of every element of the exact tier is a multiple of: |alpha| * scale(A_s) *
    scale(B_s) over the segments, and 1 for the integer bias and old C."""
    sc = {name: tensor_scale(i, name) for i, name in enumerate(sorted(layout(c)))}
    return min([1.0] + [abs(alpha) * sc[f"a{si}"] * sc[f"b{si}"] for _, _, si, _ in seg_rows(c)])


def impulses(c):
    """[(job, row, segment index within the job, k)]: the first and the last element of the job's reduction and of its
    rows, a chunk boundary, the first k of the last segment - for the last job of the table."""
    ji = len(c.jobs) - 1
    j = c.jobs[ji]
    last = len(j.segs) - 1
    picks = {(ji, 0, 0, 0), (ji, j.M - 1, last, j.segs[last].K - 1), (ji, j.M // 2, 0, min(15, j.segs[0].K - 1)),
             (ji, (j.M - 1) // 2, last, 0), (0, c.jobs[0].M - 1, 0, min(16, c.jobs[0].segs[0].K - 1))}
    return sorted(picks)


def impulse_inputs(c, job, row, seg, k):
    """A of every segment zero but a single 1 at (row, k) of segment `seg` of `job`, in the LAST batch instance;
    B(col, k) = 1 + col * Ktot + (k counted through the job's segments): a distinct integer < 2^24 per (col, k), so
    C[row, :] must be that column of B and every other element 0.  -> buffers, expected C per job (batch x M x N)."""
    st = case_strides(c) or (0,) * 6
    t = {name: torch.zeros(n, dtype=F64) for name, (n, _) in layout(c).items()}
    want = [torch.zeros(c.batch + (j.M, j.N), dtype=F64) for j in c.jobs]
    first = {}
    for ji, j, si, s in seg_rows(c):
        first.setdefault(ji, si)
    for ji, j, si, s in seg_rows(c):
        ktot = sum(x.K for x in j.segs)
        k0 = sum(x.K for x in j.segs[:si - first[ji]])
        br, bk, _ = op_strides(s.b, j.N, s.K)
        B = view(t[f"b{si}"], j.N, s.K, br, bk, st[2], st[3], c.batch)
        vals = 1 + torch.arange(j.N, dtype=F64)[:, None] * ktot + (k0 + torch.arange(s.K, dtype=F64))[None, :]
        assert float(vals.max()) < 2 ** 24
        B[:] = vals
        if ji == job and si - first[ji] == seg:
            ar, ak, _ = op_strides(s.a, j.M, s.K)
            view(t[f"a{si}"], j.M, s.K, ar, ak, st[0], st[1], c.batch)[-1, -1, row, k] = 1.0
            want[ji][-1, -1, row, :] = vals[:, k]
    return t, want


# ------------------------------------------------------------------------------------------ mirror of gemm_plan
WS_BYTES = {"full": lambda need: need, "none": lambda need: 0, "short": lambda need: max(need - 1, 0),
            "null_sized": lambda need: need}
WS_POINTER = {"full": True, "none": False, "short": True, "null_sized": False}


def mirror(c, aligned=None, ws_bytes=None, ws_ok=None):
    """What csrc/salun_gemm.hip's gemm_plan decides for the call, as a dict with the fields of salun_gemm_route_t, or
    None where it refuses.  aligned: name -> bool (base pointer on a 16-byte boundary; default: skew == 0).
    ws_bytes: of the workspace offered (default: by c.ws); ws_ok: its pointer is non-NULL and 4-byte aligned (default:
    by c.ws)."""
    lay = layout(c)
    if aligned is None:
        aligned = {name: skew % 4 == 0 for name, (_, skew) in lay.items()}
    bo, bi = c.batch
    batch = bo * bi
    nsegs = sum(len(j.segs) for j in c.jobs)
    if bo < 1 or bi < 1 or batch > 65535 or not 1 <= len(c.jobs) <= MAXJ or not 1 <= nsegs <= MAXS:
        return None
    for j in c.jobs:
        if j.M < 1 or j.N < 1 or j.ldc < j.N or not j.segs or any(s.K < 1 for s in j.segs):
            return None
    st = case_strides(c) or (0,) * 6
    t128 = sum(-(-j.M // 128) * -(-j.N // 128) for j in c.jobs)
    bt = 128 if t128 * batch >= 512 else 64
    tiles = sum(-(-j.M // bt) * -(-j.N // bt) for j in c.jobs)
    out_elems = sum(j.M * j.N for j in c.jobs)
    nchunks = [sum(-(-s.K // BK) for s in j.segs) for j in c.jobs]
    split, wgs = 1, tiles * batch
    if wgs < 256:
        split = min(512 // wgs, 16)
        while split > 1 and min(nchunks) // split < 4:
            split -= 1
    wanted = split
    need = 4 * wanted * out_elems * batch if wanted > 1 else 0
    if ws_bytes is None:
        ws_bytes = WS_BYTES[c.ws](need)
    if ws_ok is None:
        ws_ok = WS_POINTER[c.ws]
    if split > 1 and (not ws_ok or ws_bytes < need):
        split = 1

    def mode(al, s_o, s_i, s_row, s_k):
        ok = lambda s: al and s_o % 4 == 0 and s_i % 4 == 0 and s % 4 == 0
        return 1 if (s_k == 1 and ok(s_row)) else 2 if (s_row == 1 and ok(s_k)) else 0

    r = dict(tile=bt, nsplit=split, nsplit_wanted=wanted, njobs=len(c.jobs), nsegs=nsegs, tiles=tiles, nchunks=nchunks,
             per=[-(-n // split) for n in nchunks], empty_shares=[], tile0=[], fast_tiles=[], amode=[], bmode=[], chunk0=[],
             ws_need=need)
    tile0 = 0
    for ji, j in enumerate(c.jobs):
        r["tile0"].append(tile0)
        tile0 += -(-j.M // bt) * -(-j.N // bt)
        r["empty_shares"].append(sum(1 for z in range(split) if z * r["per"][ji] >= nchunks[ji]))
    ch, vec, last = 0, {}, None
    for ji, j, si, s in seg_rows(c):
        if ji != last:
            ch, last = 0, ji
        ar, ak, _ = op_strides(s.a, j.M, s.K)
        br, bk, _ = op_strides(s.b, j.N, s.K)
        am = mode(aligned[f"a{si}"], st[0], st[1], ar, ak)
        bm = mode(aligned[f"b{si}"], st[2], st[3], br, bk)
        r["amode"].append(am), r["bmode"].append(bm), r["chunk0"].append(ch)
        ch += -(-s.K // BK)
        vec[ji] = vec.get(ji, True) and am != 0 and bm != 0 and s.K % BK == 0
    r["fast_tiles"] = [(j.M // bt) * (j.N // bt) if vec[ji] else 0 for ji, j in enumerate(c.jobs)]
    return r


def tail_arms(c, r):
    """The partial-float4 arms of stage_load the call enters: {(mode, lanes loaded)} with mode 1 (K tail) or 2 (row tail)
    and 1 <= lanes <= 3 (.x / .x.y / .x.y.z).  A FAST tile never enters stage_load; a ragged dimension always has a
    guarded tile.  The route query has no field for the arms: this is a restatement by hand of what stage_load does with
    the query's modes and the case's M, N and K (mode 1 loads K % 4 lanes of the last float4 of a row, mode 2
    rows % 4 lanes of the last float4 of a column), read off the kernel source."""
    arms = set()
    for ji, j, si, s in seg_rows(c):
        for m, rows in ((r["amode"][si], j.M), (r["bmode"][si], j.N)):
            if m == 1 and s.K % 4:
                arms.add((1, s.K % 4))
            if m == 2 and rows % 4:
                arms.add((2, rows % 4))
    return arms


# ------------------------------------------------------------------------------------------ the cases
def _one(id, M, N, K, a=Op("k"), b=Op("k"), ldc=None, **kw):
    return Case(id, (JobSpec(M, N, ldc or N, (SegSpec(K, a, b),)),), **kw)


def _mode_op(mode, rows, K, how):
    """An operand in load mode `mode`; mode 0 by a skewed base pointer (how = 0) or by a stride-2 view (how = 1)."""
    if mode == 1:
        return Op("k")
    if mode == 2:
        return Op("r")
    return Op("k", None, 1) if how == 0 else Op("s2")


K1 = lambda w: Op("k", w)
R1 = lambda w: Op("r", w)
_B2 = (16020, 8004, 9640, 4808, 1960, 964)                      # six distinct strides, outer != inner * count
_B2U = (16020, 8001, 9641, 4808, 1960, 964)                     # A's inner and B's outer stride off the float4 grid

CASES = [
    _one("one", 1, 1, 1),
    _one("scalar_ragged", 65, 63, 17),
    *[_one(f"m1_tail_{K - 12}", 33, 31, K, K1(16), K1(16)) for K in (13, 14, 15)],
    *[_one(f"m2_tail_{M - 32}", M, M, 20, R1(36), R1(36)) for M in (33, 34, 35)],
    *[_one(f"modes_{am}{bm}", 36, 40, 32, _mode_op(am, 36, 32, bm % 2), _mode_op(bm, 40, 32, 1 - am % 2))
      for am in range(3) for bm in range(3)],
    _one("modes_00_swapped", 36, 40, 32, Op("s2"), Op("k", None, 1)),
    _one("fast_and_edge", 130, 70, 32),
    _one("fast_k_ragged", 128, 128, 40),
    _one("split16", 64, 64, 1024),
    _one("split_empty_1060", 64, 64, 1060),
    _one("split_empty_1057", 64, 64, 1057, K1(1060), K1(1060)),
    _one("split_empty_10", 64, 64, 656),
    Case("split_finish_all", (JobSpec(40, 24, 29, (SegSpec(200, Op("k"), Op("k")),)),)),
    _one("split_no_ws_null", 64, 64, 1024, ws="none"),
    _one("split_no_ws_short", 64, 64, 1024, ws="short"),
    _one("split_no_ws_null_sized", 64, 64, 1024, ws="null_sized"),
    Case("segs_mixed", (JobSpec(33, 31, 31, (SegSpec(16, K1(16), K1(16)), SegSpec(5, Op("k"), Op("k")),
                                             SegSpec(40, R1(36), K1(40)), SegSpec(64, K1(64), R1(32)),
                                             SegSpec(3, Op("k"), R1(32)))),)),
    Case("segs_32x1", (JobSpec(7, 5, 5, tuple(SegSpec(1, Op("k"), Op("k")) for _ in range(32))),)),
    Case("jobs_mixed", (JobSpec(64, 64, 64, (SegSpec(128, Op("k"), Op("k")),), bias=True),
                        JobSpec(3, 200, 200, (SegSpec(64, Op("k"), Op("r", 200)),), accumulate=True),
                        JobSpec(129, 1, 1, (SegSpec(100, Op("k"), Op("k")), SegSpec(28, R1(132), Op("k")))))),
    Case("jobs_split", (JobSpec(33, 31, 35, (SegSpec(256, Op("k"), Op("k")),)),
                        JobSpec(5, 70, 70, (SegSpec(128, Op("k"), R1(72)), SegSpec(5, Op("k"), Op("k")))))),
    Case("jobs_32", tuple(JobSpec(1, 1, 1, (SegSpec(3, Op("k"), Op("k")),)) for _ in range(32))),
    Case("batch_2level", (JobSpec(40, 24, 24, (SegSpec(200, Op("k"), Op("k")),)),), (3, 2), _B2),
    Case("batch_unaligned", (JobSpec(40, 24, 24, (SegSpec(200, Op("k"), Op("k")),)),), (3, 2), _B2U),
    Case("t128_ragged", (JobSpec(130, 129, 129, (SegSpec(18, K1(20), K1(20)),)),), (32, 16)),
    Case("t128_fast", (JobSpec(256, 256, 256, (SegSpec(32, Op("k"), Op("r")),)),), (16, 8)),
    _one("t128_single", 65536, 128, 4),
    Case("t128_jobs", (JobSpec(130, 129, 132, (SegSpec(18, R1(132), K1(20)),)),
                       JobSpec(5, 200, 200, (SegSpec(18, Op("k"), R1(200)),))), (16, 16)),
]
assert len({c.id for c in CASES}) == len(CASES)
BY_ID = {c.id: c for c in CASES}

# ------------------------------------------------------------------------------------------ refusals
# Every call outside the library's domain, as a change to the arguments dict(J, nj, S, ns, bo, bi) of a valid call of the
# case REFUSAL_BASE (2 jobs, 3 segments).
def _setj(i, field, v):
    return lambda a: setattr(a["J"][i], field, v)


def _sets(i, field, v):
    return lambda a: setattr(a["S"][i], field, v)


REFUSAL_BASE = "jobs_split"
REFUSALS = {"njobs_0": lambda a: a.update(nj=0), "njobs_33": lambda a: a.update(nj=33),
            "nsegs_0": lambda a: a.update(ns=0), "nsegs_33": lambda a: a.update(ns=33),
            "ldc_below_N": _setj(0, "ldc", 30), "K_0": _sets(1, "K", 0), "M_0": _setj(1, "M", 0),
            "segs_past_the_table": _setj(1, "nseg", 3), "null_C": _setj(0, "C", None), "null_A": _sets(0, "A", None),
            "null_B": _sets(2, "B", None), "batch_65536": lambda a: a.update(bo=256, bi=256)}

# (M, N, ld) of the column-sum tests and (rows, n) of the softmax tests
COLSUM_SHAPES = [(1, 1, 1), (15, 64, 64), (17, 65, 70), (8197, 3, 8), (300, 130, 130)]
SOFTMAX_N = (1, 3, 63, 64, 65, 77, 256)
SOFTMAX_ROWS = (1, 5, 8197)


def colsum_slabs(M, N):
    s = max(1024 // ((N + 63) // 64), 1)
    s = max(min(s, (M + 15) // 16), 1)
    return min(s, 512)


def colsum_inputs(M, N, ld, kind):
    g = torch.Generator().manual_seed(M * 131 + N * 7 + ld)
    if kind == "int":
        return torch.randint(-8, 9, (M * ld,), generator=g).to(F64) * 0.25, torch.randint(-1024, 1025, (N,), generator=g).to(F64)
    return torch.randn(M * ld, generator=g, dtype=F64).float().to(F64), torch.randn(N, generator=g, dtype=F64).float().to(F64) * 8
