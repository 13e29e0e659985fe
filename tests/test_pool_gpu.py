"""K24 (csrc/salun_pool.hip) through the C-ABI inside the guarded arena (guarded_arena.py): MaxPool2d(2, 2) forward and
backward bit for bit against `F.max_pool2d(..., return_indices=True)` and its autograd on the CPU, on both routes,
for the value families where the selection rule matters (ties, signed zeros, -inf, NaN); nothing outside y, idx and
dx changes, no element of them stays unwritten, and every refused call leaves the arena as it was."""
import functools
import itertools
from ctypes import c_int64, c_void_p

import pytest
import torch
import torch.nn.functional as F

from guarded_arena import SENTINEL, Arena

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 2), (6, 4, 4), (15, 2, 8), (2, 6, 10), (3, 8, 2), (64, 32, 32)]
# the launches cap their grid at 2048 workgroups of 256 threads; the vector route takes two items (four outputs) per
# thread and trip, the scalar route one output: 2100 * 32 * 16 = 1,075,200 items > 2 * 2048 * 256, so threads of both
# routes go round their loop more than once
BIG = (2100, 64, 64)
KINDS = ("random", "equal", "zeros", "neginf", "nan1", "nan2")
NAN, NINF = float("nan"), float("-inf")


def _lib():
    from unlearn_saliency_amd import _lib
    return _lib.lib()


def _patterns(kind):
    """Rows of four window values (top-left, top-right, bottom-left, bottom-right)."""
    if kind == "equal":
        return [[1.5] * 4, [-2.0] * 4]
    if kind == "zeros":                                   # +0 / -0 in every order
        return [list(s) for s in itertools.product((0.0, -0.0), repeat=4)]
    if kind == "neginf":
        return [[NINF] * 4, [NINF, NINF, NINF, -3.0], [-3.0, NINF, NINF, NINF]]
    if kind == "nan1":                                    # one NaN at each position, also beside a larger value
        rows = []
        for k in range(4):
            for big in (1.0, 1e30):
                r = [big * (j + 1) for j in range(4)]
                r[k] = NAN
                rows.append(r)
        return rows
    if kind == "nan2":                                    # two NaNs: the later one is selected
        rows = []
        for a, b in itertools.combinations(range(4), 2):
            r = [float(j) for j in range(4)]
            r[a] = r[b] = NAN
            rows.append(r)
        return rows + [[NAN] * 4]
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """-> x, y, pos (uint8), dy, dx of the library on the CPU (torch tensors; treated as read-only)."""
    NC, H, W = shape
    g = torch.Generator().manual_seed(1000 * NC + 10 * H + W)
    x = torch.randn(NC, H, W, generator=g)
    if kind != "random":
        nwin = NC * (H // 2) * (W // 2)
        pat = torch.tensor(_patterns(kind), dtype=torch.float32)
        win = pat[torch.arange(nwin) % pat.shape[0]]
        x = win.view(NC, H // 2, W // 2, 2, 2).permute(0, 1, 3, 2, 4).reshape(NC, H, W).contiguous()
    xr = x.clone().view(1, NC, H, W).requires_grad_()
    y, ind = F.max_pool2d(xr, 2, 2, return_indices=True)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    pos = (((ind // W) % 2) * 2 + (ind % W) % 2).to(torch.uint8)
    return x, y.detach().view(NC, H // 2, W // 2), pos.view(NC, H // 2, W // 2), dy.view(NC, H // 2, W // 2), \
        xr.grad.view(NC, H, W)


def _words(b):
    """uint8 tensor -> int32 words (little endian), padded with sentinel bytes."""
    n = b.numel()
    buf = torch.full(((n + 3) // 4,), SENTINEL, dtype=torch.int32)
    buf.view(torch.uint8)[:n] = b.reshape(-1)
    return buf


def _bits(t):
    return t.contiguous().view(torch.int32)


def run_forward(shape, x, skew=(0, 0, 0)):
    NC, H, W = shape
    nout = NC * (H // 2) * (W // 2)
    a = Arena().put("x", x, skew=skew[0]).put("y", shape=(nout,), out=True, skew=skew[1])
    a.put("idx", shape=((nout + 3) // 4,), out=True, skew=skew[2]).upload()
    code = _lib().salun_maxpool2x2_forward(a.ptr("x"), a.ptr("y"), a.ptr("idx"), c_int64(NC), H, W, c_void_p(None))
    after = a.download()                                   # guards and x intact
    y = a.part(after, "y")
    idx_words = _bits(a.part(after, "idx"))
    return code, y, idx_words.view(torch.uint8), nout


def run_backward(shape, dy, pos, skew=(0, 0, 0)):
    NC, H, W = shape
    a = Arena().put("dy", dy, skew=skew[0]).put("idx", _words(pos), skew=skew[2])
    a.put("dx", shape=(NC * H * W,), out=True, skew=skew[1]).upload()
    code = _lib().salun_maxpool2x2_backward(a.ptr("dy"), a.ptr("idx"), a.ptr("dx"), c_int64(NC), H, W, c_void_p(None))
    return code, a.result("dx")


def check(shape, kind, skew=(0, 0, 0)):
    x, y, pos, dy, dx = case(shape, kind)
    code, gy, gidx, nout = run_forward(shape, x, skew)
    assert code == 0
    assert torch.equal(_bits(gy), _bits(y.reshape(-1))), "y differs"         # bit for bit: NaN payloads, signed zeros
    assert torch.equal(gidx[:nout], pos.reshape(-1)), "idx differs"          # (so every byte is 0..3: none unwritten)
    tail = torch.tensor([SENTINEL], dtype=torch.int32).view(torch.uint8)[nout % 4:] if nout % 4 else gidx[:0]
    assert torch.equal(gidx[nout:], tail), "bytes behind idx were written"
    code, gdx = run_backward(shape, dy, pos, skew)
    assert code == 0
    assert torch.equal(_bits(gdx), _bits(dx.reshape(-1))), "dx differs"      # +0.0 at the unselected positions


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_and_backward_equal_the_library_bit_for_bit(shape, kind):
    check(shape, kind)


@pytest.mark.parametrize("skew", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (3, 2, 1)])
@pytest.mark.parametrize("shape", [(6, 4, 4), (15, 2, 8), (64, 32, 32)])
def test_bases_off_the_16_byte_grid_take_the_scalar_route_and_stay_exact(shape, skew):
    """x / dy, y / dx or idx 4 (8, 12) bytes off the grid: widths that would take the vector route."""
    check(shape, "random", skew)
    check(shape, "nan1", skew)


@pytest.mark.parametrize("skew", [(0, 0, 0), (1, 1, 1)])
def test_grid_stride_loops_run_more_than_once(skew):
    check(BIG, "random", skew)


def test_two_runs_are_bit_identical():
    x, _, pos, dy, _ = case((64, 32, 32), "random")
    runs = []
    for _ in range(2):
        _, y, idx, _ = run_forward((64, 32, 32), x)
        runs.append((_bits(y), idx, _bits(run_backward((64, 32, 32), dy, pos)[1])))
    assert all(torch.equal(u, v) for u, v in zip(*runs))


def test_refused_calls_return_einval_and_write_nothing():
    from unlearn_saliency_amd import _lib
    L, EINVAL = _lib.lib(), _lib.SALUN_EINVAL
    x, _, pos, dy, _ = case((6, 4, 4), "random")
    a = Arena().put("x", x).put("dy", dy).put("idx_in", _words(pos))
    a.put("y", shape=(6 * 2 * 2,), out=True).put("idx", shape=(6,), out=True).put("dx", shape=(6 * 4 * 4,), out=True)
    a.put("dyx", dy, out=True)                                               # an in-place candidate for dx == dy
    a.upload()
    P, NULL = a.ptr, c_void_p(None)
    fwd = lambda NC=6, H=4, W=4: L.salun_maxpool2x2_forward(P("x"), P("y"), P("idx"), c_int64(NC), H, W, NULL)
    bwd = lambda NC=6, H=4, W=4: L.salun_maxpool2x2_backward(P("dy"), P("idx_in"), P("dx"), c_int64(NC), H, W, NULL)
    codes = [fwd(H=3), fwd(W=3), fwd(H=0), fwd(W=0), fwd(NC=0), fwd(NC=-1), fwd(H=-2),
             L.salun_maxpool2x2_forward(NULL, P("y"), P("idx"), c_int64(6), 4, 4, NULL),
             L.salun_maxpool2x2_forward(P("x"), NULL, P("idx"), c_int64(6), 4, 4, NULL),
             L.salun_maxpool2x2_forward(P("x"), P("y"), NULL, c_int64(6), 4, 4, NULL),
             bwd(H=3), bwd(W=3), bwd(H=0), bwd(NC=0),
             L.salun_maxpool2x2_backward(NULL, P("idx_in"), P("dx"), c_int64(6), 4, 4, NULL),
             L.salun_maxpool2x2_backward(P("dy"), NULL, P("dx"), c_int64(6), 4, 4, NULL),
             L.salun_maxpool2x2_backward(P("dy"), P("idx_in"), NULL, c_int64(6), 4, 4, NULL),
             L.salun_maxpool2x2_backward(P("dyx"), P("idx_in"), P("dyx"), c_int64(6), 2, 2, NULL)]
    assert codes == [EINVAL] * len(codes), codes
    after = a.download()                                                     # guards and inputs intact ...
    for n in ("y", "idx", "dx"):                                             # ... and no output was touched
        s, k = a.parts[n][0], a.parts[n][1]
        assert (after[s:s + k] == SENTINEL).all(), n
    assert torch.equal(a.part(after, "dyx").view(torch.int32).reshape(-1), _bits(dy.reshape(-1)))
    assert fwd() == 0 and bwd() == 0                                         # the same arena, accepted as it should be
    torch.cuda.synchronize()


def test_autograd_node_saves_the_byte_map_only_and_counts_library_calls():
    """`pool.maxpool2x2`: output and input gradient equal the library's bit for bit, the node keeps idx (uint8) and no
    float tensor, and inputs outside K24's domain go to the library, counted."""
    from unlearn_saliency_amd import pool
    x, y, _, dy, dx = case((64, 32, 32), "random")
    xd = x.view(4, 16, 32, 32).cuda().requires_grad_()
    pool.reset_library_pool_calls()
    out = pool.maxpool2x2(xd)
    saved = out.grad_fn.saved_tensors
    assert [t.dtype for t in saved] == [torch.uint8] and saved[0].shape == out.shape
    out.backward(dy.view(4, 16, 16, 16).cuda())
    assert torch.equal(_bits(out.detach().cpu().reshape(-1)), _bits(y.reshape(-1)))
    assert torch.equal(_bits(xd.grad.cpu().reshape(-1)), _bits(dx.reshape(-1)))
    assert pool.library_pool_calls() == 0
    odd = torch.rand(2, 3, 5, 6, device="cuda")
    assert torch.equal(pool.maxpool2x2(odd), F.max_pool2d(odd, 2, 2))
    assert pool.LIBRARY_POOL_CALLS["shape"] == 1
    half = torch.rand(2, 3, 4, 4, device="cuda", dtype=torch.float16)
    cpu = torch.rand(2, 3, 4, 4)
    assert torch.equal(pool.maxpool2x2(half), F.max_pool2d(half, 2, 2))
    assert torch.equal(pool.maxpool2x2(cpu), F.max_pool2d(cpu, 2, 2))
    with torch.autocast("cuda", dtype=torch.float16):
        pool.maxpool2x2(torch.rand(2, 3, 4, 4, device="cuda"))
    assert pool.LIBRARY_POOL_CALLS["dtype_or_autocast"] == 3 and pool.library_pool_calls() == 4
    pool.reset_library_pool_calls()
