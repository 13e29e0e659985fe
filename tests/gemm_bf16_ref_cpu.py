"""torch-float64 restatement of K16, the bf16 GEMMs of csrc/salun_gemm.hip (k_gemm_bf16_nt, _nt_p, _nt_r, k_gemm_bf16_tn with
k_tn_reduce, k_pack_bf16, k_pack_bf16_t), on the CPU (test infrastructure only, like gemm_ref_cpu.py): the exact answer of
one salun_gemm_bf16_nt / salun_gemm_bf16_tn / salun_pack_bf16 call with the quantity its error bound is a multiple of; the
input makers of the exact, impulse and bound tiers; the case tables NT_CASES / TN_CASES, one row per edge of the kernels;
and `nt_facts` / `tn_facts` (`plan_facts`), a restatement by hand from the kernel source of what the route query has no
field for.  Validated by test_gemm_bf16_ref_cpu.py; used by test_gemm_bf16_exact_gpu.py.

  NT    y[M][N] (bf16) = ((x[M][K] . w[N][K]^T) + bias[N]) + addend[M][N]: the kernels' epilogue order, everything in fp32
        and ONE rounding to bf16, nearest even (pack2)
  TN    dw[Na][Nb] (fp32) = dy[M][Na]^T . x[M][Nb] (+ dw0): split over ranges of whole stages, folded in index order
  pack  fp32 -> bf16 nearest even, [N][K] as it lies or transposed to [K][N]

Inputs, all seeded per case.  A tensor is small integers times ONE power of two (gemm_ref_cpu.tensor_scale's scheme: 2^-1,
1 or 2 per operand), so every term of an element is a whole multiple of the element's unit 2^(ex + ew):
  int      x, w, dy integers of [-8, 8]; bias (fp32) +-[1024, 4096] units, so y lies in the thousands of units and the
           rounding to bf16 (8 significand bits) really happens, a fair share of the sums being ties; addend (bf16)
           an integer of [-255, 255] times 2^(0..3) units: 8 significant bits; dw0 (fp32) integers of [-4096, 4096] units.
           The worst-case sum of magnitudes, epilogue terms included, stays below 2^24 units (`nt_worst_units` /
           `tn_worst_units`; asserted per case by test_gemm_bf16_ref_cpu.py): the fp32 value before the final rounding
           is exact in every order, under every split.
  gauss    normal draws rounded to bf16 (fp32 for bias / dw0) times the same scales.
  impulse  a single 1 in x at (row, k) - TN: in dy at (m, a) -; the other operand holds a DISTINCT bf16 value per
           (column, k): +-(128 + j) 2^e (plain integers run out at 256; 128 significands x 201 exponents x 2 signs)."""
import math
from collections import namedtuple
from types import SimpleNamespace

import torch

from conv_bf16_ref_cpu import U, U16, bound_gamma, is_bf16_tie, to_bf16_rne  # noqa: F401  (the helpers the tests share)

F64 = torch.float64


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------ the forms (from the source)
# variant -> (family, WGM, WGN, NST, BK): the rows of NT_ROWS (salun_bf16_plan.h); a workgroup computes 64 WGM tokens x
# 64 WGN features; the plain family has 2 (double-buffered) or 1 stage, the persistent one 2
NT_FORMS = {1: ("nt", 2, 2, 2, 64), 2: ("nt", 2, 2, 1, 64), 3: ("nt", 4, 1, 2, 64), 4: ("nt", 4, 1, 1, 64),
            5: ("nt_p", 2, 2, 2, 64), 6: ("nt_p", 4, 1, 2, 64), 7: ("nt_r", 2, 2, 4, 64), 8: ("nt_r", 4, 2, 3, 64),
            9: ("nt_r", 4, 1, 3, 64), 10: ("nt_r", 2, 2, 3, 64), 11: ("nt_r", 4, 2, 3, 32), 12: ("nt_r", 2, 2, 4, 32),
            13: ("nt_r", 4, 1, 3, 32)}
# variant -> (WGA, WGB, RST, NST): salun_gemm_bf16_tn's three launches; the tile is 64 WGA x 64 WGB features, a stage
# RST tokens
TN_FORMS = {1: (2, 2, 64, 3), 2: (2, 2, 32, 4), 3: (4, 2, 64, 3)}
TN_TARGET = 256
KEEP, ONE, DRAIN = "later >= NST - 2", "NST == 4 && later == 1", "vmcnt(0)"   # the arms of the ring's wait selection


def nt_label(v):
    fam, wgm, wgn, nst, bk = NT_FORMS[v]
    if fam == "nt":
        return "nt<%d,%d,%s>" % (wgm, wgn, "db" if nst == 2 else "sb")
    return "nt_p<%d,%d>" % (wgm, wgn) if fam == "nt_p" else "nt_r<%d,%d,%d,%d>" % (wgm, wgn, nst, bk)


def nt_choose(M, N):
    """nt_choose (salun_bf16_plan.h): what variant 0 runs"""
    return 13 if N % 128 else (11 if _cdiv(M, 256) * (N // 128) >= 128 else 10)


def _ring_walk(nk, nst):
    """The loop both rings share (k_gemm_bf16_nt_r, k_gemm_bf16_tn) over nk stages: the class of nk against NST and the arms
    of the wait selection it enters."""
    cls = "< NST-1" if nk < nst - 1 else "= NST-1" if nk == nst - 1 else "= NST" if nk == nst else "> NST"
    arms = set()
    for f in range(nk):
        later = nk - 1 - f
        arms.add(KEEP if later >= nst - 2 else ONE if (nst == 4 and later == 1) else DRAIN)
    return cls, arms


def ring_classes_reachable(nst, bk):
    """The classes of nk = K / BK against NST a call can reach at all: K is a multiple of 64, so the 32-deep forms only see
    even nk >= 2 (never nk < NST - 1 = 2, never nk = 3)."""
    return {_ring_walk(K // bk, nst)[0] for K in range(64, 64 * 12, 64)}


def nt_facts(c):
    """What a salun_gemm_bf16_nt call of the case does that the route query has no field for, read off the kernels."""
    v = c.variant or nt_choose(c.M, c.N)
    fam, wgm, wgn, nst, bk = NT_FORMS[v]
    bm, bn = 64 * wgm, 64 * wgn
    tiles_m, tiles_n = _cdiv(c.M, bm), c.N // bn
    ntile = tiles_m * tiles_n
    f = SimpleNamespace(variant=v, family=fam, nst=nst, bk=bk, bm=bm, bn=bn, tiles=ntile, nk=c.K // bk,
                        tile_class="ntile < 8" if ntile < 8 else "ntile = 8q" if ntile % 8 == 0 else "ntile = 8q + r",
                        rows_past_m=c.M % bm != 0,          # the DMA of rows past M re-reads row M - 1
                        mfma_tile_partial=c.M % 32 != 0,    # the last 32-token MFMA tile is partly stored
                        nk_class=None, arms=set(), ep=None, ep2_second_pass_partial=False,
                        tiles_per_wg=0, early_return=False, one_tile_wg=False, crosses_tile=False)
    if fam == "nt_r":
        f.nk_class, f.arms = _ring_walk(f.nk, nst)
        # EP: passes of the epilogue staging; a wave's 64 tokens x 64 features in fp32 rows of EROW = 272 bytes must fit the ring
        f.ep = 1 if wgm * wgn * 64 * 272 <= nst * (bm + bn) * bk * 2 else 2
        # pass 1 holds tokens 32..63 of a wave's 64: partly stored where M ends inside them.  The flag describes the wave that
        # holds row M - 1; the other waves of the last tile are wholly stored or wholly past M
        f.ep2_second_pass_partial = f.ep == 2 and c.M % 64 > 32
    if fam == "nt_p":
        per_xcd = _cdiv(ntile, 8)
        runs = min(64, per_xcd)
        f.tiles_per_wg = _cdiv(per_xcd, runs)
        runs = _cdiv(per_xcd, f.tiles_per_wg)
        q, r = ntile // 8, ntile % 8
        mine = [min(f.tiles_per_wg, (q + 1 if wg % 8 < r else q) - (wg // 8) * f.tiles_per_wg) for wg in range(8 * runs)]
        f.early_return = any(m <= 0 for m in mine)
        f.one_tile_wg = f.tiles_per_wg >= 2 and any(m == 1 for m in mine)
        f.crosses_tile = any(m >= 2 for m in mine)           # the flattened (tile, k-step) pipeline passes a tile boundary
        f.empty_xcds = sorted({wg % 8 for wg, m in enumerate(mine) if m <= 0})
    return f


def tn_facts(c):
    """The same for a salun_gemm_bf16_tn call: tn_plan's split and what k_gemm_bf16_tn's workgroups see of it."""
    v = c.variant or 2
    wga, wgb, rst, nst = TN_FORMS[v]
    ta, tb = 64 * wga, 64 * wgb
    tiles = _cdiv(c.Na, ta) * _cdiv(c.Nb, tb)
    stages = _cdiv(c.M, rst)
    s = max(1, min(_cdiv(TN_TARGET, tiles), stages // (256 // rst), 64))
    per = _cdiv(stages, s)
    splits = _cdiv(stages, per)
    nks = [min(stages, (z + 1) * per) - z * per for z in range(splits)]
    walks = [_ring_walk(nk, nst) for nk in nks]
    work = tiles * splits
    return SimpleNamespace(variant=v, rst=rst, nst=nst, tiles=tiles, stages=stages, splits=splits, per_split=per,
                           stages_per_split=nks, label="tn<v%d>/S%d" % (v, splits),
                           nk_classes={w[0] for w in walks}, arms=set().union(*[w[1] for w in walks]),
                           last_split_shorter=splits > 1 and nks[-1] < per,
                           last_stage_partial=c.M % rst != 0,              # tokens past M read the zero word
                           zero_blocks=_cdiv(c.Na, ta) * ta > c.Na or _cdiv(c.Nb, tb) * tb > c.Nb,  # feature blocks past Na / Nb
                           work=work, work_class="work < 8" if work < 8 else "work = 8q" if work % 8 == 0 else "work = 8q + r",
                           ws_bytes=splits * c.Na * c.Nb * 4 if splits > 1 else 0)


def plan_facts(c):
    return nt_facts(c) if isinstance(c, Nt) else tn_facts(c)


# ------------------------------------------------------------------------------------------ the cases
class Nt(namedtuple("Nt", "M N K variant label why big", defaults=(False,))):
    __slots__ = ()

    @property
    def id(self):
        return "%dx%dx%d-v%d" % (self.M, self.N, self.K, self.variant)


class Tn(namedtuple("Tn", "M Na Nb variant label splits why")):
    __slots__ = ()

    @property
    def id(self):
        return "%dx%dx%d-v%d" % (self.M, self.Na, self.Nb, self.variant)


K_STEPS = (64, 128, 192, 256, 320)


def _nt_cases():
    rows = []
    for v in range(1, 14):
        _, wgm, wgn, nst, bk = NT_FORMS[v]
        bm, bn = 64 * wgm, 64 * wgn
        # M: one token; one past an MFMA tile; one short of and one past the block tile; the context length of the text encoder
        ms = (1, 33, bm - 1, bm + 1, 77)
        for i, K in enumerate(K_STEPS):                       # one feature tile (N = 64 / 128), 1 .. 5 (2 .. 10) k-steps
            M = ms[(i + v) % 5]
            rows.append(Nt(M, bn, K, v, nt_label(v), "%d k-steps of %d, M = %d" % (K // bk, bk, M)))
        rows.append(Nt(8 * bm - 3, bn, 128, v, nt_label(v), "8 tiles (ntile = 8q), ragged last token tile"))
        rows.append(Nt(2 * bm + 1, 3 * bn, 192, v, nt_label(v), "3 x 3 tiles (ntile = 8q + 1), N = %d" % (3 * bn)))
    rows += [Nt(77, 64, 128, 0, nt_label(13), "variant 0, N % 128 != 0: nt_choose = 13"),
             Nt(77, 128, 128, 0, nt_label(10), "variant 0, one tile: nt_choose = 10"),
             Nt(33, 16384, 64, 0, nt_label(11), "variant 0, 128 tiles of 256 x 128: nt_choose = 11"),
             Nt(128 * 513 - 5, 128, 128, 5, nt_label(5), "persistent, 513 tiles: tiles_per_wg = 2", True),
             Nt(256 * 513 - 5, 64, 64, 6, nt_label(6), "persistent, 513 tiles: tiles_per_wg = 2", True)]
    return rows


_FEATS = ((32, 32), (96, 160), (160, 96), (288, 32), (32, 288), (288, 288))


def _tn_row(M, Na, Nb, v, why):
    f = tn_facts(SimpleNamespace(M=M, Na=Na, Nb=Nb, variant=v))
    return Tn(M, Na, Nb, v, f.label, f.splits, why)


def _tn_cases():
    rows = []
    for v in (1, 2, 3):
        _, _, rst, nst = TN_FORMS[v]
        # 1 stage (one token; one short of a stage), 2 stages, NST - 1 and NST stages in ONE split; 513: two splits, the
        # second shorter, the last stage one token
        ms = list(dict.fromkeys([1, rst - 1, rst + 1, rst * (nst - 2) + 1, rst * (nst - 1) + 1, 513]))
        for i, M in enumerate(ms):
            Na, Nb = _FEATS[(i + v) % 6]
            rows.append(_tn_row(M, Na, Nb, v, "%d stages of %d tokens" % (_cdiv(M, rst), rst)))
        rows.append(_tn_row(513, 288, 288, v, "3 x 3 (2 x 3) tiles, two splits: a total that is no multiple of 8"))
        rows.append(_tn_row(513, 160, 96, v, "two splits, few enough elements for the impulse codes"))
        rows.append(_tn_row(2053, 96, 160, v,"several splits, the last one shorter, ragged last stage"))
        rows.append(_tn_row(16384, 32, 32, v, "the 64-split cap"))
    rows += [_tn_row(513, 96, 160, 0, "variant 0 = 2"), _tn_row(2053, 32, 288, 0, "variant 0 = 2, split")]
    return list({r[:4]: r for r in reversed(rows)}.values())[::-1]       # a shape the rotation names twice: once


NT_CASES = _nt_cases()
TN_CASES = _tn_cases()
assert len({c.id for c in NT_CASES}) == len(NT_CASES) and len({c.id for c in TN_CASES}) == len(TN_CASES)
NT_SMALL = [c for c in NT_CASES if not c.big]          # the bound tier and the full epilogue table leave the two large ones out
NT_EPILOGUES = ((), ("bias",), ("bias", "addend"))
BIG_EPILOGUE = ("bias", "addend")                       # the one combination the two 513-tile cases run

# shapes on which every variant that accepts them must give the same bits (N = 64: the 64-feature forms only)
AGREE = [(77, 128, 320), (257, 384, 256), (129, 64, 192), (1, 128, 64)]


# ------------------------------------------------------------------------------------------ the model
def nt_model(x, w, bias=None, addend=None, absolute=False):
    """((x . w^T) + bias) + addend in float64, summed k-step by k-step (64 columns at a time) as the kernels walk the
    reduction; absolute=True: the same over absolute values."""
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    x, w = f(x.to(F64)), f(w.to(F64))
    y = torch.zeros((x.shape[0], w.shape[0]), dtype=F64)
    for k0 in range(0, x.shape[1], 64):
        y += torch.einsum("mk,nk->mn", x[:, k0:k0 + 64], w[:, k0:k0 + 64])
    if bias is not None:
        y = y + f(bias.to(F64))
    if addend is not None:
        y = y + f(addend.to(F64))
    return y


def tn_model(dy, x, dw0=None, absolute=False):
    """dy^T . x (+ dw0) in float64"""
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    dw = torch.einsum("ma,mb->ab", f(dy.to(F64)), f(x.to(F64)))
    return dw if dw0 is None else dw + f(dw0.to(F64))


def pack_model(w, transposed=False):
    """fp32 [N][K] -> the bf16 image (as float64 values), plain or transposed to [K][N]; zeros keep their sign"""
    w = w.to(F64)
    out = torch.where(w == 0, w, to_bf16_rne(w))
    return out.t().contiguous() if transposed else out


# ------------------------------------------------------------------------------------------ inputs
A_INT, BIAS_LO, BIAS_HI, ADD_INT, ADD_SHIFT, DW0_INT = 8, 1024, 4096, 255, 3, 4096


def _gen(c, salt):
    return torch.Generator().manual_seed(((c[0] * 131 + c[1]) * 137 + c[2]) * 17 + c.variant * 3 + salt)


def scales(c):
    """(exponent of the first operand, of the second): one power of two per tensor, 2^-1 .. 2^1 by the shape"""
    return (c[0] + c[2]) % 3 - 1, (c[1] + c[2] // 32) % 3 - 1


def unit_of(c):
    ex, ew = scales(c)
    return 2.0 ** (ex + ew)


def nt_worst_units(c, terms=("bias", "addend")):
    """The largest sum of magnitudes an element of the integer tier can reach, in units"""
    return c.K * A_INT * A_INT + (BIAS_HI if "bias" in terms else 0) + (ADD_INT * 2 ** ADD_SHIFT if "addend" in terms else 0)


def tn_worst_units(c, accumulate=True):
    return c.M * A_INT * A_INT + (DW0_INT if accumulate else 0)


def _ints(shape, lim, g):
    return torch.randint(-lim, lim + 1, tuple(shape), generator=g).to(F64)


def _bf16(t):
    return t.float().bfloat16().to(F64)


def nt_inputs(c, kind):
    """-> x [M][K], w [N][K], bias [N], addend [M][N] (float64 values the kernels' formats hold exactly) and `unit`"""
    g = _gen(c, 1 if kind == "int" else 2)
    ex, ew = scales(c)
    sx, sw, unit = 2.0 ** ex, 2.0 ** ew, unit_of(c)
    if kind == "int":
        x, w = _ints((c.M, c.K), A_INT, g) * sx, _ints((c.N, c.K), A_INT, g) * sw
        mag = torch.randint(BIAS_LO, BIAS_HI + 1, (c.N,), generator=g).to(F64)
        bias = mag * (torch.randint(0, 2, (c.N,), generator=g).to(F64) * 2 - 1) * unit
        addend = _ints((c.M, c.N), ADD_INT, g) * 2.0 ** torch.randint(0, ADD_SHIFT + 1, (c.M, c.N), generator=g).to(F64) * unit
    else:
        x = _bf16(torch.randn((c.M, c.K), generator=g)) * sx
        w = _bf16(torch.randn((c.N, c.K), generator=g)) * sw
        bias = torch.randn((c.N,), generator=g).to(F64) * unit
        addend = _bf16(torch.randn((c.M, c.N), generator=g)) * unit
    return SimpleNamespace(x=x, w=w, bias=bias, addend=addend, unit=unit)


def tn_inputs(c, kind):
    """-> dy [M][Na], x [M][Nb], dw0 [Na][Nb] and `unit`"""
    g = _gen(c, 3 if kind == "int" else 4)
    ex, ew = scales(c)
    sy, sx, unit = 2.0 ** ex, 2.0 ** ew, unit_of(c)
    if kind == "int":
        dy, x = _ints((c.M, c.Na), A_INT, g) * sy, _ints((c.M, c.Nb), A_INT, g) * sx
        dw0 = _ints((c.Na, c.Nb), DW0_INT, g) * unit
    else:
        dy = _bf16(torch.randn((c.M, c.Na), generator=g)) * sy
        x = _bf16(torch.randn((c.M, c.Nb), generator=g)) * sx
        dw0 = torch.randn((c.Na, c.Nb), generator=g).to(F64) * unit
    return SimpleNamespace(dy=dy, x=x, dw0=dw0, unit=unit)


def pick(t, terms):
    """(bias, addend) of the epilogue combination `terms`"""
    return (t.bias if "bias" in terms else None), (t.addend if "addend" in terms else None)


# ------------------------------------------------------------------------------------------ impulses
CODE_EXP = range(-100, 101)
MAX_CODES = 2 * 128 * len(CODE_EXP)


def codes(rows, cols):
    """[rows][cols] distinct bf16 values +-(128 + j) 2^e, all normal numbers"""
    n = rows * cols
    assert n <= MAX_CODES, "more elements than distinct codes"
    i = torch.arange(n, dtype=torch.int64)
    j, rest = i % 128, i // 128
    sign, e = 1 - 2 * (rest % 2), rest // 2 + CODE_EXP[0]
    v = torch.ldexp((128 + j).to(F64) * sign.to(F64), e)
    return v.view(rows, cols)


def nt_impulse_points(c):
    """[(row, k)]: first and last row, first and last k, a k on each side of a stage boundary, and the last token of a
    ragged M (the last row, where M is no multiple of the tile)"""
    bk = NT_FORMS[c.variant or nt_choose(c.M, c.N)][4]
    side = min(bk, c.K - 1)
    return sorted({(0, 0), (c.M - 1, c.K - 1), (0, c.K - 1), (c.M - 1, 0), (c.M // 2, side - 1), ((c.M - 1) // 2, side)})


def nt_impulse(c, row, k):
    """-> x (a single 1 at (row, k)), w (codes), the product: w[:, k] in row `row`, 0 elsewhere"""
    x = torch.zeros((c.M, c.K), dtype=F64)
    x[row, k] = 1.0
    w = codes(c.N, c.K)
    want = torch.zeros((c.M, c.N), dtype=F64)
    want[row] = w[:, k]
    return x, w, want


def tn_impulse_points(c):
    rst = TN_FORMS[c.variant or 2][2]
    side = min(rst, c.M - 1)
    return sorted({(0, 0), (c.M - 1, c.Na - 1), (0, c.Na - 1), (c.M - 1, 0), (max(side - 1, 0), c.Na // 2), (side, c.Na // 2)})


def tn_impulse(c, m, a):
    """-> dy (a single 1 at (m, a)), x (codes per (token, feature)), dw: x[m] in row a, 0 elsewhere"""
    dy = torch.zeros((c.M, c.Na), dtype=F64)
    dy[m, a] = 1.0
    x = codes(c.M, c.Nb)
    want = torch.zeros((c.Na, c.Nb), dtype=F64)
    want[a] = x[m]
    return dy, x, want


NT_IMPULSE = [c for c in NT_SMALL if c.N * c.K <= MAX_CODES and c.variant and c.K in (128, 320) and c.M < 1000]
TN_IMPULSE = [c for c in TN_CASES if c.M * c.Nb <= MAX_CODES and c.M in (65, 97, 129, 513)]

# ------------------------------------------------------------------------------------------ refusals
# (M, N, K, variant) outside salun_gemm_bf16_nt's domain; (M, Na, Nb, variant) outside salun_gemm_bf16_tn's
NT_REFUSED = [(77, 96, 64, 0), (77, 64, 96, 0), (77, 128, 40, 0), (77, 32, 64, 13), (77, 192, 64, 1), (77, 64, 64, 8),
              (77, 192, 128, 10), (77, 128, 64, 14), (77, 128, 64, -1), (0, 128, 64, 0)]
TN_REFUSED = [(513, 48, 32, 0), (513, 32, 48, 1), (513, 32, 32, 4), (513, 32, 32, -1), (0, 32, 32, 0), (513, 16, 32, 2)]
TN_SHORT_WS = (513, 96, 160, 2)          # two splits: needs a workspace

# salun_pack_bf16: (N, K) of the plain form (N K % 4 = 0, 1, 2, 3: the scalar tail arm) and of the transposed one
PACK_PLAIN = [(4, 8), (3, 7), (5, 6), (9, 7), (37, 53), (1, 1), (64, 320)]
PACK_T = [(37, 53), (32, 32), (1, 1), (33, 64), (64, 320)]


def pack_specials():
    """fp32 values whose rounding the pack kernels must get right, with the bf16 answer: exact halves between two bf16
    numbers of both parities (ties to even), +-0, the largest finite bf16, a value that rounds up into the next binade."""
    v, want = [], []
    for base in (1.0, 1.0 + 2.0 ** -7, 1.5, 255.0, -3.0, 2.0 ** -20 * 1.25, -(2.0 ** 40) * (1 + 3 * 2.0 ** -7)):
        ulp = 2.0 ** (math.frexp(base)[1] - 8)            # base = m 2^e with 0.5 <= |m| < 1: 8 significand bits
        lo, hi = base, base + (ulp if base > 0 else -ulp)
        m_lo = round(abs(lo) / ulp)
        v.append((lo + hi) / 2)
        want.append(lo if m_lo % 2 == 0 else hi)          # the even significand of the two
        v += [lo, lo + (hi - lo) * 0.25, lo + (hi - lo) * 0.75]
        want += [lo, lo, hi]
    big = (2.0 - 2.0 ** -7) * 2.0 ** 127                  # the largest finite bf16 number
    v += [0.0, -0.0, big, -big, 2.0 - 2.0 ** -9, -(4.0 - 2.0 ** -8), 2.0 - 2.0 ** -8]
    want += [0.0, -0.0, big, -big, 2.0, -4.0, 2.0]      # the last: a tie that rounds (to even) into the next binade
    return torch.tensor(v, dtype=F64), torch.tensor(want, dtype=F64)


def pack_inputs(N, K, seed):
    """fp32 values: the specials first (as many as fit), then normal draws"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N * K, generator=g, dtype=torch.float32).to(F64)
    sv, _ = pack_specials()
    n = min(len(sv), N * K)
    w[:n] = sv[:n]
    return w.view(N, K)
