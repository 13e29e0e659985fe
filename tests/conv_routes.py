"""Which kernel the fp32 convolution family picks for a shape: a pure-Python mirror of the host-side plans of
csrc/salun_conv.hip (make_geom, pick_tile / pick_tile_s2, plan_data with igemm_split, plan_dgrad_s2, plan_wgrad with
salun_ring_wgrad_fits) and of ring_launch's domain in csrc/salun_conv_ring.hip.  It exists so that test_conv_ref_cpu.py
can show that conv_ref_cpu.CASES reaches every variant, and so that test_conv_exact_gpu.py knows which calls the library
must refuse; test_conv_ref_cpu.py holds it, label for label, to salun_conv2d_route, which prints the plan the library
launches from, and to the library's workspace queries.  A route is a label; None means SALUN_EINVAL.
Shapes are conv_ref_cpu.Case: (N, C, H, W, K, R, stride, pad) with P, Q."""
from collections import namedtuple

Geom = namedtuple("Geom", "NI TP IH IW nt psz")
RING_TILES = {1: (256, 64, 2), 2: (128, 64, 2), 3: (64, 64, 2), 4: (128, 128, 4), 5: (64, 128, 4)}  # TPIX, KB, WK*KT


def _cdiv(a, b):
    return -(-a // b)


def geom(N, P, Q, pixt, cs, RH, RW=None):
    """make_geom: tiles of `pixt` output pixels; None outside the domain."""
    if Q <= 0 or Q & (Q - 1) or Q > pixt:
        return None
    PQ = P * Q
    if PQ >= pixt:
        if PQ % pixt:
            return None
        NI, TP, nt = 1, pixt // Q, N * (PQ // pixt)
    else:
        if pixt % PQ:
            return None
        NI, TP, nt = pixt // PQ, P, _cdiv(N, pixt // PQ)
    IH, IW = (TP - 1) * cs + RH, (Q - 1) * cs + (RH if RW is None else RW)
    return Geom(NI, TP, IH, IW, nt, NI * IH * IW) if NI * IH * IW <= 768 else None


def _pick(N, P, Q, blocks, need, cs, RH, RW=None):
    g, pixt = geom(N, P, Q, 128, cs, RH, RW), 128
    if g is None or g.nt * blocks < need:
        g64 = geom(N, P, Q, 64, cs, RH, RW)
        if g64:
            g, pixt = g64, 64
    return g, pixt


def _tile(g, pixt, yC):
    """-> name, channels per workgroup, whether the variant can split its reduction"""
    if pixt == 128:
        kt = 4 if yC > 64 else 2 if yC > 32 else 1
        return f"128/KT{kt}", 32 * kt, False
    if yC > 64 and g.nt * _cdiv(yC, 128) >= 384:
        return "64/KT2WK2", 128, False
    return "64/KT1WK2", 64, True


def igemm_split(wgs, xC, chunk, out_elems, HW):
    if wgs > 256 or HW % 4 or out_elems % 4:
        return 1
    S = min(8, 512 // max(wgs, 1))
    while S > 1 and (xC % (S * chunk) or xC // S < 4 * chunk):
        S -= 1
    return max(S, 1)


def igemm(N, xC, yC, yH, yW, R, stride, dgrad, wC, epi=False, ws=False, w_al=True, al=True):
    """plan_data: forward, or stride-1 backward-data (stride = 1, x = dy).  `al`: the output, the addend and the
    workspace on 16-byte boundaries (the finishing kernel of a split launch moves float4)."""
    g, pixt = _pick(N, yH, yW, _cdiv(yC, 128), 384, 1 if dgrad else stride, R)
    if g is None:
        return None
    CC = 32 if (R == 1 and stride == 1) else 8
    name, KB, can_split = _tile(g, pixt, yC)
    ok = xC % CC == 0 and w_al and (wC * R * R) % 4 == 0
    fast = ok and (not dgrad or yC % KB == 0)
    if epi and (not fast or dgrad or stride != 1):
        return None
    head = f"igemm<{R},{stride}{',dgrad' if dgrad else ''}>"
    if name == "128/KT2" and not epi:
        g2 = geom(N, yH, yW, 256, 1 if dgrad else stride, R)
        if g2 and g2.nt >= 512 and ok and (not dgrad or yC % 64 == 0):
            return f"{head}/256/PT2/fast/S1"
    S, note, wgs = 1, "", g.nt * _cdiv(yC, KB)
    if fast and can_split:
        if ws and al:
            S = igemm_split(wgs, xC, CC, N * yC * yH * yW, yH * yW)
        if wgs <= 256 and (yH * yW) % 4:
            note = "/hw-declined"
    return f"{head}/{name}/{'fast' if fast else 'slow'}/S{S}{note}{'/epi' if epi else ''}"


def data_ws_bytes(N, outC, outH, outW, R, cs):
    """salun_conv2d_data_workspace_bytes"""
    g, pixt = _pick(N, outH, outW, _cdiv(outC, 128), 384, cs, R)
    if g is None or (outH * outW) % 4:
        return 0
    wgs = g.nt * _cdiv(outC, _tile(g, pixt, outC)[1])
    return 0 if wgs > 256 else 8 * N * outC * outH * outW * 4


def forward(c, epi=False, ws=False, w_al=True, al=True):
    return igemm(c.N, c.C, c.K, c.P, c.Q, c.R, c.stride, False, c.C, epi, ws, w_al, al)


def _dgrad_s2_merged(c, w_al, al):
    N, C, H, W, K, R, pad, P, Q = c.N, c.C, c.H, c.W, c.K, c.R, c.pad, c.P, c.Q
    if H != 2 * P or W != 2 * Q or not ((R == 3 and pad in (0, 1)) or (R == 1 and pad == 0)):
        return None
    if K % 8 or not w_al or (C * R * R) % 4 or not al:
        return None
    g, pixt = _pick(N, P, Q, _cdiv(C, 64), 256, 1, 1 if R == 1 else 2)
    if g is None or g.psz > 256:
        return None
    if pixt == 128:
        name, kb = ("128/KT2", 64) if C % 64 == 0 else ("128/KT1", 32)
    else:
        name, kb = ("64/KT2WK2", 128) if (C % 128 == 0 and g.nt * (C // 128) >= 256) else ("64/KT1WK2", 64)
    return None if C % kb else f"dgrad_s2<{R},pad{pad}>/{name}"


def backward_data(c, ws=False, w_al=True, al=True):
    """plan_data (stride 1) / plan_dgrad_s2; `al`: dx, the addend and the workspace on a 16-byte boundary."""
    if c.stride == 1:
        return igemm(c.N, c.K, c.C, c.H, c.W, c.R, 1, True, c.C, False, ws, w_al, al)
    if c.H & 1 or c.W & 1:
        return None
    merged = _dgrad_s2_merged(c, w_al, al)
    if merged:
        return merged
    ntap = [((c.R - 1 - ((p + c.pad) & 1)) // 2 + 1) if ((p + c.pad) & 1) < c.R else 0 for p in (0, 1)]
    taps = []
    for rh in ntap:
        for rw in ntap:
            if rh and rw:
                g, pixt = _pick(c.N, c.H // 2, c.W // 2, _cdiv(c.C, 128), 384, 1, rh, rw)
                if g is None:
                    return None
                taps.append(f"<{rh},{rw}>/{_tile(g, pixt, c.C)[0]}{'/P3' if g.psz > 256 else ''}")
    return "dgrad_tap[" + " ".join(taps) + "]" + ("/empty" if 0 in ntap else "")


def _chunks_1x1(N, P, Q, stride):
    PQ = P * Q
    if PQ % 4 or (stride == 2 and Q % 4):
        return 0
    if PQ >= 64:
        return 0 if PQ % 64 else N * (PQ // 64)
    return 0 if 64 % PQ else _cdiv(N, 64 // PQ)


def _nsplit(K, C, nchunks, tile):
    return max(1, min(_cdiv(256, _cdiv(K, tile) * _cdiv(C, tile)), nchunks))


def backward_weight(c, shared=False):
    """plan_wgrad -> (route, partial images the reduce adds), or (None, 0)."""
    N, C, H, W, K, R, s, pad, P, Q = c.N, c.C, c.H, c.W, c.K, c.R, c.stride, c.pad, c.P, c.Q
    if R == 1 and pad == 0 and C >= 32 and H == P * s and W == Q * s and W % 4 == 0 and _chunks_1x1(N, P, Q, s):
        return f"wgrad_1x1<{s}>", _nsplit(K, C, _chunks_1x1(N, P, Q, s), 128)
    pixc = 64 if s == 1 else 32
    g = geom(N, P, Q, pixc, s, R)
    if g is None or g.psz > 256:
        return None, 0
    pow2 = g.TP & (g.TP - 1) == 0
    if C * R * R <= 32 and C <= 4 and Q >= 4 and pow2:
        return f"wgrad_smallc<{R},{s}>", 2 * max(1, min(1024 // _cdiv(K, 64), g.nt))
    if Q < 4 or not pow2 or 8 * (64 * (g.psz | 1) + 64 * (pixc + 1) + 256) > 160 * 1024:
        return None, 0
    ns = _nsplit(K, C, g.nt, 64)
    if R == 3 and s == 1 and pad == 1 and P == H and Q == W and not shared:
        if H == W and C % 64 == 0 and K % 32 == 0 and W in (4, 8, 16, 32):
            return f"wgrad_ring<W{W}>", ns
    if R == 3 and pad == 1 and C % 64 == 0 and W % 4 == 0 and Q * s == W and P * s == H:
        f4c = g.NI * g.IH * (W // 4)
        if f4c % 4 == 0 and f4c // 4 in ((5, 6, 8) if s == 1 else (9, 10)):
            return f"wgrad_v<{s},{f4c // 4}>", ns
    return f"wgrad<{R},{s},{'true' if C % 64 == 0 else 'false'}>", ns


def wgrad_ws_bytes(c):
    """salun_conv2d_wgrad_workspace_bytes: an upper bound over the kernels a shape may get."""
    g = geom(c.N, c.P, c.Q, 32, 1, c.R) or geom(c.N, c.P, c.Q, 64, 1, c.R)
    if g is None:
        return 0
    ns = _nsplit(c.K, c.C, g.nt, 64)
    if c.C * c.R * c.R <= 32 and c.C <= 4:
        g64 = geom(c.N, c.P, c.Q, 64, 1, c.R)
        ns = max(ns, 2 * min(1024 // _cdiv(c.K, 64), max(g.nt, g64.nt if g64 else 0)))
    if c.R == 1 and _chunks_1x1(c.N, c.P, c.Q, 1):
        ns = max(ns, _nsplit(c.K, c.C, _chunks_1x1(c.N, c.P, c.Q, 1), 128))
    return 4 * ns * c.K * c.C * c.R * c.R


def ring(N, Cred, H, W, Kout, cfg):
    """ring_launch's domain for the pinned tile `cfg`: the route, or None."""
    TPIX, KB, wkkt = RING_TILES[cfg]
    HW = H * W
    if Cred % 8 or W not in (4, 8, 16, 32) or TPIX % W or (HW % TPIX if HW >= TPIX else TPIX % HW):
        return None
    NI, TP = (1, TPIX // W) if HW >= TPIX else (TPIX // HW, H)
    irs = 12 if (W == 4 and NI > 1) else TP + 2
    npiece = 2 * NI * irs * W
    if irs < TP + 2 or npiece > 768 or 2 * (wkkt * 9 + _cdiv(npiece, 64)) * 1024 > 80 * 1024:
        return None
    return f"ring<W{W},cfg{cfg}>{'/NI' if NI > 1 else ''}"


def ring_pack_bytes(K, C, dgrad):
    rows, red = (C, K) if dgrad else (K, C)
    return 0 if red % 8 else _cdiv(rows, 32) * (red // 8) * 9 * 1024
