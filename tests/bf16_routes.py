"""Which kernel, tile and split the bf16 families pick for a shape: a pure-Python mirror of the host code of K11
(csrc/salun_conv_bf16.hip: convolution forward / backward-data / backward-weight) and K16 (csrc/salun_gemm.hip: the NT and
TN GEMMs, the ring form of the convolution forward), written from the code as it stood BEFORE the plans moved into
csrc/salun_bf16_plan.h - entry-point checks, the ring probe, dispatch_igemm / launch_igemm, tn_route, wgrad_splits, the
13-arm switch of salun_gemm_bf16_nt - in a default build (no tile pin, default split targets).  One check is later than that:
backward-weight refuses an empty input or output extent, as the data kernels always have.
test_bf16_routes_cpu.py holds it, label for label, to salun_conv2d_bf16_route / salun_gemm_bf16_route and to the
library's workspace and *_supported queries.

A route is (label, nsplit); None means SALUN_EINVAL, ENOSPC means SALUN_ENOSPC.  Convolution shapes are
(N, H, W, C, K, R, stride, pad); `ring` / `tn` are the values of SALUN_CONV_RING / SALUN_WGRAD_TN (defaults 1, 1)."""
ENOSPC = "ENOSPC"
COLSUM_CHUNKS = 128
SPLIT_TARGET, WGRAD_TARGET, TN_TARGET = 768, 384, 256


def _cdiv(a, b):
    return -(-a // b)


def conv_supported(C, K, R, stride, pad):
    return R in (1, 3) and stride in (1, 2) and 0 <= pad <= R - 1 and C % 32 == 0 and K % 32 == 0 and C >= 32 and K >= 32


def _out(H, R, stride, pad):
    """(H + 2*pad - R) / stride + 1 with C's division (truncating)"""
    a = H + 2 * pad - R
    return (a // stride if a >= 0 else -((-a) // stride)) + 1


# ------------------------------------------------------------------------------------------------ forward / backward-data
def plan_split(tiles, nstage):
    s = SPLIT_TARGET // max(tiles, 1)
    s = max(1, min(s, nstage // 6, 16))
    per = _cdiv(nstage, s)
    return _cdiv(nstage, per), per


def igemm_tile(Kout):
    """dispatch_igemm in a default build: 128 x 256 where the output channels tile it"""
    return (2, 4, 32) if Kout % 256 == 0 else (2, 2, 32)


def _igemm_split(M, Cin, Kout, R):
    wm, wn, bk = igemm_tile(Kout)
    tiles = _cdiv(M, 64 * wm) * _cdiv(Kout, 64 * wn)
    s, per = plan_split(tiles, R * R * (Cin // bk))
    return (wm, wn, bk), s, ((s * M * Kout * 4) % 2 ** 64 if s > 1 else 0)  # (size_t arithmetic: M < 0 where H < R - 2 * pad)


def _data_domain(N, H, W, C, K, R, stride, pad):
    """the checks salun_conv2d_bf16_forward and _backward_data share -> (OH, OW) or None"""
    if N < 1 or H < 1 or W < 1 or not conv_supported(C, K, R, stride, pad):
        return None
    OH, OW = _out(H, R, stride, pad), _out(W, R, stride, pad)
    if OH < 1 or OW < 1 or N * H * W * C >= 2 ** 31 or N * OH * OW * K >= 2 ** 31:
        return None
    if N * H * W >= 2 ** 24 or N * OH * OW >= 2 ** 24 or C >= 2 ** 24 or K >= 2 ** 24:
        return None
    return OH, OW


def ring_form(M, C, K, R, aligned, ring):
    """salun_conv2d_bf16_forward_ring: the tile form (WGM, WGN, NST), or None where it leaves the call to conv_bf16_igemm"""
    if not ring or C % 32 or K % 64 or R not in (1, 3) or M >= 2 ** 30:
        return None
    if R != 1 and ring not in (2, 3):
        return None
    if not aligned:
        return None
    t256 = _cdiv(M, 256)
    if ring == 2 and K % 128 == 0:
        return 2, 2, 4
    if K % 128 == 0 and t256 * (K // 128) >= 128:
        return 4, 2, 3
    if K % 128 != 0 and t256 * (K // 64) >= 128:
        return 4, 1, 3
    if K % 128 == 0 and _cdiv(M, 128) * (K // 128) >= 128:
        return 2, 2, 4
    return None


def _igemm_route(M, Cin, Kout, R, x_bytes, w_bytes, ws_bytes, dgrad):
    """launch_igemm: a missing or short workspace only disables the split; the buffer descriptors bound the tensors"""
    tile, s, want = _igemm_split(M, Cin, Kout, R)
    if s > 1 and (ws_bytes == 0 or ws_bytes < want):
        s = 1
    if x_bytes >= 2 ** 31 or w_bytes >= 2 ** 32:
        return None
    return "igemm<%d,%d,%d%s>/S%d" % (*tile, ",dgrad" if dgrad else "", s), s


def forward(shape, ws_bytes=0, aligned=True, ring=1):
    N, H, W, C, K, R, stride, pad = shape
    d = _data_domain(*shape)
    if d is None:
        return None
    M = N * d[0] * d[1]
    form = ring_form(M, C, K, R, aligned, ring)
    if form:
        return "ring<%d,%d,%d>" % form, 1
    return _igemm_route(M, C, K, R, N * H * W * C * 2, K * R * R * C * 2, ws_bytes, False)


def backward_data(shape, ws_bytes=0):
    N, H, W, C, K, R, stride, pad = shape
    d = _data_domain(*shape)
    if d is None:
        return None
    return _igemm_route(N * H * W, K, C, R, N * d[0] * d[1] * K * 2, K * R * R * C * 2, ws_bytes, True)


def data_workspace_bytes(shape):
    """salun_conv2d_bf16_data_workspace_bytes: the larger of the two directions' splits (0 where it refuses; the query
    checks the channel / filter domain and a positive INPUT extent only)"""
    N, H, W, C, K, R, stride, pad = shape
    if N < 1 or H < 1 or W < 1 or not conv_supported(C, K, R, stride, pad):
        return 0
    OH, OW = _out(H, R, stride, pad), _out(W, R, stride, pad)
    return max(_igemm_split(N * OH * OW, C, K, R)[2], _igemm_split(N * H * W, K, C, R)[2])


# ------------------------------------------------------------------------------------------------ GEMM TN / backward-weight
def tn_supported(M, Na, Nb):
    return (1 <= M < 2 ** 24 and Na >= 32 and Nb >= 32 and Na % 32 == 0 and Nb % 32 == 0 and M * Na < 2 ** 31
            and M * Nb < 2 ** 31)


def tn_plan(M, Na, Nb, variant=0):
    """-> (variant, splits)"""
    v = variant or 2
    ta, rst = (256 if v == 3 else 128), (32 if v == 2 else 64)
    tiles = _cdiv(Na, ta) * _cdiv(Nb, 128)
    stages = _cdiv(M, rst)
    s = max(1, min(_cdiv(TN_TARGET, tiles), stages // (256 // rst), 64))
    per = _cdiv(stages, s)
    return v, _cdiv(stages, per)


def tn_workspace_bytes(M, Na, Nb, variant=0):
    if not tn_supported(M, Na, Nb):
        return 0
    s = tn_plan(M, Na, Nb, variant)[1]
    return s * Na * Nb * 4 if s > 1 else 0


def gemm_tn(M, Na, Nb, variant=0, ws_bytes=0):
    if not tn_supported(M, Na, Nb) or not 0 <= variant <= 3:
        return None
    if ws_bytes < tn_workspace_bytes(M, Na, Nb, variant):
        return ENOSPC
    v, s = tn_plan(M, Na, Nb, variant)
    return "tn<v%d>/S%d" % (v, s), s


def _tn_route(M, C, K, R, stride, pad, tn):
    return bool(tn) and R == 1 and stride == 1 and pad == 0 and M >= 1024 and tn_supported(M, K, C)


def _tap_plan(shape):
    """-> splits, bytes of the partials"""
    N, H, W, C, K, R, stride, pad = shape
    OH, OW = _out(H, R, stride, pad), _out(W, R, stride, pad)
    chunks = N * ((OH + 7) // 8) * ((OW + 7) // 8)
    tiles = _cdiv(K, 64) * _cdiv(C, 64)
    s = max(1, min(_cdiv(WGRAD_TARGET, tiles), chunks, 64))
    return s, s * R * R * K * C * 4


def wgrad_layout(shape, aligned=True, tn=1):
    """The workspace of a backward-weight call, [GEMM or tap partials | column-sum partials]: -> (offset of the
    column-sum partials, end of them) on the route the call takes"""
    N, H, W, C, K, R, stride, pad = shape
    if _tn_route(N * H * W, C, K, R, stride, pad, tn) and aligned:
        off = (tn_workspace_bytes(N * H * W, K, C) + 255) & ~255
    else:
        off = _tap_plan(shape)[1]
    return off, off + COLSUM_CHUNKS * K * 4


def wgrad_workspace_bytes(shape, tn=1):
    """salun_conv2d_bf16_wgrad_workspace_bytes: the larger of the two routes (the query does not see dw's alignment)"""
    N, H, W, C, K, R, stride, pad = shape
    if N < 1 or not conv_supported(C, K, R, stride, pad):
        return 0
    need = wgrad_layout(shape, False, tn)[1]
    if _tn_route(N * H * W, C, K, R, stride, pad, tn):
        need = max(need, wgrad_layout(shape, True, tn)[1])
    return need


def backward_weight(shape, ws_bytes=0, aligned=True, tn=1):
    N, H, W, C, K, R, stride, pad = shape
    if N < 1 or not conv_supported(C, K, R, stride, pad):
        return None
    if H < 1 or W < 1 or _out(H, R, stride, pad) < 1 or _out(W, R, stride, pad) < 1:  # no pixel to reduce over
        return None
    if ws_bytes < wgrad_workspace_bytes(shape, tn):
        return ENOSPC
    if _tn_route(N * H * W, C, K, R, stride, pad, tn) and aligned:
        v, s = tn_plan(N * H * W, K, C)
        return "wgrad_tn<v%d>/S%d" % (v, s), s
    OH, OW = _out(H, R, stride, pad), _out(W, R, stride, pad)
    if N * H * W * C * 2 >= 2 ** 31 or N * OH * OW * K * 2 >= 2 ** 31:  # launch_wgrad's buffer descriptors
        return None
    s = _tap_plan(shape)[0]
    return "wgrad_tap<%d,%d>/S%d" % (R, stride, s), s


# ------------------------------------------------------------------------------------------------ GEMM NT
def nt_supported(M, N, K):
    return M >= 1 and N >= 64 and K >= 64 and N % 64 == 0 and K % 64 == 0 and M * K < 2 ** 31 and N * K < 2 ** 31


# the 13 arms of salun_gemm_bf16_nt's switch: the launch and whether the arm (or the check in front of the switch) wants
# N % 128 == 0
NT_ARMS = {1: ("nt<2,2,db>", True), 2: ("nt<2,2,sb>", True), 3: ("nt<4,1,db>", False), 4: ("nt<4,1,sb>", False),
           5: ("nt_p<2,2>", True), 6: ("nt_p<4,1>", False), 7: ("nt_r<2,2,4,64>", True), 8: ("nt_r<4,2,3,64>", True),
           9: ("nt_r<4,1,3,64>", False), 10: ("nt_r<2,2,3,64>", True), 11: ("nt_r<4,2,3,32>", True),
           12: ("nt_r<2,2,4,32>", True), 13: ("nt_r<4,1,3,32>", False)}


def gemm_nt(M, N, K, variant=0):
    if not nt_supported(M, N, K):
        return None
    if variant == 0:
        variant = 13 if N % 128 else (11 if _cdiv(M, 256) * (N // 128) >= 128 else 10)
    if variant not in NT_ARMS:
        return None
    label, n128 = NT_ARMS[variant]
    return None if n128 and N % 128 else (label, 1)
