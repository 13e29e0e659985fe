// salun_bf16_plan.h - which kernel, tile and split a call of the bf16 families runs, and how its workspace is laid out:
// K11 (salun_conv_bf16.hip: convolution forward / backward-data / backward-weight) and K16 (salun_gemm.hip: the NT and TN
// GEMMs and the ring form of the convolution forward).
//
// A call is PLANNED by a pure function of its shape - no HIP call, no pointer: a pointer enters as "is 16-byte aligned",
// reduced to a boolean at the C-ABI entry; the two environment switches enter as a Bf16Switches value - and then
// LAUNCHED from the plan.  salun_conv2d_bf16_route / salun_gemm_bf16_route print the plan an entry point would execute
// as a label, which is how tests/bf16_routes.py is held to this file.  Labels are built by the queries only.
//
//   conv forward     ring<WGM,WGN,NST>                k_conv_bf16_ring<WGM, WGN, NST>
//                    igemm<WM,WN,BK>/S<s>             conv_bf16_igemm<WM, WN, BK, false>, s reduction splits
//   conv bwd-data    igemm<WM,WN,BK,dgrad>/S<s>       conv_bf16_igemm<WM, WN, BK, true>
//   conv bwd-weight  wgrad_tn<v<n>>/S<s>              k_gemm_bf16_tn, variant n
//                    wgrad_tap<R,stride>/S<s>         conv_bf16_wgrad<R, stride>
//   gemm NT          nt<WGM,WGN,db|sb>                k_gemm_bf16_nt<WGM, WGN, DB>
//                    nt_p<WGM,WGN>                    k_gemm_bf16_nt_p<WGM, WGN>
//                    nt_r<WGM,WGN,NST,BK>             k_gemm_bf16_nt_r<WGM, WGN, NST, BK>
//   gemm TN          tn<v<n>>/S<s>                    k_gemm_bf16_tn, variant n
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../../include/salun.h"

// Build macros of the lab builds (tools/lab_build.sh).  This header is read by salun_conv_bf16.hip AND salun_gemm.hip:
// SALUN_TN_TARGET shapes the backward-weight workspace of the former through tn_plan, so a lab build that changes it
// recompiles both.
#ifndef SALUN_BF16_TILE
#define SALUN_BF16_TILE 0  // lab builds pin one tile shape of conv_bf16_igemm (igemm_tile); 0 = choose per problem
#endif
#ifndef SALUN_BF16_SPLIT_TARGET
#define SALUN_BF16_SPLIT_TARGET 768  // lab builds: other targets (profiles/r06_sd_split_targets.txt)
#endif
#ifndef SALUN_BF16_WGRAD_TARGET
#define SALUN_BF16_WGRAD_TARGET 384  // lab builds: other split targets (profiles/r05_wgrad_phases.txt, table 2)
#endif
#ifndef SALUN_TN_TARGET
#define SALUN_TN_TARGET 256  // workgroups a launch is split up to: 512 until backward-weight moved to the side stream (profiles/r06_sd_split_targets.txt)
#endif

namespace {

constexpr int COLSUM_CHUNKS = 128;  // row chunks of the bf16 column sums (k_colsum_partial, salun_conv_bf16.hip)

// The two environment switches, read once per process:
//   SALUN_CONV_RING  0 = no forward on the ring kernel, 1 (default) = the 1x1 convolutions with enough tiles, 2 = A/B: pin
//                    its 128 x 128 form where K % 128 == 0, 3 = every eligible shape (tests, A/B)
//   SALUN_WGRAD_TN   0 keeps the 1x1 weight gradients on the tap kernel (A/B measurements); default 1
struct Bf16Switches { int conv_ring, wgrad_tn; };
inline const Bf16Switches &bf16_switches() {
  static const Bf16Switches s = [] {
    const char *r = getenv("SALUN_CONV_RING"), *t = getenv("SALUN_WGRAD_TN");
    return Bf16Switches{r ? atoi(r) : 1, t ? atoi(t) : 1};
  }();
  return s;
}

// ------------------------------------------------------------------------------------------------ gemm_bf16_tn
inline bool gemm_bf16_tn_supported(int64_t M, int Na, int Nb) {
  return M >= 1 && M < (int64_t(1) << 24) && Na >= 32 && Nb >= 32 && Na % 32 == 0 && Nb % 32 == 0 &&
         (int64_t)M * Na < (int64_t(1) << 31) && (int64_t)M * Nb < (int64_t(1) << 31);
}

struct TnPlan {
  int variant, ta, tb, rst, tiles_a, tiles_b, stages, splits, per_split;
  size_t ws_bytes(int Na, int Nb) const { return splits > 1 ? (size_t)splits * Na * Nb * sizeof(float) : 0; }
};

// variant 1: 128 x 128, 64-token stages x 3 (96 KB, one workgroup per CU); 2: 128 x 128, 32-token stages x 4 (64 KB, two
// per CU); 3: 256 x 128, 8 waves, 64-token stages x 3 (144 KB)
inline TnPlan tn_plan(int64_t M, int Na, int Nb, int variant) {
  TnPlan p;
  if (variant == 0) variant = 2;
  p.variant = variant;
  p.ta = variant == 3 ? 256 : 128; p.tb = 128;
  p.rst = variant == 2 ? 32 : 64;
  p.tiles_a = (Na + p.ta - 1) / p.ta; p.tiles_b = (Nb + p.tb - 1) / p.tb;
  p.stages = (int)((M + p.rst - 1) / p.rst);
  const int tiles = p.tiles_a * p.tiles_b;
  const int min_stages = 256 / p.rst;           // a split reduces over >= 256 tokens
  int splits = (SALUN_TN_TARGET + tiles - 1) / tiles;
  if (splits > p.stages / min_stages) splits = p.stages / min_stages;
  if (splits > 64) splits = 64;
  if (splits < 1) splits = 1;
  p.per_split = (p.stages + splits - 1) / splits;
  p.splits = (p.stages + p.per_split - 1) / p.per_split;
  return p;
}

// what salun_gemm_bf16_tn returns for the shape before it launches; `ws_al16`: a workspace on a 16-byte boundary is given
inline int plan_gemm_tn(int64_t M, int Na, int Nb, int variant, bool ws_al16, size_t ws_bytes, TnPlan &p) {
  if (!gemm_bf16_tn_supported(M, Na, Nb) || variant < 0 || variant > 3) return SALUN_EINVAL;
  p = tn_plan(M, Na, Nb, variant);
  const size_t need = p.ws_bytes(Na, Nb);
  return need && (!ws_al16 || ws_bytes < need) ? SALUN_ENOSPC : SALUN_OK;
}

// ------------------------------------------------------------------------------------------------ gemm_bf16_nt
inline bool gemm_bf16_nt_supported(int64_t M, int N, int K) {
  return M >= 1 && N >= 64 && K >= 64 && N % 64 == 0 && K % 64 == 0 && M * (int64_t)K < (1ll << 31) &&
         (int64_t)N * K < (1ll << 31);
}

enum NtFamily { NT_PLAIN, NT_PERSISTENT, NT_RING };
// One row per variant number: a workgroup of WGM x WGN waves computes 64*WGM tokens x 64*WGN features (whole feature
// tiles only: N % (64*WGN) == 0), NST stages of BK reduction elements in LDS.
struct NtRow {
  NtFamily family;
  int wgm, wgn, nst, bk;
  constexpr int bm() const { return 64 * wgm; }
  constexpr int bn() const { return 64 * wgn; }
  constexpr size_t lds() const { return (size_t)nst * (bm() + bn()) * bk * 2; }
};
constexpr int NT_VARIANTS = 13;
constexpr NtRow NT_ROWS[NT_VARIANTS + 1] = {
    {},                         //  0 = choose (nt_choose)
    {NT_PLAIN, 2, 2, 2, 64},       //  1: 128 x 128 double-buffered
    {NT_PLAIN, 2, 2, 1, 64},       //  2: the same single-buffered
    {NT_PLAIN, 4, 1, 2, 64},       //  3: 256 x 64 double-buffered
    {NT_PLAIN, 4, 1, 1, 64},       //  4: the same single-buffered
    {NT_PERSISTENT, 2, 2, 2, 64},  //  5 / 6: the persistent forms of 1 / 3
    {NT_PERSISTENT, 4, 1, 2, 64},
    {NT_RING, 2, 2, 4, 64},        //  7: 128 x 128, 4 stages (128 KB)
    {NT_RING, 4, 2, 3, 64},        //  8: 256 x 128, 8 waves, 3 stages (144 KB)
    {NT_RING, 4, 1, 3, 64},        //  9: 256 x 64, 3 stages (120 KB)
    {NT_RING, 2, 2, 3, 64},        // 10: 128 x 128, 3 stages (96 KB)
    {NT_RING, 4, 2, 3, 32},        // 11: 256 x 128, 32-deep stages (72 KB: two per CU)
    {NT_RING, 2, 2, 4, 32},        // 12: 128 x 128, 32-deep x 4 (64 KB: two per CU)
    {NT_RING, 4, 1, 3, 32},        // 13: 256 x 64, 32-deep (60 KB: two per CU)
};

// measured on the SD shapes (profiles/r04_gemmbench_bf16.txt): the 8-wave 256 x 128 ring with 32-deep stages (two
// workgroups per CU) wins wherever it has >= ~128 tiles; the 4-wave 128 x 128 ring on smaller problems; feature counts
// that are multiples of 64 only: 256 x 64, 32-deep
inline int nt_choose(int64_t M, int N) {
  if (N % 128 != 0) return 13;
  return (((M + 255) / 256) * (int64_t)(N / 128) >= 128) ? 11 : 10;
}

struct NtPlan {
  int rc, variant;
  NtRow row;
  int tiles_m, tiles_n, grid, tiles_per_wg;  // tiles_per_wg: the persistent form only, else 0
};

inline NtPlan plan_gemm_nt(int64_t M, int N, int K, int variant) {
  NtPlan p{};
  p.rc = SALUN_EINVAL;
  if (!gemm_bf16_nt_supported(M, N, K) || variant < 0 || variant > NT_VARIANTS) return p;
  p.variant = variant ? variant : nt_choose(M, N);
  p.row = NT_ROWS[p.variant];
  if (N % p.row.bn() != 0) return p;
  p.tiles_m = (int)((M + p.row.bm() - 1) / p.row.bm());
  p.tiles_n = N / p.row.bn();
  p.grid = p.tiles_m * p.tiles_n;
  if (p.row.family == NT_PERSISTENT) {
    // 2 workgroups per CU (LDS: 2 x 64-80 KB); each walks a run of tiles inside its XCD's contiguous range
    const int per_xcd = (p.grid + 7) / 8;
    int runs = 64;  // workgroups per XCD
    if (runs > per_xcd) runs = per_xcd;
    p.tiles_per_wg = (per_xcd + runs - 1) / runs;
    runs = (per_xcd + p.tiles_per_wg - 1) / p.tiles_per_wg;
    p.grid = runs * 8;
  }
  p.rc = SALUN_OK;
  return p;
}

// ------------------------------------------------------------------------------------------------ convolution: domain
// (The kernels lean on this domain: aim_tap's `tap / 3` as (tap * 11) >> 5 is exact for tap < 9 only, i.e. R in {1, 3}, and
// the backward-weight epilogue guards whole waves with K % 32 == 0.  Widening it means revisiting both - ADVICE r5.)
inline bool conv_bf16_supported(int C, int K, int R, int stride, int pad) {
  return (R == 1 || R == 3) && (stride == 1 || stride == 2) && pad >= 0 && pad <= R - 1 && C % 32 == 0 && K % 32 == 0 &&
         C >= 32 && K >= 32;
}
inline int conv_out(int H, int R, int stride, int pad) { return (H + 2 * pad - R) / stride + 1; }

// ------------------------------------------------------------------------------------- convolution: forward / backward-data
struct IgemmTile { int wm, wn, bk; };  // conv_bf16_igemm<WM, WN, BK, BTR>: 64*WM pixels x 64*WN channels, BK-deep stages
// `Cin`: the reduction's channels, `Kout`: the output's (forward: C, K; backward-data: K, C)
inline IgemmTile igemm_tile(int Cin, int Kout) {
  const bool bk64 = Cin % 64 == 0;
  if (SALUN_BF16_TILE == 1 && bk64) return {2, 2, 64};
  if (SALUN_BF16_TILE == 2) return {2, 2, 32};
  if (SALUN_BF16_TILE == 3 && bk64) return {4, 1, 64};
  if (SALUN_BF16_TILE == 4) return {4, 1, 32};
  if (SALUN_BF16_TILE == 5) return {4, 2, 32};
  if (SALUN_BF16_TILE == 6) return {2, 4, 32};
  // 128 x 256 (eight waves) where the channel count tiles it: a third less operand traffic per MFMA, +5..13 % on the
  // 1280-channel levels; 128 x 128 otherwise (K = 320 / 640 would pad a 256-wide tile by 37 % / 17 %)
  if (Kout % 256 == 0) return {2, 4, 32};
  return {2, 2, 32};
}

// Reduction split of the data kernels: a convolution with few output tiles (the 16x16 and 8x8 levels of the U-Net)
// leaves most CUs without a workgroup, and a lone workgroup pays the full memory latency on every stage; splitting
// the (tap, channel) reduction over blockIdx.z fills the chip (target: 3 workgroups per CU) at the price of one fp32
// round trip of the output tile.
struct SplitPlan { int splits, per; };
inline SplitPlan plan_split(int64_t tiles, int nstage) {
  int s = (int)(SALUN_BF16_SPLIT_TARGET / (tiles < 1 ? 1 : tiles));
  if (s > nstage / 6) s = nstage / 6;  // at least 6 stages per workgroup
  if (s > 16) s = 16;
  if (s < 1) s = 1;
  const int per = (nstage + s - 1) / s;
  s = (nstage + per - 1) / per;
  return {s, per};
}

struct RingTile { int wgm, wgn, nst; };  // k_conv_bf16_ring<WGM, WGN, NST>; wgm == 0: the shape is not the ring's
// The LDS-DMA ring form of the forward (salun_gemm.hip), where the launch has enough tiles to do without a reduction
// split.  Measured on the SD layer table (tools/convbench_bf16.py, round 4): the ring wins the 1 x 1 convolutions (299 vs
// 229 and 282 vs 188 TFLOP/s) and LOSES the 3 x 3 ones (442 vs 540 TFLOP/s over the table: 90 .. 720 stages of 8 MFMAs
// per wave, gathered 64-byte rows through the LDS-DMA path, which the register-staged kernel with its 128 x 256 tiles
// out-runs).  `epi_al16`: y and the bias / nbias / addend that are given lie on 16-byte boundaries.
inline RingTile ring_tile(int64_t M, int K, int R, bool epi_al16, int on) {
  const RingTile none{0, 0, 0};
  if (!on || K % 64 != 0) return none;
  if (R != 1 && on != 3 && on != 2) return none;
  if (!epi_al16) return none;
  const int64_t t256 = (M + 255) / 256;
  if (on == 2 && K % 128 == 0) return {2, 2, 4};
  if (K % 128 == 0 && t256 * (K / 128) >= 128) return {4, 2, 3};
  if (K % 128 != 0 && t256 * (K / 64) >= 128) return {4, 1, 3};
  if (K % 128 == 0 && ((M + 127) / 128) * (K / 128) >= 128) return {2, 2, 4};
  return none;
}

struct ConvDataPlan {
  int rc;
  int OH, OW;        // extent of the forward's output
  int64_t M;         // output pixels of this direction
  RingTile ring;     // ring.wgm != 0: the ring kernel runs the call and the igemm fields below are not used
  IgemmTile tile;
  int mt, nt, nstage, splits, per;
  size_t ws_want;    // bytes the split this shape asks for uses (0: none); short of them, splits == 1
  uint32_t x_bytes, w_bytes;  // extents of the input and the weight image (conv_bf16_igemm's buffer descriptors)
};

// forward (dgrad = false): x[N][H][W][C] -> y[N][OH][OW][K]; backward-data: dy[N][OH][OW][K] -> dx[N][H][W][C].
// `ws_ok`: a workspace pointer was given.  rc != SALUN_OK: refused; ws_want is filled for every shape of the channel /
// filter domain with a positive input extent (the workspace query has always sized those, whatever a launch would say).
inline ConvDataPlan plan_conv_data(bool dgrad, int N, int H, int W, int C, int K, int R, int stride, int pad, bool epi_al16,
                                   bool ws_ok, size_t ws_bytes, const Bf16Switches &sw) {
  ConvDataPlan p{};
  p.rc = SALUN_EINVAL;
  if (N < 1 || H < 1 || W < 1 || !conv_bf16_supported(C, K, R, stride, pad)) return p;
  p.OH = conv_out(H, R, stride, pad); p.OW = conv_out(W, R, stride, pad);
  const int64_t in_px = (int64_t)N * H * W, out_px = (int64_t)N * p.OH * p.OW;
  const int Cin = dgrad ? K : C, Kout = dgrad ? C : K;
  p.M = dgrad ? in_px : out_px;
  p.tile = igemm_tile(Cin, Kout);
  const int BM = 64 * p.tile.wm, BN = 64 * p.tile.wn;
  const int64_t mt = (p.M + BM - 1) / BM;
  p.nt = (Kout + BN - 1) / BN;
  p.nstage = R * R * (Cin / p.tile.bk);
  SplitPlan sp = plan_split(mt * p.nt, p.nstage);
  p.ws_want = sp.splits > 1 ? (size_t)sp.splits * p.M * Kout * sizeof(float) : 0;
  if (sp.splits > 1 && (!ws_ok || ws_bytes < p.ws_want)) sp = {1, p.nstage};
  p.splits = sp.splits; p.per = sp.per;
  if (p.OH < 1 || p.OW < 1 || in_px * C >= (int64_t(1) << 31) || out_px * K >= (int64_t(1) << 31)) return p;
  // the staging addresses use 24-bit multiplies: pixel counts and channel counts below 2^24
  if (in_px >= (1 << 24) || out_px >= (1 << 24) || C >= (1 << 24) || K >= (1 << 24)) return p;
  p.mt = (int)mt;
  if (!dgrad) p.ring = ring_tile(p.M, K, R, epi_al16, sw.conv_ring);
  if (!p.ring.wgm) {
    // conv_bf16_igemm's buffer descriptors: an out-of-image tap reads at byte offset 2^31, which must lie past the end
    const int64_t xb = (dgrad ? out_px * K : in_px * C) * 2, wb = (int64_t)K * R * R * C * 2;
    if (xb >= (int64_t(1) << 31) || wb >= (int64_t(1) << 32)) return p;
    p.x_bytes = (uint32_t)xb; p.w_bytes = (uint32_t)wb;
  }
  p.rc = SALUN_OK;
  return p;
}

// what salun_conv2d_bf16_data_workspace_bytes answers: the larger of the two directions' splits on conv_bf16_igemm (the
// query does not see the pointers whose alignment admits the ring kernel)
inline size_t conv_data_ws_bytes(int N, int H, int W, int C, int K, int R, int stride, int pad) {
  const Bf16Switches no_ring{0, 0};
  const size_t f = plan_conv_data(false, N, H, W, C, K, R, stride, pad, true, true, SIZE_MAX, no_ring).ws_want;
  const size_t d = plan_conv_data(true, N, H, W, C, K, R, stride, pad, true, true, SIZE_MAX, no_ring).ws_want;
  return f > d ? f : d;
}

// --------------------------------------------------------------------------------------- convolution: backward-weight
// about 1.5 workgroups per CU, never more splits than chunks
// measured on the SD-v1 step (round 3, one box, four builds): 1536 / 768 / 384 / 256 target workgroups ->
// 219.3 / 209.3 / 205.7 / 206.6 ms; again with the paired 3x3 kernel (round 5, layer table): 512 / 384 / 256 ->
// 2.39 / 1.99 / 2.08 ms - every split adds a K*C*R*R fp32 partial to write and re-read (59 MB for a
// 1280x1280 3x3 layer), which costs more than the second resident round of workgroups gives back
inline int wgrad_splits(int tiles, int chunks) {
  int s = (SALUN_BF16_WGRAD_TARGET + tiles - 1) / tiles;
  if (s > chunks) s = chunks;
  if (s > 64) s = 64;
  if (s < 1) s = 1;
  return s;
}

// The workspace of a backward-weight call: [GEMM or tap partials | column-sum partials of the bias gradient]
struct WgradLayout {
  size_t colsum_off, total;
  static WgradLayout after(size_t partial_bytes, int K) {
    return {partial_bytes, partial_bytes + (size_t)COLSUM_CHUNKS * K * sizeof(float)};
  }
};

struct WgradPlan {
  int rc;
  bool tn;            // the TN GEMM runs the call (tnp, M); else conv_bf16_wgrad<R, stride> over the fields below
  int64_t M;          // tokens of the TN product
  TnPlan tnp;
  int OH, OW, tiles_h, tiles_w, chunks, splits, per_split;
  bool direct;        // one split: the tap kernel adds straight into dw
  uint32_t x_bytes, dy_bytes;
  WgradLayout lay;    // of the route taken
  size_t need;        // what salun_conv2d_bf16_wgrad_workspace_bytes answers: the larger of the two routes' totals
};

// 1x1 stride-1 unpadded convolutions (and the Linear layers, which arrive as such) are plain dY^T . X products: K16's TN
// kernel takes them where dw lies on a 16-byte boundary (the tap kernels take any dw: a gradient behind an odd-sized
// parameter of the flat arena).  Short reductions (the 8 x 8 level: M = 512) keep the tap kernel: with one split it adds
// straight into the gradient, the GEMM would need partials there (profiles/r04_gemmbench_bf16.txt: 11.6 vs 17.5 us,
// 51 vs 61 us).  `ws_bytes` short of `need`: SALUN_ENOSPC.
inline WgradPlan plan_conv_wgrad(int N, int H, int W, int C, int K, int R, int stride, int pad, bool dw_al16,
                                 size_t ws_bytes, const Bf16Switches &sw) {
  WgradPlan p{};
  p.rc = SALUN_EINVAL;
  if (N < 1 || !conv_bf16_supported(C, K, R, stride, pad)) return p;
  p.OH = conv_out(H, R, stride, pad); p.OW = conv_out(W, R, stride, pad);
  p.tiles_h = (p.OH + 7) / 8; p.tiles_w = (p.OW + 7) / 8;
  p.chunks = N * p.tiles_h * p.tiles_w;
  p.splits = wgrad_splits(((K + 63) / 64) * ((C + 63) / 64), p.chunks);
  p.per_split = (p.chunks + p.splits - 1) / p.splits;
  p.direct = p.splits == 1;
  const WgradLayout tap = WgradLayout::after((size_t)p.splits * R * R * K * C * sizeof(float), K);
  p.lay = tap;
  p.need = tap.total;
  p.M = (int64_t)N * H * W;
  if (sw.wgrad_tn && R == 1 && stride == 1 && pad == 0 && p.M >= 1024 && gemm_bf16_tn_supported(p.M, K, C)) {
    p.tnp = tn_plan(p.M, K, C, 0);
    const WgradLayout tn = WgradLayout::after((p.tnp.ws_bytes(K, C) + 255) & ~(size_t)255, K);
    if (tn.total > p.need) p.need = tn.total;
    p.tn = dw_al16;
    if (p.tn) p.lay = tn;
  }
  // an empty input or output extent (H < R - 2 * pad) is refused as forward and backward-data refuse it: there is no pixel
  // to reduce over, and the column sums would walk N * OH * OW rows of a dy that has none
  if (H < 1 || W < 1 || p.OH < 1 || p.OW < 1) return p;
  if (ws_bytes < p.need) { p.rc = SALUN_ENOSPC; return p; }
  if (!p.tn) {
    // conv_bf16_wgrad's buffer descriptors: an out-of-image lane reads at byte offset 2^31, past the end of both tensors
    const int64_t xb = p.M * C * 2, db = (int64_t)N * p.OH * p.OW * K * 2;
    if (xb >= (int64_t(1) << 31) || db >= (int64_t(1) << 31)) { p.rc = SALUN_EINVAL; return p; }
    p.x_bytes = (uint32_t)xb; p.dy_bytes = (uint32_t)db;
  }
  p.rc = SALUN_OK;
  return p;
}

// ------------------------------------------------------------------------------------------------ labels (queries only)
inline int conv_data_label(char *buf, size_t n, const ConvDataPlan &p, bool dgrad) {
  if (p.ring.wgm) return snprintf(buf, n, "ring<%d,%d,%d>", p.ring.wgm, p.ring.wgn, p.ring.nst);
  return snprintf(buf, n, "igemm<%d,%d,%d%s>/S%d", p.tile.wm, p.tile.wn, p.tile.bk, dgrad ? ",dgrad" : "", p.splits);
}
inline int conv_wgrad_label(char *buf, size_t n, const WgradPlan &p, int R, int stride) {
  if (p.tn) return snprintf(buf, n, "wgrad_tn<v%d>/S%d", p.tnp.variant, p.tnp.splits);
  return snprintf(buf, n, "wgrad_tap<%d,%d>/S%d", R, stride, p.splits);
}
inline int nt_label(char *buf, size_t n, const NtPlan &p) {
  const NtRow &r = p.row;
  if (r.family == NT_PLAIN) return snprintf(buf, n, "nt<%d,%d,%s>", r.wgm, r.wgn, r.nst == 2 ? "db" : "sb");
  if (r.family == NT_PERSISTENT) return snprintf(buf, n, "nt_p<%d,%d>", r.wgm, r.wgn);
  return snprintf(buf, n, "nt_r<%d,%d,%d,%d>", r.wgm, r.wgn, r.nst, r.bk);
}
inline int tn_label(char *buf, size_t n, const TnPlan &p) { return snprintf(buf, n, "tn<v%d>/S%d", p.variant, p.splits); }

// the switches a route query plans with: the process's, or what the SALUN_ROUTE_RING / SALUN_ROUTE_WGRAD_TN bits carry
inline Bf16Switches route_switches(unsigned flags) {
  Bf16Switches sw = bf16_switches();
  const unsigned ring = (flags >> SALUN_ROUTE_RING_SHIFT) & 7u, tn = (flags >> SALUN_ROUTE_WGRAD_TN_SHIFT) & 3u;
  if (ring) sw.conv_ring = (int)ring - 1;
  if (tn) sw.wgrad_tn = (int)tn - 1;
  return sw;
}

}  // namespace
