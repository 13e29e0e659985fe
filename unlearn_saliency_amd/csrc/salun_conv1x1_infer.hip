// salun_conv1x1_infer.hip — K30: forward-only fp32 POINTWISE (1 x 1, stride 1, no padding) convolution with K27's
// inference epilogue, on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 FMA chains).
// gfx950 / CDNA4, wave64, 256-thread workgroups, compiled with -ffp-contract=off.
//
//   y[n,k,g] = act( (sum_c w[k,c] x[n,c,g]) * scale[k] + shift[k] + addend[n,k,g] ),   g in [0, HW)
//
// Why it exists: K27 gathers ONE input element per thread and load, evaluates a halo predicate per (pixel, tap) and
// decomposes its pixel into (n, p, q).  For a 1 x 1 / stride-1 convolution none of that does any work: x[n] IS the dense
// [C, HW] right-hand side of W[K, C] . x[n], every row contiguous.  ResNet-50 (SD/resnet50.py) has 33 such layers, about
// half of its FLOPs.  K30 is the same implicit GEMM over linearised pixels n HW + g - tiles may span images, the last
// pixel tile and a channel tile that K does not fill are masked - with the staging a dense operand allows:
//   * 16-byte path (HW % 4 == 0, x, w and y 16-byte aligned): a thread stages float4s - four consecutive pixels of one
//     input row, four consecutive input channels of one weight row.  A group of four pixels that starts at a multiple
//     of four never straddles an image (HW % 4 == 0), so it is inside the tensor or wholly outside: no per-element mask.
//   * 4-byte path (anything else, HW = 49 of ResNet-50's layer4 among it): one pixel per thread, as K27, without the halo
//     test and the (p, q) decomposition; the weights stay on float4 loads (4-byte loads only for a w off 16 bytes).
//     Same LDS image, same MFMA section: the same bits.
//   * stages of CC = 32 products (K27: 16), two LDS buffers, ONE barrier per stage: the global loads of stage i + 1 are
//     issued before the MFMA section of stage i and written to the OTHER buffer after it.
//
// Work split, operand layout and epilogue are K27's: 4 waves as 2 (pixels) x 2 (channels), a wave owns (PB/64) x (KB/64)
// accumulator tiles of 32 x 32; operand A is the weight, operand B the input; lane = pixel, register = channel.
//
// Reduction (fixed, tested): ONE chain over c in ascending order, two products per MFMA, no split over C.  That is the
// chain K27 runs for R = 1, so K30 returns K27's bits and a plan may route a layer to either kernel.  A last stage that C
// does not fill is padded with (+0) . (+0) products on BOTH operands; fma(0, 0, acc) == acc for every acc but -0, which
// an accumulator that started at +0 reaches only through underflow below the subnormals.
// LDS (one dynamic array): per buffer B rows of PB floats (a half-wave reads 32 consecutive floats), then A rows of
// KB + 4 floats (channel fastest; the pad spreads the staging store's rows over the banks).  2 x 33,280 B at 128 x 128.
// No atomics, no workspace; indexing is 64-bit wherever a tensor offset is formed.
#include "salun_device.h"
#include <stdio.h>
#include <string.h>

namespace {

constexpr int CC = 32;  // reduction products per stage

struct PwArgs {
  const float *x, *w, *scale, *shift, *addend;
  float *y;
  int C, K, relu, nkt;
  long long HW, npq;  // pixels of an image, N * HW
};

// MODE 2: float4 loads of x and w; 1: float4 loads of w, one pixel per thread; 0: 4-byte loads of both (w off 16 bytes)
template <int PB, int KB, int MODE>
__global__ __launch_bounds__(256) void conv1x1_infer(const PwArgs g) {
  constexpr int PT = PB / 64, KT = KB / 64;  // 32 x 32 accumulator tiles of a wave
  constexpr int AROW = KB + 4;
  constexpr int BUF = CC * PB + CC * AROW;  // floats of one buffer: B image, then A image
  constexpr int BE = CC * PB / 256;         // input floats a thread stages per stage
  constexpr int AE = CC * KB / 256;         // weight floats a thread stages per stage
  constexpr bool VEC = MODE == 2, AVEC = MODE >= 1;
  extern __shared__ __attribute__((aligned(16))) float lds[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lo = lane & 31, hi = lane >> 5;
  const int wp = wave & 1, wk = wave >> 1;
  const long long tile = static_cast<long long>(blockIdx.x) / g.nkt;
  const int k0 = static_cast<int>(static_cast<long long>(blockIdx.x) - tile * g.nkt) * KB;
  const long long g0 = tile * PB;
  const size_t HW = static_cast<size_t>(g.HW);
  const int C = g.C;

  // ---- what this thread stages.  B: VEC one float4 of pixels (column group bcol) in rows brow0, brow0 + BSTEP, ...;
  // else one pixel (bcol) in rows brow0, brow0 + BSTEP, ...  The pixel (group) is decomposed once, in 64 bits.
  constexpr int BW = VEC ? 4 : 1;          // floats per B load
  constexpr int BCOLS = PB / BW;           // loads per row
  constexpr int BSTEP = 256 / BCOLS;       // rows between two loads of a thread
  constexpr int BN = BE / BW;              // B loads per thread and stage
  const int bcol = tid % BCOLS, brow0 = tid / BCOLS;
  const long long gp = g0 + static_cast<long long>(bcol) * BW;
  const bool pvalid = gp < g.npq;  // VEC: npq and gp are multiples of 4: the whole group is valid or none of it
  const float *__restrict__ xb = g.x;
  if (pvalid) {
    const long long n = gp / g.HW;
    xb = g.x + static_cast<size_t>(n) * C * HW + static_cast<size_t>(gp - n * g.HW);
  }
  // A: VEC one float4 of input channels (c4) of weight row kk; else one element (cc, kk) as K27
  constexpr int AW = AVEC ? 4 : 1;
  constexpr int ACOLS = CC / AW;
  constexpr int AN = AE / AW;
  const float *__restrict__ wrow[AN];
#pragma unroll
  for (int i = 0; i < AN; ++i) {
    const int e = tid + i * 256, kk = e / ACOLS;
    const int k = (k0 + kk < g.K) ? k0 + kk : g.K - 1;  // a channel past the tensor: any real row (never stored)
    wrow[i] = g.w + static_cast<size_t>(k) * C;
  }

  f32x16 acc[PT][KT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt)
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[pt][t][v] = 0.f;

  // Staging is branch free, as in K27: every load goes to an address inside its tensor (clamped where the row is past C
  // or the pixel past the last one) and what must be zero is zeroed when the register is written to LDS.
  float breg[BE], areg[AE];
  const int nstage = (C + CC - 1) / CC;

  auto load_stage = [&](int st) {
    const int c0 = st * CC;
#pragma unroll
    for (int i = 0; i < BN; ++i) {
      const int c = c0 + brow0 + i * BSTEP;
      const float *src = xb + static_cast<size_t>(c < C ? c : C - 1) * HW;
      if (VEC) {
        const f32x4v v = *reinterpret_cast<const f32x4v *>(src);
#pragma unroll
        for (int j = 0; j < 4; ++j) breg[4 * i + j] = v[j];
      } else {
        breg[i] = *src;
      }
    }
#pragma unroll
    for (int i = 0; i < AN; ++i) {
      const int c = c0 + ((tid + i * 256) % ACOLS) * AW;
      if (AVEC) {  // C is a multiple of 8: a float4 of channels is inside the row or wholly past it
        const f32x4v v = *reinterpret_cast<const f32x4v *>(wrow[i] + (c < C ? c : C - 4));
#pragma unroll
        for (int j = 0; j < 4; ++j) areg[4 * i + j] = v[j];
      } else {
        areg[i] = wrow[i][c < C ? c : C - 1];
      }
    }
  };
  auto store_stage = [&](int st, float *buf) {
    const int c0 = st * CC;
    float *Bs = buf, *As = buf + CC * PB;
#pragma unroll
    for (int i = 0; i < BN; ++i) {
      const int row = brow0 + i * BSTEP;
      const bool ok = pvalid && c0 + row < C;
      if (VEC) {
        f32x4v v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ok ? breg[4 * i + j] : 0.f;
        *reinterpret_cast<f32x4v *>(Bs + row * PB + 4 * bcol) = v;
      } else {
        Bs[row * PB + bcol] = ok ? breg[i] : 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < AN; ++i) {
      const int e = tid + i * 256, cc = (e % ACOLS) * AW, kk = e / ACOLS;
      const bool ok = c0 + cc < C;
#pragma unroll
      for (int j = 0; j < AW; ++j) As[(cc + j) * AROW + kk] = ok ? areg[AW * i + j] : 0.f;
    }
  };

  const int boff = hi * PB + wp * (PT * 32) + lo;
  const int aoff = CC * PB + hi * AROW + wk * (KT * 32) + lo;
  load_stage(0);
  store_stage(0, lds);
  __syncthreads();
  for (int st = 0; st < nstage; ++st) {
    const float *buf = lds + (st & 1) * BUF;
    if (st + 1 < nstage) load_stage(st + 1);  // in flight during the MFMA section
    const float *bp = buf + boff, *ap = buf + aoff;
    // the operands of step i + 1 are read from LDS while the MFMAs of step i run
    float a_cur[KT], b_cur[PT], a_nxt[KT], b_nxt[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) b_cur[pt] = bp[pt * 32];
#pragma unroll
    for (int t = 0; t < KT; ++t) a_cur[t] = ap[t * 32];
#pragma unroll
    for (int step = 0; step < CC / 2; ++step) {
      if (step + 1 < CC / 2) {
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) b_nxt[pt] = bp[2 * (step + 1) * PB + pt * 32];
#pragma unroll
        for (int t = 0; t < KT; ++t) a_nxt[t] = ap[2 * (step + 1) * AROW + t * 32];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int pt = 0; pt < PT; ++pt)
#pragma unroll
        for (int t = 0; t < KT; ++t)
          acc[pt][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[t], b_cur[pt], acc[pt][t], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (step + 1 < CC / 2) {
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) b_cur[pt] = b_nxt[pt];
#pragma unroll
        for (int t = 0; t < KT; ++t) a_cur[t] = a_nxt[t];
      }
    }
    // the other buffer was last read in stage st - 1, which every wave left before the barrier that ended it
    if (st + 1 < nstage) store_stage(st + 1, lds + ((st + 1) & 1) * BUF);
    __syncthreads();
  }

  // ---- epilogue (K27's): lane = pixel, register = channel; the terms of a 32-channel tile are all read before its
  // first store (addend never aliases y: the entry point refuses it).
  const float *__restrict__ scale = g.scale;
  const float *__restrict__ shift = g.shift;
  const float *__restrict__ addend = g.addend;
  float *__restrict__ y = g.y;
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const long long go = g0 + (wp * PT + pt) * 32 + lo;
    if (go >= g.npq) continue;
    const long long n = go / g.HW;
    const size_t obase = static_cast<size_t>(n) * g.K * HW + static_cast<size_t>(go - n * g.HW);
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      const int kbase = k0 + (wk * KT + t) * 32 + 4 * hi;
      if (kbase >= g.K) continue;  // K is a multiple of 32: a 32-channel tile is inside the tensor or wholly outside
      float sv[16], hv[16], av[16];
      if (scale) {
#pragma unroll
        for (int v = 0; v < 16; ++v) sv[v] = scale[kbase + acc_row(v)];
      }
      if (shift) {
#pragma unroll
        for (int v = 0; v < 16; ++v) hv[v] = shift[kbase + acc_row(v)];
      }
      if (addend) {
#pragma unroll
        for (int v = 0; v < 16; ++v) av[v] = addend[obase + static_cast<size_t>(kbase + acc_row(v)) * HW];
      }
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        float o = acc[pt][t][v];
        if (scale) o = o * sv[v];
        if (shift) o = o + hv[v];
        if (addend) o = o + av[v];
        if (g.relu) o = (o < 0.f) ? 0.f : o;
        y[obase + static_cast<size_t>(kbase + acc_row(v)) * HW] = o;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- the plan
struct PwPlan {
  bool ok;
  int pb, kb;
  int mode;  // the kernel's MODE
  long long npq, blocks;
  int nkt;
};

constexpr int TILE_PB[4] = {0, 64, 128, 128};
constexpr int TILE_KB[4] = {0, 64, 64, 128};
constexpr long long FILL = 256;  // one workgroup per CU

// The ONE place that says whether a shape is served and by which instantiation: salun_conv1x1_infer launches from it
// and salun_conv1x1_infer_route prints it.  aligned16: x and y are 16-byte aligned; w_aligned16: w is.
PwPlan plan_pw(int N, int C, long long HW, int K, int tile, bool aligned16, bool w_aligned16) {
  PwPlan pl{};
  if (N < 1 || HW < 1 || HW > (1ll << 40) || static_cast<long long>(N) > (1ll << 40) / HW) return pl;
  if (C < 8 || C > 65536 || C % 8 != 0 || K < 32 || K > 65536 || K % 32 != 0) return pl;
  if (tile < SALUN_INFER_TILE_AUTO || tile > SALUN_INFER_TILE_128X128) return pl;
  const long long npq = static_cast<long long>(N) * HW;
  auto blocks_of = [&](int t) {
    return ((npq + TILE_PB[t] - 1) / TILE_PB[t]) * ((K + TILE_KB[t] - 1) / TILE_KB[t]);
  };
  int t = tile;
  if (t == SALUN_INFER_TILE_AUTO) {
    // K27's rule: the largest tile that still gives every CU a workgroup; 128 channels only where K fills them
    t = SALUN_INFER_TILE_64X64;
    if (K % 128 == 0 && blocks_of(SALUN_INFER_TILE_128X128) >= FILL) t = SALUN_INFER_TILE_128X128;
    else if (blocks_of(SALUN_INFER_TILE_128X64) >= FILL) t = SALUN_INFER_TILE_128X64;
  }
  pl.pb = TILE_PB[t];
  pl.kb = TILE_KB[t];
  pl.nkt = (K + pl.kb - 1) / pl.kb;
  pl.blocks = blocks_of(t);
  if (pl.blocks > 0x7FFFFFFFll) return pl;
  pl.mode = !w_aligned16 ? 0 : (aligned16 && HW % 4 == 0) ? 2 : 1;
  pl.npq = npq;
  pl.ok = true;
  return pl;
}

template <int PB, int KB>
int launch(const PwPlan &pl, const PwArgs &a, hipStream_t st) {
  const size_t ldsb = 2 * static_cast<size_t>(CC * PB + CC * (KB + 4)) * sizeof(float);
  const dim3 grid(static_cast<unsigned>(pl.blocks)), block(256);
  if (pl.mode == 2) return salun_launch_lds<conv1x1_infer<PB, KB, 2>>(grid, block, ldsb, st, a);
  if (pl.mode == 1) return salun_launch_lds<conv1x1_infer<PB, KB, 1>>(grid, block, ldsb, st, a);
  return salun_launch_lds<conv1x1_infer<PB, KB, 0>>(grid, block, ldsb, st, a);
}

}  // namespace

SALUN_EXPORT int salun_conv1x1_infer(const float *x, const float *w, const float *scale, const float *shift,
                                     const float *addend, float *y, int N, int C, int64_t HW, int K, int relu, int tile,
                                     salun_stream_t stream) {
  const PwPlan pl = plan_pw(N, C, HW, K, tile, salun_aligned16(x) && salun_aligned16(y), salun_aligned16(w));
  if (!pl.ok || !x || !w || !y || addend == y || x == y) return SALUN_EINVAL;
  if (!salun_aligned4(x) || !salun_aligned4(w) || !salun_aligned4(y) || !salun_aligned4(scale) || !salun_aligned4(shift) ||
      !salun_aligned4(addend))
    return SALUN_EINVAL;
  PwArgs a{x, w, scale, shift, addend, y, C, K, relu ? 1 : 0, pl.nkt, static_cast<long long>(HW), pl.npq};
  hipStream_t st = salun_hip_stream(stream);
  if (pl.pb == 64) return launch<64, 64>(pl, a, st);
  if (pl.kb == 64) return launch<128, 64>(pl, a, st);
  return launch<128, 128>(pl, a, st);
}

SALUN_EXPORT int salun_conv1x1_infer_route(int N, int C, int64_t HW, int K, int tile, int aligned16, int w_aligned16,
                                           char *buf, size_t buflen) {
  const PwPlan pl = plan_pw(N, C, HW, K, tile, aligned16 != 0, w_aligned16 != 0);
  if (!pl.ok || !buf) return SALUN_EINVAL;
  char tmp[96];
  snprintf(tmp, sizeof tmp, "pw/%dx%d/%s/B%lld", pl.pb, pl.kb, pl.mode == 2 ? "vec16" : pl.mode == 1 ? "vec4" : "scalar", pl.blocks);
  if (strlen(tmp) + 1 > buflen) return SALUN_ENOSPC;
  memcpy(buf, tmp, strlen(tmp) + 1);
  return SALUN_OK;
}
