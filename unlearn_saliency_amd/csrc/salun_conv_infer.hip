// salun_conv_infer.hip — K27: forward-only fp32 2-D convolution for ARBITRARY map sizes, with the inference epilogue
// of a folded BatchNorm, on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 FMA chains, as K8).
// gfx950 / CDNA4, wave64, 256-thread workgroups, compiled with -ffp-contract=off.
//
//   y[n,k,p,q] = act( conv(x, w)[n,k,p,q] * scale[k] + shift[k] + addend[n,k,p,q] )
//
// Why it exists: every kernel of K8 / K8r tiles the output by rows and needs a power-of-two output width.  The
// classifier that scores generated images (torchvision's ResNet-34 at 224 x 224: maps 112, 56, 28, 14 and 7 wide, a
// 7 x 7 / stride-2 stem) has none.  K27 is an implicit GEMM over LINEARISED output pixels g = (n P + p) Q + q, so no
// property of P or Q matters: a tile is PB consecutive g (64 or 128) by KB output channels (64 or 128), the last pixel
// tile is masked, and so is a channel tile that K (a multiple of 32) does not fill.
//
// Work split.  4 waves as 2 (pixels) x 2 (channels); a wave owns PB/2 pixels x KB/2 channels = (PB/64) x (KB/64)
// accumulator tiles of 32 x 32.  MFMA operand A is the weight (rows = channels), operand B the gathered input
// (columns = pixels): lane l feeds A[k = l & 31][j = l >> 5] and B[j = l >> 5][g = l & 31], and accumulator register v
// of lane l is channel (v & 3) + 8 (v >> 2) + 4 (l >> 5), pixel l & 31.
//
// Reduction.  The C R R products of an output element are walked in stages of CC = 16 through LDS; within a stage the
// MFMA takes them two at a time in ascending order.  Two orders, chosen by the plan:
//   fast     (C % 16 == 0)  tap outermost, then channels: a stage is 16 consecutive channels of ONE tap, so a thread
//            evaluates one halo predicate per (pixel, tap) and the decomposition of its pixel once per tile.
//   generic  (any C)        the OIHW order j = (c R + r) R + s, stages of 16 consecutive j, the last one padded with
//            zeros (the stem's 147 products make 10 stages): weights are read as contiguous runs; the input gather
//            decomposes j per element (two divisions by small numbers), which only the three-channel stem and the
//            C % 16 == 8 layers pay.
// Staging is through registers: the global loads of stage i + 1 are issued before the MFMA section of stage i and
// written to LDS after it.  A thread stages ONE pixel (tid % PB) for the whole tile - (n, p, q) is decomposed once, in
// 64-bit arithmetic - and the rows tid / PB, tid / PB + 256 / PB, ... of the stage.  Every staging load is
// unconditional, from an address clamped into its tensor; padding, the tail of the reduction and the pixels past the
// last one become zeros when the registers are written to LDS (so a halo position contributes 0 * w, as in K8).
// Inside a stage the LDS operands of MFMA step i + 1 are read while the MFMAs of step i run.
// LDS: B rows of PB floats (a half-wave reads 32 consecutive floats: conflict free), A rows of KB + 4 floats (the
// staging store walks the reduction index fastest; the pad spreads its 16 rows over all banks).
//
// Epilogue, per element and in this order, every operation rounded by itself (no contraction):
//   o = acc;  o = o * scale[k];  o = o + shift[k];  o = o + addend;  o = o < 0 ? 0 : o.
// No atomics, no workspace: an element's bits depend on its own reduction only, not on the tile, the batch or the run.
// Indexing is 64-bit wherever a tensor offset is formed.
//
// salun_conv2d_infer_up2 is the same kernel with UP2 = true: the input is gathered through the virtual nearest-neighbour
// 2x map (x[ih >> 1][iw >> 1]), which the first-stage decoder's Upsample would otherwise write out at four times the
// size of x and read back once.  The instantiations with UP2 = false compile as they did without it
// (profiles/conv_infer_up2_resource_usage_{parent,head}.txt).
#include "salun_device.h"
#include <stdio.h>
#include <string.h>

namespace {

constexpr int CC = 16;  // reduction products per stage

struct InferArgs {
  const float *x, *w, *scale, *shift, *addend;
  float *y;
  int N, C, H, W, K, R, stride, pad, P, Q;
  int relu;
  long long npq;  // N * P * Q
  int nkt;        // channel tiles
};

// UP2: x is read through the virtual nearest-neighbour map up2(x)[n,c,i,j] = x[n,c,i>>1,j>>1] of 2H x 2W (g.H, g.W stay
// the STORED sizes).  The halo test is made in virtual coordinates and the shift comes after it: virtual row -1 or 2H
// is padding, not stored row 0 or H - 1.  Nothing else differs, so the bits are those of the plain kernel on the
// materialised map.
template <int PB, int KB, bool GENERIC, bool UP2>
__global__ __launch_bounds__(256) void conv_infer(const InferArgs g) {
  constexpr int PT = PB / 64, KT = KB / 64;  // 32 x 32 accumulator tiles of a wave
  constexpr int AROW = KB + 4;
  constexpr int BN = CC * PB / 256;  // input elements a thread stages per stage
  constexpr int BSTEP = 256 / PB;    // rows between two of them
  constexpr int AN = CC * KB / 256;  // weight elements a thread stages per stage
  __shared__ float Bs[CC * PB];
  __shared__ float As[CC * AROW];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lo = lane & 31, hi = lane >> 5;
  const int wp = wave & 1, wk = wave >> 1;
  const long long tile = static_cast<long long>(blockIdx.x) / g.nkt;
  const int k0 = static_cast<int>(static_cast<long long>(blockIdx.x) - tile * g.nkt) * KB;
  const long long g0 = tile * PB;
  const int RS = g.R * g.R;
  const size_t HW = static_cast<size_t>(g.H) * g.W;
  const long long PQ = static_cast<long long>(g.P) * g.Q;
  const int J = g.C * RS;  // products per output element
  const int VH = UP2 ? 2 * g.H : g.H, VW = UP2 ? 2 * g.W : g.W;  // the map the taps walk

  // ---- the pixel this thread stages: decomposed once
  const int bpix = tid % PB, brow0 = tid / PB;
  const long long gp = g0 + bpix;
  const bool pvalid = gp < g.npq;
  int ih0 = 0, iw0 = 0;
  const float *ximg = g.x;
  if (pvalid) {
    const long long n = gp / PQ;
    const int rem = static_cast<int>(gp - n * PQ);
    const int p = rem / g.Q, q = rem - p * g.Q;
    ih0 = p * g.stride - g.pad;
    iw0 = q * g.stride - g.pad;
    ximg = g.x + static_cast<size_t>(n) * g.C * HW;
  }

  f32x16 acc[PT][KT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt)
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[pt][t][v] = 0.f;

  const int cchunks = GENERIC ? 1 : g.C / CC;
  const int nstage = GENERIC ? (J + CC - 1) / CC : RS * cchunks;
  // Staging is branch free: every load goes to an address inside its tensor (clamped where the element is padding, past
  // the reduction or past the last channel) and what must be zero is zeroed when the register is written to LDS.  A
  // conditional load costs more than its branch here: it made the compiler wait for ALL loads in flight in the middle
  // of issuing them.
  const float *__restrict__ xr = ximg;
  const float *__restrict__ wr = g.w;
  float breg[BN], areg[AN];
  unsigned bmask = 0;  // bit i: breg[i] is a real input element (fast: all bits alike)
  // the weight element of this thread in row i of its share: its offset for stage 0 (64-bit once, 32-bit steps after)
  size_t woff[AN];
#pragma unroll
  for (int i = 0; i < AN; ++i) {
    const int e = tid + i * 256, cc = e % CC, kk = e / CC;
    const int k = (k0 + kk < g.K) ? k0 + kk : g.K - 1;  // a channel past the tensor: any real row (never stored)
    woff[i] = GENERIC ? static_cast<size_t>(k) * J + cc : (static_cast<size_t>(k) * g.C + cc) * RS;
  }

  auto load_stage = [&](int st) {
    if (!GENERIC) {
      const int tap = st / cchunks, c0 = (st - tap * cchunks) * CC;
      const int r = tap / g.R, s = tap - r * g.R;
      const int ih = ih0 + r, iw = iw0 + s;
      const bool ok = pvalid && ih >= 0 && ih < VH && iw >= 0 && iw < VW;  // the one halo test of (pixel, tap)
      bmask = ok ? ~0u : 0u;
      const int sh = UP2 ? ih >> 1 : ih, sw = UP2 ? iw >> 1 : iw;
      const float *src = xr + static_cast<size_t>(c0 + brow0) * HW + (ok ? static_cast<size_t>(sh) * g.W + sw : 0);
#pragma unroll
      for (int i = 0; i < BN; ++i) breg[i] = src[static_cast<size_t>(i * BSTEP) * HW];
      const int wstep = c0 * RS + tap;
#pragma unroll
      for (int i = 0; i < AN; ++i) areg[i] = wr[woff[i] + wstep];
    } else {
      const int j0 = st * CC;
      bmask = 0;
#pragma unroll
      for (int i = 0; i < BN; ++i) {
        const int j = j0 + brow0 + i * BSTEP;
        const int jc = j < J ? j : J - 1;
        const int c = jc / RS, tap = jc - c * RS;
        const int r = tap / g.R, s = tap - r * g.R;
        const int ih = ih0 + r, iw = iw0 + s;
        const bool ok = pvalid && j < J && ih >= 0 && ih < VH && iw >= 0 && iw < VW;
        bmask |= ok ? (1u << i) : 0u;
        const int sh = UP2 ? ih >> 1 : ih, sw = UP2 ? iw >> 1 : iw;
        breg[i] = xr[ok ? static_cast<size_t>(c) * HW + static_cast<size_t>(sh) * g.W + sw : 0];
      }
#pragma unroll
      for (int i = 0; i < AN; ++i) {
        const int cc = (tid + i * 256) % CC;
        const int back = (j0 + cc < J) ? 0 : j0 + cc - (J - 1);  // past the reduction: the row's last element
        areg[i] = wr[woff[i] + j0 - back];
      }
    }
  };
  auto store_stage = [&](int st) {
#pragma unroll
    for (int i = 0; i < BN; ++i) Bs[(brow0 + i * BSTEP) * PB + bpix] = ((bmask >> i) & 1u) ? breg[i] : 0.f;
#pragma unroll
    for (int i = 0; i < AN; ++i) {
      const int e = tid + i * 256, cc = e % CC, kk = e / CC;
      As[cc * AROW + kk] = (!GENERIC || st * CC + cc < J) ? areg[i] : 0.f;
    }
  };

  const float *bp = Bs + hi * PB + wp * (PT * 32) + lo;
  const float *ap = As + hi * AROW + wk * (KT * 32) + lo;
  load_stage(0);
  for (int st = 0; st < nstage; ++st) {
    __syncthreads();  // the previous stage has been consumed
    store_stage(st);
    __syncthreads();
    if (st + 1 < nstage) load_stage(st + 1);  // in flight during the MFMA section
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
  }

  // ---- epilogue: lane = pixel, register = channel.  The terms of a 32-channel tile are ALL read before its first
  // store (addend never aliases y - the entry point refuses it - so the loads may run ahead of the stores).
  const float *__restrict__ scale = g.scale;
  const float *__restrict__ shift = g.shift;
  const float *__restrict__ addend = g.addend;
  float *__restrict__ y = g.y;
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const long long go = g0 + (wp * PT + pt) * 32 + lo;
    if (go >= g.npq) continue;
    const long long n = go / PQ;
    const size_t obase = static_cast<size_t>(n) * g.K * PQ + static_cast<size_t>(go - n * PQ);
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
        for (int v = 0; v < 16; ++v) av[v] = addend[obase + static_cast<size_t>(kbase + acc_row(v)) * PQ];
      }
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        float o = acc[pt][t][v];
        if (scale) o = o * sv[v];
        if (shift) o = o + hv[v];
        if (addend) o = o + av[v];
        if (g.relu) o = (o < 0.f) ? 0.f : o;
        y[obase + static_cast<size_t>(kbase + acc_row(v)) * PQ] = o;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- the plan
struct InferPlan {
  bool ok;
  int pb, kb;
  bool generic;
  long long npq, blocks;
  int nkt;
};

constexpr int TILE_PB[4] = {0, 64, 128, 128};
constexpr int TILE_KB[4] = {0, 64, 64, 128};
constexpr long long FILL = 256;  // one workgroup per CU

// The ONE place that says whether a shape is served and by which instantiation: salun_conv2d_infer[_up2] launch from it
// and salun_conv2d_infer[_up2]_route print it.  up2: H and W are the STORED sizes; the domain is the plain one applied
// to the virtual 2H x 2W map, narrowed to what the decoder's Upsample needs (3 x 3, stride 1, C % 8 == 0, H, W <= 512).
InferPlan plan_infer(int N, int C, int H, int W, int K, int R, int stride, int pad, int P, int Q, int tile,
                     bool up2 = false) {
  InferPlan pl{};
  if (up2) {
    if (R != 3 || stride != 1 || C < 8 || C % 8 != 0 || H < 1 || H > 512 || W < 1 || W > 512) return pl;
    H *= 2;
    W *= 2;
  }
  if (N < 1 || C < 1 || C > 65536 || K < 32 || K % 32 != 0 || K > 65536) return pl;
  if (R != 1 && R != 3 && R != 7) return pl;
  if (R != 7 && C % 8 != 0) return pl;
  if (stride != 1 && stride != 2) return pl;
  if (pad < 0 || pad >= R) return pl;
  if (H < 1 || H > 1024 || W < 1 || W > 1024 || P < 1 || P > 1024 || Q < 1 || Q > 1024) return pl;
  if ((P - 1) * stride - pad >= H || (Q - 1) * stride - pad >= W) return pl;  // an output row / column that reads nothing
  if (tile < SALUN_INFER_TILE_AUTO || tile > SALUN_INFER_TILE_128X128) return pl;
  const long long npq = static_cast<long long>(N) * P * Q;
  if (static_cast<long long>(N) > ((1ll << 40) / (static_cast<long long>(P) * Q))) return pl;
  auto blocks_of = [&](int t) {
    return ((npq + TILE_PB[t] - 1) / TILE_PB[t]) * ((K + TILE_KB[t] - 1) / TILE_KB[t]);
  };
  int t = tile;
  if (t == SALUN_INFER_TILE_AUTO) {
    // the largest tile that still gives every CU a workgroup; 128 channels only where K fills them
    t = SALUN_INFER_TILE_64X64;
    if (K % 128 == 0 && blocks_of(SALUN_INFER_TILE_128X128) >= FILL) t = SALUN_INFER_TILE_128X128;
    else if (blocks_of(SALUN_INFER_TILE_128X64) >= FILL) t = SALUN_INFER_TILE_128X64;
  }
  pl.pb = TILE_PB[t];
  pl.kb = TILE_KB[t];
  pl.nkt = (K + pl.kb - 1) / pl.kb;
  pl.blocks = blocks_of(t);
  if (pl.blocks > 0x7FFFFFFFll) return pl;
  pl.generic = (C % CC) != 0;
  pl.npq = npq;
  pl.ok = true;
  return pl;
}

template <int PB, int KB, bool UP2>
void launch(const InferPlan &pl, const InferArgs &a, hipStream_t st) {
  if (pl.generic) hipLaunchKernelGGL((conv_infer<PB, KB, true, UP2>), dim3(static_cast<unsigned>(pl.blocks)), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((conv_infer<PB, KB, false, UP2>), dim3(static_cast<unsigned>(pl.blocks)), dim3(256), 0, st, a);
}

template <bool UP2>
int run_infer(const float *x, const float *w, const float *scale, const float *shift, const float *addend, float *y, int N,
              int C, int H, int W, int K, int R, int stride, int pad, int P, int Q, int relu, int tile,
              salun_stream_t stream) {
  const InferPlan pl = plan_infer(N, C, H, W, K, R, stride, pad, P, Q, tile, UP2);
  if (!pl.ok || !x || !w || !y || addend == y || x == y) return SALUN_EINVAL;
  if (!salun_aligned4(x) || !salun_aligned4(w) || !salun_aligned4(y) || !salun_aligned4(scale) || !salun_aligned4(shift) ||
      !salun_aligned4(addend))
    return SALUN_EINVAL;
  InferArgs a{x, w, scale, shift, addend, y, N, C, H, W, K, R, stride, pad, P, Q, relu ? 1 : 0, pl.npq, pl.nkt};
  hipStream_t st = salun_hip_stream(stream);
  if (pl.pb == 64) launch<64, 64, UP2>(pl, a, st);
  else if (pl.kb == 64) launch<128, 64, UP2>(pl, a, st);
  else launch<128, 128, UP2>(pl, a, st);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

int route_infer(int N, int C, int H, int W, int K, int R, int stride, int pad, int P, int Q, int tile, bool up2, char *buf,
                size_t buflen) {
  const InferPlan pl = plan_infer(N, C, H, W, K, R, stride, pad, P, Q, tile, up2);
  if (!pl.ok) return SALUN_EINVAL;
  if (!buf) return SALUN_EINVAL;
  char tmp[96];
  snprintf(tmp, sizeof tmp, "infer<%d,%d>%s/%dx%d/%s/B%lld", R, stride, up2 ? "^2" : "", pl.pb, pl.kb,
           pl.generic ? "generic" : "fast", pl.blocks);
  if (strlen(tmp) + 1 > buflen) return SALUN_ENOSPC;
  memcpy(buf, tmp, strlen(tmp) + 1);
  return SALUN_OK;
}

}  // namespace

SALUN_EXPORT int salun_conv2d_infer(const float *x, const float *w, const float *scale, const float *shift,
                                    const float *addend, float *y, int N, int C, int H, int W, int K, int R, int stride,
                                    int pad, int P, int Q, int relu, int tile, salun_stream_t stream) {
  return run_infer<false>(x, w, scale, shift, addend, y, N, C, H, W, K, R, stride, pad, P, Q, relu, tile, stream);
}

SALUN_EXPORT int salun_conv2d_infer_route(int N, int C, int H, int W, int K, int R, int stride, int pad, int P, int Q,
                                          int tile, char *buf, size_t buflen) {
  return route_infer(N, C, H, W, K, R, stride, pad, P, Q, tile, false, buf, buflen);
}

SALUN_EXPORT int salun_conv2d_infer_up2(const float *x, const float *w, const float *scale, const float *shift,
                                        const float *addend, float *y, int N, int C, int H, int W, int K, int R,
                                        int stride, int pad, int P, int Q, int relu, int tile, salun_stream_t stream) {
  return run_infer<true>(x, w, scale, shift, addend, y, N, C, H, W, K, R, stride, pad, P, Q, relu, tile, stream);
}

SALUN_EXPORT int salun_conv2d_infer_up2_route(int N, int C, int H, int W, int K, int R, int stride, int pad, int P, int Q,
                                              int tile, char *buf, size_t buflen) {
  return route_infer(N, C, H, W, K, R, stride, pad, P, Q, tile, true, buf, buflen);
}
