// salun_pool.hip — K24: MaxPool2d(kernel 2, stride 2, no padding) of an fp32 NCHW tensor, forward and backward.
// gfx950 / CDNA4, wave64.  The one operator of VGG-16-BN that had no kernel here.
//
// The tensor is NC planes of H x W floats; a "row pair" is two consecutive input rows 2r, 2r + 1 of one plane, and
// because H is even the row pairs of ALL planes are one flat sequence: row pair R starts at float R * 2W and produces
// the W / 2 outputs that start at float R * (W / 2).
//
// Selection (that of torch.nn.functional.max_pool2d): scan the window as 0 top-left, 1 top-right, 2 bottom-left,
// 3 bottom-right from (-inf, position 0) and take a value when it is greater than the running maximum or is NaN.  The
// first of equal maxima wins, a later NaN replaces an earlier one, +0 after -0 does not replace it.  idx keeps the
// position (0..3) as one byte per output; backward needs nothing else.
//
// Vector route (W % 4 == 0, every base 16-byte aligned).  One item is four input columns of a row pair: two 16-byte
// loads, two outputs (one 8-byte store, one 2-byte store).  With W / 4 items per row pair, item i writes outputs
// 2i, 2i + 1 — the output side is one flat float2 / uchar2 stream, and a wave's loads cover whole 64-byte pieces of two
// rows.  A thread walks items grid-stride two at a time and issues all four loads before the first use.  Backward is
// the mirror image: 8 + 2 bytes read, two 16-byte stores, so every element of dx is written exactly once.
// Scalar route (any even W, W = 2 included; any 4-byte aligned bases): one output per thread, grid-stride.
//
// No atomics, no workspace, no LDS; an element's value does not depend on the launch geometry.  Indexing is 64-bit.
#include "salun_common.h"

namespace {

struct Pick {
  float v;
  unsigned int k;
};

__device__ __forceinline__ Pick pick4(float a, float b, float c, float d) {
  Pick p{-INFINITY, 0u};
  if (a > p.v || a != a) { p.v = a; p.k = 0u; }
  if (b > p.v || b != b) { p.v = b; p.k = 1u; }
  if (c > p.v || c != c) { p.v = c; p.k = 2u; }
  if (d > p.v || d != d) { p.v = d; p.k = 3u; }
  return p;
}

__device__ __forceinline__ void fwd_item(const float4 top, const float4 bot, float2 *y2, uchar2 *i2, int64_t i) {
  const Pick l = pick4(top.x, top.y, bot.x, bot.y), r = pick4(top.z, top.w, bot.z, bot.w);
  y2[i] = make_float2(l.v, r.v);
  i2[i] = make_uchar2(static_cast<unsigned char>(l.k), static_cast<unsigned char>(r.k));
}

// items = NC * (H / 2) * (W / 4); w4 = W / 4.
__global__ __launch_bounds__(SALUN_BLOCK) void k_maxpool_fwd_vec(const float *__restrict__ x, float *__restrict__ y,
                                                                 uint8_t *__restrict__ idx, int64_t items, int w4) {
  const float4 *x4 = reinterpret_cast<const float4 *>(x);
  float2 *y2 = reinterpret_cast<float2 *>(y);
  uchar2 *i2 = reinterpret_cast<uchar2 *>(idx);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * SALUN_BLOCK;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * SALUN_BLOCK + threadIdx.x; i < items; i += 2 * stride) {
    const int64_t j = i + stride;
    const bool two = j < items;
    const int64_t ri = i / w4, rj = two ? j / w4 : ri;
    const int64_t ai = ri * (2 * static_cast<int64_t>(w4)) + (i - ri * w4);
    const int64_t aj = two ? rj * (2 * static_cast<int64_t>(w4)) + (j - rj * w4) : ai;
    const float4 ti = x4[ai], bi = x4[ai + w4];
    const float4 tj = x4[aj], bj = x4[aj + w4];  // (a repeat of item i when there is no second item: in range)
    fwd_item(ti, bi, y2, i2, i);
    if (two) fwd_item(tj, bj, y2, i2, j);
  }
}

// outs = NC * (H / 2) * (W / 2); w2 = W / 2.
__global__ __launch_bounds__(SALUN_BLOCK) void k_maxpool_fwd_scalar(const float *__restrict__ x, float *__restrict__ y,
                                                                    uint8_t *__restrict__ idx, int64_t outs, int w2) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * SALUN_BLOCK;
  for (int64_t o = static_cast<int64_t>(blockIdx.x) * SALUN_BLOCK + threadIdx.x; o < outs; o += stride) {
    const int64_t r = o / w2;
    const float *top = x + r * (4 * static_cast<int64_t>(w2)) + 2 * (o - r * w2);
    const float *bot = top + 2 * w2;
    const Pick p = pick4(top[0], top[1], bot[0], bot[1]);
    y[o] = p.v;
    idx[o] = static_cast<uint8_t>(p.k);
  }
}

__device__ __forceinline__ void bwd_item(const float2 g, const uchar2 k, float4 *dx4, int64_t a, int w4) {
  dx4[a] = make_float4(k.x == 0 ? g.x : 0.0f, k.x == 1 ? g.x : 0.0f, k.y == 0 ? g.y : 0.0f, k.y == 1 ? g.y : 0.0f);
  dx4[a + w4] = make_float4(k.x == 2 ? g.x : 0.0f, k.x == 3 ? g.x : 0.0f, k.y == 2 ? g.y : 0.0f, k.y == 3 ? g.y : 0.0f);
}

__global__ __launch_bounds__(SALUN_BLOCK) void k_maxpool_bwd_vec(const float *__restrict__ dy,
                                                                 const uint8_t *__restrict__ idx, float *__restrict__ dx,
                                                                 int64_t items, int w4) {
  const float2 *g2 = reinterpret_cast<const float2 *>(dy);
  const uchar2 *i2 = reinterpret_cast<const uchar2 *>(idx);
  float4 *dx4 = reinterpret_cast<float4 *>(dx);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * SALUN_BLOCK;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * SALUN_BLOCK + threadIdx.x; i < items; i += 2 * stride) {
    const int64_t j = i + stride;
    const bool two = j < items;
    const int64_t jj = two ? j : i;
    const float2 gi = g2[i], gj = g2[jj];
    const uchar2 ki = i2[i], kj = i2[jj];
    const int64_t ri = i / w4, rj = jj / w4;
    bwd_item(gi, ki, dx4, ri * (2 * static_cast<int64_t>(w4)) + (i - ri * w4), w4);
    if (two) bwd_item(gj, kj, dx4, rj * (2 * static_cast<int64_t>(w4)) + (jj - rj * w4), w4);
  }
}

__global__ __launch_bounds__(SALUN_BLOCK) void k_maxpool_bwd_scalar(const float *__restrict__ dy,
                                                                    const uint8_t *__restrict__ idx,
                                                                    float *__restrict__ dx, int64_t outs, int w2) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * SALUN_BLOCK;
  for (int64_t o = static_cast<int64_t>(blockIdx.x) * SALUN_BLOCK + threadIdx.x; o < outs; o += stride) {
    const int64_t r = o / w2;
    float *top = dx + r * (4 * static_cast<int64_t>(w2)) + 2 * (o - r * w2);
    float *bot = top + 2 * w2;
    const float g = dy[o];
    const unsigned int k = idx[o];
    top[0] = k == 0 ? g : 0.0f;
    top[1] = k == 1 ? g : 0.0f;
    bot[0] = k == 2 ? g : 0.0f;
    bot[1] = k == 3 ? g : 0.0f;
  }
}

// NC >= 1, H and W even and >= 2, and an element count that the 64-bit index arithmetic cannot overflow.
bool shape_ok(int64_t NC, int H, int W) {
  if (NC < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) return false;
  return NC <= (int64_t(1) << 62) / (static_cast<int64_t>(H) * W);
}

// ---- MaxPool2d(kernel 3, stride 2, padding 1), forward only: the pool behind the stem of an ImageNet-style ResNet.
// One output per thread, grid-stride.  The window is scanned row by row, left to right, from (-inf); positions in the
// padding are skipped (padding acts as -inf); a value is taken when it is greater than the running maximum or is NaN:
// F.max_pool2d's rule (first of equal maxima, NaN wins, +0 after -0 does not replace it).
__global__ __launch_bounds__(SALUN_BLOCK) void k_maxpool3x3s2_fwd(const float *__restrict__ x, float *__restrict__ y,
                                                                  int64_t outs, int H, int W, int OH, int OW) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * SALUN_BLOCK;
  const int64_t plane_out = static_cast<int64_t>(OH) * OW;
  for (int64_t o = static_cast<int64_t>(blockIdx.x) * SALUN_BLOCK + threadIdx.x; o < outs; o += stride) {
    const int64_t nc = o / plane_out;
    const int rem = static_cast<int>(o - nc * plane_out);
    const int oh = rem / OW, ow = rem - oh * OW;
    const float *xp = x + nc * (static_cast<int64_t>(H) * W);
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int ih = 2 * oh - 1 + r;
      if (ih < 0 || ih >= H) continue;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int iw = 2 * ow - 1 + s;
        if (iw < 0 || iw >= W) continue;
        const float v = xp[static_cast<int64_t>(ih) * W + iw];
        if (v > m || v != v) m = v;
      }
    }
    y[o] = m;
  }
}

}  // namespace

SALUN_EXPORT int salun_maxpool3x3s2_forward(const float *x, float *y, int64_t NC, int H, int W, salun_stream_t stream) {
  if (NC < 1 || H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20)) return SALUN_EINVAL;
  if (NC > (int64_t(1) << 62) / (static_cast<int64_t>(H) * W)) return SALUN_EINVAL;
  if (!x || !y || x == y || !salun_aligned4(x) || !salun_aligned4(y)) return SALUN_EINVAL;
  const int OH = (H + 1) / 2, OW = (W + 1) / 2;
  const int64_t outs = NC * OH * OW;
  hipLaunchKernelGGL(k_maxpool3x3s2_fwd, dim3(salun_grid_for(outs, SALUN_BLOCK)), dim3(SALUN_BLOCK), 0,
                     salun_hip_stream(stream), x, y, outs, H, W, OH, OW);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_maxpool2x2_forward(const float *x, float *y, uint8_t *idx, int64_t NC, int H, int W,
                                          salun_stream_t stream) {
  if (!shape_ok(NC, H, W) || !x || !y || !idx) return SALUN_EINVAL;
  if (!salun_aligned4(x) || !salun_aligned4(y)) return SALUN_EINVAL;
  hipStream_t st = salun_hip_stream(stream);
  const int64_t outs = NC * (H / 2) * (W / 2);
  if (W % 4 == 0 && salun_aligned16(x) && salun_aligned16(y) && salun_aligned16(idx)) {
    const int64_t items = outs / 2;
    hipLaunchKernelGGL(k_maxpool_fwd_vec, dim3(salun_grid_for(items, 2 * SALUN_BLOCK)), dim3(SALUN_BLOCK), 0, st, x, y,
                       idx, items, W / 4);
  } else {
    hipLaunchKernelGGL(k_maxpool_fwd_scalar, dim3(salun_grid_for(outs, SALUN_BLOCK)), dim3(SALUN_BLOCK), 0, st, x, y,
                       idx, outs, W / 2);
  }
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_maxpool2x2_backward(const float *dy, const uint8_t *idx, float *dx, int64_t NC, int H, int W,
                                           salun_stream_t stream) {
  if (!shape_ok(NC, H, W) || !dy || !idx || !dx || dx == dy) return SALUN_EINVAL;
  if (!salun_aligned4(dy) || !salun_aligned4(dx)) return SALUN_EINVAL;
  hipStream_t st = salun_hip_stream(stream);
  const int64_t outs = NC * (H / 2) * (W / 2);
  if (W % 4 == 0 && salun_aligned16(dy) && salun_aligned16(dx) && salun_aligned16(idx)) {
    const int64_t items = outs / 2;
    hipLaunchKernelGGL(k_maxpool_bwd_vec, dim3(salun_grid_for(items, 2 * SALUN_BLOCK)), dim3(SALUN_BLOCK), 0, st, dy,
                       idx, dx, items, W / 4);
  } else {
    hipLaunchKernelGGL(k_maxpool_bwd_scalar, dim3(salun_grid_for(outs, SALUN_BLOCK)), dim3(SALUN_BLOCK), 0, st, dy, idx,
                       dx, outs, W / 2);
  }
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}
