// salun_imgnorm.hip — uint8 HWC images to normalised fp32 CHW planes: transforms.ToTensor() then
// transforms.Normalize(mean, std), bit for bit.  gfx950 / CDNA4, wave64, compiled with -ffp-contract=off.
//
// An output depends on one byte and one channel only, so the whole operator is a 256 x C table:
//   table[c][u] = ((float(u) / 255.0f) - mean[c]) / std[c]
// with every step rounded to fp32 (ToTensor divides the fp32 image by 255; Normalize subtracts and divides by fp32
// tensors).  salun_u8_norm_table computes it on the HOST (IEEE fp32 division; no contraction) into host memory; the
// caller uploads it once and hands the device copy to every salun_u8_to_chw_norm call.  The kernel keeps the table in LDS
// and moves one pixel (C bytes in, C floats out, one per plane) per thread, grid-stride; plane stores are coalesced.
#include "salun_common.h"

namespace {

constexpr int MAX_C = SALUN_U8_NORM_MAX_C;

__global__ __launch_bounds__(SALUN_BLOCK) void k_u8_to_chw_norm(const uint8_t *__restrict__ src,
                                                                const float *__restrict__ table, float *__restrict__ dst,
                                                                int64_t pixels, int64_t HW, int C) {
  __shared__ float tab[MAX_C * 256];
  for (int i = threadIdx.x; i < C * 256; i += SALUN_BLOCK) tab[i] = table[i];
  __syncthreads();
  const int64_t stride = static_cast<int64_t>(gridDim.x) * SALUN_BLOCK;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * SALUN_BLOCK + threadIdx.x; i < pixels; i += stride) {
    const int64_t b = i / HW, hw = i - b * HW;
    const uint8_t *s = src + i * C;
    float *d = dst + b * C * HW + hw;
    for (int c = 0; c < C; ++c) d[c * HW] = tab[c * 256 + s[c]];
  }
}

}  // namespace

SALUN_EXPORT int salun_u8_norm_table(const float *mean, const float *std, int C, float *table) {
  if (!mean || !std || !table || C < 1 || C > MAX_C) return SALUN_EINVAL;
  for (int c = 0; c < C; ++c)
    for (int u = 0; u < 256; ++u) {
      volatile float t = static_cast<float>(u) / 255.0f;  // (volatile: each step is an fp32 number of its own)
      volatile float d = t - mean[c];
      table[c * 256 + u] = d / std[c];
    }
  return SALUN_OK;
}

SALUN_EXPORT int salun_u8_to_chw_norm(const uint8_t *src, const float *table, float *dst, int64_t B, int H, int W, int C,
                                      salun_stream_t stream) {
  if (B < 1 || H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20) || C < 1 || C > MAX_C) return SALUN_EINVAL;
  if (B > (int64_t(1) << 60) / (static_cast<int64_t>(H) * W * C)) return SALUN_EINVAL;
  if (!src || !table || !dst || !salun_aligned4(table) || !salun_aligned4(dst)) return SALUN_EINVAL;
  const int64_t HW = static_cast<int64_t>(H) * W, pixels = B * HW;
  hipLaunchKernelGGL(k_u8_to_chw_norm, dim3(salun_grid_for(pixels, SALUN_BLOCK)), dim3(SALUN_BLOCK), 0,
                     salun_hip_stream(stream), src, table, dst, pixels, HW, C);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

// ---- the same operator on a WINDOW of the source: torchvision's preset is resize -> centre crop -> normalise, and the
// crop is an address offset here, not a copy.  One output pixel per thread, grid-stride; the table is the one above.
namespace {

__global__ __launch_bounds__(SALUN_BLOCK) void k_u8_crop_to_chw_norm(const uint8_t *__restrict__ src,
                                                                     const float *__restrict__ table,
                                                                     float *__restrict__ dst, int64_t pixels, int H, int W,
                                                                     int C, int top, int left, int OH, int OW) {
  __shared__ float tab[MAX_C * 256];
  for (int i = threadIdx.x; i < C * 256; i += SALUN_BLOCK) tab[i] = table[i];
  __syncthreads();
  const int64_t OHW = static_cast<int64_t>(OH) * OW;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * SALUN_BLOCK;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * SALUN_BLOCK + threadIdx.x; i < pixels; i += stride) {
    const int64_t b = i / OHW, hw = i - b * OHW;
    const int oh = static_cast<int>(hw / OW), ow = static_cast<int>(hw - static_cast<int64_t>(oh) * OW);
    const uint8_t *s = src + ((b * H + (top + oh)) * W + (left + ow)) * C;
    float *d = dst + b * C * OHW + hw;
    for (int c = 0; c < C; ++c) d[c * OHW] = tab[c * 256 + s[c]];
  }
}

}  // namespace

SALUN_EXPORT int salun_u8_crop_to_chw_norm(const uint8_t *src, const float *table, float *dst, int64_t B, int H, int W,
                                           int C, int top, int left, int OH, int OW, salun_stream_t stream) {
  if (B < 1 || H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20) || C < 1 || C > MAX_C) return SALUN_EINVAL;
  if (B > (int64_t(1) << 60) / (static_cast<int64_t>(H) * W * C)) return SALUN_EINVAL;
  if (top < 0 || left < 0 || OH < 1 || OW < 1 || OH > H || OW > W || top > H - OH || left > W - OW) return SALUN_EINVAL;
  if (!src || !table || !dst || !salun_aligned4(table) || !salun_aligned4(dst)) return SALUN_EINVAL;
  const int64_t pixels = B * OH * OW;
  hipLaunchKernelGGL(k_u8_crop_to_chw_norm, dim3(salun_grid_for(pixels, SALUN_BLOCK)), dim3(SALUN_BLOCK), 0,
                     salun_hip_stream(stream), src, table, dst, pixels, H, W, C, top, left, OH, OW);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}
