// salun_resample.hip — K26: antialiased bilinear resample of uint8 NHWC images, bit-identical to Pillow's 8-bit path
// (PIL.Image.resize(size, Image.BILINEAR) == torchvision's transforms.Resize on a PIL image).  gfx950 / CDNA4, wave64.
// The data path of the STL-10 diffusion runs (96 x 96 -> 64 x 64, once, on the device).
//
// Pillow resamples separably, horizontal pass first, in integer arithmetic: per axis a table of (first tap, tap count,
// 22-bit fixed-point weights) per output sample, an output byte is clip8((2^21 + sum k * pixel) >> 22), and the
// horizontal result is a uint8 image that the vertical pass reads.  Only the TABLES involve floating point; they are
// computed here on the host in doubles, statement by statement as Pillow's precompute_coeffs / normalize_coeffs_8bpc
// do (this file is compiled with -ffp-contract=off: a fused multiply-add in `center - support + 0.5` or in the weight
// could move a k by one), uploaded once per (device, in, out) pair and kept.  The pixel work is integer and exact.
//
// One launch.  A workgroup owns a band of output rows [oy0, oy1) of one image.  Because first-tap and end-tap indices
// are non-decreasing in the output index, the source rows the band needs are the contiguous range
// [ymin[oy0], ymin[oy1 - 1] + n[oy1 - 1]).  Phase 1 resamples those rows horizontally into LDS (rows x OW x C bytes),
// phase 2 reads LDS column-wise and writes the band.  The intermediate never reaches memory.  The band height is the
// largest of 16, 8, 4, 2, 1 whose worst band fits SALUN_RESAMPLE_MAX_LDS; a size pair whose one-row band does not fit
// (a strong downscale of a wide image) is refused.  Byte loads and stores: no alignment is asked of either pointer.
// No atomics, no workspace; a byte of dst does not depend on the launch geometry.  Indexing into src / dst is 64-bit.
#include "salun_common.h"

#include <math.h>
#include <mutex>
#include <vector>

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;  // Pillow's PRECISION_BITS
constexpr int kMaxBand = 16;
constexpr size_t kMaxCached = 64;

// ---- host: Pillow's coefficient table of one axis ----------------------------------------------------------------
// layout (int32): [0, out) first tap, [out, 2 out) tap count, then out rows of ksize weights (unused tail 0).
struct AxisTable {
  int in = 0, out = 0, ksize = 0;
  std::vector<int32_t> v;
  int first(int i) const { return v[i]; }
  int count(int i) const { return v[out + i]; }
};

double bilinear_filter(double x) {
  if (x < 0.0) x = -x;
  if (x < 1.0) return 1.0 - x;
  return 0.0;
}

AxisTable make_axis(int in, int out) {
  AxisTable t;
  t.in = in;
  t.out = out;
  const double scale = static_cast<double>(in) / out;
  double filterscale = scale;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = 1.0 * filterscale;
  t.ksize = static_cast<int>(ceil(support)) * 2 + 1;
  t.v.assign(static_cast<size_t>(out) * (2 + t.ksize), 0);
  std::vector<double> w(t.ksize);
  const double ss = 1.0 / filterscale;
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = static_cast<int>(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = static_cast<int>(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    for (int x = 0; x < xmax; ++x) {
      w[x] = bilinear_filter((x + xmin - center + 0.5) * ss);
      ww += w[x];
    }
    int32_t *k = &t.v[static_cast<size_t>(2) * out + static_cast<size_t>(xx) * t.ksize];
    for (int x = 0; x < xmax; ++x) {
      if (ww != 0.0) w[x] /= ww;
      k[x] = w[x] < 0.0 ? static_cast<int32_t>(-0.5 + w[x] * (1 << kPrecisionBits))
                        : static_cast<int32_t>(0.5 + w[x] * (1 << kPrecisionBits));
    }
    t.v[xx] = xmin;
    t.v[out + xx] = xmax;
  }
  return t;
}

// source rows of the tallest band when the output rows go in bands of `band`
int band_rows(const AxisTable &ty, int band) {
  int worst = 0;
  for (int oy0 = 0; oy0 < ty.out; oy0 += band) {
    const int last = (oy0 + band < ty.out ? oy0 + band : ty.out) - 1;
    const int rows = ty.first(last) + ty.count(last) - ty.first(oy0);
    if (rows > worst) worst = rows;
  }
  return worst;
}

bool shape_ok(int H, int W, int C, int OH, int OW) {
  const int m = SALUN_RESAMPLE_MAX_SIDE;
  return (C == 1 || C == 3 || C == 4) && H >= 1 && W >= 1 && OH >= 1 && OW >= 1 && H <= m && W <= m && OH <= m && OW <= m;
}

// -> band height (0: refused) and the LDS bytes of its tallest band
int pick_band(const AxisTable &ty, int OW, int C, size_t *lds) {
  for (int band = kMaxBand; band >= 1; band >>= 1) {
    const size_t bytes = static_cast<size_t>(band_rows(ty, band)) * OW * C;
    if (bytes <= SALUN_RESAMPLE_MAX_LDS) {
      *lds = bytes;
      return band;
    }
  }
  *lds = 0;
  return 0;
}

// ---- host: device copies of the tables, one per (device, in, out), made once -------------------------------------
struct Cached {
  int dev, in, out, ksize;
  int32_t *d;
  AxisTable host;
};
std::mutex g_mu;
std::vector<Cached> g_cache;

// Caller holds g_mu.  nullptr: the allocation or the copy failed.  `keep`: a table this call must not evict.
const Cached *table_for(int in, int out, const int32_t *keep = nullptr) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  for (const Cached &c : g_cache)
    if (c.dev == dev && c.in == in && c.out == out) return &c;
  if (g_cache.size() >= kMaxCached) {  // (hipFree waits for the device: no kernel still reads the evicted table)
    const size_t victim = g_cache.front().d == keep ? 1 : 0;
    (void)hipFree(g_cache[victim].d);
    g_cache.erase(g_cache.begin() + victim);
  }
  Cached c{dev, in, out, 0, nullptr, make_axis(in, out)};
  c.ksize = c.host.ksize;
  const size_t bytes = c.host.v.size() * sizeof(int32_t);
  if (hipMalloc(reinterpret_cast<void **>(&c.d), bytes) != hipSuccess) return nullptr;
  if (hipMemcpy(c.d, c.host.v.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {  // blocks: done before any launch
    (void)hipFree(c.d);
    return nullptr;
  }
  g_cache.push_back(std::move(c));
  return &g_cache.back();
}

// ---- device -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint8_t clip8(int v) {
  v >>= kPrecisionBits;
  return static_cast<uint8_t>(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// grid.x = B * nbands; dynamic LDS = (rows of the tallest band) * OW * C bytes.
template <int C>
__global__ __launch_bounds__(SALUN_BLOCK) void k_resample_u8(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                             const int32_t *__restrict__ tx,
                                                             const int32_t *__restrict__ ty, int H, int W, int OH, int OW,
                                                             int ksx, int ksy, int band, int nbands) {
  extern __shared__ uint8_t hrow[];  // [rows][OW][C]
  const int64_t img = blockIdx.x / nbands;
  const int oy0 = static_cast<int>(blockIdx.x - img * nbands) * band;
  const int oy1 = oy0 + band < OH ? oy0 + band : OH;
  const int r0 = ty[oy0];
  const int rows = ty[oy1 - 1] + ty[OH + oy1 - 1] - r0;
  const uint8_t *s = src + img * (static_cast<int64_t>(H) * W * C);
  uint8_t *d = dst + img * (static_cast<int64_t>(OH) * OW * C);

  // phase 1: source rows [r0, r0 + rows) -> hrow, each resampled to OW columns
  for (int i = threadIdx.x; i < rows * OW; i += SALUN_BLOCK) {
    const int r = i / OW, ox = i - r * OW;
    const int xmin = tx[ox], n = tx[OW + ox];
    const int32_t *k = tx + 2 * OW + ox * ksx;
    const uint8_t *p = s + (static_cast<int64_t>(r0 + r) * W + xmin) * C;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (kPrecisionBits - 1);
    for (int t = 0; t < n; ++t) {
      const int kk = k[t];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += kk * static_cast<int>(p[t * C + c]);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) hrow[i * C + c] = clip8(acc[c]);
  }
  __syncthreads();

  // phase 2: output rows [oy0, oy1) from hrow
  for (int i = threadIdx.x; i < (oy1 - oy0) * OW; i += SALUN_BLOCK) {
    const int q = i / OW, ox = i - q * OW, oy = oy0 + q;
    const int ymin = ty[oy], n = ty[OH + oy];
    const int32_t *k = ty + 2 * OH + oy * ksy;
    const uint8_t *p = hrow + (static_cast<int64_t>(ymin - r0) * OW + ox) * C;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (kPrecisionBits - 1);
    for (int t = 0; t < n; ++t) {
      const int kk = k[t];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += kk * static_cast<int>(p[t * OW * C + c]);
    }
    uint8_t *o = d + (static_cast<int64_t>(oy) * OW + ox) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = clip8(acc[c]);
  }
}

}  // namespace

SALUN_EXPORT size_t salun_resample_u8_lds_bytes(int H, int W, int C, int OH, int OW) {
  if (!shape_ok(H, W, C, OH, OW)) return 0;
  size_t lds = 0;
  (void)pick_band(make_axis(H, OH), OW, C, &lds);
  return lds;
}

SALUN_EXPORT int salun_resample_u8_table(int in, int out, int32_t *table, size_t n_ints, int *ksize) {
  const int m = SALUN_RESAMPLE_MAX_SIDE;
  if (in < 1 || out < 1 || in > m || out > m || !ksize) return SALUN_EINVAL;
  const AxisTable t = make_axis(in, out);
  *ksize = t.ksize;
  if (!table) return SALUN_OK;
  if (n_ints < t.v.size()) return SALUN_ENOSPC;
  for (size_t i = 0; i < t.v.size(); ++i) table[i] = t.v[i];
  return SALUN_OK;
}

SALUN_EXPORT int salun_resample_u8(const uint8_t *src, uint8_t *dst, int64_t B, int H, int W, int C, int OH, int OW,
                                   salun_stream_t stream) {
  if (!shape_ok(H, W, C, OH, OW) || B < 1 || !src || !dst || src == dst) return SALUN_EINVAL;
  std::lock_guard<std::mutex> lock(g_mu);
  const Cached *cy = table_for(H, OH);
  if (!cy) return SALUN_EIO;
  size_t lds = 0;
  const int band = pick_band(cy->host, OW, C, &lds);
  if (band == 0) return SALUN_EINVAL;
  const int nbands = (OH + band - 1) / band;
  if (B > INT32_MAX / nbands) return SALUN_EINVAL;
  const int32_t *ty = cy->d;  // (table_for may move the vector's elements; the device pointers stay)
  const int ksy = cy->ksize;
  const Cached *cx = table_for(W, OW, ty);
  if (!cx) return SALUN_EIO;
  const int32_t *tx = cx->d;
  const int ksx = cx->ksize;
  hipStream_t st = salun_hip_stream(stream);
  const dim3 grid(static_cast<unsigned>(B * nbands)), block(SALUN_BLOCK);
  if (C == 1)
    hipLaunchKernelGGL(k_resample_u8<1>, grid, block, lds, st, src, dst, tx, ty, H, W, OH, OW, ksx, ksy, band, nbands);
  else if (C == 3)
    hipLaunchKernelGGL(k_resample_u8<3>, grid, block, lds, st, src, dst, tx, ty, H, W, OH, OW, ksx, ksy, band, nbands);
  else
    hipLaunchKernelGGL(k_resample_u8<4>, grid, block, lds, st, src, dst, tx, ty, H, W, OH, OW, ksx, ksy, band, nbands);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}
