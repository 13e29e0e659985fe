// salun_gn_split.hip — K28: GroupNorm (+ SiLU) forward for groups too large for one workgroup.
//
// salun_gn_forward (salun_norm.hip) gives a whole (image, group) to one workgroup: at the first level of the
// Stable-Diffusion VAE encoder (128 channels in 32 groups at 512 x 512: 2^20 values per group) that is 32 workgroups
// for one image on a 256-CU chip, and the shape is outside its domain anyway.  Here a group's cpg * HW contiguous values
// are cut into S slabs of `slab` float4s and the work is two launches over a grid of N * G * S:
//   phase 1  workgroup (n, g, s) reduces slab s to one (sum, sum of squares) pair of doubles in the workspace;
//   phase 2  every workgroup folds its group's S pairs in index order (so all S hold the same mean / rstd bits), slab 0
//            writes save_mean / save_rstd, and each applies gamma, beta and SiLU over its own slab.
// No atomics, no ticket: the kernel boundary is the barrier.  The arithmetic is k_gn_fwd's re-read mode statement for
// statement: a lane adds float4 trees into fp32 accumulators and folds them into doubles every SALUN_GN_SPLIT_FLUSH
// float4s, the block sum is in double, mu = t1 / L, var = max(t2 / L - mu^2, 0), rstd = (float)(1 / sqrt(var + eps)),
// a = rstd * gamma[c], b = beta[c] - mu * a, o = x * a + b (the file is compiled without contraction), SiLU =
// o * (1 / (1 + expf(-o))).  All loads and stores of x and y are 16 bytes.  S depends on cpg * HW and slab_vec4 only,
// never on N or the device: the same inputs give the same bits and an image does not depend on the rest of its batch.
#include "salun_device.h"

namespace {

// float4s per slab when the caller leaves the choice to us: 8 per lane.  The smallest GroupNorm of the VAE encoder at
// 512 x 512 (512 channels in 32 groups at 64 x 64: 16384 float4s per group) then gives 32 * 8 = 256 workgroups for one
// image, one per CU; every larger map gives more.
constexpr int GNS_AUTO_SLAB = 2048;

struct GnsPlan {
  int cpg;
  int64_t nvec;   // float4s per group
  int64_t slab;   // float4s per slab
  int64_t S;      // slabs per group
  int64_t grid;   // N * G * S
};

inline bool gns_plan(int N, int C, int64_t HW, int G, int slab_vec4, GnsPlan *p) {
  if (N < 1 || C < 1 || G < 1 || C % G != 0 || HW < 4 || (HW & 3) != 0 || slab_vec4 < 0) return false;
  p->cpg = C / G;
  if (HW >= ((int64_t)1 << 31) || (int64_t)p->cpg * HW >= ((int64_t)1 << 31)) return false;
  p->nvec = (int64_t)p->cpg * HW / 4;
  p->slab = slab_vec4 > 0 ? slab_vec4 : GNS_AUTO_SLAB;
  p->S = (p->nvec + p->slab - 1) / p->slab;
  p->grid = (int64_t)N * G * p->S;
  return p->grid <= 0x7fffffff;
}

__global__ __launch_bounds__(256) void k_gns_reduce(const float *__restrict__ x, double *__restrict__ part, int C,
                                                    int HW, int G, int S, int slab, int nvec) {
  __shared__ double lds[4];
  const int ng = blockIdx.x / S, s = blockIdx.x - ng * S;
  const int cpg = C / G;
  const int n = ng / G, g = ng - n * G;
  const size_t base = ((size_t)n * C + (size_t)g * cpg) * (size_t)HW;
  const float4 *xv = reinterpret_cast<const float4 *>(x + base);
  const int lo = s * slab;                      // s * slab < nvec < 2^29
  const int hi = nvec - lo < slab ? nvec : lo + slab;
  float s1 = 0.f, s2 = 0.f;
  double d1 = 0.0, d2 = 0.0;
  int it = 0;
  for (int e = lo + (int)threadIdx.x; e < hi; e += 256, ++it) {
    const float4 t = xv[e];
    s1 += (t.x + t.y) + (t.z + t.w);
    s2 += (t.x * t.x + t.y * t.y) + (t.z * t.z + t.w * t.w);
    if ((it & (SALUN_GN_SPLIT_FLUSH - 1)) == SALUN_GN_SPLIT_FLUSH - 1) { d1 += s1; d2 += s2; s1 = 0.f; s2 = 0.f; }
  }
  d1 += s1; d2 += s2;
  const double t1 = salun_block_sum(d1, lds);
  const double t2 = salun_block_sum(d2, lds);
  if (threadIdx.x == 0) {
    part[2 * (size_t)blockIdx.x] = t1;
    part[2 * (size_t)blockIdx.x + 1] = t2;
  }
}

// x and y may be the same buffer: no __restrict__ on them; a lane reads a float4 before it writes it.
template <bool SILU>
__global__ __launch_bounds__(256) void k_gns_apply(const float *x, float *y, const float *__restrict__ gamma,
                                                   const float *__restrict__ beta, const double *__restrict__ part,
                                                   float *__restrict__ mean, float *__restrict__ rstd, int C, int HW,
                                                   int G, int S, int slab, int nvec, float eps) {
  __shared__ float st[2];
  const int ng = blockIdx.x / S, s = blockIdx.x - ng * S;
  const int cpg = C / G;
  const int n = ng / G, g = ng - n * G;
  if (threadIdx.x == 0) {
    const double *p = part + 2 * (size_t)ng * S;
    double t1 = 0.0, t2 = 0.0;
    for (int j = 0; j < S; ++j) { t1 += p[2 * j]; t2 += p[2 * j + 1]; }
    const int L = cpg * HW;
    const double mu = t1 / L;
    double var = t2 / L - mu * mu;
    if (var < 0.0) var = 0.0;
    st[0] = (float)mu;
    st[1] = (float)(1.0 / sqrt(var + (double)eps));
    if (s == 0) {
      mean[ng] = st[0];
      rstd[ng] = st[1];
    }
  }
  __syncthreads();
  const float mu = st[0], rs = st[1];
  const int hw4 = HW >> 2;
  const size_t base = ((size_t)n * C + (size_t)g * cpg) * (size_t)HW;
  const float4 *xv = reinterpret_cast<const float4 *>(x + base);
  float4 *yv = reinterpret_cast<float4 *>(y + base);
  const int lo = s * slab;
  const int hi = nvec - lo < slab ? nvec : lo + slab;
  for (int e = lo + (int)threadIdx.x; e < hi; e += 256) {
    const float4 t = xv[e];
    const int c = g * cpg + e / hw4;
    const float a = rs * gamma[c];
    const float b = beta[c] - mu * a;
    float4 o;
    o.x = t.x * a + b; o.y = t.y * a + b; o.z = t.z * a + b; o.w = t.w * a + b;
    if (SILU) {
      o.x = o.x * salun_sigmoid(o.x); o.y = o.y * salun_sigmoid(o.y);
      o.z = o.z * salun_sigmoid(o.z); o.w = o.w * salun_sigmoid(o.w);
    }
    yv[e] = o;
  }
}

}  // namespace

SALUN_EXPORT int salun_gn_split_slabs(int C, int64_t HW, int G, int slab_vec4) {
  GnsPlan p;
  if (!gns_plan(1, C, HW, G, slab_vec4, &p)) return 0;
  return (int)p.S;
}

SALUN_EXPORT size_t salun_gn_split_workspace_bytes(int N, int C, int64_t HW, int G, int slab_vec4) {
  GnsPlan p;
  if (!gns_plan(N, C, HW, G, slab_vec4, &p)) return 0;
  return (size_t)p.grid * 2 * sizeof(double);
}

SALUN_EXPORT int salun_gn_split_forward(const float *x, float *y, const float *gamma, const float *beta,
                                        float *save_mean, float *save_rstd, int N, int C, int64_t HW, int G, double eps,
                                        int silu, int slab_vec4, void *ws, size_t ws_bytes, salun_stream_t stream) {
  GnsPlan p;
  if (!x || !y || !gamma || !beta || !save_mean || !save_rstd || !ws || !gns_plan(N, C, HW, G, slab_vec4, &p))
    return SALUN_EINVAL;
  if (!salun_aligned16(x) || !salun_aligned16(y) || (reinterpret_cast<uintptr_t>(ws) & 7u) != 0) return SALUN_EINVAL;
  if (ws_bytes < (size_t)p.grid * 2 * sizeof(double)) return SALUN_EINVAL;
  hipStream_t st = salun_hip_stream(stream);
  double *part = static_cast<double *>(ws);
  const int S = (int)p.S, slab = (int)(p.slab < p.nvec ? p.slab : p.nvec), nvec = (int)p.nvec;
  hipLaunchKernelGGL(k_gns_reduce, dim3((unsigned)p.grid), dim3(256), 0, st, x, part, C, (int)HW, G, S, slab, nvec);
  SALUN_LAUNCH_CHECK();
  if (silu)
    hipLaunchKernelGGL(k_gns_apply<true>, dim3((unsigned)p.grid), dim3(256), 0, st, x, y, gamma, beta, part, save_mean,
                       save_rstd, C, (int)HW, G, S, slab, nvec, (float)eps);
  else
    hipLaunchKernelGGL(k_gns_apply<false>, dim3((unsigned)p.grid), dim3(256), 0, st, x, y, gamma, beta, part, save_mean,
                       save_rstd, C, (int)HW, G, S, slab, nvec, (float)eps);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}
