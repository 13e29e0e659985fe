// salun_ff.hip — K18: Fisher forgetting (`fisher_new`, reference Classification/unlearn/fisher.py:50-114) from ONE
// eval-mode backward over the activations per batch of 32.  For class tangent y the batch gradient of
// a layer is linear in that layer's output gradient dy_y, so the reference's C full backwards per batch become C
// "groups" of a batched dy [G*B, ...] that all share the layer input x [B, ...]:
//   K18a conv      F[k,c,r,s] += sum_g w_g (sum_{i in g, pix} dy[k, pix] x[c, pix + (r,s)])^2
//                  — each group's sum is the package's backward-weight kernel (salun_conv.hip: conv_wgrad_v, the ring
//                    kernel, conv_wgrad_1x1, conv_wgrad_smallc; MFMA main loops, fixed-order partial reduce) writing
//                    into a per-group slot of the workspace; one epilogue squares, weights and adds the G slots in
//                    group order.  Linear weights: K18c, the same sums with P = Q = 1.
//   K18b vectors   F_beta[c] += sum_g w_g (sum_{i in g, pix} dy)^2,  F_gamma[c] += sum_g w_g (sum dy x^)^2
//                  (conv / Linear bias, eval BatchNorm with x^ from the running statistics)
//   K18d apply     var from F by the reference's get_mean_var rules (dim-1 mean, class-row override, x10), then
//                  p = mu + sqrt(var) z in place, z = the counter-based normal of salun_fill_normal at the flat index.
// No group sum is squared before its reduction is complete; every reduction runs in a fixed order and there are no
// float atomics, so two launches on the same inputs give bit-identical results.
#include "salun_device.h"

namespace {

// F[e] += sum_g w[g] gs[g * n + e]^2, g in increasing order, fp64      (float4 path: n % 4 == 0, all bases aligned)
__global__ __launch_bounds__(SALUN_BLOCK) void k_ff_sq_acc4(const float *__restrict__ gs, const float *__restrict__ w,
                                                            int G, int64_t n, float *__restrict__ F) {
  const int64_t n4 = n >> 2;
  for (int64_t v = (int64_t)blockIdx.x * SALUN_BLOCK + threadIdx.x; v < n4; v += (int64_t)gridDim.x * SALUN_BLOCK) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    const float4 *src = reinterpret_cast<const float4 *>(gs) + v;
    int g = 0;
    for (; g + 4 <= G; g += 4) {  // four independent loads in flight per step
      float4 s[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) s[u] = src[(int64_t)(g + u) * n4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double wg = w[g + u];
        a0 += wg * ((double)s[u].x * s[u].x);
        a1 += wg * ((double)s[u].y * s[u].y);
        a2 += wg * ((double)s[u].z * s[u].z);
        a3 += wg * ((double)s[u].w * s[u].w);
      }
    }
    for (; g < G; ++g) {
      const float4 s = src[(int64_t)g * n4];
      const double wg = w[g];
      a0 += wg * ((double)s.x * s.x);
      a1 += wg * ((double)s.y * s.y);
      a2 += wg * ((double)s.z * s.z);
      a3 += wg * ((double)s.w * s.w);
    }
    float4 f = reinterpret_cast<float4 *>(F)[v];
    f.x += (float)a0; f.y += (float)a1; f.z += (float)a2; f.w += (float)a3;
    reinterpret_cast<float4 *>(F)[v] = f;
  }
}

__global__ __launch_bounds__(SALUN_BLOCK) void k_ff_sq_acc(const float *__restrict__ gs, const float *__restrict__ w,
                                                           int G, int64_t n, float *__restrict__ F) {
  for (int64_t e = (int64_t)blockIdx.x * SALUN_BLOCK + threadIdx.x; e < n; e += (int64_t)gridDim.x * SALUN_BLOCK) {
    double a = 0.0;
    for (int g = 0; g < G; ++g) {
      const double s = gs[(int64_t)g * n + e];
      a += (double)w[g] * (s * s);
    }
    F[e] += (float)a;
  }
}

// Group sums of one channel: block (c, g) reduces dy (and dy * x^ when x is given) of channel c over the B samples of
// group g and all HW pixels, fp64, fixed tree; part[(g * C + c) * 2 + {0: beta, 1: gamma}]
__global__ __launch_bounds__(SALUN_BLOCK) void k_ff_vec_partial(const float *__restrict__ x, const float *__restrict__ dy,
                                                                const float *__restrict__ rm, const float *__restrict__ rv,
                                                                double eps, int B, int C, int HW,
                                                                double *__restrict__ part) {
  __shared__ double lds[4];
  const int c = blockIdx.x, g = blockIdx.y;
  const int64_t m = (int64_t)B * HW, CHW = (int64_t)C * HW;
  const float *d = dy + (int64_t)g * B * CHW + (int64_t)c * HW;
  double tb = 0.0, tg = 0.0;
  if (x) {
    const float *xs = x + (int64_t)c * HW;
    const double mean = rm[c], inv = 1.0 / sqrt((double)rv[c] + eps);
    for (int64_t e = threadIdx.x; e < m; e += SALUN_BLOCK) {
      const int64_t i = e / HW, q = e - i * HW;
      const double v = d[i * CHW + q];
      tb += v;
      tg += v * (((double)xs[i * CHW + q] - mean) * inv);
    }
  } else {
    for (int64_t e = threadIdx.x; e < m; e += SALUN_BLOCK) {
      const int64_t i = e / HW, q = e - i * HW;
      tb += d[i * CHW + q];
    }
  }
  const double sb = salun_block_sum(tb, lds);
  const double sg = x ? salun_block_sum(tg, lds) : 0.0;
  if (threadIdx.x == 0) {
    part[((int64_t)g * C + c) * 2 + 0] = sb;
    part[((int64_t)g * C + c) * 2 + 1] = sg;
  }
}

// F_beta[c] += sum_g w_g part_beta^2, F_gamma[c] += sum_g w_g part_gamma^2 (either may be NULL), g in increasing order
__global__ __launch_bounds__(SALUN_BLOCK) void k_ff_vec_finish(const double *__restrict__ part, const float *__restrict__ w,
                                                               int G, int C, float *__restrict__ Fg,
                                                               float *__restrict__ Fb) {
  const int c = blockIdx.x * SALUN_BLOCK + threadIdx.x;
  if (c >= C) return;
  double ab = 0.0, ag = 0.0;
  for (int g = 0; g < G; ++g) {
    const double sb = part[((int64_t)g * C + c) * 2 + 0], sg = part[((int64_t)g * C + c) * 2 + 1];
    const double wg = w[g];
    ab += wg * (sb * sb);
    ag += wg * (sg * sg);
  }
  if (Fb) Fb[c] += (float)ab;
  if (Fg) Fg[c] += (float)ag;
}

// Linear weight: F[m, k] += sum_g w_g (sum_{i < B} dy[g*B + i, m] x[i, k])^2      one thread per (m, k), fp64
__global__ __launch_bounds__(SALUN_BLOCK) void k_ff_linear_sq(const float *__restrict__ x, const float *__restrict__ dy,
                                                              const float *__restrict__ w, int G, int B, int M, int K,
                                                              float *__restrict__ F) {
  const int64_t t = (int64_t)blockIdx.x * SALUN_BLOCK + threadIdx.x;
  if (t >= (int64_t)M * K) return;
  const int m = static_cast<int>(t / K), k = static_cast<int>(t - (int64_t)m * K);
  double a = 0.0;
  for (int g = 0; g < G; ++g) {
    const float *d = dy + (int64_t)g * B * M + m;
    double s0 = 0.0, s1 = 0.0;  // two chains: loads of sample i + 1 issue before sample i's product is added
    int i = 0;
    for (; i + 2 <= B; i += 2) {
      const float d0 = d[(int64_t)i * M], d1 = d[(int64_t)(i + 1) * M];
      const float x0 = x[(int64_t)i * K + k], x1 = x[(int64_t)(i + 1) * K + k];
      s0 += (double)d0 * x0;
      s1 += (double)d1 * x1;
    }
    if (i < B) s0 += (double)d[(int64_t)i * M] * x[(int64_t)i * K + k];
    const double s = s0 + s1;
    a += (double)w[g] * (s * s);
  }
  F[t] += (float)a;
}

// ---------------------------------------------------------------------------------------------- K18d apply
// table row per parameter (int64): offset, n0 = shape[0], d1 = shape[1] (1 for 1-D), inner = prod(shape[2:]),
// flags, row (class row to override, -1 none), first tile.  A tile is one dim-0 row of a multi-dimensional parameter
// (the dim-1 mean lives inside it) or 256 elements of a 1-D one.
constexpr int FF_TAB = 7;
constexpr int64_t FF_CLASSROW = 1;  // shape[0] == num_classes: clamp at 1e2 and x10
constexpr int64_t FF_MULTI = 2;     // ndim > 1: var replaced by its mean over dim 1

__device__ __forceinline__ float ff_var_elem(float f, float nb, float alpha, bool classrow) {
  float v = 1.0f / (f / nb + 1e-8f);  // grad2_acc /= len(loader), then 1 / (grad2_acc + 1e-8)
  v = fminf(v, 1e3f);
  if (classrow) v = fminf(v, 1e2f);
  return alpha * v;
}

__global__ __launch_bounds__(SALUN_BLOCK) void k_ff_apply(float *__restrict__ p, const float *__restrict__ F,
                                                          const int64_t *__restrict__ tab, int nparam, int64_t ntiles,
                                                          float nb, float alpha, uint64_t seed) {
  __shared__ double part[SALUN_BLOCK];
  __shared__ float varc[SALUN_BLOCK];
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int lo = 0, hi = nparam - 1;  // last parameter whose first tile <= tile
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (tab[mid * FF_TAB + 6] <= tile) lo = mid; else hi = mid - 1;
    }
    const int64_t *t = tab + lo * FF_TAB;
    const int64_t off = t[0], n0 = t[1], d1 = t[2], inner = t[3], flags = t[4], row = t[5], t0 = t[6];
    const bool classrow = (flags & FF_CLASSROW) != 0;
    if (!(flags & FF_MULTI)) {  // 1-D: element-wise; x10 always (last layer or BatchNorm)
      const int64_t e = (tile - t0) * SALUN_BLOCK + threadIdx.x;
      if (e < n0) {
        const int64_t idx = off + e;
        float v = ff_var_elem(F[idx], nb, alpha, classrow);
        float mu = p[idx];
        if (e == row) { mu = 0.0f; v = 1e-4f; }
        v = v * 10.0f;
        p[idx] = mu + sqrtf(v) * salun_ih12(seed, (uint64_t)idx);
      }
      continue;
    }
    const int64_t a = tile - t0, base = off + a * d1 * inner, len = d1 * inner;
    const int js = SALUN_BLOCK / (int)inner;  // threads per column (inner <= SALUN_BLOCK, checked on the host)
    double s = 0.0;
    if (threadIdx.x < js * inner) {
      const int r = threadIdx.x % (int)inner, j0 = threadIdx.x / (int)inner;
      for (int64_t j = j0; j < d1; j += js) s += (double)ff_var_elem(F[base + j * inner + r], nb, alpha, classrow);
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < inner) {
      double m = 0.0;
      for (int q = 0; q < js; ++q) m += part[q * inner + threadIdx.x];
      float v = (float)(m / (double)d1);
      if (a == row) v = 1e-4f;
      if (classrow) v = v * 10.0f;
      varc[threadIdx.x] = sqrtf(v);
    }
    __syncthreads();
    for (int64_t e = threadIdx.x; e < len; e += SALUN_BLOCK) {
      const int64_t idx = base + e;
      const float mu = (a == row) ? 0.0f : p[idx];
      p[idx] = mu + varc[e % inner] * salun_ih12(seed, (uint64_t)idx);
    }
    __syncthreads();  // part / varc are reused by the next tile
  }
}

}  // namespace

// ================================================================== C-ABI =======
SALUN_EXPORT size_t salun_ff_conv_sq_workspace_bytes(int G, int B, int C, int K, int R, int P, int Q) {
  if (G < 1 || B < 1 || C < 1 || K < 1 || R < 1 || P < 1 || Q < 1) return 0;
  const size_t wg = salun_conv2d_wgrad_workspace_bytes(B, C, K, R, P, Q);
  if (wg == 0) return 0;
  return align256(sizeof(float) * (size_t)G * K * C * R * R) + wg;
}

SALUN_EXPORT int salun_ff_conv_sq(const float *x, const float *dy, const float *w, float *F, int G, int B, int C, int H,
                                  int W, int K, int R, int stride, int pad, int P, int Q, void *ws, size_t ws_bytes,
                                  salun_stream_t stream) {
  if (G < 1 || B < 1 || C < 1 || H < 1 || W < 1 || K < 1 || P < 1 || Q < 1) return SALUN_EINVAL;
  if (!x || !dy || !w || !F || !ws) return SALUN_EINVAL;
  const size_t need = salun_ff_conv_sq_workspace_bytes(G, B, C, K, R, P, Q);
  if (need == 0) return SALUN_EINVAL;
  if (ws_bytes < need) return SALUN_ENOSPC;
  const int64_t n = (int64_t)K * C * R * R;
  const int64_t dyg = (int64_t)B * K * P * Q;
  float *gs = static_cast<float *>(ws);
  const size_t gbytes = align256(sizeof(float) * (size_t)G * n);
  void *wws = static_cast<char *>(ws) + gbytes;
  const size_t wbytes = ws_bytes - gbytes;
  // one group at a time: its weight gradient is reduced to completion (fixed order) before anything squares it
  for (int g = 0; g < G; ++g) {
    const int rc = salun_conv2d_backward_weight_ex(x, dy + g * dyg, gs + g * n, B, C, H, W, K, R, stride, pad, P, Q, 0,
                                                   0, wws, wbytes, stream);
    if (rc != SALUN_OK) return rc;
  }
  hipStream_t st = salun_hip_stream(stream);
  if ((n & 3) == 0 && salun_aligned16(F) && salun_aligned16(gs)) {
    hipLaunchKernelGGL(k_ff_sq_acc4, dim3(salun_grid_for(n >> 2, SALUN_BLOCK)), dim3(SALUN_BLOCK), 0, st, gs, w, G, n,
                       F);
  } else {
    hipLaunchKernelGGL(k_ff_sq_acc, dim3(salun_grid_for(n, SALUN_BLOCK)), dim3(SALUN_BLOCK), 0, st, gs, w, G, n, F);
  }
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_ff_linear_sq(const float *x, const float *dy, const float *w, float *F, int G, int B, int M,
                                    int K, salun_stream_t stream) {
  if (G < 1 || B < 1 || M < 1 || K < 1) return SALUN_EINVAL;
  if (!x || !dy || !w || !F) return SALUN_EINVAL;
  const int64_t mk = (int64_t)M * K;
  hipLaunchKernelGGL(k_ff_linear_sq, dim3((unsigned)((mk + SALUN_BLOCK - 1) / SALUN_BLOCK)), dim3(SALUN_BLOCK), 0,
                     salun_hip_stream(stream), x, dy, w, G, B, M, K, F);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT size_t salun_ff_vec_sq_workspace_bytes(int G, int C) {
  if (G < 1 || C < 1) return 0;
  return (size_t)G * C * 2 * sizeof(double);
}

SALUN_EXPORT int salun_ff_vec_sq(const float *x, const float *dy, const float *running_mean, const float *running_var,
                                 double eps, const float *w, int G, int B, int C, int HW, float *F_gamma, float *F_beta,
                                 void *ws, size_t ws_bytes, salun_stream_t stream) {
  if (G < 1 || B < 1 || C < 1 || HW < 1 || G > 65535) return SALUN_EINVAL;
  if (!dy || !w || !ws || (!F_gamma && !F_beta)) return SALUN_EINVAL;
  if (F_gamma && (!x || !running_mean || !running_var)) return SALUN_EINVAL;  // the gamma sums need x^
  if (ws_bytes < salun_ff_vec_sq_workspace_bytes(G, C)) return SALUN_ENOSPC;
  hipStream_t st = salun_hip_stream(stream);
  double *part = static_cast<double *>(ws);
  hipLaunchKernelGGL(k_ff_vec_partial, dim3(C, G), dim3(SALUN_BLOCK), 0, st, F_gamma ? x : nullptr, dy, running_mean,
                     running_var, eps, B, C, HW, part);
  SALUN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ff_vec_finish, dim3((C + SALUN_BLOCK - 1) / SALUN_BLOCK), dim3(SALUN_BLOCK), 0, st, part, w, G,
                     C, F_gamma, F_beta);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_ff_apply(float *p, const float *F, const int64_t *table, int nparam, int64_t ntiles,
                                double nbatches, double alpha, uint64_t seed, salun_stream_t stream) {
  if (nparam < 0 || ntiles < 0 || !(nbatches > 0.0)) return SALUN_EINVAL;
  if (nparam == 0 || ntiles == 0) return SALUN_OK;
  if (!p || !F || !table) return SALUN_EINVAL;
  const int64_t grid = ntiles < 4096 ? ntiles : 4096;
  hipLaunchKernelGGL(k_ff_apply, dim3((unsigned)grid), dim3(SALUN_BLOCK), 0, salun_hip_stream(stream), p, F, table,
                     nparam, ntiles, (float)nbatches, (float)alpha, seed);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}
