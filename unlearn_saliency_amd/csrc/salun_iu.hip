// salun_iu.hip — the IU / WoodFisher baseline (reference Classification/unlearn/Wfisher.py:47-198) without per-sample
// gradients.  The reference loop keeps two flat vectors, o and k; o is only ever rescaled, so o_i = s_i g_0 and
// k_i = v - beta_i g_0, and each retain sample enters through two scalars a_i = <g_0, g_i>, b_i = <v, g_i>
// (DESIGN.md §9b).  Those scalars come from ONE batched eval-mode backward per batch through per-layer identities:
//   K17a conv      <dW l_i, U> = <dy_i, conv(x_i, U)>     (the tangent conv runs on conv_igemm; this file dots it)
//   K17b BN, eval  sum_c u_gamma[c] sum_pq dy_i x^_i + u_beta[c] sum_pq dy_i,   x^ from the running statistics
//   K17c linear    sum_m dy_i[m] (U x_i + u_b)[m]
//   K17d the scalar recurrence, one thread, fp64, reading a/b and writing beta on the device
//   K17e p += alpha (v - beta g_0) (* m), beta read from device memory; an op on stream_tiles (salun_stream.h)
// Every reduction is deterministic: per-workgroup fp64 partials in a fixed order, then a fixed-order finish;
// no float atomics.  Two launches on the same inputs give bit-identical outputs.
#include "salun_stream.h"

namespace {

constexpr int DOT_ELEMS_PER_BLOCK = 4096;  // 16 elements per thread: enough work per workgroup to hide the launch
constexpr int DOT_MAX_BLOCKS = 64;          // per sample

// workgroups per sample for a per-sample reduction of n elements
inline int dot_blocks(int64_t n) {
  int64_t nb = (n + DOT_ELEMS_PER_BLOCK - 1) / DOT_ELEMS_PER_BLOCK;
  if (nb < 1) nb = 1;
  if (nb > DOT_MAX_BLOCKS) nb = DOT_MAX_BLOCKS;
  return static_cast<int>(nb);
}

// the chunk [lo, hi) of [0, n) that workgroup `blk` of `nb` owns; chunk boundaries are multiples of 4
__device__ __forceinline__ void chunk_of(int64_t n, int nb, int blk, int64_t &lo, int64_t &hi) {
  int64_t c = (n + nb - 1) / nb;
  c = (c + 3) & ~int64_t(3);
  lo = c * blk;
  hi = lo + c;
  if (lo > n) lo = n;
  if (hi > n) hi = n;
}

// Two block sums (tangent 0, tangent 1) -> partial[(i * nb + blk) * 2 + j]
__device__ __forceinline__ void write_partials(double t0, double t1, double *partial, int64_t slot) {
  __shared__ double lds[4];
  const double s0 = salun_block_sum(t0, lds);
  const double s1 = salun_block_sum(t1, lds);
  if (threadIdx.x == 0) {
    partial[slot * 2 + 0] = s0;
    partial[slot * 2 + 1] = s1;
  }
}

// out[i, j] += sum_c y2[i, j*n + c] * dy[i, c]      grid (nb, B)
template <bool VEC>
__global__ __launch_bounds__(SALUN_BLOCK) void k_conv_dot(const float *__restrict__ y2, const float *__restrict__ dy,
                                                          int64_t n, double *__restrict__ partial) {
  const int i = blockIdx.y, nb = gridDim.x, blk = blockIdx.x;
  int64_t lo, hi;
  chunk_of(n, nb, blk, lo, hi);
  const float *a0 = y2 + (int64_t)i * 2 * n;
  const float *a1 = a0 + n;
  const float *d = dy + (int64_t)i * n;
  double t0 = 0.0, t1 = 0.0;
  if (VEC) {  // n % 4 == 0 and every base 16-byte aligned: lo, hi are multiples of 4
    for (int64_t v = (lo >> 2) + threadIdx.x; v < (hi >> 2); v += SALUN_BLOCK) {
      const float4 g = reinterpret_cast<const float4 *>(d)[v];
      const float4 p = reinterpret_cast<const float4 *>(a0)[v];
      const float4 q = reinterpret_cast<const float4 *>(a1)[v];
      t0 += (double)g.x * p.x + (double)g.y * p.y + (double)g.z * p.z + (double)g.w * p.w;
      t1 += (double)g.x * q.x + (double)g.y * q.y + (double)g.z * q.z + (double)g.w * q.w;
    }
  } else {
    for (int64_t e = lo + threadIdx.x; e < hi; e += SALUN_BLOCK) {
      const double g = d[e];
      t0 += g * a0[e];
      t1 += g * a1[e];
    }
  }
  write_partials(t0, t1, partial, (int64_t)i * nb + blk);
}

// Eval BatchNorm: out[i, j] += sum_{c,pq} dy * (ug_j[c] * (x - rm[c]) / sqrt(rv[c] + eps) + ub_j[c])   grid (nb, B)
__global__ __launch_bounds__(SALUN_BLOCK) void k_bn_dot(const float *__restrict__ x, const float *__restrict__ dy,
                                                        const float *__restrict__ rm, const float *__restrict__ rv,
                                                        double eps, const float *__restrict__ ug0,
                                                        const float *__restrict__ ub0, const float *__restrict__ ug1,
                                                        const float *__restrict__ ub1, int C, int HW,
                                                        double *__restrict__ partial) {
  const int i = blockIdx.y, nb = gridDim.x, blk = blockIdx.x;
  const int64_t n = (int64_t)C * HW;
  int64_t lo, hi;
  chunk_of(n, nb, blk, lo, hi);
  const float *xs = x + (int64_t)i * n;
  const float *ds = dy + (int64_t)i * n;
  double t0 = 0.0, t1 = 0.0;
  int cc = -1;
  double mean = 0.0, inv = 0.0, g0 = 0.0, b0 = 0.0, g1 = 0.0, b1 = 0.0;
  for (int64_t e = lo + threadIdx.x; e < hi; e += SALUN_BLOCK) {
    const int c = static_cast<int>(e / HW);
    if (c != cc) {  // a thread walks channels in increasing order: the per-channel terms change rarely for HW >= 256
      cc = c;
      mean = rm[c];
      inv = 1.0 / sqrt((double)rv[c] + eps);
      g0 = ug0[c]; b0 = ub0[c]; g1 = ug1[c]; b1 = ub1[c];
    }
    const double g = ds[e];
    const double xh = ((double)xs[e] - mean) * inv;
    t0 += g * (g0 * xh + b0);
    t1 += g * (g1 * xh + b1);
  }
  write_partials(t0, t1, partial, (int64_t)i * nb + blk);
}

// out[i, j] += sum_b partial[(i * nb + b) * 2 + j]      one thread per (i, j), b in increasing order
__global__ __launch_bounds__(SALUN_BLOCK) void k_finish(const double *__restrict__ partial, int B, int nb,
                                                        double *__restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * SALUN_BLOCK + threadIdx.x;
  if (t >= (int64_t)B * 2) return;
  const int64_t i = t >> 1, j = t & 1;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += partial[(i * nb + b) * 2 + j];
  out[t] += s;
}

// Linear: out[i, j] += sum_m dy[i, m] * (sum_k U_j[m, k] x[i, k] + ub_j[m])     one workgroup per sample
__global__ __launch_bounds__(SALUN_BLOCK) void k_linear_dot(const float *__restrict__ x, const float *__restrict__ dy,
                                                            const float *__restrict__ u0w, const float *__restrict__ u0b,
                                                            const float *__restrict__ u1w, const float *__restrict__ u1b,
                                                            int M, int K, double *__restrict__ out) {
  __shared__ double lds[4];
  const int i = blockIdx.x;
  const float *xs = x + (int64_t)i * K;
  const float *ds = dy + (int64_t)i * M;
  double t0 = 0.0, t1 = 0.0;
  const int64_t mk = (int64_t)M * K;
  for (int64_t e = threadIdx.x; e < mk; e += SALUN_BLOCK) {
    const int m = static_cast<int>(e / K), k = static_cast<int>(e - (int64_t)m * K);
    const double gx = (double)ds[m] * xs[k];
    t0 += gx * u0w[e];
    t1 += gx * u1w[e];
  }
  if (u0b) {
    for (int m = threadIdx.x; m < M; m += SALUN_BLOCK) {
      t0 += (double)ds[m] * u0b[m];
      t1 += (double)ds[m] * u1b[m];
    }
  }
  const double s0 = salun_block_sum(t0, lds);
  const double s1 = salun_block_sum(t1, lds);
  if (threadIdx.x == 0) {
    out[(int64_t)i * 2 + 0] += s0;
    out[(int64_t)i * 2 + 1] += s1;
  }
}

// s = 1, beta = 0; for each sample: t = s a ; beta += (b - beta a) s / (N + t) ; s *= N / (N + t)
__global__ void k_recurrence(const double *__restrict__ ab, int64_t n, double N, double *__restrict__ out) {
  if (threadIdx.x != 0) return;
  double s = 1.0, beta = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    const double a = ab[2 * i], b = ab[2 * i + 1];
    const double t = s * a;
    const double den = N + t;
    beta += (b - beta * a) * s / den;
    s *= N / den;
  }
  out[0] = beta;
  out[1] = s;
}

__device__ __forceinline__ float iu_step(float p, float v, float g, double beta, double alpha) {
  return static_cast<float>((double)p + alpha * ((double)v - beta * (double)g));
}

// p <- p + alpha (v - beta g0) where m != 0 (everywhere when m is NULL); masked-out weights are not written
template <bool MASK>
struct ApplyOp {
  float *p;
  const float *v, *g0;
  const uint8_t *m;
  double beta, alpha;
  struct Vec { float4 p, v, g; uint32_t m; };
  __device__ void load(Vec &x, int64_t e) const {
    x.p = ld4(p, e);
    x.v = ld4(v, e);
    x.g = ld4(g0, e);
    if (MASK) x.m = ldm(m, e);
  }
  __device__ void vec(Vec &x, int64_t e) const {
    float4 r = x.p;
    if (!MASK || mbyte(x.m, 0)) r.x = iu_step(x.p.x, x.v.x, x.g.x, beta, alpha);
    if (!MASK || mbyte(x.m, 1)) r.y = iu_step(x.p.y, x.v.y, x.g.y, beta, alpha);
    if (!MASK || mbyte(x.m, 2)) r.z = iu_step(x.p.z, x.v.z, x.g.z, beta, alpha);
    if (!MASK || mbyte(x.m, 3)) r.w = iu_step(x.p.w, x.v.w, x.g.w, beta, alpha);
    st4(p, e, r);
  }
  __device__ void one(int64_t e) const {
    if (!MASK || m[e]) p[e] = iu_step(p[e], v[e], g0[e], beta, alpha);
  }
};

template <bool VEC, bool MASK>
__global__ __launch_bounds__(SALUN_BLOCK) void k_apply(float *__restrict__ p, const float *__restrict__ v,
                                                       const float *__restrict__ g0, const double *__restrict__ beta_ptr,
                                                       const uint8_t *__restrict__ m, double alpha, int64_t n) {
  ApplyOp<MASK> op{p, v, g0, m, *beta_ptr, alpha};
  stream_tiles<VEC>(n, op);
}

int finish(const double *partial, int B, int nb, double *out, hipStream_t st) {
  const int grid = static_cast<int>(((int64_t)B * 2 + SALUN_BLOCK - 1) / SALUN_BLOCK);
  hipLaunchKernelGGL(k_finish, dim3(grid), dim3(SALUN_BLOCK), 0, st, partial, B, nb, out);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

}  // namespace

SALUN_EXPORT size_t salun_iu_dot_workspace_bytes(int B, int64_t n) {
  if (B < 0 || n < 0) return 0;
  return (size_t)B * (size_t)dot_blocks(n) * 2 * sizeof(double);
}

SALUN_EXPORT int salun_iu_conv_dot(const float *y2, const float *dy, int B, int64_t n, double *out, void *ws,
                                   size_t ws_bytes, salun_stream_t stream) {
  if (B < 0 || n < 0 || B > 65535) return SALUN_EINVAL;
  if (B == 0 || n == 0) return SALUN_OK;
  if (!y2 || !dy || !out || !ws) return SALUN_EINVAL;
  if (ws_bytes < salun_iu_dot_workspace_bytes(B, n)) return SALUN_ENOSPC;
  hipStream_t st = salun_hip_stream(stream);
  const int nb = dot_blocks(n);
  double *partial = static_cast<double *>(ws);
  const bool vec = (n & 3) == 0 && salun_aligned16(y2) && salun_aligned16(dy);
  if (vec)
    hipLaunchKernelGGL(k_conv_dot<true>, dim3(nb, B), dim3(SALUN_BLOCK), 0, st, y2, dy, n, partial);
  else
    hipLaunchKernelGGL(k_conv_dot<false>, dim3(nb, B), dim3(SALUN_BLOCK), 0, st, y2, dy, n, partial);
  SALUN_LAUNCH_CHECK();
  return finish(partial, B, nb, out, st);
}

SALUN_EXPORT int salun_iu_bn_dot(const float *x, const float *dy, const float *running_mean, const float *running_var,
                                 double eps, const float *u0_gamma, const float *u0_beta, const float *u1_gamma,
                                 const float *u1_beta, int B, int C, int HW, double *out, void *ws, size_t ws_bytes,
                                 salun_stream_t stream) {
  if (B < 0 || C < 0 || HW < 0 || B > 65535) return SALUN_EINVAL;
  if (B == 0 || C == 0 || HW == 0) return SALUN_OK;
  if (!x || !dy || !running_mean || !running_var || !u0_gamma || !u0_beta || !u1_gamma || !u1_beta || !out || !ws)
    return SALUN_EINVAL;
  const int64_t n = (int64_t)C * HW;
  if (ws_bytes < salun_iu_dot_workspace_bytes(B, n)) return SALUN_ENOSPC;
  hipStream_t st = salun_hip_stream(stream);
  const int nb = dot_blocks(n);
  double *partial = static_cast<double *>(ws);
  hipLaunchKernelGGL(k_bn_dot, dim3(nb, B), dim3(SALUN_BLOCK), 0, st, x, dy, running_mean, running_var, eps, u0_gamma,
                     u0_beta, u1_gamma, u1_beta, C, HW, partial);
  SALUN_LAUNCH_CHECK();
  return finish(partial, B, nb, out, st);
}

SALUN_EXPORT int salun_iu_linear_dot(const float *x, const float *dy, const float *u0_w, const float *u0_b,
                                     const float *u1_w, const float *u1_b, int B, int M, int K, double *out,
                                     salun_stream_t stream) {
  if (B < 0 || M < 0 || K < 0) return SALUN_EINVAL;
  if ((u0_b == nullptr) != (u1_b == nullptr)) return SALUN_EINVAL;
  if (B == 0 || M == 0) return SALUN_OK;
  if (!x || !dy || !u0_w || !u1_w || !out) return SALUN_EINVAL;
  hipLaunchKernelGGL(k_linear_dot, dim3(B), dim3(SALUN_BLOCK), 0, salun_hip_stream(stream), x, dy, u0_w, u0_b, u1_w,
                     u1_b, M, K, out);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_iu_recurrence(const double *ab, int64_t n, double N, double *out, salun_stream_t stream) {
  if (n < 0 || !out || (n > 0 && !ab)) return SALUN_EINVAL;
  hipLaunchKernelGGL(k_recurrence, dim3(1), dim3(64), 0, salun_hip_stream(stream), ab, n, N, out);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_iu_apply(float *p, const float *v, const float *g0, const double *beta, const uint8_t *mask,
                                double alpha, int64_t n, salun_stream_t stream) {
  if (n < 0) return SALUN_EINVAL;
  if (n == 0) return SALUN_OK;
  if (!p || !v || !g0 || !beta) return SALUN_EINVAL;
  hipStream_t st = salun_hip_stream(stream);
  const bool vec = salun_aligned16(p) && salun_aligned16(v) && salun_aligned16(g0) &&
                   (!mask || salun_aligned4(mask));
  return with_bools(
      [&](auto M) {
        return stream_launch(k_apply<true, M.value>, k_apply<false, M.value>, vec, n, SALUN_MAX_GRID, st, p, v, g0, beta,
                             mask, alpha, n);
      },
      mask != nullptr);
}
