// salun_svc.hip — K25: RBF C-SVC fit and predict for the membership-inference attack.
// gfx950 / CDNA4, wave64.
//
// The problem is libsvm's C-SVC dual (Fan, Chen, Lin 2005):  min 1/2 a'Qa - e'a,  0 <= a <= C,  y'a = 0,
// Q_ts = y_t y_s K_ts, K_ts = exp(-gamma |x_t - x_s|^2).  With v_t = -y_t G_t (G the gradient Qa - e),
//   I_up  = {y = +1, a < C} u {y = -1, a > 0}     m(a) = max over I_up  of v
//   I_low = {y = +1, a > 0} u {y = -1, a < C}     M(a) = min over I_low of v
// and a is eps-optimal when m - M < eps.
//
// Three kernels.
//   k_svc_gram      K [n, n] fp32, all CUs: distance and exponential in fp64, ONE rounding to fp32 per entry.
//   k_svc_fit       the whole SMO loop in ONE workgroup of 1024 threads.  An iteration is latency-bound, not
//                   throughput-bound (two or three kernel rows of n floats, the gradient, three block reductions), and
//                   what it would need from other workgroups is a grid barrier per reduction; DESIGN.md §8 item 5
//                   records what hand-rolled grid barriers do on a shared machine.  So: no grid barrier, no
//                   cooperative launch, no cross-workgroup flag, nothing that spins.  Every loop here is a counted
//                   `for` over n or is bounded by max_iter.
//   k_svc_decision  one workgroup per query point, fp64, fixed summation order, all CUs.
// k_svc_gram_wide / k_svc_decision_wide are the same two for up to SALUN_SVC_WIDE_MAX_D features (below).
//
// One iteration of k_svc_fit (all values that steer control flow come out of LDS, so every thread takes the same path):
//   pass 1  G += Q_i da_i, then += Q_j da_j (the previous update; skipped before the first), and in the same sweep
//           m, i = lowest index of the maximum, M.                     -> reduction -> stop?  (m - M < eps, max_iter)
//   pass 2  j = lowest index of min -(m - v_t)^2 / a_it over {t in I_low, v_t < m}, a_it = 2 - 2 K_it, a <= 0 -> 1e-12
//                                                                      -> reduction
//   update  thread 0: libsvm's clipped two-variable step on (a_i, a_j); a clipped value is assigned 0 or C, never
//           computed; the two deltas go through LDS.                   -> barrier
// Per element the passes read one state byte (y, t in I_up, t in I_low) instead of alpha: only i and j change state.
// No atomics: the same inputs give the same bits of alpha and rho.
#include "salun_common.h"
#include <math.h>
#include <limits.h>

namespace {

constexpr int SVC_THREADS = 1024;
constexpr int SVC_WAVES = SVC_THREADS / SALUN_WAVE;
constexpr double SVC_TAU = 1e-12;
constexpr unsigned F_POS = 1u, F_UP = 2u, F_LOW = 4u;

__device__ __forceinline__ unsigned svc_state(bool pos, double a, double C) {
  return pos ? (F_POS | (a < C ? F_UP : 0u) | (a > 0.0 ? F_LOW : 0u)) : ((a > 0.0 ? F_UP : 0u) | (a < C ? F_LOW : 0u));
}

// (greatest value, lowest index among equals) over a wave; result in lane 0.
__device__ __forceinline__ void wave_argmax(double &v, int &i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double v2 = __shfl_down(v, off, 64);
    const int i2 = __shfl_down(i, off, 64);
    if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
  }
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_down(v, off, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  return v;
}

// Block argmax over SVC_THREADS threads: every thread returns the same (v, i).  `sv`, `si` hold SVC_WAVES entries; the
// caller alternates between two pairs so that a pair is rewritten only after a later barrier.
__device__ __forceinline__ void block_argmax(double &v, int &i, double *sv, int *si) {
  wave_argmax(v, i);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sv[wave] = v; si[wave] = i; }
  __syncthreads();
  v = sv[0]; i = si[0];
#pragma unroll
  for (int w = 1; w < SVC_WAVES; ++w) {
    const double v2 = sv[w];
    const int i2 = si[w];
    if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
  }
}

__global__ __launch_bounds__(SALUN_BLOCK) void k_svc_gram(const float *__restrict__ X, float *__restrict__ K, int n, int d,
                                                          double gamma) {
  const int chunks = (n + SALUN_BLOCK - 1) / SALUN_BLOCK;
  const int64_t items = static_cast<int64_t>(n) * chunks;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int t = static_cast<int>(item / chunks);
    const int s = static_cast<int>(item - static_cast<int64_t>(t) * chunks) * SALUN_BLOCK + threadIdx.x;
    if (s < n) {
      const float *xt = X + static_cast<int64_t>(t) * d, *xs = X + static_cast<int64_t>(s) * d;
      double acc = 0.0;
      for (int k = 0; k < d; ++k) {
        const double df = static_cast<double>(xt[k]) - static_cast<double>(xs[k]);
        acc = acc + df * df;
      }
      K[static_cast<int64_t>(t) * n + s] = static_cast<float>(exp(-gamma * acc));
    }
  }
}

__global__ __launch_bounds__(SVC_THREADS) void k_svc_fit(const float *__restrict__ K, const uint8_t *__restrict__ y01,
                                                         int n, double C, double eps, int64_t max_iter,
                                                         double *__restrict__ alpha, double *__restrict__ G,
                                                         uint8_t *__restrict__ state, double *__restrict__ rho_out,
                                                         int64_t *__restrict__ status) {
  __shared__ double s_v[2][SVC_WAVES];
  __shared__ int s_i[2][SVC_WAVES];
  __shared__ double s_lo[SVC_WAVES], s_hi[SVC_WAVES], s_sum[SVC_WAVES];
  __shared__ int s_cnt[SVC_WAVES];
  __shared__ double s_upd[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  for (int t = tid; t < n; t += SVC_THREADS) {
    alpha[t] = 0.0;
    G[t] = -1.0;
    state[t] = static_cast<uint8_t>(svc_state(y01[t] != 0, 0.0, C));
  }
  __syncthreads();

  int64_t it = 0;
  int converged = 0, i = 0, j = 0;
  double dai = 0.0, daj = 0.0;
  bool upd = false;
  for (;;) {  // leaves by the stopping rule or by it >= max_iter; `it` grows by one per trip
    // ---- pass 1: apply the previous update to G; m, i, M
    double m = -INFINITY, M = INFINITY;
    int bi = INT_MAX;
    {
      const float *Ki = K + static_cast<int64_t>(i) * n, *Kj = K + static_cast<int64_t>(j) * n;
      const bool pi = (state[i] & F_POS) != 0, pj = (state[j] & F_POS) != 0;
      for (int t = tid; t < n; t += SVC_THREADS) {
        const unsigned f = state[t];
        const bool pos = (f & F_POS) != 0;
        double g = G[t];
        if (upd) {
          const float ki = Ki[t], kj = Kj[t];
          const double qi = static_cast<double>(pos == pi ? ki : -ki), qj = static_cast<double>(pos == pj ? kj : -kj);
          g = g + qi * dai;
          g = g + qj * daj;
          G[t] = g;
        }
        const double v = pos ? -g : g;
        if ((f & F_UP) && v > m) { m = v; bi = t; }
        if ((f & F_LOW) && v < M) M = v;
      }
    }
    M = wave_min(M);
    if (lane == 0) s_lo[wave] = M;
    block_argmax(m, bi, s_v[0], s_i[0]);  // its barrier also publishes s_lo
    M = s_lo[0];
#pragma unroll
    for (int w = 1; w < SVC_WAVES; ++w) M = fmin(M, s_lo[w]);
    if (!(m - M >= eps)) { converged = 1; break; }
    if (it >= max_iter) break;
    i = bi;

    // ---- pass 2: j by the second-order rule
    double best = -INFINITY;  // maximise (m - v)^2 / a  ==  minimise -(m - v)^2 / a
    int bj = INT_MAX;
    {
      const float *Ki = K + static_cast<int64_t>(i) * n;
      for (int t = tid; t < n; t += SVC_THREADS) {
        const unsigned f = state[t];
        const double g = G[t];
        const double kit = static_cast<double>(Ki[t]);
        const double v = (f & F_POS) ? -g : g;
        const double b = m - v;
        double a = 2.0 - 2.0 * kit;
        if (!(a > 0.0)) a = SVC_TAU;
        const double gain = (b * b) / a;
        if ((f & F_LOW) && v < m && gain > best) { best = gain; bj = t; }
      }
    }
    block_argmax(best, bj, s_v[1], s_i[1]);
    if (bj == INT_MAX) { converged = 1; break; }
    j = bj;

    // ---- update (thread 0), libsvm's clipped step
    if (tid == 0) {
      const bool pi = (state[i] & F_POS) != 0, pj = (state[j] & F_POS) != 0;
      const double ai = alpha[i], aj = alpha[j], gi = G[i], gj = G[j];
      const double kij = static_cast<double>(K[static_cast<int64_t>(i) * n + j]);
      double ni, nj;
      if (pi != pj) {
        double quad = 2.0 + 2.0 * kij;
        if (!(quad > 0.0)) quad = SVC_TAU;
        const double delta = (-gi - gj) / quad, diff = ai - aj;
        ni = ai + delta;
        nj = aj + delta;
        if (diff > 0.0) {
          if (nj < 0.0) { nj = 0.0; ni = diff; }
        } else {
          if (ni < 0.0) { ni = 0.0; nj = -diff; }
        }
        if (diff > 0.0) {
          if (ni > C) { ni = C; nj = C - diff; }
        } else {
          if (nj > C) { nj = C; ni = C + diff; }
        }
      } else {
        double quad = 2.0 - 2.0 * kij;
        if (!(quad > 0.0)) quad = SVC_TAU;
        const double delta = (gi - gj) / quad, sum = ai + aj;
        ni = ai - delta;
        nj = aj + delta;
        if (sum > C) {
          if (ni > C) { ni = C; nj = sum - C; }
        } else {
          if (nj < 0.0) { nj = 0.0; ni = sum; }
        }
        if (sum > C) {
          if (nj > C) { nj = C; ni = sum - C; }
        } else {
          if (ni < 0.0) { ni = 0.0; nj = sum; }
        }
      }
      alpha[i] = ni;
      alpha[j] = nj;
      state[i] = static_cast<uint8_t>(svc_state(pi, ni, C));
      state[j] = static_cast<uint8_t>(svc_state(pj, nj, C));
      s_upd[0] = ni - ai;
      s_upd[1] = nj - aj;
    }
    __syncthreads();
    dai = s_upd[0];
    daj = s_upd[1];
    upd = true;
    ++it;
  }

  // ---- rho: mean of y_t G_t over free variables, else the midpoint of the bounds
  __syncthreads();
  double sum = 0.0, ub = INFINITY, lb = -INFINITY;
  int cnt = 0;
  for (int t = tid; t < n; t += SVC_THREADS) {
    const unsigned f = state[t];
    const double g = G[t];
    const double yg = (f & F_POS) ? g : -g;
    if ((f & F_UP) && (f & F_LOW)) { sum = sum + yg; ++cnt; }
    else if (!(f & F_LOW)) ub = fmin(ub, yg);
    else lb = fmax(lb, yg);
  }
  sum = salun_wave_sum(sum);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
  ub = wave_min(ub);
  lb = wave_max(lb);
  if (lane == 0) { s_sum[wave] = sum; s_cnt[wave] = cnt; s_lo[wave] = ub; s_hi[wave] = lb; }
  __syncthreads();
  if (tid == 0) {
    sum = s_sum[0]; cnt = s_cnt[0]; ub = s_lo[0]; lb = s_hi[0];
    for (int w = 1; w < SVC_WAVES; ++w) {
      sum = sum + s_sum[w];
      cnt += s_cnt[w];
      ub = fmin(ub, s_lo[w]);
      lb = fmax(lb, s_hi[w]);
    }
    *rho_out = cnt > 0 ? sum / static_cast<double>(cnt) : (ub + lb) / 2.0;
    status[0] = it;
    status[1] = converged;
  }
}

__global__ __launch_bounds__(SALUN_BLOCK) void k_svc_decision(const float *__restrict__ X, const double *__restrict__ coef,
                                                              const double *__restrict__ rho, int n, int d, double gamma,
                                                              const float *__restrict__ Z, int64_t m,
                                                              double *__restrict__ dec, uint8_t *__restrict__ pred) {
  __shared__ double lds[4];
  for (int64_t q = blockIdx.x; q < m; q += gridDim.x) {
    double z[SALUN_SVC_MAX_D];
#pragma unroll
    for (int k = 0; k < SALUN_SVC_MAX_D; ++k) z[k] = k < d ? static_cast<double>(Z[q * d + k]) : 0.0;
    double part = 0.0;
    for (int t = threadIdx.x; t < n; t += SALUN_BLOCK) {
      const double c = coef[t];
      if (c != 0.0) {
        const float *xt = X + static_cast<int64_t>(t) * d;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < SALUN_SVC_MAX_D; ++k) {
          if (k < d) {
            const double df = static_cast<double>(xt[k]) - z[k];
            acc = acc + df * df;
          }
        }
        part = part + c * exp(-gamma * acc);
      }
    }
    const double total = salun_block_sum(part, lds);
    if (threadIdx.x == 0) {
      const double f = total - *rho;
      if (dec) dec[q] = f;
      if (pred) pred[q] = f > 0.0 ? 1 : 0;
    }
  }
}

// ---- wide features (d up to SALUN_SVC_WIDE_MAX_D): the probability-vector feature of a 100- / 200-class model.
// Same arithmetic, in the same order, as the two kernels above: for d <= SALUN_SVC_MAX_D the results are the same bits.
constexpr int GW_KC = 32;             // features per LDS tile
constexpr int GW_LD = GW_KC + 1;      // tile row stride in floats: lane r reads bank (r * 33 + c) % 32, all distinct

// One work item = row t of K against SALUN_BLOCK consecutive columns s.  x_t sits in LDS as doubles (read as a
// broadcast); the SALUN_BLOCK rows x_s pass through LDS in tiles of GW_KC features, loaded coalesced (GW_KC consecutive
// floats of a row per 32 lanes) and read back one row per lane.  Without the tile every lane walks its own row of
// d floats in global memory, d * 4 bytes apart from its neighbour's.
__global__ __launch_bounds__(SALUN_BLOCK) void k_svc_gram_wide(const float *__restrict__ X, float *__restrict__ K, int n,
                                                               int d, double gamma) {
  __shared__ double s_xt[SALUN_SVC_WIDE_MAX_D];
  __shared__ float s_tile[SALUN_BLOCK * GW_LD];
  const int chunks = (n + SALUN_BLOCK - 1) / SALUN_BLOCK;
  const int64_t items = static_cast<int64_t>(n) * chunks;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int t = static_cast<int>(item / chunks);
    const int s0 = static_cast<int>(item - static_cast<int64_t>(t) * chunks) * SALUN_BLOCK;
    const int rows = min(SALUN_BLOCK, n - s0);
    __syncthreads();  // the previous item's reads of s_xt and s_tile are done
    for (int k = threadIdx.x; k < d; k += SALUN_BLOCK) s_xt[k] = static_cast<double>(X[static_cast<int64_t>(t) * d + k]);
    double acc = 0.0;
    for (int k0 = 0; k0 < d; k0 += GW_KC) {
      const int kc = min(GW_KC, d - k0);
      if (k0) __syncthreads();  // the previous tile has been read
      for (int e = threadIdx.x; e < SALUN_BLOCK * GW_KC; e += SALUN_BLOCK) {
        const int r = e / GW_KC, c = e - r * GW_KC;
        if (r < rows && c < kc) s_tile[r * GW_LD + c] = X[static_cast<int64_t>(s0 + r) * d + k0 + c];
      }
      __syncthreads();
      if (static_cast<int>(threadIdx.x) < rows) {
        const float *row = s_tile + threadIdx.x * GW_LD;
        for (int c = 0; c < kc; ++c) {
          const double df = s_xt[k0 + c] - static_cast<double>(row[c]);
          acc = acc + df * df;
        }
      }
    }
    if (static_cast<int>(threadIdx.x) < rows)
      K[static_cast<int64_t>(t) * n + s0 + threadIdx.x] = static_cast<float>(exp(-gamma * acc));
  }
}

// k_svc_decision with the query point in LDS instead of SALUN_SVC_MAX_D registers; one workgroup per query point.
__global__ __launch_bounds__(SALUN_BLOCK) void k_svc_decision_wide(const float *__restrict__ X,
                                                                   const double *__restrict__ coef,
                                                                   const double *__restrict__ rho, int n, int d,
                                                                   double gamma, const float *__restrict__ Z, int64_t m,
                                                                   double *__restrict__ dec, uint8_t *__restrict__ pred) {
  __shared__ double lds[4];
  __shared__ double s_z[SALUN_SVC_WIDE_MAX_D];
  for (int64_t q = blockIdx.x; q < m; q += gridDim.x) {
    __syncthreads();  // the previous query's reads of s_z are done
    for (int k = threadIdx.x; k < d; k += SALUN_BLOCK) s_z[k] = static_cast<double>(Z[q * d + k]);
    __syncthreads();
    double part = 0.0;
    for (int t = threadIdx.x; t < n; t += SALUN_BLOCK) {
      const double c = coef[t];
      if (c != 0.0) {
        const float *xt = X + static_cast<int64_t>(t) * d;
        double acc = 0.0;
        for (int k = 0; k < d; ++k) {
          const double df = static_cast<double>(xt[k]) - s_z[k];
          acc = acc + df * df;
        }
        part = part + c * exp(-gamma * acc);
      }
    }
    const double total = salun_block_sum(part, lds);
    if (threadIdx.x == 0) {
      const double f = total - *rho;
      if (dec) dec[q] = f;
      if (pred) pred[q] = f > 0.0 ? 1 : 0;
    }
  }
}

size_t align16(size_t b) { return (b + 15u) & ~static_cast<size_t>(15u); }
bool n_ok(int64_t n) { return n >= 2 && n <= SALUN_SVC_MAX_N; }
bool positive_finite(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

}  // namespace

SALUN_EXPORT size_t salun_svc_rbf_workspace_bytes(int64_t n) {
  if (!n_ok(n)) return 0;
  const size_t N = static_cast<size_t>(n);
  return align16(N * N * sizeof(float)) + align16(N * sizeof(double)) + align16(N);
}

SALUN_EXPORT int salun_svc_rbf_gram(const float *X, int64_t n, int d, double gamma, void *ws, size_t ws_bytes,
                                    salun_stream_t stream) {
  if (!n_ok(n) || d < 1 || d > SALUN_SVC_MAX_D || !X || !ws || !positive_finite(gamma)) return SALUN_EINVAL;
  if (!salun_aligned4(X) || !salun_aligned16(ws)) return SALUN_EINVAL;
  if (ws_bytes < salun_svc_rbf_workspace_bytes(n)) return SALUN_ENOSPC;
  const int64_t items = n * ((n + SALUN_BLOCK - 1) / SALUN_BLOCK);
  hipLaunchKernelGGL(k_svc_gram, dim3(salun_grid_for(items, 1)), dim3(SALUN_BLOCK), 0, salun_hip_stream(stream), X,
                     static_cast<float *>(ws), static_cast<int>(n), d, gamma);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_svc_rbf_fit(const uint8_t *y01, int64_t n, double C, double eps, int64_t max_iter, double *alpha,
                                   double *rho, int64_t *status, void *ws, size_t ws_bytes, salun_stream_t stream) {
  if (!n_ok(n) || !y01 || !alpha || !rho || !status || !ws) return SALUN_EINVAL;
  if (!positive_finite(C) || !positive_finite(eps) || max_iter < 0) return SALUN_EINVAL;
  if ((reinterpret_cast<uintptr_t>(alpha) & 7u) || (reinterpret_cast<uintptr_t>(rho) & 7u) ||
      (reinterpret_cast<uintptr_t>(status) & 7u) || !salun_aligned16(ws))
    return SALUN_EINVAL;
  if (ws_bytes < salun_svc_rbf_workspace_bytes(n)) return SALUN_ENOSPC;
  const size_t N = static_cast<size_t>(n);
  char *base = static_cast<char *>(ws);
  const float *K = reinterpret_cast<const float *>(base);
  double *G = reinterpret_cast<double *>(base + align16(N * N * sizeof(float)));
  uint8_t *state = reinterpret_cast<uint8_t *>(base + align16(N * N * sizeof(float)) + align16(N * sizeof(double)));
  hipLaunchKernelGGL(k_svc_fit, dim3(1), dim3(SVC_THREADS), 0, salun_hip_stream(stream), K, y01, static_cast<int>(n), C, eps,
                     max_iter, alpha, G, state, rho, status);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_svc_rbf_decision(const float *X, const double *coef, const double *rho, int64_t n, int d,
                                        double gamma, const float *Z, int64_t m, double *dec, uint8_t *pred,
                                        salun_stream_t stream) {
  if (n < 1 || n > SALUN_SVC_MAX_N || d < 1 || d > SALUN_SVC_MAX_D || m < 1 || m > (int64_t(1) << 40)) return SALUN_EINVAL;
  if (!X || !coef || !rho || !Z || (!dec && !pred) || !positive_finite(gamma)) return SALUN_EINVAL;
  if (!salun_aligned4(X) || !salun_aligned4(Z) || (reinterpret_cast<uintptr_t>(coef) & 7u) ||
      (reinterpret_cast<uintptr_t>(rho) & 7u) || (reinterpret_cast<uintptr_t>(dec) & 7u))
    return SALUN_EINVAL;
  hipLaunchKernelGGL(k_svc_decision, dim3(salun_grid_for(m, 1)), dim3(SALUN_BLOCK), 0, salun_hip_stream(stream), X, coef,
                     rho, static_cast<int>(n), d, gamma, Z, m, dec, pred);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_svc_rbf_gram_wide(const float *X, int64_t n, int d, double gamma, void *ws, size_t ws_bytes,
                                         salun_stream_t stream) {
  if (!n_ok(n) || d < 1 || d > SALUN_SVC_WIDE_MAX_D || !X || !ws || !positive_finite(gamma)) return SALUN_EINVAL;
  if (!salun_aligned4(X) || !salun_aligned16(ws)) return SALUN_EINVAL;
  if (ws_bytes < salun_svc_rbf_workspace_bytes(n)) return SALUN_ENOSPC;
  const int64_t items = n * ((n + SALUN_BLOCK - 1) / SALUN_BLOCK);
  hipLaunchKernelGGL(k_svc_gram_wide, dim3(salun_grid_for(items, 1)), dim3(SALUN_BLOCK), 0, salun_hip_stream(stream), X,
                     static_cast<float *>(ws), static_cast<int>(n), d, gamma);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_svc_rbf_decision_wide(const float *X, const double *coef, const double *rho, int64_t n, int d,
                                             double gamma, const float *Z, int64_t m, double *dec, uint8_t *pred,
                                             salun_stream_t stream) {
  if (n < 1 || n > SALUN_SVC_MAX_N || d < 1 || d > SALUN_SVC_WIDE_MAX_D || m < 1 || m > (int64_t(1) << 40))
    return SALUN_EINVAL;
  if (!X || !coef || !rho || !Z || (!dec && !pred) || !positive_finite(gamma)) return SALUN_EINVAL;
  if (!salun_aligned4(X) || !salun_aligned4(Z) || (reinterpret_cast<uintptr_t>(coef) & 7u) ||
      (reinterpret_cast<uintptr_t>(rho) & 7u) || (reinterpret_cast<uintptr_t>(dec) & 7u))
    return SALUN_EINVAL;
  hipLaunchKernelGGL(k_svc_decision_wide, dim3(salun_grid_for(m, 1)), dim3(SALUN_BLOCK), 0, salun_hip_stream(stream), X,
                     coef, rho, static_cast<int>(n), d, gamma, Z, m, dec, pred);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}
