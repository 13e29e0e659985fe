// salun_cls_head.hip — K23: the classifier head of a CIFAR ResNet as one forward launch and two backward launches.
// gfx950 / CDNA4, wave64, compiled with -ffp-contract=off (fused multiply-adds only where fmaf() is written).
//
//   AdaptiveAvgPool2d(1) -> flatten -> Linear -> CrossEntropyLoss(mean) -> argmax == target
//
// Layout.  One 256-thread workgroup owns one sample at a time (grid-stride over the batch).  x[b] is C planes of HW
// contiguous floats; lane t owns channels t, t + 256, ... and reads each plane front to back (float4 loads when HW is a
// multiple of 4 and x is 16-byte aligned: 16 x 512 floats per sample at the CIFAR shape).  The pooled row, the logits
// and the exponentials of the sample live in dynamic LDS (16-byte aligned base; (C + 2K) floats rounded up, at most
// 40 KiB), so the weight matrix is the only operand read from memory more than once (20 KiB at K = 10: L2 resident).
//
// Every reduction has ONE order, a function of the shape alone: per-lane chains in ascending index, the 64-lane
// shfl_down tree (offsets 32, 16, ..., 1), the four wave results through LDS folded as (w0 + w1) + (w2 + w3).  There
// is no floating-point atomic anywhere: the same inputs give the same bits on every run.
//
// Rounding points (tests/cls_head_ref_cpu.py derives its bounds from exactly these):
//   pooled   chain of the plane's float4 sums ((x + y) + (z + w)) [scalar route: of its elements], then ONE division by
//            (float)HW
//   logit_k  per-lane fmaf chain over c = lane, lane + 64, ..., the shuffle tree, then + bias[k]
//   t_k = logit_k - max;  e_k = expf(t_k);  S = sum_k e_k (per-lane chain over k = tid, tid + 256, ..., tree, fold)
//   p_k = e_k / S;  loss = logf(S) - t_y;  hit = (lowest index of the maximum == y)
//   scale = g / (float)B;  dlogit_k = (p_k - [k == y]) * scale
//   dx[c, :] = (fmaf chain over k = 0 .. K-1 of dlogit_k W[k, c]) / (float)HW
//   dW[k, c] = wave w's fmaf chain over b = w, w + 4, ..., folded (w0 + w1) + (w2 + w3);  accumulate: old + that
//   db[k]    = per-lane chain over b = tid, tid + 256, ..., tree, fold;  accumulate: old + that
//
// A label outside [0, K) reads and writes nothing out of range: the sample's loss and its dlogits / dx rows are NaN,
// its hit is 0, it is counted, and the NaN reaches loss_sum, loss_mean, dW and db through the sums.
//
// Accumulators.  hits is advanced with one integer atomic per workgroup (the order of integer adds does not matter).
// loss_sum needs one order: every workgroup stores its per-sample losses, fences and takes a ticket; the workgroup
// that draws the last ticket re-reads all B losses (device-scope loads), sums them in float64 in the fixed block order
// and adds the total to *loss_sum, B to *count, and writes the mean to *loss_mean.  The ticket (4 bytes of `ws`) is
// cleared by a memset ahead of the launch.
#include "salun_device.h"

namespace {

constexpr int MAX_C = SALUN_CLS_HEAD_MAX_C;
constexpr int MAX_K = SALUN_CLS_HEAD_MAX_K;

// Sum over the 256 threads, valid in EVERY thread.  `lds` holds 4 floats.
__device__ __forceinline__ float block_sum_f32(float v, float *lds) {
  v = salun_wave_sum_lane0(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  const float r = (lds[0] + lds[1]) + (lds[2] + lds[3]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ float quiet_nan() { return __int_as_float(0x7FC00000); }

__global__ __launch_bounds__(SALUN_BLOCK) void k_cls_head_fwd(
    const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias,
    const long long *__restrict__ labels, float *__restrict__ pooled, float *__restrict__ logits, float *__restrict__ p,
    float *loss, float *__restrict__ loss_mean, double *__restrict__ loss_sum, unsigned long long *__restrict__ hits,
    long long *__restrict__ count, int64_t B, int C, int HW, int K, int vec, unsigned int *ticket) {
  extern __shared__ float4 dyn4[];  // float4: the dynamic LDS base is 16-byte aligned
  float *pool_s = reinterpret_cast<float *>(dyn4);
  float *logit_s = pool_s + ((C + 3) & ~3);
  float *exp_s = logit_s + ((K + 3) & ~3);
  __shared__ float red_v[4];
  __shared__ int red_i[4];
  __shared__ double red_d[4];
  __shared__ unsigned int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float hwf = static_cast<float>(HW);
  unsigned int my_hits = 0;  // thread 0 only

  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    // ---- pooled[c] = mean over the plane
    for (int c = tid; c < C; c += SALUN_BLOCK) {
      const float *xc = x + (b * C + c) * static_cast<int64_t>(HW);
      float acc = 0.0f;
      if (vec) {
        const float4 *x4 = reinterpret_cast<const float4 *>(xc);
        for (int j = 0; j < (HW >> 2); ++j) {
          const float4 v = x4[j];
          acc = acc + ((v.x + v.y) + (v.z + v.w));
        }
      } else {
        for (int j = 0; j < HW; ++j) acc = acc + xc[j];
      }
      const float pv = acc / hwf;
      pool_s[c] = pv;
      pooled[b * C + c] = pv;
    }
    __syncthreads();
    // ---- logits: one wave per class
    for (int k = wave; k < K; k += 4) {
      const float *wk = w + static_cast<int64_t>(k) * C;
      float acc = 0.0f;
      for (int c = lane; c < C; c += 64) acc = fmaf(pool_s[c], wk[c], acc);
      acc = salun_wave_sum_lane0(acc);
      if (lane == 0) {
        const float l = acc + bias[k];
        logit_s[k] = l;
        logits[b * K + k] = l;
      }
    }
    __syncthreads();
    // ---- maximum and its lowest index
    float mv = -INFINITY;
    int mi = 0x7FFFFFFF;
    for (int k = tid; k < K; k += SALUN_BLOCK) {
      const float v = logit_s[k];
      if (v > mv || mi == 0x7FFFFFFF) { mv = v; mi = k; }  // ascending k: a later equal value does not replace
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_down(mv, off, 64);
      const int oi = __shfl_down(mi, off, 64);
      if (oi != 0x7FFFFFFF && (mi == 0x7FFFFFFF || ov > mv || (ov == mv && oi < mi))) { mv = ov; mi = oi; }
    }
    if (lane == 0) { red_v[wave] = mv; red_i[wave] = mi; }
    __syncthreads();
    mv = red_v[0];
    mi = red_i[0];
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      const float ov = red_v[q];
      const int oi = red_i[q];
      if (oi != 0x7FFFFFFF && (mi == 0x7FFFFFFF || ov > mv || (ov == mv && oi < mi))) { mv = ov; mi = oi; }
    }
    __syncthreads();
    // ---- exponentials and their sum
    float part = 0.0f;
    for (int k = tid; k < K; k += SALUN_BLOCK) {
      const float e = expf(logit_s[k] - mv);
      exp_s[k] = e;
      part = part + e;
    }
    const float S = block_sum_f32(part, red_v);
    for (int k = tid; k < K; k += SALUN_BLOCK) p[b * K + k] = exp_s[k] / S;
    if (tid == 0) {
      const long long y = labels[b];
      const bool ok = y >= 0 && y < K;
      loss[b] = ok ? (logf(S) - (logit_s[y] - mv)) : quiet_nan();
      if (ok && mi == static_cast<int>(y)) ++my_hits;
    }
    __syncthreads();  // the LDS rows are rewritten by the next sample
  }

  if (!ticket) return;
  // ---- accumulators: the workgroup with the last ticket folds the per-sample losses in one fixed order
  if (tid == 0) {
    if (hits && my_hits) atomicAdd(hits, static_cast<unsigned long long>(my_hits));
    __threadfence();  // thread 0 wrote this workgroup's losses itself: its release covers them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the write-back has landed before the ticket is drawn
    s_last = (atomicAdd(ticket, 1u) == gridDim.x - 1) ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  double acc = 0.0;
  for (int64_t b = tid; b < B; b += SALUN_BLOCK) {
    const int bits = __hip_atomic_load(reinterpret_cast<int *>(loss) + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    acc += static_cast<double>(__int_as_float(bits));
  }
  const double tot = salun_block_sum(acc, red_d);
  if (tid == 0) {
    if (loss_sum) *loss_sum += tot;
    if (count) *count += static_cast<long long>(B);
    if (loss_mean) *loss_mean = static_cast<float>(tot / static_cast<double>(B));
  }
}

// dlogits, and dx = (dlogits W) / HW broadcast over the plane.
__global__ __launch_bounds__(SALUN_BLOCK) void k_cls_head_bwd_x(
    const float *__restrict__ p, const float *__restrict__ w, const long long *__restrict__ labels,
    const float *__restrict__ grad_out, float *__restrict__ dlogits, float *__restrict__ dx, int64_t B, int C, int HW,
    int K, int vec) {
  extern __shared__ float4 dyn4[];
  float *d_s = reinterpret_cast<float *>(dyn4);
  const int tid = threadIdx.x;
  const float g = grad_out ? grad_out[0] : 1.0f;
  const float scale = g / static_cast<float>(B);
  const float hwf = static_cast<float>(HW);
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const long long y = labels[b];
    const bool ok = y >= 0 && y < K;
    for (int k = tid; k < K; k += SALUN_BLOCK) {
      const float pk = p[b * K + k];
      const float q = (k == y) ? (pk - 1.0f) : pk;
      const float d = ok ? (q * scale) : quiet_nan();
      d_s[k] = d;
      dlogits[b * K + k] = d;
    }
    __syncthreads();
    if (dx) {
      for (int c = tid; c < C; c += SALUN_BLOCK) {
        float acc = 0.0f;
        for (int k = 0; k < K; ++k) acc = fmaf(d_s[k], w[static_cast<int64_t>(k) * C + c], acc);
        const float v = acc / hwf;
        float *dst = dx + (b * C + c) * static_cast<int64_t>(HW);
        if (vec) {
          const float4 v4 = make_float4(v, v, v, v);
          for (int j = 0; j < (HW >> 2); ++j) reinterpret_cast<float4 *>(dst)[j] = v4;
        } else {
          for (int j = 0; j < HW; ++j) dst[j] = v;
        }
      }
    }
    __syncthreads();
  }
}

// grid (ctiles + 1, K): column x < ctiles is the 64-channel tile x of dW[k, :], column ctiles is db[k].
__global__ __launch_bounds__(SALUN_BLOCK) void k_cls_head_bwd_w(const float *__restrict__ dlogits,
                                                                const float *__restrict__ pooled, float *dw, float *db,
                                                                int acc_w, int acc_b, int64_t B, int C, int K,
                                                                int ctiles) {
  __shared__ float part[4][64];
  __shared__ float red_v[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = blockIdx.y;
  if (static_cast<int>(blockIdx.x) < ctiles) {
    if (!dw) return;
    const int c = blockIdx.x * 64 + lane;
    float acc = 0.0f;
    if (c < C)
      for (int64_t b = wave; b < B; b += 4) acc = fmaf(dlogits[b * K + k], pooled[b * C + c], acc);
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && c < C) {
      const float r = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
      float *dst = dw + static_cast<int64_t>(k) * C + c;
      *dst = acc_w ? (*dst + r) : r;
    }
  } else {
    if (!db) return;
    float acc = 0.0f;
    for (int64_t b = tid; b < B; b += SALUN_BLOCK) acc = acc + dlogits[b * K + k];
    const float r = block_sum_f32(acc, red_v);
    if (tid == 0) db[k] = acc_b ? (db[k] + r) : r;
  }
}

// ---- the evaluation head: pool -> fc -> softmax of K23's forward (the same statements, the same rounding points), then
// the three figures DDPM/classifier_evaluation.py reports, for ONE label shared by the whole batch:
//   ent_b  = -(sum_k p_k * logf(p_k))   per-lane chain over k = tid, tid + 256, ..., tree, fold; zero_safe: a term with
//            p_k == 0 is 0 instead of 0 * -inf = NaN
//   prob_b = p[b, label]                hit_b = (lowest index of the row's maximum == label)
// ent_b and prob_b go to `ws` (floats 4 .. 4 + 2B after the 16-byte ticket); the workgroup with the last ticket folds
// them in float64 in index order and adds the totals to the caller's meters.
__global__ __launch_bounds__(SALUN_BLOCK) void k_cls_head_eval(
    const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias, int label,
    float *__restrict__ logits, float *__restrict__ p, float *per, double *__restrict__ entropy_sum,
    double *__restrict__ prob_sum, unsigned long long *__restrict__ hits, long long *__restrict__ count, int64_t B, int C,
    int HW, int K, int vec, int zero_safe, unsigned int *ticket) {
  extern __shared__ float4 dyn4[];
  float *pool_s = reinterpret_cast<float *>(dyn4);
  float *logit_s = pool_s + ((C + 3) & ~3);
  float *exp_s = logit_s + ((K + 3) & ~3);
  __shared__ float red_v[4];
  __shared__ int red_i[4];
  __shared__ double red_d[4];
  __shared__ unsigned int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float hwf = static_cast<float>(HW);
  unsigned int my_hits = 0;  // thread 0 only

  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    for (int c = tid; c < C; c += SALUN_BLOCK) {
      const float *xc = x + (b * C + c) * static_cast<int64_t>(HW);
      float acc = 0.0f;
      if (vec) {
        const float4 *x4 = reinterpret_cast<const float4 *>(xc);
        for (int j = 0; j < (HW >> 2); ++j) {
          const float4 v = x4[j];
          acc = acc + ((v.x + v.y) + (v.z + v.w));
        }
      } else {
        for (int j = 0; j < HW; ++j) acc = acc + xc[j];
      }
      pool_s[c] = acc / hwf;
    }
    __syncthreads();
    for (int k = wave; k < K; k += 4) {
      const float *wk = w + static_cast<int64_t>(k) * C;
      float acc = 0.0f;
      for (int c = lane; c < C; c += 64) acc = fmaf(pool_s[c], wk[c], acc);
      acc = salun_wave_sum_lane0(acc);
      if (lane == 0) {
        const float l = acc + bias[k];
        logit_s[k] = l;
        logits[b * K + k] = l;
      }
    }
    __syncthreads();
    float mv = -INFINITY;
    int mi = 0x7FFFFFFF;
    for (int k = tid; k < K; k += SALUN_BLOCK) {
      const float v = logit_s[k];
      if (v > mv || mi == 0x7FFFFFFF) { mv = v; mi = k; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_down(mv, off, 64);
      const int oi = __shfl_down(mi, off, 64);
      if (oi != 0x7FFFFFFF && (mi == 0x7FFFFFFF || ov > mv || (ov == mv && oi < mi))) { mv = ov; mi = oi; }
    }
    if (lane == 0) { red_v[wave] = mv; red_i[wave] = mi; }
    __syncthreads();
    mv = red_v[0];
    mi = red_i[0];
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      const float ov = red_v[q];
      const int oi = red_i[q];
      if (oi != 0x7FFFFFFF && (mi == 0x7FFFFFFF || ov > mv || (ov == mv && oi < mi))) { mv = ov; mi = oi; }
    }
    __syncthreads();
    float part = 0.0f;
    for (int k = tid; k < K; k += SALUN_BLOCK) {
      const float e = expf(logit_s[k] - mv);
      exp_s[k] = e;
      part = part + e;
    }
    const float S = block_sum_f32(part, red_v);
    float epart = 0.0f;
    for (int k = tid; k < K; k += SALUN_BLOCK) {
      const float pk = exp_s[k] / S;
      p[b * K + k] = pk;
      const float term = (zero_safe && pk == 0.0f) ? 0.0f : pk * logf(pk);
      epart = epart + term;
    }
    const float esum = block_sum_f32(epart, red_v);
    if (tid == 0) {
      per[b] = -esum;
      per[B + b] = exp_s[label] / S;
      if (mi == label) ++my_hits;
    }
    __syncthreads();
  }

  if (tid == 0) {
    if (hits && my_hits) atomicAdd(hits, static_cast<unsigned long long>(my_hits));
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = (atomicAdd(ticket, 1u) == gridDim.x - 1) ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  double e_acc = 0.0, p_acc = 0.0;
  for (int64_t b = tid; b < B; b += SALUN_BLOCK) {
    const int eb = __hip_atomic_load(reinterpret_cast<int *>(per) + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int pb = __hip_atomic_load(reinterpret_cast<int *>(per) + B + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    e_acc += static_cast<double>(__int_as_float(eb));
    p_acc += static_cast<double>(__int_as_float(pb));
  }
  const double e_tot = salun_block_sum(e_acc, red_d);
  const double p_tot = salun_block_sum(p_acc, red_d);
  if (tid == 0) {
    if (entropy_sum) *entropy_sum += e_tot;
    if (prob_sum) *prob_sum += p_tot;
    if (count) *count += static_cast<long long>(B);
  }
}

bool shape_ok(int64_t B, int C, int HW, int K) {
  return B >= 1 && B <= (int64_t(1) << 31) - 1 && C >= 1 && C <= MAX_C && HW >= 1 && HW <= (1 << 20) && K >= 1 &&
         K <= MAX_K;
}
bool aligned8(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 7u) == 0; }

}  // namespace

SALUN_EXPORT size_t salun_cls_head_workspace_bytes(int64_t B, int C, int K) {
  if (B < 1 || C < 1 || C > MAX_C || K < 1 || K > MAX_K) return 0;
  return 16;  // the ticket
}

SALUN_EXPORT int salun_cls_head_forward(const float *x, const float *w, const float *bias, const int64_t *labels,
                                        float *pooled, float *logits, float *p, float *loss, float *loss_mean,
                                        double *loss_sum, int64_t *hits, int64_t *count, int64_t B, int C, int HW, int K,
                                        void *ws, size_t ws_bytes, salun_stream_t stream) {
  if (!shape_ok(B, C, HW, K)) return SALUN_EINVAL;
  if (!x || !w || !bias || !labels || !pooled || !logits || !p || !loss) return SALUN_EINVAL;
  if (!salun_aligned4(x) || !salun_aligned4(w) || !salun_aligned4(bias) || !aligned8(labels) || !salun_aligned4(pooled) ||
      !salun_aligned4(logits) || !salun_aligned4(p) || !salun_aligned4(loss) || !salun_aligned4(loss_mean) ||
      !aligned8(loss_sum) || !aligned8(hits) || !aligned8(count))
    return SALUN_EINVAL;
  const bool folds = loss_mean || loss_sum || hits || count;
  if (folds) {
    if (!ws || !salun_aligned4(ws)) return SALUN_EINVAL;
    if (ws_bytes < salun_cls_head_workspace_bytes(B, C, K)) return SALUN_ENOSPC;
  }
  hipStream_t st = salun_hip_stream(stream);
  unsigned int *ticket = folds ? static_cast<unsigned int *>(ws) : nullptr;
  if (ticket && hipMemsetAsync(ticket, 0, sizeof(unsigned int), st) != hipSuccess) return SALUN_EIO;
  const int vec = salun_aligned16(x) && (HW % 4 == 0);
  const size_t lds = sizeof(float) * static_cast<size_t>(((C + 3) & ~3) + 2 * ((K + 3) & ~3));
  hipLaunchKernelGGL(k_cls_head_fwd, dim3(salun_grid_for(B, 1)), dim3(SALUN_BLOCK), lds, st, x, w, bias,
                     reinterpret_cast<const long long *>(labels), pooled, logits, p, loss, loss_mean, loss_sum,
                     reinterpret_cast<unsigned long long *>(hits), reinterpret_cast<long long *>(count), B, C, HW, K, vec,
                     ticket);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_cls_head_backward(const float *p, const float *pooled, const float *w, const int64_t *labels,
                                         const float *grad_out, float *dlogits, float *dx, float *dw, float *db,
                                         int accumulate_w, int accumulate_b, int64_t B, int C, int HW, int K,
                                         salun_stream_t stream) {
  if (!shape_ok(B, C, HW, K)) return SALUN_EINVAL;
  if (!p || !pooled || !w || !labels || !dlogits) return SALUN_EINVAL;
  if (!salun_aligned4(p) || !salun_aligned4(pooled) || !salun_aligned4(w) || !aligned8(labels) ||
      !salun_aligned4(grad_out) || !salun_aligned4(dlogits) || !salun_aligned4(dx) || !salun_aligned4(dw) ||
      !salun_aligned4(db))
    return SALUN_EINVAL;
  hipStream_t st = salun_hip_stream(stream);
  const int vec = dx && salun_aligned16(dx) && (HW % 4 == 0);
  hipLaunchKernelGGL(k_cls_head_bwd_x, dim3(salun_grid_for(B, 1)), dim3(SALUN_BLOCK),
                     sizeof(float) * static_cast<size_t>((K + 3) & ~3), st, p, w,
                     reinterpret_cast<const long long *>(labels), grad_out, dlogits, dx, B, C, HW, K, vec);
  SALUN_LAUNCH_CHECK();
  if (dw || db) {
    const int ctiles = (C + 63) / 64;
    hipLaunchKernelGGL(k_cls_head_bwd_w, dim3(ctiles + 1, K), dim3(SALUN_BLOCK), 0, st, dlogits, pooled, dw, db,
                       accumulate_w ? 1 : 0, accumulate_b ? 1 : 0, B, C, K, ctiles);
    SALUN_LAUNCH_CHECK();
  }
  return SALUN_OK;
}

SALUN_EXPORT size_t salun_cls_head_eval_workspace_bytes(int64_t B, int C, int K) {
  if (B < 1 || B > (int64_t(1) << 31) - 1 || C < 1 || C > MAX_C || K < 1 || K > MAX_K) return 0;
  return 16 + 2 * sizeof(float) * static_cast<size_t>(B);  // the ticket, then ent[B] and prob[B]
}

SALUN_EXPORT int salun_cls_head_eval(const float *x, const float *w, const float *bias, int label, float *logits, float *p,
                                     double *entropy_sum, double *prob_sum, int64_t *hits, int64_t *count, int64_t B,
                                     int C, int HW, int K, int zero_safe, void *ws, size_t ws_bytes,
                                     salun_stream_t stream) {
  if (!shape_ok(B, C, HW, K) || label < 0 || label >= K) return SALUN_EINVAL;
  if (!x || !w || !bias || !logits || !p || !ws) return SALUN_EINVAL;
  if (!salun_aligned4(x) || !salun_aligned4(w) || !salun_aligned4(bias) || !salun_aligned4(logits) || !salun_aligned4(p) ||
      !aligned8(entropy_sum) || !aligned8(prob_sum) || !aligned8(hits) || !aligned8(count) || !salun_aligned4(ws))
    return SALUN_EINVAL;
  if (ws_bytes < salun_cls_head_eval_workspace_bytes(B, C, K)) return SALUN_ENOSPC;
  hipStream_t st = salun_hip_stream(stream);
  unsigned int *ticket = static_cast<unsigned int *>(ws);
  if (hipMemsetAsync(ticket, 0, sizeof(unsigned int), st) != hipSuccess) return SALUN_EIO;
  const int vec = salun_aligned16(x) && (HW % 4 == 0);
  const size_t lds = sizeof(float) * static_cast<size_t>(((C + 3) & ~3) + 2 * ((K + 3) & ~3));
  hipLaunchKernelGGL(k_cls_head_eval, dim3(salun_grid_for(B, 1)), dim3(SALUN_BLOCK), lds, st, x, w, bias, label, logits, p,
                     reinterpret_cast<float *>(ticket + 4), entropy_sum, prob_sum,
                     reinterpret_cast<unsigned long long *>(hits), reinterpret_cast<long long *>(count), B, C, HW, K, vec,
                     zero_safe ? 1 : 0, ticket);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}
