// salun_sampler.hip — K19: the reverse-process sampler's own kernels (include/salun.h).
//
//   salun_sampler_step    one reverse step of the CFG-DDPM in one launch: guidance combine, x0 estimate (clamped for the
//                         ancestral variant), posterior mean or DDIM update, noise term.  The coefficients are computed
//                         in the kernel from two entries of the device alpha-bar table, in the operation order of
//                         DDPM/functions/denoising.py:_loop.  The noise is an explicit tensor or the counter-based
//                         normal of salun_fill_normal on the key (seed, step, image id): row b of the batch gets
//                         fill_normal(chw, salun_sampler key)[e], so an image does not depend on the batch around it.
//   salun_sampler_noise   the same keyed normal written out (the start noise x_T; the parity tests).
//   salun_minmax          min and max of a vector in two fixed-order stages (no float atomics).
//   salun_images_to_u8    inverse data transform + min-max normalisation + *255 + 0.5 -> uint8 HWC, one workgroup per
//                         image; the image is read once into LDS and reduced there.
//
// K21: salun_ldm_ddim_step  one reverse step of the LDM DDIM sampler (ldm/models/diffusion/ddim.py, p_sample_ddim) on
//                         latents: guidance combine over the two halves of ONE batched U-Net output (read in place, no
//                         chunk copy), x0 estimate, direction term, optional noise.  The five coefficients are fp32 scalars
//                         the host computed from the DDIM tables; the kernel recomputes none.  Every operation is one
//                         correctly rounded fp32 operation in the reference's order (this file is built with
//                         -ffp-contract=off, IEEE division, no fast-math), so the result is bit-comparable with numpy.
//                         At the workload's size (4 x 64 x 64 = 16,384 elements) the step is bound by launch latency, not
//                         by bandwidth: what it buys is one launch in place of the ~20 small ones the expression costs in
//                         torch (cat, chunk, four torch.full, ten elementwise operations) between two U-Net passes, 50
//                         times per ESD iteration.
//
//     salun_lms_step      one step of the evaluation script's linear multistep sampler (SD/lms.py): the
//                         guided derivative from the two halves of ONE batched U-Net output, stored into a 4-deep ring,
//                         x + c0 d + c1 d1 + ... accumulated in that order, the new x written, and x_new / den written
//                         into both halves of the tensor the next pass reads.  The coefficients are the host's (closed
//                         form in float64); same rounding rules as salun_ldm_ddim_step.
//
// All of them are memory / latency bound; 16-byte loads and stores where the shapes allow.
#include "salun_common.h"

namespace {

__device__ __forceinline__ uint64_t sampler_key(uint64_t seed, uint64_t step, uint64_t image_id) {
  return salun_splitmix64(salun_splitmix64(salun_splitmix64(seed) + step) + image_id);
}

struct StepCoef {
  // ancestral: x0 = clamp(a * x - b * e), next = (m1 * x0 + m2 * x) / den + sig * z
  // generalized: x0 = (x - e * b) / a, next = m1 * x0 + sig * z + m2 * e
  float a, b, m1, m2, den, sig;
};

// Same operations in the same order as denoising._loop (fp32, no contraction): the scalars there are 0-dim fp32 tensors.
__device__ __forceinline__ StepCoef step_coef(float at, float an, int ancestral, float eta, int first) {
  StepCoef k;
  if (ancestral) {
    const float beta_t = 1.0f - at / an;
    k.a = sqrtf(1.0f / at);
    k.b = sqrtf(1.0f / at - 1.0f);
    k.m1 = sqrtf(an) * beta_t;
    k.m2 = sqrtf(1.0f - beta_t) * (1.0f - an);
    k.den = 1.0f - at;
    k.sig = first ? 0.0f : expf(0.5f * logf(beta_t));
  } else {
    k.a = sqrtf(at);
    k.b = sqrtf(1.0f - at);
    k.m1 = sqrtf(an);
    const float c1 = eta * sqrtf((1.0f - at / an) * (1.0f - an) / (1.0f - at));
    k.m2 = sqrtf((1.0f - an) - c1 * c1);
    k.den = 1.0f;
    k.sig = c1;
  }
  return k;
}

__device__ __forceinline__ void step_elem(float x, float ec, float en, float z, int guided, float s1, float s,
                                          int ancestral, const StepCoef &k, float &nxt, float &x0) {
  const float e = guided ? (s1 * ec - s * en) : ec;
  if (ancestral) {
    float v = k.a * x - k.b * e;
    v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
    x0 = v;
    const float mean = (k.m1 * v + k.m2 * x) / k.den;
    nxt = mean + k.sig * z;
  } else {
    x0 = (x - e * k.b) / k.a;
    nxt = (k.m1 * x0 + k.sig * z) + k.m2 * e;
  }
}

// x_next may alias x_t (and x0 nothing else): every element is read before it is written, by the same thread.
template <int VEC>
__global__ __launch_bounds__(SALUN_BLOCK) void k_sampler_step(const float *x, const float *ec, const float *en, float s1,
                                                              float s, const float *__restrict__ abar, int it, int in,
                                                              int ancestral, float eta, const float *noise, int draw,
                                                              uint64_t seed, const long long *__restrict__ ids,
                                                              uint64_t step, float *xn, float *x0, int64_t B,
                                                              int64_t chw) {
  const StepCoef k = step_coef(abar[it], abar[in], ancestral, eta, it == 1);
  const uint64_t skey = salun_splitmix64(salun_splitmix64(seed) + step);
  const int guided = en != nullptr;
  const int64_t per = chw / VEC, total = B * per;
  for (int64_t i = (int64_t)blockIdx.x * SALUN_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * SALUN_BLOCK) {
    const int64_t row = i / per, e0 = (i - row * per) * VEC, off = row * chw + e0;
    float vx[VEC], vc[VEC], vn[VEC], vz[VEC], o[VEC], p[VEC];
    if (VEC == 4) {
      *reinterpret_cast<float4 *>(vx) = *reinterpret_cast<const float4 *>(x + off);
      *reinterpret_cast<float4 *>(vc) = *reinterpret_cast<const float4 *>(ec + off);
      if (guided) *reinterpret_cast<float4 *>(vn) = *reinterpret_cast<const float4 *>(en + off);
      if (noise) *reinterpret_cast<float4 *>(vz) = *reinterpret_cast<const float4 *>(noise + off);
    } else {
      vx[0] = x[off];
      vc[0] = ec[off];
      if (guided) vn[0] = en[off];
      if (noise) vz[0] = noise[off];
    }
    if (!noise) {
      if (draw) {
        const uint64_t key = salun_splitmix64(skey + (uint64_t)ids[row]);
#pragma unroll
        for (int j = 0; j < VEC; ++j) vz[j] = salun_ih12(key, (uint64_t)(e0 + j));
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) vz[j] = 0.0f;
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) step_elem(vx[j], vc[j], guided ? vn[j] : 0.0f, vz[j], guided, s1, s, ancestral, k, o[j], p[j]);
    if (VEC == 4) {
      *reinterpret_cast<float4 *>(xn + off) = *reinterpret_cast<const float4 *>(o);
      if (x0) *reinterpret_cast<float4 *>(x0 + off) = *reinterpret_cast<const float4 *>(p);
    } else {
      xn[off] = o[0];
      if (x0) x0[off] = p[0];
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(SALUN_BLOCK) void k_sampler_noise(float *__restrict__ out, uint64_t seed,
                                                               const long long *__restrict__ ids, uint64_t step,
                                                               int64_t B, int64_t chw) {
  const uint64_t skey = salun_splitmix64(salun_splitmix64(seed) + step);
  const int64_t per = chw / VEC, total = B * per;
  for (int64_t i = (int64_t)blockIdx.x * SALUN_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * SALUN_BLOCK) {
    const int64_t row = i / per, e0 = (i - row * per) * VEC, off = row * chw + e0;
    const uint64_t key = salun_splitmix64(skey + (uint64_t)ids[row]);
    float z[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) z[j] = salun_ih12(key, (uint64_t)(e0 + j));
    if (VEC == 4) {
      *reinterpret_cast<float4 *>(out + off) = *reinterpret_cast<const float4 *>(z);
    } else {
      out[off] = z[0];
    }
  }
}

// ------------------------------------------------------------------ min / max
__device__ __forceinline__ void wave_minmax(float &lo, float &hi) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off, 64));
    hi = fmaxf(hi, __shfl_xor(hi, off, 64));
  }
}
// Block min / max for 256 threads, valid in every thread.  `lds` needs 8 floats.
__device__ __forceinline__ void block_minmax(float &lo, float &hi, float *lds) {
  wave_minmax(lo, hi);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    lds[wave] = lo;
    lds[4 + wave] = hi;
  }
  __syncthreads();
  lo = fminf(fminf(lds[0], lds[1]), fminf(lds[2], lds[3]));
  hi = fmaxf(fmaxf(lds[4], lds[5]), fmaxf(lds[6], lds[7]));
  __syncthreads();
}

#define MINMAX_BLOCKS 256

__global__ __launch_bounds__(SALUN_BLOCK) void k_minmax_partial(const float *__restrict__ x, int64_t n, int vec,
                                                                float *__restrict__ partial) {
  __shared__ float lds[8];
  float lo = INFINITY, hi = -INFINITY;
  const int64_t tid = (int64_t)blockIdx.x * SALUN_BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * SALUN_BLOCK;
  if (vec) {
    const int64_t n4 = n >> 2;
    for (int64_t i = tid; i < n4; i += stride) {
      const float4 v = reinterpret_cast<const float4 *>(x)[i];
      lo = fminf(fminf(lo, v.x), fminf(v.y, fminf(v.z, v.w)));
      hi = fmaxf(fmaxf(hi, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
    }
    for (int64_t i = (n4 << 2) + tid; i < n; i += stride) {
      lo = fminf(lo, x[i]);
      hi = fmaxf(hi, x[i]);
    }
  } else {
    for (int64_t i = tid; i < n; i += stride) {
      lo = fminf(lo, x[i]);
      hi = fmaxf(hi, x[i]);
    }
  }
  block_minmax(lo, hi, lds);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = lo;
    partial[2 * blockIdx.x + 1] = hi;
  }
}
__global__ __launch_bounds__(SALUN_BLOCK) void k_minmax_final(const float *__restrict__ partial, int nblocks,
                                                              float *__restrict__ lohi) {
  __shared__ float lds[8];
  float lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < nblocks; i += SALUN_BLOCK) {
    lo = fminf(lo, partial[2 * i]);
    hi = fmaxf(hi, partial[2 * i + 1]);
  }
  block_minmax(lo, hi, lds);
  if (threadIdx.x == 0) {
    lohi[0] = lo;
    lohi[1] = hi;
  }
}

// ------------------------------------------------------------------ float CHW -> uint8 HWC
// `inverse_data_transform` ((x + 1) / 2 when rescaled, clamp to [0, 1]) followed by torchvision's
// save_image(normalize=True): clamp to [lo, hi], (v - lo) / max(hi - lo, 1e-5), * 255 + 0.5, clamp to [0, 255], truncate.
__device__ __forceinline__ float to_unit(float x, int rescaled) {
  float v = rescaled ? (x + 1.0f) / 2.0f : x;
  return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
}
__device__ __forceinline__ uint32_t to_byte(float v, float lo, float hi, float den) {
  v = v < lo ? lo : (v > hi ? hi : v);
  float q = ((v - lo) / den) * 255.0f + 0.5f;
  q = q < 0.0f ? 0.0f : (q > 255.0f ? 255.0f : q);
  return (uint32_t)q;
}

__global__ __launch_bounds__(SALUN_BLOCK) void k_images_to_u8(const float *__restrict__ x, uint8_t *__restrict__ out,
                                                              int C, int HW, int rescaled,
                                                              const float *__restrict__ range, int vec_in, int vec_out) {
  extern __shared__ __attribute__((aligned(16))) float img[];  // chw floats, then 8 for the reduction
  const int chw = C * HW;
  float *red = img + ((chw + 3) & ~3);
  const float *src = x + (int64_t)blockIdx.x * chw;
  float lo = INFINITY, hi = -INFINITY;
  if (vec_in) {
    for (int i = threadIdx.x; i < (chw >> 2); i += SALUN_BLOCK) {
      float4 v = reinterpret_cast<const float4 *>(src)[i];
      v.x = to_unit(v.x, rescaled);
      v.y = to_unit(v.y, rescaled);
      v.z = to_unit(v.z, rescaled);
      v.w = to_unit(v.w, rescaled);
      reinterpret_cast<float4 *>(img)[i] = v;
      lo = fminf(fminf(lo, v.x), fminf(v.y, fminf(v.z, v.w)));
      hi = fmaxf(fmaxf(hi, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
    }
  } else {
    for (int i = threadIdx.x; i < chw; i += SALUN_BLOCK) {
      const float v = to_unit(src[i], rescaled);
      img[i] = v;
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
  }
  block_minmax(lo, hi, red);  // (its barrier also publishes img[])
  if (range) {  // the caller's range is in the units of x: mapped like the pixels (the map is monotone)
    lo = to_unit(range[0], rescaled);
    hi = to_unit(range[1], rescaled);
  }
  const float den = fmaxf(hi - lo, 1e-5f);
  uint8_t *dst = out + (int64_t)blockIdx.x * chw;
  if (vec_out) {  // four output bytes (HWC order) per store
    for (int w = threadIdx.x; w < (chw >> 2); w += SALUN_BLOCK) {
      uint32_t word = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int o = 4 * w + j, p = o / C, c = o - p * C;
        word |= to_byte(img[c * HW + p], lo, hi, den) << (8 * j);
      }
      reinterpret_cast<uint32_t *>(dst)[w] = word;
    }
  } else {
    for (int o = threadIdx.x; o < chw; o += SALUN_BLOCK) {
      const int p = o / C, c = o - p * C;
      dst[o] = (uint8_t)to_byte(img[c * HW + p], lo, hi, den);
    }
  }
}

// ------------------------------------------------------------------ K21: LDM DDIM step on latents
struct LdmCoef {
  float scale, s1m, sqrt_at, dir, sqrt_aprev, sigma;
};

__device__ __forceinline__ void ldm_elem(float x, float eu, float ec, float z, int guided, int noisy, const LdmCoef &k,
                                         float &nxt, float &x0) {
  float e = ec;
  if (guided) {
    const float d = ec - eu;
    const float sd = k.scale * d;
    e = eu + sd;
  }
  const float se = k.s1m * e;
  const float num = x - se;
  x0 = num / k.sqrt_at;
  const float dir = k.dir * e;
  const float ax = k.sqrt_aprev * x0;
  float v = ax + dir;
  if (noisy) {
    const float sz = k.sigma * z;
    v = v + sz;
  }
  nxt = v;
}

// x_prev may alias x: every element is read before it is written, by the same thread.  eu == nullptr: no guidance.
template <int VEC>
__global__ __launch_bounds__(SALUN_BLOCK) void k_ldm_ddim_step(const float *x, const float *eu, const float *ec,
                                                               LdmCoef k, const float *z, float *xp, float *x0,
                                                               int64_t total) {
  const int guided = eu != nullptr, noisy = z != nullptr;
  for (int64_t i = (int64_t)blockIdx.x * SALUN_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * SALUN_BLOCK) {
    const int64_t off = i * VEC;
    float vx[VEC], vu[VEC], vc[VEC], vz[VEC], o[VEC], p[VEC];
    if (VEC == 4) {
      *reinterpret_cast<float4 *>(vx) = *reinterpret_cast<const float4 *>(x + off);
      *reinterpret_cast<float4 *>(vc) = *reinterpret_cast<const float4 *>(ec + off);
      if (guided) *reinterpret_cast<float4 *>(vu) = *reinterpret_cast<const float4 *>(eu + off);
      if (noisy) *reinterpret_cast<float4 *>(vz) = *reinterpret_cast<const float4 *>(z + off);
    } else {
      vx[0] = x[off];
      vc[0] = ec[off];
      if (guided) vu[0] = eu[off];
      if (noisy) vz[0] = z[off];
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      ldm_elem(vx[j], guided ? vu[j] : 0.0f, vc[j], noisy ? vz[j] : 0.0f, guided, noisy, k, o[j], p[j]);
    if (VEC == 4) {
      *reinterpret_cast<float4 *>(xp + off) = *reinterpret_cast<const float4 *>(o);
      if (x0) *reinterpret_cast<float4 *>(x0 + off) = *reinterpret_cast<const float4 *>(p);
    } else {
      xp[off] = o[0];
      if (x0) x0[off] = p[0];
    }
  }
}

#define IMAGES_U8_MAX_CHW 16000  // 64000 bytes of LDS for the image + the reduction slots: no dynamic-LDS opt-in needed

int step_grid(int64_t items) {
  int64_t b = (items + SALUN_BLOCK - 1) / SALUN_BLOCK;
  if (b < 1) b = 1;
  if (b > 16 * SALUN_MAX_GRID) b = 16 * SALUN_MAX_GRID;
  return (int)b;
}

struct LmsCoef {
  float scale, c[4], den;
};

// One element per thread, grid-stride.  x_new may alias x (an element is read before it is written, by one thread);
// hist and x_in alias nothing (the entry point refuses it).  eu == nullptr: no guidance.
__global__ __launch_bounds__(SALUN_BLOCK) void k_lms_step(const float *x, const float *eu, const float *ec, LmsCoef k,
                                                          float *hist, int slot, int order, float *xn, float *xin,
                                                          int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * SALUN_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * SALUN_BLOCK) {
    float d = ec[i];
    if (eu) {
      const float u = eu[i];
      const float df = d - u;
      const float sd = k.scale * df;
      d = u + sd;
    }
    hist[(int64_t)slot * total + i] = d;
    const float t0 = k.c[0] * d;
    float a = x[i] + t0;
    for (int j = 1; j < order; ++j) {
      const float dj = hist[(int64_t)((slot - j) & 3) * total + i];
      const float t = k.c[j] * dj;
      a = a + t;
    }
    xn[i] = a;
    if (xin) {
      const float v = a / k.den;
      xin[i] = v;
      if (eu) xin[total + i] = v;
    }
  }
}

}  // namespace

// ================================================================== C-ABI =======
SALUN_EXPORT int salun_sampler_step(const float *x_t, const float *eps_cond, const float *eps_null, double cond_scale,
                                    const float *abar, int table_len, int idx_t, int idx_next, int variant, double eta,
                                    const float *noise, uint64_t seed, const int64_t *image_ids, int64_t step,
                                    float *x_next, float *x0, int64_t B, int64_t chw, salun_stream_t stream) {
  if (B < 0 || chw < 0 || step < 0) return SALUN_EINVAL;
  if (variant != SALUN_SAMPLER_ANCESTRAL && variant != SALUN_SAMPLER_GENERALIZED) return SALUN_EINVAL;
  if (table_len < 2 || idx_t < 1 || idx_t >= table_len || idx_next < 0 || idx_next >= table_len) return SALUN_EINVAL;
  if (B == 0 || chw == 0) return SALUN_OK;
  if (!x_t || !eps_cond || !abar || !x_next) return SALUN_EINVAL;
  const int ancestral = variant == SALUN_SAMPLER_ANCESTRAL;
  // the step has a noise term unless it is the ancestral sampler's last step (t = 0) or DDIM with eta = 0
  const int noisy = ancestral ? (idx_t != 1) : (eta != 0.0);
  const int draw = noisy && !noise;
  if (draw && !image_ids) return SALUN_EINVAL;
  if (!noisy) noise = nullptr;
  const int vec = (chw % 4 == 0) && salun_aligned16(x_t) && salun_aligned16(eps_cond) && salun_aligned16(x_next) &&
                  (!eps_null || salun_aligned16(eps_null)) && (!noise || salun_aligned16(noise)) &&
                  (!x0 || salun_aligned16(x0));
  const float s1 = (float)(1.0 + cond_scale), s = (float)cond_scale;
  const long long *ids = reinterpret_cast<const long long *>(image_ids);
  hipStream_t st = salun_hip_stream(stream);
  if (vec) {
    hipLaunchKernelGGL(k_sampler_step<4>, dim3(step_grid(B * (chw / 4))), dim3(SALUN_BLOCK), 0, st, x_t, eps_cond,
                       eps_null, s1, s, abar, idx_t, idx_next, ancestral, (float)eta, noise, draw, seed, ids,
                       (uint64_t)step, x_next, x0, B, chw);
  } else {
    hipLaunchKernelGGL(k_sampler_step<1>, dim3(step_grid(B * chw)), dim3(SALUN_BLOCK), 0, st, x_t, eps_cond, eps_null,
                       s1, s, abar, idx_t, idx_next, ancestral, (float)eta, noise, draw, seed, ids, (uint64_t)step,
                       x_next, x0, B, chw);
  }
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_ldm_ddim_step(const float *x, const float *eps2, int guided, double scale, double c_s1m,
                                     double c_sqrt_at, double c_dir, double c_sqrt_aprev, double c_sigma, const float *z,
                                     float *x_prev, float *x0_out, int64_t B, int64_t chw, salun_stream_t stream) {
  if (B < 0 || chw < 0) return SALUN_EINVAL;
  if (!guided && scale != 1.0) return SALUN_EINVAL;
  if (c_sigma != 0.0 && !z) return SALUN_EINVAL;
  if (B == 0 || chw == 0) return SALUN_OK;
  if (!x || !eps2 || !x_prev) return SALUN_EINVAL;
  if (c_sigma == 0.0) z = nullptr;  // the reference adds 0 * z there
  const int64_t n = B * chw;
  const float *eu = guided ? eps2 : nullptr;       // rows [0, B): unconditional
  const float *ec = guided ? eps2 + n : eps2;      // rows [B, 2B): conditional
  const LdmCoef k = {(float)scale, (float)c_s1m, (float)c_sqrt_at, (float)c_dir, (float)c_sqrt_aprev, (float)c_sigma};
  const int vec = (chw % 4 == 0) && salun_aligned16(x) && salun_aligned16(eps2) && salun_aligned16(x_prev) &&
                  (!z || salun_aligned16(z)) && (!x0_out || salun_aligned16(x0_out));
  hipStream_t st = salun_hip_stream(stream);
  if (vec) {
    hipLaunchKernelGGL(k_ldm_ddim_step<4>, dim3(step_grid(n / 4)), dim3(SALUN_BLOCK), 0, st, x, eu, ec, k, z, x_prev,
                       x0_out, n / 4);
  } else {
    hipLaunchKernelGGL(k_ldm_ddim_step<1>, dim3(step_grid(n)), dim3(SALUN_BLOCK), 0, st, x, eu, ec, k, z, x_prev, x0_out,
                       n);
  }
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_lms_step(const float *x, const float *eps2, int guided, double scale, float *hist, int slot,
                                int order, double c0, double c1, double c2, double c3, double den, float *x_new,
                                float *x_in, int64_t B, int64_t chw, salun_stream_t stream) {
  static_assert(SALUN_LMS_ORDER == 4, "the ring index is masked with 3");
  if (B < 0 || chw < 0 || order < 1 || order > SALUN_LMS_ORDER || slot < 0 || slot >= SALUN_LMS_ORDER) return SALUN_EINVAL;
  if (!guided && scale != 1.0) return SALUN_EINVAL;
  if ((float)den == 0.0f) return SALUN_EINVAL;
  if (B == 0 || chw == 0) return SALUN_OK;
  if (!x || !eps2 || !hist || !x_new) return SALUN_EINVAL;
  if (hist == x || hist == eps2 || hist == x_new || hist == x_in) return SALUN_EINVAL;
  if (x_in && (x_in == x || x_in == eps2 || x_in == x_new)) return SALUN_EINVAL;
  if (chw > ((int64_t)1 << 40) / B) return SALUN_EINVAL;
  const int64_t n = B * chw;
  const float *eu = guided ? eps2 : nullptr;   // rows [0, B): unconditional
  const float *ec = guided ? eps2 + n : eps2;  // rows [B, 2B): conditional
  const LmsCoef k = {(float)scale, {(float)c0, (float)c1, (float)c2, (float)c3}, (float)den};
  hipLaunchKernelGGL(k_lms_step, dim3(step_grid(n)), dim3(SALUN_BLOCK), 0, salun_hip_stream(stream), x, eu, ec, k, hist,
                     slot, order, x_new, x_in, n);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_sampler_noise(float *out, uint64_t seed, const int64_t *image_ids, int64_t step, int64_t B,
                                     int64_t chw, salun_stream_t stream) {
  if (B < 0 || chw < 0 || step < 0) return SALUN_EINVAL;
  if (B == 0 || chw == 0) return SALUN_OK;
  if (!out || !image_ids) return SALUN_EINVAL;
  const long long *ids = reinterpret_cast<const long long *>(image_ids);
  hipStream_t st = salun_hip_stream(stream);
  if (chw % 4 == 0 && salun_aligned16(out)) {
    hipLaunchKernelGGL(k_sampler_noise<4>, dim3(step_grid(B * (chw / 4))), dim3(SALUN_BLOCK), 0, st, out, seed, ids,
                       (uint64_t)step, B, chw);
  } else {
    hipLaunchKernelGGL(k_sampler_noise<1>, dim3(step_grid(B * chw)), dim3(SALUN_BLOCK), 0, st, out, seed, ids,
                       (uint64_t)step, B, chw);
  }
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT size_t salun_minmax_workspace_bytes(int64_t n) {
  if (n < 1) return 0;
  return sizeof(float) * 2 * MINMAX_BLOCKS;
}

SALUN_EXPORT int salun_minmax(const float *x, int64_t n, float *lohi, void *ws, size_t ws_bytes, salun_stream_t stream) {
  if (n < 1 || !x || !lohi || !ws) return SALUN_EINVAL;
  if (ws_bytes < salun_minmax_workspace_bytes(n)) return SALUN_ENOSPC;
  hipStream_t st = salun_hip_stream(stream);
  int nblocks = salun_grid_for(n, SALUN_BLOCK * 4);
  if (nblocks > MINMAX_BLOCKS) nblocks = MINMAX_BLOCKS;
  float *partial = static_cast<float *>(ws);
  hipLaunchKernelGGL(k_minmax_partial, dim3(nblocks), dim3(SALUN_BLOCK), 0, st, x, n, (int)salun_aligned16(x), partial);
  SALUN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_minmax_final, dim3(1), dim3(SALUN_BLOCK), 0, st, partial, nblocks, lohi);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_images_to_u8(const float *x, uint8_t *out, int64_t B, int C, int HW, int rescaled,
                                    const float *range, salun_stream_t stream) {
  if (B < 0 || C < 1 || HW < 1) return SALUN_EINVAL;
  if ((int64_t)C * HW > IMAGES_U8_MAX_CHW || B > 0x7fffffffll) return SALUN_EINVAL;
  if (B == 0) return SALUN_OK;
  if (!x || !out) return SALUN_EINVAL;
  const int chw = C * HW;
  const int vec_in = (chw % 4 == 0) && salun_aligned16(x);   // every image then starts 16-byte aligned
  const int vec_out = (chw % 4 == 0) && salun_aligned4(out);
  const size_t lds = sizeof(float) * (size_t)(((chw + 3) & ~3) + 8);
  hipLaunchKernelGGL(k_images_to_u8, dim3((unsigned)B), dim3(SALUN_BLOCK), lds, salun_hip_stream(stream), x, out, C, HW,
                     rescaled ? 1 : 0, range, vec_in, vec_out);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}
