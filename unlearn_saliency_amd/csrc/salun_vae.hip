// salun_vae.hip — the posterior of the Stable-Diffusion first stage.
//
// salun_vae_posterior_sample  DiagonalGaussianDistribution.sample() / .mode() of ldm/modules/distributions followed by
//                             the scale of get_first_stage_encoding, read from the (possibly channel-padded) output of
//                             quant_conv in place:  z = scale * (mean + expf(0.5 * clamp(logvar, -30, 20)) * eps).
//                             eps is the counter-based normal of salun_sampler_noise on the key (seed, draw, image id)
//                             at the element's index within the image's latent, so an image's latent does not depend on
//                             the batch around it, and salun_sampler_noise(step = draw) writes the very draw out.
// salun_decoded_to_u8         the decoded image of the evaluation script, (image / 2 + 0.5).clamp(0, 1) then
//                             (image * 255).round().astype("uint8") in NHWC, read from the first C of Cp planes (the
//                             channel-padded output of the decoder's conv_out in place).  Half to even, NaN -> 0.
// One thread per output element, grid-stride; memory bound and tiny (4 x 64 x 64 per image).
#include "salun_common.h"

namespace {

__global__ __launch_bounds__(SALUN_BLOCK) void k_vae_sample(const float *__restrict__ mom, float *__restrict__ z,
                                                            const long long *__restrict__ ids, uint64_t seed,
                                                            uint64_t draw, int Cm, int zc, int64_t hw, int64_t B,
                                                            float scale, int deterministic) {
  const uint64_t skey = salun_splitmix64(salun_splitmix64(seed) + draw);
  const int64_t per = (int64_t)zc * hw, total = B * per;
  for (int64_t i = (int64_t)blockIdx.x * SALUN_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * SALUN_BLOCK) {
    const int64_t b = i / per, e = i - b * per;
    const int64_t src = b * (int64_t)Cm * hw + e;      // channel c, pixel p of the mean: c * hw + p = e
    const float mean = mom[src];
    if (deterministic) {
      z[i] = scale * mean;
      continue;
    }
    float lv = mom[src + per];                          // the log-variance sits zc channels further on
    lv = fminf(fmaxf(lv, -30.0f), 20.0f);
    const float sd = expf(0.5f * lv);
    const uint64_t key = salun_splitmix64(skey + (uint64_t)ids[b]);
    const float n = salun_ih12(key, (uint64_t)e);
    z[i] = scale * (mean + sd * n);
  }
}

// One thread per (image, pixel): C coalesced plane reads, C adjacent bytes written.  Each operation is rounded by itself
// (the file is compiled without contraction): x * 0.5f is x / 2 exactly; fmaxf(NaN, 0) = 0, so a NaN gives 0.
__global__ __launch_bounds__(SALUN_BLOCK) void k_decoded_to_u8(const float *__restrict__ x, uint8_t *__restrict__ out,
                                                               int Cp, int C, int64_t hw, int64_t B) {
  const int64_t total = B * hw;
  for (int64_t i = (int64_t)blockIdx.x * SALUN_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * SALUN_BLOCK) {
    const int64_t b = i / hw, p = i - b * hw;
    const float *src = x + b * (int64_t)Cp * hw + p;
    uint8_t *dst = out + i * C;
    for (int c = 0; c < C; ++c) {
      float v = src[(int64_t)c * hw] * 0.5f;
      v = v + 0.5f;
      v = fminf(fmaxf(v, 0.0f), 1.0f);
      v = v * 255.0f;
      dst[c] = (uint8_t)(int)rintf(v);
    }
  }
}

}  // namespace

SALUN_EXPORT int salun_decoded_to_u8(const float *x, int Cp, int C, int64_t hw, int64_t B, uint8_t *out,
                                     salun_stream_t stream) {
  if (!x || !out || C < 1 || C > SALUN_DECODED_U8_MAX_C || Cp < C || hw < 1 || B < 1) return SALUN_EINVAL;
  if (!salun_aligned4(x) || (const void *)x == (const void *)out) return SALUN_EINVAL;
  if (hw > ((int64_t)1 << 40) / Cp || B > ((int64_t)1 << 40) / ((int64_t)Cp * hw)) return SALUN_EINVAL;
  hipLaunchKernelGGL(k_decoded_to_u8, dim3(salun_grid_for(B * hw, SALUN_BLOCK)), dim3(SALUN_BLOCK), 0,
                     salun_hip_stream(stream), x, out, Cp, C, hw, B);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_vae_posterior_sample(const float *moments, int Cm, int zc, int64_t hw, int64_t B,
                                            const int64_t *image_ids, uint64_t seed, int64_t draw, double scale,
                                            int deterministic, float *z, salun_stream_t stream) {
  if (!moments || !z || (!deterministic && !image_ids) || zc < 1 || Cm < 2 * zc || hw < 1 || B < 1 || draw < 0)
    return SALUN_EINVAL;
  if (!salun_aligned4(moments) || !salun_aligned4(z) || moments == z) return SALUN_EINVAL;
  if (hw > ((int64_t)1 << 40) / Cm || B > ((int64_t)1 << 40) / ((int64_t)Cm * hw)) return SALUN_EINVAL;
  hipLaunchKernelGGL(k_vae_sample, dim3(salun_grid_for(B * zc * hw, SALUN_BLOCK)), dim3(SALUN_BLOCK), 0,
                     salun_hip_stream(stream), moments, z, reinterpret_cast<const long long *>(image_ids), seed,
                     (uint64_t)draw, Cm, zc, hw, B, (float)scale, deterministic);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}
