// salun_update.hip — HBM-bound element-wise kernels over the flat parameter arena:
//   K1 saliency accumulate, K3+K4 masked SGD-momentum, K5 grad sq-norm + masked Adam,
//   K7 Fisher square-accumulate, K20 masked Adam + EMA shadow in one pass.
//   gfx950 / CDNA4, compiled with -ffp-contract=off.
//
// Every kernel here is an op on the streaming shape of salun_stream.h (stream_tiles); the gradient, streamed once,
// is the only operand read with non-temporal loads.
#include "salun_stream.h"

namespace {

// ------------------------------------------------------------------------ K1 ----
struct AccumArgs {
  float *acc;
  const float *g;
  const float *sqnorm;
  float scale;
  float max_norm;
  int64_t n;
};

__device__ __forceinline__ float accum_elem(float a, float g, float s) { return a + (g * s); }

struct AccumOp {
  const AccumArgs &a;
  const float s;
  struct Vec { float4 acc, g; };
  __device__ AccumOp(const AccumArgs &a) : a(a), s(a.sqnorm ? salun_clip_coef(*a.sqnorm, a.max_norm) : a.scale) {}
  __device__ void load(Vec &x, int64_t v) const { x.acc = ld4(a.acc, v); x.g = ld4_nt(a.g, v); }
  __device__ void vec(Vec &x, int64_t v) const {
    st4(a.acc, v, make_float4(accum_elem(x.acc.x, x.g.x, s), accum_elem(x.acc.y, x.g.y, s),
                              accum_elem(x.acc.z, x.g.z, s), accum_elem(x.acc.w, x.g.w, s)));
  }
  __device__ void one(int64_t i) const { a.acc[i] = accum_elem(a.acc[i], a.g[i], s); }
};

template <bool VEC>
__global__ __launch_bounds__(SALUN_BLOCK) void k_saliency_accumulate(AccumArgs a) {
  AccumOp op(a);
  stream_tiles<VEC>(a.n, op);
}

// --------------------------------------------------------------------- K3+K4 ----
struct SgdArgs {
  float *p;
  const float *g;
  float *buf;
  const uint8_t *m;
  float neg_lr, mu, wd;
  int first_step;
  int64_t n;
};

template <bool HAS_WD, bool HAS_MOM>
__device__ __forceinline__ void sgd_elem(float &p, float g, float &b, bool on, const SgdArgs &a) {
  if (on) {
    const float d = HAS_WD ? __builtin_fmaf(a.wd, p, g) : g;
    float nb = d;
    if (HAS_MOM) {
      nb = a.first_step ? d : (a.mu * b) + d;
      b = nb;
    }
    p = __builtin_fmaf(a.neg_lr, nb, p);
  } else if (HAS_MOM) {
    b = 0.0f;
  }
}

template <bool HAS_MASK, bool HAS_WD, bool HAS_MOM>
struct SgdOp {
  const SgdArgs &a;
  struct Vec { float4 p, g, b; uint32_t m; };
  __device__ void load(Vec &x, int64_t v) const {
    x.m = HAS_MASK ? ldm(a.m, v) : 0x01010101u;
    x.p = ld4(a.p, v);
    x.g = ld4_nt(a.g, v);
    if (HAS_MOM) x.b = ld4(a.buf, v);
  }
  __device__ void vec(Vec &x, int64_t v) const {
    sgd_elem<HAS_WD, HAS_MOM>(x.p.x, x.g.x, x.b.x, mbyte(x.m, 0), a);
    sgd_elem<HAS_WD, HAS_MOM>(x.p.y, x.g.y, x.b.y, mbyte(x.m, 1), a);
    sgd_elem<HAS_WD, HAS_MOM>(x.p.z, x.g.z, x.b.z, mbyte(x.m, 2), a);
    sgd_elem<HAS_WD, HAS_MOM>(x.p.w, x.g.w, x.b.w, mbyte(x.m, 3), a);
    st4(a.p, v, x.p);
    if (HAS_MOM) st4(a.buf, v, x.b);
  }
  __device__ void one(int64_t i) const {
    float p = a.p[i], b = HAS_MOM ? a.buf[i] : 0.0f;
    sgd_elem<HAS_WD, HAS_MOM>(p, a.g[i], b, HAS_MASK ? a.m[i] != 0 : true, a);
    a.p[i] = p;
    if (HAS_MOM) a.buf[i] = b;
  }
};

template <bool HAS_MASK, bool HAS_WD, bool HAS_MOM>
__global__ __launch_bounds__(SALUN_BLOCK) void k_masked_sgd_vec(SgdArgs a) {
  SgdOp<HAS_MASK, HAS_WD, HAS_MOM> op{a};
  stream_tiles<true>(a.n, op);
}

template <bool HAS_MASK, bool HAS_WD, bool HAS_MOM>
__global__ __launch_bounds__(SALUN_BLOCK) void k_masked_sgd_scalar(SgdArgs a) {
  SgdOp<HAS_MASK, HAS_WD, HAS_MOM> op{a};
  stream_tiles<false>(a.n, op);
}

// ------------------------------------------------------------------------ K5 ----
constexpr int REDUCE_MAX_BLOCKS = 1024;

// Four component accumulators in tile order; the tail and the scalar route add into the first.
struct SqnormOp {
  const float *g;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  struct Vec { float4 g; };
  __device__ void load(Vec &x, int64_t v) const { x.g = ld4(g, v); }
  __device__ void vec(Vec &x, int64_t) {
    s0 = __builtin_fmaf(x.g.x, x.g.x, s0);
    s1 = __builtin_fmaf(x.g.y, x.g.y, s1);
    s2 = __builtin_fmaf(x.g.z, x.g.z, s2);
    s3 = __builtin_fmaf(x.g.w, x.g.w, s3);
  }
  __device__ void one(int64_t i) { s0 = __builtin_fmaf(g[i], g[i], s0); }
};

__global__ __launch_bounds__(SALUN_BLOCK) void k_sqnorm_partial(const float *__restrict__ g, int64_t n,
                                                                double *__restrict__ partial, int vec) {
  __shared__ double lds[4];
  SqnormOp op{g};
  if (vec) stream_tiles<true>(n, op);
  else stream_tiles<false>(n, op);
  const double tot = salun_block_sum(((double)op.s0 + (double)op.s1) + ((double)op.s2 + (double)op.s3), lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// One workgroup folds <= REDUCE_MAX_BLOCKS partials in a fixed order.
__global__ __launch_bounds__(SALUN_BLOCK) void k_sum_partials_f32(const double *__restrict__ partial, int count,
                                                                   float *__restrict__ out) {
  __shared__ double lds[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < count; i += SALUN_BLOCK) s += partial[i];
  const double tot = salun_block_sum(s, lds);
  if (threadIdx.x == 0) *out = (float)tot;
}

struct AdamArgs {
  float *p;
  const float *g;
  float *m1;
  float *v;
  const uint8_t *mask;
  const float *sqnorm;
  float max_norm, gscale;
  float b1, omb1, b2, omb2, eps, wd;
  float bc2_sqrt, neg_step_size;
  const float *coef;  // optional device pair {sqrt(1 - b2^t), -lr / (1 - b1^t)}: replaces the two host values above
  int64_t n;
};

template <bool HAS_WD>
__device__ __forceinline__ void adam_elem(float &p, float g, float &m1, float &v, float mf, float s,
                                          const AdamArgs &a) {
  float ge = (g * s) * mf;
  if (HAS_WD) ge = __builtin_fmaf(a.wd, p, ge);
  m1 = (a.b1 * m1) + (a.omb1 * ge);
  v = (a.b2 * v) + ((a.omb2 * ge) * ge);
  const float den = (sqrtf(v) / a.bc2_sqrt) + a.eps;
  p = p + (a.neg_step_size * (m1 / den));
}

// step-dependent scalars of Adam computed ON THE DEVICE from a device-resident step counter (a captured HIP graph
// replays the same kernel arguments every step: the host cannot pass t).  Same double arithmetic as the host path.
__global__ void k_adam_coefficients(long long *step, double lr, double b1, double b2, float *coef) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const long long t = *step + 1;
    *step = t;
    const double bc1 = 1.0 - pow(b1, (double)t);
    const double bc2 = 1.0 - pow(b2, (double)t);
    coef[0] = (float)sqrt(bc2);
    coef[1] = (float)(-(lr / bc1));
  }
}

template <bool HAS_MASK, bool HAS_WD>
struct AdamOp {
  AdamArgs &a;
  const float s;
  struct Vec { float4 p, g, m1, v; uint32_t m; };
  __device__ AdamOp(AdamArgs &a) : a(a), s(a.sqnorm ? salun_clip_coef(*a.sqnorm, a.max_norm) : a.gscale) {
    if (a.coef) { a.bc2_sqrt = a.coef[0]; a.neg_step_size = a.coef[1]; }
  }
  __device__ void load(Vec &x, int64_t v) const {
    x.m = HAS_MASK ? ldm(a.mask, v) : 0x01010101u;
    x.p = ld4(a.p, v);
    x.g = ld4_nt(a.g, v);
    x.m1 = ld4(a.m1, v);
    x.v = ld4(a.v, v);
  }
  __device__ void vec(Vec &x, int64_t v) const {
    adam_elem<HAS_WD>(x.p.x, x.g.x, x.m1.x, x.v.x, mbyte(x.m, 0) ? 1.f : 0.f, s, a);
    adam_elem<HAS_WD>(x.p.y, x.g.y, x.m1.y, x.v.y, mbyte(x.m, 1) ? 1.f : 0.f, s, a);
    adam_elem<HAS_WD>(x.p.z, x.g.z, x.m1.z, x.v.z, mbyte(x.m, 2) ? 1.f : 0.f, s, a);
    adam_elem<HAS_WD>(x.p.w, x.g.w, x.m1.w, x.v.w, mbyte(x.m, 3) ? 1.f : 0.f, s, a);
    st4(a.p, v, x.p);
    st4(a.m1, v, x.m1);
    st4(a.v, v, x.v);
  }
  __device__ float one(int64_t i) const {  // returns the new p
    float p = a.p[i], m1 = a.m1[i], v = a.v[i];
    adam_elem<HAS_WD>(p, a.g[i], m1, v, HAS_MASK ? (a.mask[i] ? 1.f : 0.f) : 1.f, s, a);
    a.p[i] = p;
    a.m1[i] = m1;
    a.v[i] = v;
    return p;
  }
};

template <bool HAS_MASK, bool HAS_WD, bool VEC>
__global__ __launch_bounds__(SALUN_BLOCK) void k_masked_adam(AdamArgs a) {
  AdamOp<HAS_MASK, HAS_WD> op(a);
  stream_tiles<VEC>(a.n, op);
}

// ----------------------------------------------------------------------- K20 ----
// K5's Adam step with the EMA shadow of the parameters updated in the same pass: the new p never leaves the registers
// between the two (36 B / element in one launch instead of 28 + 12 in two).  The Adam part is K5's op, untouched.
struct AdamEmaArgs {
  AdamArgs a;
  float *shadow;
  float w;  // 1 - mu, evaluated in double on the host
};

// Tensor.lerp_(p, w) for w < 0.5 (ATen/native/Lerp.h): shadow + w * (p - shadow).  ATen's device code is compiled with
// floating-point contraction on, so its product and sum are ONE fused multiply-add; this file is compiled with
// contraction off, so the fma is written out.
__device__ __forceinline__ float ema_elem(float sh, float p, float w) { return __builtin_fmaf(w, p - sh, sh); }

template <bool HAS_MASK, bool HAS_WD>
struct AdamEmaOp {
  AdamOp<HAS_MASK, HAS_WD> adam;
  float *const shadow;
  const float w;
  struct Vec { typename AdamOp<HAS_MASK, HAS_WD>::Vec a; float4 sh; };
  __device__ AdamEmaOp(AdamEmaArgs &e) : adam(e.a), shadow(e.shadow), w(e.w) {}
  __device__ void load(Vec &x, int64_t v) const { adam.load(x.a, v); x.sh = ld4(shadow, v); }
  __device__ void vec(Vec &x, int64_t v) const {
    adam.vec(x.a, v);
    st4(shadow, v, make_float4(ema_elem(x.sh.x, x.a.p.x, w), ema_elem(x.sh.y, x.a.p.y, w),
                               ema_elem(x.sh.z, x.a.p.z, w), ema_elem(x.sh.w, x.a.p.w, w)));
  }
  __device__ void one(int64_t i) const { shadow[i] = ema_elem(shadow[i], adam.one(i), w); }
};

template <bool HAS_MASK, bool HAS_WD, bool VEC>
__global__ __launch_bounds__(SALUN_BLOCK) void k_adam_ema(AdamEmaArgs e) {
  AdamEmaOp<HAS_MASK, HAS_WD> op(e);
  stream_tiles<VEC>(e.a.n, op);
}

// ------------------------------------------------------------------------ K7 ----
// F += tmp^2 / n_data ; tmp <- 0
struct FimOp {
  float *F, *tmp;
  float n_data;
  struct Vec { float4 f, t; };
  __device__ static float elem(float f, float t, float n_data) { return f + ((t * t) / n_data); }
  __device__ void load(Vec &x, int64_t v) const { x.f = ld4(F, v); x.t = ld4(tmp, v); }
  __device__ void vec(Vec &x, int64_t v) const {
    st4(F, v, make_float4(elem(x.f.x, x.t.x, n_data), elem(x.f.y, x.t.y, n_data), elem(x.f.z, x.t.z, n_data),
                          elem(x.f.w, x.t.w, n_data)));
    st4(tmp, v, make_float4(0.f, 0.f, 0.f, 0.f));
  }
  __device__ void one(int64_t i) const {
    F[i] = elem(F[i], tmp[i], n_data);
    tmp[i] = 0.f;
  }
};

template <bool VEC>
__global__ __launch_bounds__(SALUN_BLOCK) void k_fim_square_accumulate(float *__restrict__ F, float *__restrict__ tmp,
                                                                        float n_data, int64_t n) {
  FimOp op{F, tmp, n_data};
  stream_tiles<VEC>(n, op);
}

}  // namespace

// ================================================================== C-ABI =======
SALUN_EXPORT int salun_saliency_accumulate(float *acc, const float *g, double scale, const float *sqnorm,
                                           double max_norm, int64_t n, salun_stream_t stream) {
  if (n < 0 || (n > 0 && (!acc || !g))) return SALUN_EINVAL;
  if (n == 0) return SALUN_OK;
  AccumArgs a{acc, g, sqnorm, (float)scale, (float)max_norm, n};
  const bool vec = salun_aligned16(acc) && salun_aligned16(g);
  return stream_launch(k_saliency_accumulate<true>, k_saliency_accumulate<false>, vec, n, SALUN_MAX_GRID,
                       salun_hip_stream(stream), a);
}

SALUN_EXPORT int salun_masked_sgd_step(float *p, const float *g, float *buf, const uint8_t *m, double lr,
                                       double mu, double wd, int first_step, int64_t n,
                                       salun_stream_t stream) {
  if (n < 0 || (n > 0 && (!p || !g))) return SALUN_EINVAL;
  const bool has_mom = (mu != 0.0);
  if (n > 0 && has_mom && !buf) return SALUN_EINVAL;
  if (n == 0) return SALUN_OK;
  SgdArgs a{p, g, buf, m, (float)(-lr), (float)mu, (float)wd, first_step, n};
  const bool has_wd = (wd != 0.0), has_mask = (m != nullptr);
  const bool vec = salun_aligned16(p) && salun_aligned16(g) && (!has_mom || salun_aligned16(buf)) &&
                   (!has_mask || salun_aligned4(m));
  hipStream_t st = salun_hip_stream(stream);
  return with_bools(
      [&](auto M, auto W, auto O) {
        return stream_launch(k_masked_sgd_vec<M.value, W.value, O.value>, k_masked_sgd_scalar<M.value, W.value, O.value>,
                             vec, n, SALUN_MAX_GRID, st, a);
      },
      has_mask, has_wd, has_mom);
}

SALUN_EXPORT size_t salun_reduce_workspace_bytes(int64_t n) {
  (void)n;
  return sizeof(double) * REDUCE_MAX_BLOCKS * 4;  // partial sums (+ slack for sqerr per-sample staging)
}

SALUN_EXPORT int salun_grad_sqnorm(const float *g, int64_t n, float *out, void *ws, size_t ws_bytes,
                                   salun_stream_t stream) {
  if (n < 0 || !out || !ws || (n > 0 && !g)) return SALUN_EINVAL;
  if (ws_bytes < sizeof(double) * REDUCE_MAX_BLOCKS) return SALUN_ENOSPC;
  hipStream_t st = salun_hip_stream(stream);
  double *partial = static_cast<double *>(ws);
  const int vec = salun_aligned16(g) ? 1 : 0;
  // one kernel for both routes, sized as the float4 route on both: the returned float depends on the partition
  const int grid = stream_grid(n, true, REDUCE_MAX_BLOCKS);
  hipLaunchKernelGGL(k_sqnorm_partial, dim3(grid), dim3(SALUN_BLOCK), 0, st, g, n, partial, vec);
  SALUN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_sum_partials_f32, dim3(1), dim3(SALUN_BLOCK), 0, st, partial, grid, out);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

static int masked_adam_impl(float *p, const float *g, float *m1, float *v, const uint8_t *mask, const float *sqnorm,
                            double max_norm, double gscale, double lr, double b1, double b2, double eps, double wd,
                            int step, const float *coef, int64_t n, salun_stream_t stream);

SALUN_EXPORT int salun_masked_adam_step(float *p, const float *g, float *m1, float *v, const uint8_t *mask,
                                        const float *sqnorm, double max_norm, double gscale, double lr,
                                        double b1, double b2, double eps, double wd, int step, int64_t n,
                                        salun_stream_t stream) {
  if (step < 1) return SALUN_EINVAL;
  return masked_adam_impl(p, g, m1, v, mask, sqnorm, max_norm, gscale, lr, b1, b2, eps, wd, step, nullptr, n, stream);
}

SALUN_EXPORT int salun_adam_coefficients(int64_t *step, double lr, double b1, double b2, float *coef,
                                         salun_stream_t stream) {
  if (!step || !coef) return SALUN_EINVAL;
  hipLaunchKernelGGL(k_adam_coefficients, dim3(1), dim3(64), 0, salun_hip_stream(stream),
                     reinterpret_cast<long long *>(step), lr, b1, b2, coef);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_masked_adam_step_coef(float *p, const float *g, float *m1, float *v, const uint8_t *mask,
                                             const float *sqnorm, double max_norm, double gscale, const float *coef,
                                             double b1, double b2, double eps, double wd, int64_t n,
                                             salun_stream_t stream) {
  if (!coef) return SALUN_EINVAL;
  return masked_adam_impl(p, g, m1, v, mask, sqnorm, max_norm, gscale, 0.0, b1, b2, eps, wd, 1, coef, n, stream);
}

static AdamArgs adam_args(float *p, const float *g, float *m1, float *v, const uint8_t *mask, const float *sqnorm,
                          double max_norm, double gscale, double lr, double b1, double b2, double eps, double wd,
                          int step, const float *coef, int64_t n) {
  // Python-scalar arithmetic of torch.optim.adam._single_tensor_adam, in double.
  const double bc1 = 1.0 - pow(b1, (double)step);
  const double bc2 = 1.0 - pow(b2, (double)step);
  AdamArgs a;
  a.coef = coef;
  a.p = p; a.g = g; a.m1 = m1; a.v = v; a.mask = mask; a.sqnorm = sqnorm;
  a.max_norm = (float)max_norm; a.gscale = (float)gscale;
  a.b1 = (float)b1; a.omb1 = (float)(1.0 - b1); a.b2 = (float)b2; a.omb2 = (float)(1.0 - b2);
  a.eps = (float)eps; a.wd = (float)wd;
  a.bc2_sqrt = (float)sqrt(bc2);
  a.neg_step_size = (float)(-(lr / bc1));
  a.n = n;
  return a;
}

static int masked_adam_impl(float *p, const float *g, float *m1, float *v, const uint8_t *mask, const float *sqnorm,
                            double max_norm, double gscale, double lr, double b1, double b2, double eps, double wd,
                            int step, const float *coef, int64_t n, salun_stream_t stream) {
  if (n < 0 || step < 1 || (n > 0 && (!p || !g || !m1 || !v))) return SALUN_EINVAL;
  if (n == 0) return SALUN_OK;
  const AdamArgs a = adam_args(p, g, m1, v, mask, sqnorm, max_norm, gscale, lr, b1, b2, eps, wd, step, coef, n);
  const bool has_mask = mask != nullptr, has_wd = wd != 0.0;
  const bool vec = salun_aligned16(p) && salun_aligned16(g) && salun_aligned16(m1) && salun_aligned16(v) &&
                   (!has_mask || salun_aligned4(mask));
  hipStream_t st = salun_hip_stream(stream);
  return with_bools(
      [&](auto M, auto W) {
        return stream_launch(k_masked_adam<M.value, W.value, true>, k_masked_adam<M.value, W.value, false>, vec, n,
                             SALUN_MAX_GRID, st, a);
      },
      has_mask, has_wd);
}

// K20: the five vectors are read and written by the same lane in one pass, so two of them sharing memory would make
// the result depend on the store order; refused before any launch.
static int adam_ema_impl(float *p, const float *g, float *m1, float *v, float *shadow, const uint8_t *mask,
                         const float *sqnorm, double max_norm, double gscale, double lr, double b1, double b2, double eps,
                         double wd, double mu, int step, const float *coef, int64_t n, salun_stream_t stream) {
  if (n < 0 || step < 1 || (n > 0 && (!p || !g || !m1 || !v || !shadow))) return SALUN_EINVAL;
  if (n == 0) return SALUN_OK;
  const void *bufs[5] = {p, m1, v, shadow, g};
  for (int i = 0; i < 5; ++i)
    for (int j = i + 1; j < 5; ++j)
      if (bufs[i] == bufs[j]) return SALUN_EINVAL;
  AdamEmaArgs e;
  e.a = adam_args(p, g, m1, v, mask, sqnorm, max_norm, gscale, lr, b1, b2, eps, wd, step, coef, n);
  e.shadow = shadow;
  e.w = (float)(1.0 - mu);
  const bool has_mask = mask != nullptr, has_wd = wd != 0.0;
  const bool vec = salun_aligned16(p) && salun_aligned16(g) && salun_aligned16(m1) && salun_aligned16(v) &&
                   salun_aligned16(shadow) && (!has_mask || salun_aligned4(mask));
  hipStream_t st = salun_hip_stream(stream);
  return with_bools(
      [&](auto M, auto W) {
        return stream_launch(k_adam_ema<M.value, W.value, true>, k_adam_ema<M.value, W.value, false>, vec, n,
                             SALUN_MAX_GRID, st, e);
      },
      has_mask, has_wd);
}

SALUN_EXPORT int salun_adam_ema_step(float *p, const float *g, float *m1, float *v, float *shadow, const uint8_t *mask,
                                     const float *sqnorm, double max_norm, double gscale, double lr, double b1,
                                     double b2, double eps, double wd, double mu, int step, int64_t n,
                                     salun_stream_t stream) {
  if (step < 1) return SALUN_EINVAL;
  return adam_ema_impl(p, g, m1, v, shadow, mask, sqnorm, max_norm, gscale, lr, b1, b2, eps, wd, mu, step, nullptr, n,
                       stream);
}

SALUN_EXPORT int salun_adam_ema_step_coef(float *p, const float *g, float *m1, float *v, float *shadow,
                                          const uint8_t *mask, const float *sqnorm, double max_norm, double gscale,
                                          const float *coef, double b1, double b2, double eps, double wd, double mu,
                                          int64_t n, salun_stream_t stream) {
  if (!coef) return SALUN_EINVAL;
  return adam_ema_impl(p, g, m1, v, shadow, mask, sqnorm, max_norm, gscale, 0.0, b1, b2, eps, wd, mu, 1, coef, n,
                       stream);
}

SALUN_EXPORT int salun_fim_square_accumulate(float *F, float *tmp, double n_data, int64_t n,
                                             salun_stream_t stream) {
  if (n < 0 || n_data == 0.0 || (n > 0 && (!F || !tmp))) return SALUN_EINVAL;
  if (n == 0) return SALUN_OK;
  const bool vec = salun_aligned16(F) && salun_aligned16(tmp);
  return stream_launch(k_fim_square_accumulate<true>, k_fim_square_accumulate<false>, vec, n, SALUN_MAX_GRID,
                       salun_hip_stream(stream), F, tmp, (float)n_data, n);
}


// ---------------------------------------------------------------------------------------------------
// Shader-clock probe (measurement tooling: tools/clock_probe.py).  One wave reads the shader-cycle counter (s_memtime)
// and the 100 MHz constant counter (s_memrealtime) `spins` sleeps apart: out[2i] = shader cycles, out[2i+1] = 100 MHz
// ticks of sample i — their ratio x 100 MHz is the clock the chip actually ran at while whatever else was resident ran.
namespace {
__global__ __launch_bounds__(64) void k_clock_probe(unsigned long long *__restrict__ out, int samples, int spins) {
  if (threadIdx.x != 0) return;
  for (int i = 0; i < samples; ++i) {
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int k = 0; k < spins; ++k) __builtin_amdgcn_s_sleep(127);
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    out[2 * i] = t1 - t0;
    out[2 * i + 1] = r1 - r0;
  }
}
}  // namespace

SALUN_EXPORT int salun_clock_probe(unsigned long long *out, int samples, int spins, salun_stream_t stream) {
  if (!out || samples < 1 || spins < 1) return SALUN_EINVAL;
  hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, salun_hip_stream(stream), out, samples, spins);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}
