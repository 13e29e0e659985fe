// salun_prox.hip — the "next" rows that reuse the flat-vector machinery:
//   K9   proximal / soft-threshold step of RL_proximal (Classification/unlearn/RL_pro.py:52-60):
//          d = p - p0 ; tau = ratio-th smallest |d| (radix select of salun_topk.hip on d) ;
//          p <- d >  tau ? p - tau : d < -tau ? p + tau : p0
//   K10  EWC / Selective-Amnesia penalty of DDPM train_forget (DDPM/runners/diffusion.py:343-350):
//          loss += lambda * sum F (p - p*)^2 ;  g += (lambda F) * (2 (p - p*))
// All three are ops on the streaming shape of salun_stream.h (stream_tiles); -ffp-contract=off (every rounding is the
// one written).
#include "salun_stream.h"

namespace {

constexpr int EWC_MAX_BLOCKS = 2048;

// A NaN threshold is the select's failure signal (salun_mask_topk_thresholds exports NaN when the full scan's grid
// barrier timed out, or when the ranked element itself is NaN): the weights are poisoned with it so that the next
// loss is NaN — never a silent "every weight reset to p0", which is what the comparisons below would give.
__device__ __forceinline__ float soft(float p, float p0, float tau) {
  const float d = p - p0;
  if (tau != tau) return tau;
  return d > tau ? p - tau : (d < -tau ? p + tau : p0);
}

struct Vec2 { float4 a, b; };

// out = p - p0
struct DiffOp {
  const float *p, *p0;
  float *out;
  using Vec = Vec2;
  __device__ void load(Vec &x, int64_t v) const { x.a = ld4(p, v); x.b = ld4(p0, v); }
  __device__ void vec(Vec &x, int64_t v) const {
    st4(out, v, make_float4(x.a.x - x.b.x, x.a.y - x.b.y, x.a.z - x.b.z, x.a.w - x.b.w));
  }
  __device__ void one(int64_t i) const { out[i] = p[i] - p0[i]; }
};

template <bool VEC>
__global__ __launch_bounds__(SALUN_BLOCK) void k_param_diff(const float *__restrict__ p, const float *__restrict__ p0,
                                                            float *__restrict__ out, int64_t n) {
  DiffOp op{p, p0, out};
  stream_tiles<VEC>(n, op);
}

// p <- soft-threshold towards p0 with the device-resident threshold *tau
struct SoftOp {
  float *p;
  const float *p0;
  float tau;
  using Vec = Vec2;
  __device__ void load(Vec &x, int64_t v) const { x.a = ld4(p, v); x.b = ld4(p0, v); }
  __device__ void vec(Vec &x, int64_t v) const {
    st4(p, v, make_float4(soft(x.a.x, x.b.x, tau), soft(x.a.y, x.b.y, tau), soft(x.a.z, x.b.z, tau),
                          soft(x.a.w, x.b.w, tau)));
  }
  __device__ void one(int64_t i) const { p[i] = soft(p[i], p0[i], tau); }
};

template <bool VEC>
__global__ __launch_bounds__(SALUN_BLOCK) void k_soft_threshold(float *__restrict__ p, const float *__restrict__ p0,
                                                                const float *__restrict__ tau_ptr, int64_t n) {
  SoftOp op{p, p0, *tau_ptr};
  stream_tiles<VEC>(n, op);
}

// g += (lam*F) * (2*(p - p*)) ;  partial[block] = sum F*(p-p*)^2 (fp64, one accumulator in element order)
struct EwcOp {
  const float *p, *pstar, *F;
  float *g;
  float lam;
  double acc = 0.0;
  struct Vec { float4 p, s, f, g; };
  __device__ float elem(float pv, float sv, float fv, float gv) {
    const float d = pv - sv;
    acc += (double)(fv * (d * d));
    return gv + ((lam * fv) * (2.0f * d));
  }
  __device__ void load(Vec &x, int64_t v) const { x.p = ld4(p, v); x.s = ld4(pstar, v); x.f = ld4(F, v); x.g = ld4(g, v); }
  __device__ void vec(Vec &x, int64_t v) {
    float4 o;
    o.x = elem(x.p.x, x.s.x, x.f.x, x.g.x);
    o.y = elem(x.p.y, x.s.y, x.f.y, x.g.y);
    o.z = elem(x.p.z, x.s.z, x.f.z, x.g.z);
    o.w = elem(x.p.w, x.s.w, x.f.w, x.g.w);
    st4(g, v, o);
  }
  __device__ void one(int64_t i) { g[i] = elem(p[i], pstar[i], F[i], g[i]); }
};

template <bool VEC>
__global__ __launch_bounds__(SALUN_BLOCK) void k_ewc(const float *__restrict__ p, const float *__restrict__ pstar,
                                                     const float *__restrict__ F, float *__restrict__ g, float lam,
                                                     int64_t n, double *__restrict__ partial) {
  __shared__ double lds[4];
  EwcOp op{p, pstar, F, g, lam};
  stream_tiles<VEC>(n, op);
  const double t = salun_block_sum(op.acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// loss_out[0] = (float)(lam * sum partial) ; loss_out[1] = (float)sum partial   (fixed order)
__global__ __launch_bounds__(SALUN_BLOCK) void k_ewc_final(const double *__restrict__ partial, int nblocks, float lam,
                                                           float *__restrict__ loss_out) {
  __shared__ double lds[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += SALUN_BLOCK) s += partial[i];
  const double t = salun_block_sum(s, lds);
  if (threadIdx.x == 0) {
    loss_out[0] = (float)((double)lam * t);
    loss_out[1] = (float)t;
  }
}

}  // namespace

// ================================================================== C-ABI =======
SALUN_EXPORT int salun_param_diff(const float *p, const float *p0, float *out, int64_t n, salun_stream_t stream) {
  if (n < 0 || (n > 0 && (!p || !p0 || !out))) return SALUN_EINVAL;
  if (n == 0) return SALUN_OK;
  const bool vec = salun_aligned16(p) && salun_aligned16(p0) && salun_aligned16(out);
  return stream_launch(k_param_diff<true>, k_param_diff<false>, vec, n, SALUN_MAX_GRID, salun_hip_stream(stream), p, p0,
                       out, n);
}

SALUN_EXPORT int salun_soft_threshold_step(float *p, const float *p0, const float *tau, int64_t n,
                                           salun_stream_t stream) {
  if (n < 0 || !tau || (n > 0 && (!p || !p0))) return SALUN_EINVAL;
  if (n == 0) return SALUN_OK;
  const bool vec = salun_aligned16(p) && salun_aligned16(p0);
  return stream_launch(k_soft_threshold<true>, k_soft_threshold<false>, vec, n, SALUN_MAX_GRID,
                       salun_hip_stream(stream), p, p0, tau, n);
}

SALUN_EXPORT size_t salun_ewc_workspace_bytes(int64_t n) {
  (void)n;
  return sizeof(double) * EWC_MAX_BLOCKS;
}

SALUN_EXPORT int salun_ewc_penalty_grad(const float *p, const float *p_star, const float *F, float *g, double lambda,
                                        float *loss_out, int64_t n, void *ws, size_t ws_bytes,
                                        salun_stream_t stream) {
  if (n < 0 || !loss_out || !ws || (n > 0 && (!p || !p_star || !F || !g))) return SALUN_EINVAL;
  if (ws_bytes < sizeof(double) * EWC_MAX_BLOCKS) return SALUN_ENOSPC;
  hipStream_t st = salun_hip_stream(stream);
  double *partial = static_cast<double *>(ws);
  const bool vec = salun_aligned16(p) && salun_aligned16(p_star) && salun_aligned16(F) && salun_aligned16(g);
  const int rc = stream_launch(k_ewc<true>, k_ewc<false>, vec, n, EWC_MAX_BLOCKS, st, p, p_star, F, g, (float)lambda, n,
                               partial);
  if (rc != SALUN_OK) return rc;
  hipLaunchKernelGGL(k_ewc_final, dim3(1), dim3(SALUN_BLOCK), 0, st, partial, stream_grid(n, vec, EWC_MAX_BLOCKS),
                     (float)lambda, loss_out);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}
