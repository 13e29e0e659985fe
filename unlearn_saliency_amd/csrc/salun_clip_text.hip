// salun_clip_text.hip — K29: the four kernels the CLIP text encoder of Stable Diffusion v1 needs beside the K15 GEMM.
//
// Reference: SD/ldm/modules/encoders/modules.py `FrozenCLIPEmbedder.forward` -> transformers' CLIPTextModel (ViT-L/14
// text tower): token + position embedding, 12 pre-LayerNorm blocks of causal self-attention (12 heads of 64) and a
// quick-GELU MLP, a final LayerNorm; 77 tokens, width 768, fp32.  The Linear layers run on K15 (salun_gemm.hip) as they
// are; what no other kernel of the library covers is here.  All four are fp32, forward only, deterministic (no atomics),
// launched on the caller's stream, and compiled with -ffp-contract=off: every rounding is the one written.
//
// salun_clip_embed       x[b, t, :] = tok[ids[b, t], :] + pos[t, :].
//   Rounding points: ONE fp32 add per element (bit-identical to the torch expression).  An id outside [0, V) — the host
//   wrapper refuses those before the launch — reads nothing and writes a row of NaN.
//
// salun_ln_f32_forward   LayerNorm over the last dimension of [rows, W], W % 4 == 0, W <= 2048.  One wave per row (as
//   k_ln16_fwd of salun_tok_bf16.hip); the row stays in registers between the statistics and the normalise step.
//   Rounding points, all fp32:
//     sum   a lane adds its <= 32 elements in index order (float4 index lane, lane + 64, ...; x, y, z, w inside), the 64
//           lane sums are folded by a 6-step butterfly:            at most 31 + 6 additions on any element's path
//     mean  = sum / W                                              (IEEE division, W exact)
//     d     = x - mean                                             (one subtraction; computed twice, same value)
//     q     = sum of d * d, same order as `sum`                    (one multiplication + <= 37 additions)
//     var   = q / W;  r = 1 / sqrtf(var + eps)                     (addition, IEEE sqrt, IEEE division; eps rounded to fp32)
//     y     = ((d * r) * gamma) + beta                             (two multiplications, one addition)
//
// salun_attn_causal_f32  o = softmax(scale q k^T + causal) v per (batch, head); D = 64, 1 <= T <= T_max = 128
//   (SALUN_CLIP_ATTN_MAX_T).  q, k, v are read in place from the fused projection buffer: element (b, t, h, d) of q at
//   qkv[(b T + t) ld + q_off + 64 h + d], k and v at k_off / v_off; o is written head-concatenated,
//   o[(b T + t) ld_o + 64 h + d].  One 256-thread workgroup per (b, h): the three [16 ceil(T / 16)][64] operands sit in
//   LDS at once (rows of 68 floats; rows >= T are zero, never read from memory; 102 KiB at T_max, 63.75 KiB at T = 77,
//   through the dynamic-LDS opt-in of salun_common.h).  A wave owns 16-query tiles qi = wave, wave + 4, ...; for each it
//   visits key tiles kj = 0 .. qi only: tiles wholly above the diagonal are skipped, not computed and masked.  Both
//   products run on v_mfma_f32_16x16x4_f32, kept transposed (S^T[key][query] = K . Q^T) so that the scores a lane holds
//   are already the A operand of O = P . V: no score ever leaves the registers.
//   Rounding points, all fp32:
//     s_raw = sum_d q_d k_d        one fma chain in ascending d, from 0             (64 roundings)
//     s     = s_raw * scale        (one multiplication; scale rounded to fp32)
//     m     = max of s over the allowed keys j <= t                                  (exact)
//     e_j   = expf(s_j - m) for j <= t, and EXACTLY 0 for j > t — the padding columns j >= T of the last tile included
//             (one subtraction, one expf: OCML, 1 ulp)
//     l     = sum of e_j: in a lane over its 4 keys of each visited tile in ascending order, then a 2-step butterfly
//             over the 4 lanes of a query                                            (<= 4 (qi + 1) + 1 additions)
//     acc_d = sum_j e_j v_jd       one fma chain from 0 over the keys of the visited tiles, tile after tile, inside a
//             tile in the order 0 4 8 12 1 5 9 13 ...                                (16 (qi + 1) roundings)
//     o_d   = acc_d / l            (IEEE division)
//   Rows t >= T are never stored.  A masked weight is the constant 0, not expf(-inf), and every LDS row that stands for a
//   token >= T is zero: nothing outside the [T, 3 W] operand can reach the result.
//
// salun_quick_gelu       x <- x * sigmoid(1.702 x) in place, on the streaming-tile template of salun_stream.h.
//   Rounding points:  t = 1.702f * x;  e = expf(-t);  s = 1 / (1 + e);  y = x * s   (multiplication, expf (OCML, 1 ulp),
//   addition, IEEE division, multiplication).  expf overflows to +inf below x = -52.1: s = 0 and y = -0.
#include "salun_device.h"
#include "salun_stream.h"

namespace {

// ---------------------------------------------------------------------------------------------- embedding
constexpr int EMB_ROWS_PER_WG = 4;  // one wave per token row

__global__ __launch_bounds__(256) void k_clip_embed(const int64_t *__restrict__ ids, const float *__restrict__ tok,
                                                    const float *__restrict__ pos, float *__restrict__ x, int64_t rows,
                                                    int T, int W, int64_t V) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * EMB_ROWS_PER_WG + wave;
  if (row >= rows) return;
  const int64_t id = ids[row];
  const int t = (int)(row % T);
  const bool ok = id >= 0 && id < V;
  const float4 *tp = reinterpret_cast<const float4 *>(tok + (ok ? id : 0) * W);
  const float4 *pp = reinterpret_cast<const float4 *>(pos + (int64_t)t * W);
  float4 *xp = reinterpret_cast<float4 *>(x + row * W);
  const float nan = __uint_as_float(0x7FC00000u);
  for (int i = lane; i < (W >> 2); i += 64) {
    float4 r = make_float4(nan, nan, nan, nan);
    if (ok) {
      const float4 a = tp[i], b = pp[i];
      r = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    }
    xp[i] = r;
  }
}

// ---------------------------------------------------------------------------------------------- LayerNorm
constexpr int LNF_MAXV = 8;         // float4 per lane: W <= 2048
constexpr int LNF_ROWS_PER_WG = 4;  // one wave per row

__global__ __launch_bounds__(256) void k_ln_f32_fwd(const float *__restrict__ x, const float *__restrict__ gamma,
                                                    const float *__restrict__ beta, float *__restrict__ y, int64_t rows,
                                                    int W, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * LNF_ROWS_PER_WG + wave;
  if (row >= rows) return;
  const int nv = W >> 2;
  const float4 *xp = reinterpret_cast<const float4 *>(x + row * W);
  float4 v[LNF_MAXV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < LNF_MAXV; ++i) {
    const int o = lane + 64 * i;
    if (o < nv) {
      v[i] = xp[o];
      s += v[i].x; s += v[i].y; s += v[i].z; s += v[i].w;
    }
  }
  const float mean = salun_wave_sum_all(s) / (float)W;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < LNF_MAXV; ++i)
    if (lane + 64 * i < nv) {
      float d;
      d = v[i].x - mean; q += d * d;
      d = v[i].y - mean; q += d * d;
      d = v[i].z - mean; q += d * d;
      d = v[i].w - mean; q += d * d;
    }
  const float var = salun_wave_sum_all(q) / (float)W;
  const float r = 1.0f / sqrtf(var + eps);
  float4 *yp = reinterpret_cast<float4 *>(y + row * W);
#pragma unroll
  for (int i = 0; i < LNF_MAXV; ++i) {
    const int o = lane + 64 * i;
    if (o < nv) {
      const float *g = gamma + 4 * o, *b = beta + 4 * o;  // parameters: 4-byte aligned is all that is asked of them
      float4 out;
      out.x = ((v[i].x - mean) * r) * g[0] + b[0];
      out.y = ((v[i].y - mean) * r) * g[1] + b[1];
      out.z = ((v[i].z - mean) * r) * g[2] + b[2];
      out.w = ((v[i].w - mean) * r) * g[3] + b[3];
      yp[o] = out;
    }
  }
}

// ---------------------------------------------------------------------------------------------- causal attention
constexpr int CA_D = SALUN_CLIP_ATTN_D;               // 64
constexpr int CA_MAXNT = SALUN_CLIP_ATTN_MAX_T / 16;  // 8 tiles of 16 tokens
constexpr int CA_LD = CA_D + 4;                       // LDS row in floats: 16-byte aligned rows, rows 4 banks apart

static inline size_t ca_lds_bytes(int T) { return (size_t)3 * ((T + 15) / 16 * 16) * CA_LD * sizeof(float); }

__global__ __launch_bounds__(256) void k_attn_causal_f32(const float *__restrict__ qkv, float *__restrict__ o, int H, int T,
                                                         long long ld, int q_off, int k_off, int v_off, long long ld_o,
                                                         float scale) {
  extern __shared__ __align__(16) float ca_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int NT = (T + 15) >> 4, TP = NT * 16;
  float *Qs = ca_lds, *Ks = Qs + TP * CA_LD, *Vs = Ks + TP * CA_LD;

  // global -> LDS: rows < T are read, rows in [T, TP) are zero
  const float *base = qkv + (long long)b * T * ld + h * CA_D;
  for (int id = tid; id < 3 * TP * (CA_D / 4); id += 256) {
    const int which = id / (TP * (CA_D / 4)), rem = id - which * (TP * (CA_D / 4));
    const int row = rem >> 4, c4 = rem & 15;
    float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < T) {
      const int off = which == 0 ? q_off : (which == 1 ? k_off : v_off);
      val = *reinterpret_cast<const float4 *>(base + (long long)row * ld + off + c4 * 4);
    }
    *reinterpret_cast<float4 *>(ca_lds + ((size_t)which * TP + row) * CA_LD + c4 * 4) = val;
  }
  __syncthreads();

  for (int qi = wave; qi < NT; qi += 4) {
    // B operand of S^T = K . Q^T: lane (c, g) holds Q[qi * 16 + c][4 step + g]
    float qreg[CA_D / 4];
#pragma unroll
    for (int st = 0; st < CA_D / 4; ++st) qreg[st] = Qs[(qi * 16 + c) * CA_LD + 4 * st + g];
    const int query = qi * 16 + c;

    // scores: lane (c, g), register r of tile kj = key kj * 16 + 4 g + r against query qi * 16 + c
    f32x4v s[CA_MAXNT];
    float m = -INFINITY;
#pragma unroll
    for (int kj = 0; kj < CA_MAXNT; ++kj) {
      if (kj <= qi) {
        f32x4v acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < CA_D / 4; ++st)
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Ks[(kj * 16 + c) * CA_LD + 4 * st + g], qreg[st], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float sc = acc[r] * scale;
          acc[r] = sc;
          if (kj * 16 + 4 * g + r <= query) m = fmaxf(m, sc);
        }
        s[kj] = acc;
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));  // key 0 is allowed for every query: m is a score, never -inf

    float l = 0.f;
#pragma unroll
    for (int kj = 0; kj < CA_MAXNT; ++kj) {
      if (kj <= qi) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = (kj * 16 + 4 * g + r <= query) ? expf(s[kj][r] - m) : 0.f;
          s[kj][r] = e;
          l += e;
        }
      }
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);

    // O = P . V: A = P[query c][key 4 g + r] (the registers as they are), B = V[key 4 g + r][d = 16 dt + c]
    f32x4v acc_o[CA_D / 16];
#pragma unroll
    for (int dt = 0; dt < CA_D / 16; ++dt) acc_o[dt] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kj = 0; kj < CA_MAXNT; ++kj) {
      if (kj <= qi) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float *vrow = Vs + (kj * 16 + 4 * g + r) * CA_LD + c;
#pragma unroll
          for (int dt = 0; dt < CA_D / 16; ++dt)
            acc_o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(s[kj][r], vrow[16 * dt], acc_o[dt], 0, 0, 0);
        }
      }
    }
    // lane (c, g), register r of acc_o[dt] = O[query qi * 16 + 4 g + r][d = 16 dt + c]; that query's l sits in lane 4 g + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float lq = __shfl(l, 4 * g + r, 64);
      const int t = qi * 16 + 4 * g + r;
      if (t < T) {
        float *op = o + ((long long)b * T + t) * ld_o + h * CA_D + c;
#pragma unroll
        for (int dt = 0; dt < CA_D / 16; ++dt) op[16 * dt] = acc_o[dt][r] / lq;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- quick-GELU
__device__ __forceinline__ float quick_gelu(float x) {
  const float t = 1.702f * x;
  const float e = expf(-t);
  const float s = 1.0f / (1.0f + e);
  return x * s;
}

struct QuickGeluOp {
  float *x;
  struct Vec { float4 a; };
  __device__ void load(Vec &r, int64_t v) const { r.a = ld4(x, v); }
  __device__ void vec(Vec &r, int64_t v) const {
    st4(x, v, make_float4(quick_gelu(r.a.x), quick_gelu(r.a.y), quick_gelu(r.a.z), quick_gelu(r.a.w)));
  }
  __device__ void one(int64_t i) const { x[i] = quick_gelu(x[i]); }
};

template <bool VEC>
__global__ __launch_bounds__(SALUN_BLOCK) void k_quick_gelu(float *__restrict__ x, int64_t n) {
  QuickGeluOp op{x};
  stream_tiles<VEC>(n, op);
}

}  // namespace

// ================================================================== C-ABI =======
SALUN_EXPORT int salun_clip_embed(const int64_t *ids, const float *tok, const float *pos, float *x, int64_t B, int T, int W,
                                  int64_t V, salun_stream_t stream) {
  if (B < 1 || T < 1 || W < 4 || (W & 3) || V < 1 || !ids || !tok || !pos || !x) return SALUN_EINVAL;
  if (B * (int64_t)T > (int64_t)1 << 31 || V * (int64_t)W > (int64_t)1 << 40) return SALUN_EINVAL;
  if (!salun_aligned16(tok) || !salun_aligned16(pos) || !salun_aligned16(x) || (reinterpret_cast<uintptr_t>(ids) & 7u))
    return SALUN_EINVAL;
  const int64_t rows = B * T;
  const int grid = (int)((rows + EMB_ROWS_PER_WG - 1) / EMB_ROWS_PER_WG);
  hipLaunchKernelGGL(k_clip_embed, dim3(grid), dim3(256), 0, salun_hip_stream(stream), ids, tok, pos, x, rows, T, W, V);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_ln_f32_forward(const float *x, const float *gamma, const float *beta, float *y, int64_t rows, int W,
                                      double eps, salun_stream_t stream) {
  if (rows < 1 || W < 4 || (W & 3) || W > 256 * LNF_MAXV || !x || !gamma || !beta || !y) return SALUN_EINVAL;
  if (rows > (int64_t)1 << 31 || !(eps >= 0.0)) return SALUN_EINVAL;
  if (!salun_aligned16(x) || !salun_aligned16(y) || !salun_aligned4(gamma) || !salun_aligned4(beta)) return SALUN_EINVAL;
  const int grid = (int)((rows + LNF_ROWS_PER_WG - 1) / LNF_ROWS_PER_WG);
  hipLaunchKernelGGL(k_ln_f32_fwd, dim3(grid), dim3(256), 0, salun_hip_stream(stream), x, gamma, beta, y, rows, W,
                     (float)eps);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_attn_causal_f32(const float *qkv, float *o, int B, int H, int T, int D, int64_t ld, int q_off,
                                       int k_off, int v_off, int64_t ld_o, double scale, salun_stream_t stream) {
  if (!qkv || !o || B < 1 || H < 1 || D != CA_D || T < 1 || T > SALUN_CLIP_ATTN_MAX_T) return SALUN_EINVAL;
  if ((int64_t)B * H > (int64_t)1 << 20 || (int64_t)B * T > (int64_t)1 << 24) return SALUN_EINVAL;
  if (q_off < 0 || k_off < 0 || v_off < 0 || ((q_off | k_off | v_off) & 3) || (ld & 3) || (ld_o & 3)) return SALUN_EINVAL;
  const int64_t span = (int64_t)H * CA_D;  // one operand's columns of a row
  if (ld < span || ld_o < span || q_off + span > ld || k_off + span > ld || v_off + span > ld) return SALUN_EINVAL;
  if (!salun_aligned16(qkv) || !salun_aligned16(o)) return SALUN_EINVAL;
  return salun_launch_lds<k_attn_causal_f32>(dim3(B * H), dim3(256), ca_lds_bytes(T), salun_hip_stream(stream), qkv, o, H,
                                             T, (long long)ld, q_off, k_off, v_off, (long long)ld_o, (float)scale);
}

SALUN_EXPORT int salun_quick_gelu(float *x, int64_t n, salun_stream_t stream) {
  if (n < 0 || (n > 0 && !x) || !salun_aligned4(x)) return SALUN_EINVAL;
  if (n == 0) return SALUN_OK;
  return stream_launch(k_quick_gelu<true>, k_quick_gelu<false>, salun_aligned16(x), n, SALUN_MAX_GRID,
                       salun_hip_stream(stream), x, n);
}
