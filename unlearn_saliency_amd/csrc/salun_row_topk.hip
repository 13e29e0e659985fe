// salun_row_topk.hip — the k largest entries of every row of a [B, K] fp32 matrix, sorted, with their indices: the
// torch.topk(p, k) that follows the evaluation head in SD/eval-scripts/imageclassify.py.  gfx950 / CDNA4, wave64.
//
// The order is TOTAL, so the result is defined on every input (torch.topk promises nothing on ties):
//   a larger value comes first; a NaN ranks above every number; equal values - and NaNs among themselves, and -0 with
//   +0 - go by ascending index.
// One workgroup per row, one launch, no atomics.  K <= SALUN_CLS_HEAD_MAX_K = 1024, so a row is at most four elements
// per thread and selection is by RANK: the row's order-preserving integer keys sit in LDS, a thread counts for each of
// its elements how many elements precede it (K compares from LDS, broadcast reads), and an element of rank r < k writes
// slot r.  The ranks of a total order are a permutation, so every slot is written exactly once.
#include "salun_common.h"

namespace {

constexpr int MAX_K = SALUN_CLS_HEAD_MAX_K;

// ascending unsigned order == the rule's ascending order; NaN above +inf; -0 and +0 share a key
__device__ __forceinline__ uint32_t topk_key(float v) {
  if (v != v) return 0xFFFFFFFFu;
  if (v == 0.f) return 0x80000000u;
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(SALUN_BLOCK) void k_row_topk(const float *__restrict__ p, float *__restrict__ values,
                                                          int64_t *__restrict__ indices, int K, int k) {
  __shared__ uint32_t keys[MAX_K];
  const float *row = p + static_cast<int64_t>(blockIdx.x) * K;
  for (int i = threadIdx.x; i < K; i += SALUN_BLOCK) keys[i] = topk_key(row[i]);
  __syncthreads();
  for (int e = threadIdx.x; e < K; e += SALUN_BLOCK) {
    const uint32_t mine = keys[e];
    int rank = 0;
    for (int j = 0; j < K; ++j) {
      const uint32_t o = keys[j];
      rank += (o > mine || (o == mine && j < e)) ? 1 : 0;
    }
    if (rank < k) {
      values[static_cast<int64_t>(blockIdx.x) * k + rank] = row[e];
      indices[static_cast<int64_t>(blockIdx.x) * k + rank] = e;
    }
  }
}

}  // namespace

SALUN_EXPORT int salun_row_topk(const float *p, float *values, int64_t *indices, int64_t B, int K, int k,
                                salun_stream_t stream) {
  if (B < 1 || B > 0x7FFFFFFFll || K < 1 || K > MAX_K || k < 1 || k > K) return SALUN_EINVAL;
  if (!p || !values || !indices || !salun_aligned4(p) || !salun_aligned4(values) ||
      (reinterpret_cast<uintptr_t>(indices) & 7u) != 0)
    return SALUN_EINVAL;
  hipLaunchKernelGGL(k_row_topk, dim3(static_cast<unsigned>(B)), dim3(SALUN_BLOCK), 0, salun_hip_stream(stream), p, values,
                     indices, K, k);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}
