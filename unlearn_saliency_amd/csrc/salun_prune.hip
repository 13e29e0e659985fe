// salun_prune.hip — K22: global unstructured pruning on the flat arena (include/salun.h).
//
// A pruning round of the reference (Classification/pruner/utils.py:23-35,66-80: torch.nn.utils.prune.global_unstructured
// over every nn.Conv2d weight) is a parameters_to_vector cat, a torch.topk over the ~11 M convolution weights and a
// per-layer scatter, and afterwards every forward multiplies weight_orig * weight_mask per layer.  Here a round is
//
//   k_prune_gather   |p| of the segments -> one compact key vector; already pruned entries become NaN, which the
//                    select ranks after every number, so they can never be selected again
//   salun_mask_topk  the existing select (csrc/salun_topk.hip) on the compact keys with k_keep = R - k_prune
//   k_prune_scatter  alive and not selected -> keep = 0, p = 0, buf = 0; every other byte is left alone
//
// and nothing per step: the arena holds the effective weights and the fused SGD step already keeps a weight whose mask
// byte is 0 at its value with zero momentum.
//
// The segment table lives in device memory (it is built once per model); both kernels re-derive the compact prefix
// from it in LDS and VERIFY it against n and n_sel before touching memory: a table that is not ascending, leaves
// [0, n) or does not sum to n_sel makes the round a no-op and raises the error flag that salun_prune_status reports.
#include "salun_device.h"

namespace {

constexpr int MAX_SEG = SALUN_PRUNE_MAX_SEGMENTS;
constexpr uint32_t KEY_NAN = 0x7FC00000u;
constexpr uint32_t KEY_INF = 0x7F800000u;

struct PruneHdr {
  uint32_t bad_table;  // a kernel of the last round refused the segment table
  uint32_t pad[63];
};

struct WsLayout {
  size_t off_hdr, off_keys, off_sel, bytes;
};
// [ top-k workspace (its publication block first, so salun_mask_topk_status reads it) | header | keys | selection ]
inline WsLayout ws_layout(int64_t n_sel) {
  WsLayout W;
  W.off_hdr = align256(salun_mask_topk_workspace_bytes(n_sel, 1));
  W.off_keys = W.off_hdr + sizeof(PruneHdr);
  W.off_sel = W.off_keys + align256(sizeof(float) * (size_t)n_sel);
  W.bytes = W.off_sel + align256((size_t)n_sel);
  return W;
}

// The table in LDS: s_off[s] = first flat element of segment s, s_start[s] = its first compact index
// (s_start[nseg] = n_sel).  Returns false (for the whole block) if the table is not usable.
__device__ bool load_segments(const long long *__restrict__ segs, int nseg, int64_t n, int64_t n_sel, long long *s_off,
                              long long *s_start, int *s_ok) {
  for (int s = threadIdx.x; s < nseg; s += blockDim.x) {
    s_off[s] = segs[2 * s];
    s_start[s + 1] = segs[2 * s + 1];  // lengths for now
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long run = 0, end = 0;
    int ok = 1;
    for (int s = 0; s < nseg; ++s) {
      const long long off = s_off[s], len = s_start[s + 1];
      if (off < end || len < 0 || off > n || len > n - off) { ok = 0; break; }
      end = off + len;
      s_start[s] = run;
      run += len;
    }
    if (ok) s_start[nseg] = run;
    *s_ok = ok && run == n_sel;
  }
  __syncthreads();
  return *s_ok != 0;
}

// compact index -> flat index: the last segment whose first compact index is <= j (empty segments share a start with
// their successor and are skipped by "last").
__device__ __forceinline__ int64_t flat_index(int64_t j, int nseg, const long long *s_off, const long long *s_start) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (s_start[mid] <= j) lo = mid; else hi = mid - 1;
  }
  return s_off[lo] + (j - s_start[lo]);
}

#define PRUNE_SEG_LDS                         \
  __shared__ long long s_off[MAX_SEG];        \
  __shared__ long long s_start[MAX_SEG + 1];  \
  __shared__ int s_ok;

__global__ __launch_bounds__(SALUN_BLOCK) void k_prune_gather(const float *__restrict__ p, const uint8_t *__restrict__ keep,
                                                              const float *__restrict__ rnd, const long long *__restrict__ segs,
                                                              int nseg, int64_t n, int64_t n_sel, uint32_t *__restrict__ keys,
                                                              PruneHdr *hdr) {
  PRUNE_SEG_LDS
  const bool ok = load_segments(segs, nseg, n, n_sel, s_off, s_start, &s_ok);
  if (blockIdx.x == 0 && threadIdx.x == 0) hdr->bad_table = ok ? 0u : 1u;
  if (!ok) return;
  for (int64_t j = (int64_t)blockIdx.x * SALUN_BLOCK + threadIdx.x; j < n_sel; j += (int64_t)gridDim.x * SALUN_BLOCK) {
    const int64_t i = flat_index(j, nseg, s_off, s_start);
    uint32_t key = KEY_NAN;
    if (keep[i]) {
      key = __float_as_uint(rnd ? rnd[j] : p[i]) & 0x7FFFFFFFu;
      if (key > KEY_INF) key = KEY_INF;  // a NaN weight is alive: it ranks first (as torch.topk has it), not with the pruned
    }
    keys[j] = key;
  }
}

// sel == nullptr: nothing was selected (k_keep == 0), every alive element of the segments goes.
__global__ __launch_bounds__(SALUN_BLOCK) void k_prune_scatter(float *__restrict__ p, float *__restrict__ buf,
                                                               uint8_t *__restrict__ keep, const uint8_t *__restrict__ sel,
                                                               const long long *__restrict__ segs, int nseg, int64_t n,
                                                               int64_t n_sel, PruneHdr *hdr) {
  PRUNE_SEG_LDS
  const bool ok = load_segments(segs, nseg, n, n_sel, s_off, s_start, &s_ok);
  if (!ok) {
    if (blockIdx.x == 0 && threadIdx.x == 0) hdr->bad_table = 1u;
    return;
  }
  for (int64_t j = (int64_t)blockIdx.x * SALUN_BLOCK + threadIdx.x; j < n_sel; j += (int64_t)gridDim.x * SALUN_BLOCK) {
    if (sel && sel[j]) continue;
    const int64_t i = flat_index(j, nseg, s_off, s_start);
    if (!keep[i]) continue;
    keep[i] = 0;
    p[i] = 0.0f;
    if (buf) buf[i] = 0.0f;
  }
}

__global__ __launch_bounds__(SALUN_BLOCK) void k_prune_count_zeros(const float *__restrict__ p,
                                                                   const long long *__restrict__ segs, int nseg, int64_t n,
                                                                   int64_t n_sel, unsigned long long *__restrict__ count) {
  PRUNE_SEG_LDS
  __shared__ unsigned long long lds[4];
  if (!load_segments(segs, nseg, n, n_sel, s_off, s_start, &s_ok)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *count = ~0ull;  // -1: the table was refused
    return;
  }
  unsigned long long c = 0;
  for (int64_t j = (int64_t)blockIdx.x * SALUN_BLOCK + threadIdx.x; j < n_sel; j += (int64_t)gridDim.x * SALUN_BLOCK)
    c += p[flat_index(j, nseg, s_off, s_start)] == 0.0f;
  c = salun_wave_sum_u64(c);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long s = lds[0] + lds[1] + lds[2] + lds[3];
    if (s) atomicAdd(count, s);  // integer: the order of the adds does not matter
  }
}

}  // namespace

// ================================================================== C-ABI =======
SALUN_EXPORT size_t salun_prune_workspace_bytes(int64_t n_sel) {
  if (n_sel < 0) return 0;
  return ws_layout(n_sel).bytes;
}

SALUN_EXPORT int salun_prune_global(float *p, float *buf, uint8_t *keep, int64_t n, const int64_t *segs, int nseg,
                                    int64_t n_sel, int64_t alive, int64_t k_prune, const float *rnd, unsigned flags,
                                    void *ws, size_t ws_bytes, salun_stream_t stream) {
  if (n < 0 || n_sel < 0 || n_sel > n || nseg < 0 || nseg > MAX_SEG || alive < 0 || alive > n_sel || k_prune < 0 ||
      k_prune > alive || !ws)
    return SALUN_EINVAL;
  if (n_sel > 0 && (!p || !keep || !segs || nseg < 1)) return SALUN_EINVAL;
  if (flags & ~SALUN_TOPK_FORCE_FULL_SCAN) return SALUN_EINVAL;
  const WsLayout W = ws_layout(n_sel);
  if (ws_bytes < W.bytes) return SALUN_ENOSPC;
  if (k_prune == 0 || n_sel == 0) return SALUN_OK;
  hipStream_t st = salun_hip_stream(stream);
  char *base = static_cast<char *>(ws);
  PruneHdr *hdr = reinterpret_cast<PruneHdr *>(base + W.off_hdr);
  uint32_t *keys = reinterpret_cast<uint32_t *>(base + W.off_keys);
  uint8_t *sel = reinterpret_cast<uint8_t *>(base + W.off_sel);
  const long long *tab = reinterpret_cast<const long long *>(segs);
  const int grid = salun_grid_for(n_sel, SALUN_BLOCK * 4);
  const int64_t k_keep = alive - k_prune;
  if (k_keep == 0) {  // everything alive goes: no ranking needed
    if (hipMemsetAsync(hdr, 0, sizeof(PruneHdr), st) != hipSuccess) return SALUN_EIO;
    hipLaunchKernelGGL(k_prune_scatter, dim3(grid), dim3(SALUN_BLOCK), 0, st, p, buf, keep,
                       static_cast<const uint8_t *>(nullptr), tab, nseg, n, n_sel, hdr);
    SALUN_LAUNCH_CHECK();
    return SALUN_OK;
  }
  hipLaunchKernelGGL(k_prune_gather, dim3(grid), dim3(SALUN_BLOCK), 0, st, p, keep, rnd, tab, nseg, n, n_sel, keys, hdr);
  SALUN_LAUNCH_CHECK();
  uint8_t *masks[1] = {sel};
  const int rc = salun_mask_topk_ex(reinterpret_cast<const float *>(keys), n_sel, &k_keep, 1, masks, ws, W.off_hdr, flags,
                                    stream);
  if (rc != SALUN_OK) return rc;
  hipLaunchKernelGGL(k_prune_scatter, dim3(grid), dim3(SALUN_BLOCK), 0, st, p, buf, keep, sel, tab, nseg, n, n_sel, hdr);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

SALUN_EXPORT int salun_prune_status(const void *ws, int64_t n_sel, int ranked, int *route_out, int *error_out,
                                    salun_stream_t stream) {
  if (!ws || n_sel < 0 || !route_out || !error_out) return SALUN_EINVAL;
  *route_out = 0;
  *error_out = 0;
  if (ranked) {
    const int rc = salun_mask_topk_status(ws, route_out, error_out, stream);
    if (rc != SALUN_OK) return rc;
  }
  PruneHdr host;
  hipStream_t st = salun_hip_stream(stream);
  const char *base = static_cast<const char *>(ws);
  if (hipMemcpyAsync(&host, base + ws_layout(n_sel).off_hdr, sizeof(PruneHdr), hipMemcpyDeviceToHost, st) != hipSuccess)
    return SALUN_EIO;
  if (hipStreamSynchronize(st) != hipSuccess) return SALUN_EIO;
  if (host.bad_table) *error_out |= 2;
  return SALUN_OK;
}

SALUN_EXPORT int salun_prune_count_zeros(const float *p, int64_t n, const int64_t *segs, int nseg, int64_t n_sel,
                                         int64_t *count, salun_stream_t stream) {
  if (n < 0 || n_sel < 0 || n_sel > n || nseg < 0 || nseg > MAX_SEG || !count) return SALUN_EINVAL;
  if (n_sel > 0 && (!p || !segs || nseg < 1)) return SALUN_EINVAL;
  hipStream_t st = salun_hip_stream(stream);
  if (hipMemsetAsync(count, 0, sizeof(int64_t), st) != hipSuccess) return SALUN_EIO;
  if (n_sel == 0) return SALUN_OK;
  hipLaunchKernelGGL(k_prune_count_zeros, dim3(salun_grid_for(n_sel, SALUN_BLOCK * 4)), dim3(SALUN_BLOCK), 0, st, p,
                     reinterpret_cast<const long long *>(segs), nseg, n, n_sel,
                     reinterpret_cast<unsigned long long *>(count));
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}
