// salun_stream.h — the one streaming shape of the HBM-bound element-wise kernels over the flat parameter arena
// (salun_update.hip, salun_prox.hip, salun_iu.hip; DESIGN.md §3 "Common streaming shape").
//
// 256-thread workgroups (one wave per SIMD) walk "tiles" of UNROLL x 256 float4 (= 4096 floats for UNROLL 4)
// grid-stride; inside a tile lane l of sub-vector u touches float4 index tile*UNROLL*256 + u*256 + l, so every
// global_load_dwordx4 of a wave covers one contiguous 1 KiB and all UNROLL loads of every stream are issued before the
// first use (8-20 x 16 B in flight per lane).  A u8 mask travels as one dword per float4.  Workgroup 0 handles the
// n % 4 tail; pointers that are not 16-byte aligned take the scalar grid-stride route.
//
// A kernel is an "op" object plus a two-line __global__ wrapper.  The op supplies
//   struct Vec              the registers of one float4 index (one member per stream)
//   void load(Vec &, v)     load every stream at float4 index v
//   void vec(Vec &, v)      compute and store at float4 index v
//   one(i)                  the whole element step at scalar index i (tail and scalar route)
// and may carry state (a reduction keeps its accumulators in the op and finishes with salun_block_sum).
#pragma once
#include <type_traits>
#include "salun_common.h"

constexpr int UNROLL = 4;
constexpr int TILE_VEC = UNROLL * SALUN_BLOCK;  // float4 per tile
constexpr int TILE_ELEMS = TILE_VEC * 4;        // floats per tile

__device__ __forceinline__ float4 ld4(const float *p, int64_t v) { return reinterpret_cast<const float4 *>(p)[v]; }
// Streamed-once operand (the gradient): bypass-friendly non-temporal load.
__device__ __forceinline__ float4 ld4_nt(const float *p, int64_t v) {
  const float4 *q = reinterpret_cast<const float4 *>(p) + v;
  float4 r;
  r.x = __builtin_nontemporal_load(&q->x);
  r.y = __builtin_nontemporal_load(&q->y);
  r.z = __builtin_nontemporal_load(&q->z);
  r.w = __builtin_nontemporal_load(&q->w);
  return r;
}
__device__ __forceinline__ void st4(float *p, int64_t v, float4 x) { reinterpret_cast<float4 *>(p)[v] = x; }
// Four u8 mask bytes of float4 index v as one dword: byte k belongs to component k.
__device__ __forceinline__ uint32_t ldm(const uint8_t *m, int64_t v) { return reinterpret_cast<const uint32_t *>(m)[v]; }
__device__ __forceinline__ bool mbyte(uint32_t m, int k) { return (m & (0xFFu << (8 * k))) != 0; }

template <bool VEC, class Op>
__device__ __forceinline__ void stream_tiles(int64_t n, Op &op) {
  if (VEC) {
    const int64_t nvec = n >> 2;
    const int64_t ntile = (nvec + TILE_VEC - 1) / TILE_VEC;
    for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {
      const int64_t base = t * TILE_VEC + threadIdx.x;
      typename Op::Vec x[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t v = base + u * SALUN_BLOCK;
        if (v < nvec) op.load(x[u], v);
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int64_t v = base + u * SALUN_BLOCK;
        if (v < nvec) op.vec(x[u], v);
      }
    }
    if (blockIdx.x == 0) {  // n % 4 tail
      const int64_t i = (nvec << 2) + threadIdx.x;
      if (i < n) op.one(i);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * SALUN_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SALUN_BLOCK)
      op.one(i);
  }
}

// Workgroups for n elements: one tile each on the float4 route, 4 elements per thread on the scalar route.
static inline int stream_grid(int64_t n, bool vec, int max_grid = SALUN_MAX_GRID) {
  const int grid = salun_grid_for(n, vec ? TILE_ELEMS : SALUN_BLOCK * 4);
  return grid < max_grid ? grid : max_grid;
}

// Launches the float4 kernel when every pointer passed the caller's alignment checks (`vec`), else its scalar twin.
template <class K, class... A>
int stream_launch(K kvec, K kscalar, bool vec, int64_t n, int max_grid, hipStream_t st, A... args) {
  hipLaunchKernelGGL(vec ? kvec : kscalar, dim3(stream_grid(n, vec, max_grid)), dim3(SALUN_BLOCK), 0, st, args...);
  SALUN_LAUNCH_CHECK();
  return SALUN_OK;
}

// Runtime bools -> template arguments: with_bools(f, b0, b1, ...) calls f(std::bool_constant<b0>{}, ...).
template <class F>
int with_bools(F f) {
  return f();
}
template <class F, class... Rest>
int with_bools(F f, bool b, Rest... rest) {
  if (b) return with_bools([&](auto... c) { return f(std::true_type{}, c...); }, rest...);
  return with_bools([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}
