// salun_device.h — the small device helpers and vector typedefs that several kernel files share: bf16 conversions, the
// MFMA operand types and their transposing LDS read, float wave sums, sigmoid.  One definition each; a rounding rule or
// an operand layout is changed here and nowhere else.  (Host helpers and the double / u64 reductions: salun_common.h.)
#pragma once
#include "salun_common.h"

// ---- vector types -------------------------------------------------------------------
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));   // one MFMA 32x32x16 bf16 operand
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef s16x4 __attribute__((address_space(3))) * lds_s16x4_ptr;
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));   // one MFMA 32x32 fp32 accumulator tile

// D[row][col = lane & 31] of a 32x32 tile: accumulator element v of a lane is row (v&3) + 8*(v>>2) (+ 4 * (lane >> 5)).
__device__ __forceinline__ constexpr int acc_row(int v) { return (v & 3) + 8 * (v >> 2); }

// ---- bf16 <-> fp32 --------------------------------------------------------------------
// round-to-nearest-even, NaN -> quiet NaN (what torch's float -> bfloat16 does)
__device__ __forceinline__ uint16_t f2bf(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }  // v_cvt_pk_bf16_f32: RNE
__device__ __forceinline__ float bf2f(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
// low / high bf16 of a packed pair
__device__ __forceinline__ float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }
// (a, b) -> one packed pair, a in the low half
__device__ __forceinline__ uint32_t pack2(float a, float b) {
  bf16x2_t v;
  v[0] = (__bf16)a; v[1] = (__bf16)b;
  return __builtin_bit_cast(uint32_t, v);
}
// 8 bf16 (16 bytes) <-> 8 floats, element i = f[i]
__device__ __forceinline__ void unpack8(const uint4 v, float (&f)[8]) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) { f[2 * j] = bf2f((uint16_t)(w[j] & 0xffffu)); f[2 * j + 1] = bf2f((uint16_t)(w[j] >> 16)); }
}
__device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
  return make_uint4(pack2(f[0], f[1]), pack2(f[2], f[3]), pack2(f[4], f[5]), pack2(f[6], f[7]));
}

// ---- transposing LDS read -------------------------------------------------------------
// 8 bf16 (one MFMA operand) = two transposing reads of 4: lane i of a 16-lane group receives column i of the
// [4 rows][16 columns] block its group addresses (probe: tools/micro/bf16_probe.hip); `second` is the byte distance
// of rows +4.
__device__ __forceinline__ bf16x8 tr_operand(const char *lds_base, uint32_t byte_off, int second) {
  lds_s16x4_ptr p0 = (lds_s16x4_ptr)(lds_base + byte_off);
  lds_s16x4_ptr p1 = (lds_s16x4_ptr)(lds_base + byte_off + second);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(p0);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(p1);
  union { struct { s16x4 a, b; } s; bf16x8 v; } u;
  u.s.a = lo; u.s.b = hi;
  return u.v;
}

// ---- wave sums of a float (wave = 64 lanes) ---------------------------------------------
// Two different functions: their reduction orders differ, and so do the lanes that hold the sum.  A call site stays with
// the one it has.  (salun_wave_sum of a double / u64 in salun_common.h is of the lane-0 kind.)
// Butterfly: the sum is valid in EVERY lane.
__device__ __forceinline__ float salun_wave_sum_all(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// Shift down: the sum is valid in LANE 0 only.
__device__ __forceinline__ float salun_wave_sum_lane0(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ __forceinline__ float salun_sigmoid(float y) { return 1.0f / (1.0f + expf(-y)); }

// ---- host ------------------------------------------------------------------------------
// workspace sections start on 256-byte boundaries
static inline size_t align256(size_t b) { return (b + 255) & ~size_t(255); }
