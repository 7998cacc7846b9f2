// sa_round.h — the conversions the pad kernels of the 16-bit stores round with (sa_bf16.hip, sa_f16.hip, sa_devrows.hip), and the
// int8 coding of an i8 store's rows (sa_i8.hip, sa_devrows.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// bf16(x), round-to-nearest-even on the bit pattern (include/similari_bf16.h); a NaN keeps its sign and becomes quiet
__device__ __forceinline__ uint32_t bf16_bits(float x) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// f16(x): the hardware's conversion under the default mode — round-to-nearest-even, overflow to +-inf, a NaN stays a NaN, subnormal
// results kept (f16 denormals are on by default) — and back, which is exact
__device__ __forceinline__ uint32_t f16_bits(float x) { return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)x); }
__device__ __forceinline__ float f16_widen(uint32_t h) { return (float)__builtin_bit_cast(_Float16, (uint16_t)h); }

// ---- the int8 codes of a row (include/similari_i8.h; sa_i8.hip, sa_devrows.hip) ----
// |x| as an unsigned integer: NaN > inf > every finite value, so one unsigned maximum over a row yields both m and the non-finite test
__device__ __forceinline__ uint32_t i8_abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }
__device__ __forceinline__ uint32_t i8_wave_max(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t w = (uint32_t)__shfl_xor((int)v, o);
    v = w > v ? w : v;
  }
  return v;
}
// 127 / m of a row whose absmax has the bits mb, or 0 for a ZERO ROW: m == 0, m not finite, m < 2^-100 (0x0d800000).  The division is
// the correctly rounded one (no fast-math in this build); 0 * x_k is a code of 0 for every finite x_k, and a row with a non-finite
// element never gets here with a non-zero inv.
__device__ __forceinline__ float i8_inv(uint32_t mb) { return mb >= 0x0d800000u && mb < 0x7f800000u ? 127.0f / __uint_as_float(mb) : 0.0f; }
// clamp(rintf(x * inv), -127, 127) as a byte; inv == 0 (a ZERO ROW): 0 whatever x is
__device__ __forceinline__ uint32_t i8_code(float x, float inv) {
  if (inv == 0.0f) return 0u;
  const float r = fminf(fmaxf(rintf(x * inv), -127.0f), 127.0f);
  return (uint32_t)(int)r & 0xffu;
}
__device__ __forceinline__ int i8_value(uint32_t b) { return (int)(int8_t)(b & 0xffu); }
