// sa_round.h — the conversions the pad kernels of the 16-bit stores round with (sa_bf16.hip, sa_f16.hip, sa_devrows.hip).
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
