// sa_widen.h — widen(x) of include/similari_devrows.h: the exact conversion of an f32, f16 or bf16 source element to f32, as every kernel
// that reads rows out of a caller's device memory takes it (sa_devrows.hip: k_pad_rows; sa_framerows.hip: k_widen_rows).
#pragma once
#include "sa_round.h"
#include "../../include/similari_f16.h"

// widen(h) of a 16-bit source element: exact.  An f16 NaN keeps sign and payload (the hardware's conversion would quiet it).
template <int SRC>
__device__ __forceinline__ float widen16(uint32_t h) {
  if (SRC == SA_ELEM_BF16) return __uint_as_float(h << 16);
  if ((h & 0x7fffu) > 0x7c00u) return __uint_as_float(((h & 0x8000u) << 16) | 0x7f800000u | ((h & 0x3ffu) << 13));
  return f16_widen(h);
}
// element k of a source row, widened
template <int SRC>
__device__ __forceinline__ float load_elem(const char* row, uint32_t k) {
  if (SRC == SA_ELEM_F32) return ((const float*)row)[k];
  return widen16<SRC>(((const uint16_t*)row)[k]);
}
