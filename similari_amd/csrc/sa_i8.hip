// sa_i8.hip — feature stores whose rows are int8 codes (include/similari_i8.h): the creation call and the pad kernel that takes the
// codes on the way in.  sa_store_get_info is that of sa_bf16.hip, the row movers the f32 store's (an i8 row of Dp elements is Dp / 4
// floats to them, sa_store::row_floats), launch 2 and the BestFit launches see f32 cells, and launch 1 is k_search_tile_i8<JOIN, COMPAT>
// beside k_search_tile_bf16 in sa_gemm.hip.
#include "sa_round.h"   // i8_abs_bits, i8_inv, i8_code
#include "sa_store.h"

namespace {

constexpr uint32_t PAD_THREADS = 256, PAD_ROWS = PAD_THREADS / 64;

// k_pad_features_bf16 (sa_bf16.hip) for an i8 destination, the same shape: one wave per row, four rows per workgroup; zero-pad
// D -> Dp, scatter (row r -> slots[r / K] * K + r % K, or r).  Two passes over the row: the unsigned maximum of |x_k|'s bits (one
// integer wave reduction: m and the non-finite test), then the codes, four neighbouring elements per lane and step stored as one
// 32-bit word (Dp is a multiple of 64; a row starts 64-byte aligned).  The squared norm is the integer sum of the squared codes,
// reduced in integers and converted once: no order is involved.  An absent row is zeros with norm 0.
__global__ __launch_bounds__(PAD_THREADS) void k_pad_features_i8(const float* __restrict__ src, uint32_t rows, uint32_t D, uint32_t Dp,
                                                                 uint32_t K, const uint32_t* __restrict__ slots,
                                                                 const uint8_t* __restrict__ present, uint8_t* __restrict__ dst,
                                                                 float* __restrict__ norms) {
  const uint32_t row = blockIdx.x * PAD_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= rows) return;
  const uint32_t drow = slots ? slots[row / K] * K + row % K : row;
  const bool pres = src && (present ? present[row] != 0 : true);
  const float* s = src + (size_t)row * D;
  uint32_t* d = (uint32_t*)(dst + (size_t)drow * Dp);
  uint32_t mb = 0;
  if (pres)
    for (uint32_t k = lane; k < D; k += 64u) {
      const uint32_t b = i8_abs_bits(s[k]);
      mb = b > mb ? b : mb;
    }
  const float inv = i8_inv(i8_wave_max(mb));
  uint32_t acc = 0;
  for (uint32_t k = 4 * lane; k < Dp; k += 256u) {
    uint32_t word = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t b = pres && k + j < D ? i8_code(s[k + j], inv) : 0u;
      const int q = i8_value(b);
      word |= b << (8 * j);
      acc += (uint32_t)(q * q);
    }
    d[k >> 2] = word;
  }
  for (int o = 32; o > 0; o >>= 1) acc += (uint32_t)__shfl_xor((int)acc, o);
  if (lane == 0) norms[drow] = (float)acc;
}

}  // namespace

hipError_t sa_launch_pad_features_i8(const float* src, uint32_t rows, uint32_t D, uint32_t Dp, uint32_t K, const uint32_t* slots,
                                     const uint8_t* present, uint8_t* dst, float* norms, hipStream_t st) {
  if (!rows) return hipSuccess;
  hipLaunchKernelGGL(k_pad_features_i8, dim3((rows + PAD_ROWS - 1) / PAD_ROWS), dim3(PAD_THREADS), 0, st, src, rows, D, Dp, K, slots,
                     present, dst, norms);
  return hipGetLastError();
}

extern "C" {

int sa_store_create_i8(sa_engine* e, const sa_store_options* o, sa_store** out) {
  const char* what = "sa_store_create_i8";
  if (out) *out = nullptr;
  // without an engine the answer is about the device, as sa_store_create gives it, whatever else is wrong with the call
  if (e && o && o->struct_size >= sizeof(sa_store_options)) {
    if (o->visual_kind == SA_VIS_EUCLIDEAN)
      return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: an i8 store is cosine only (per-row scales cancel in the cosine alone; the f16 store is the compact euclidean store)", what);
    if (o->feature_len > SA_I8_MAX_FEATURE_LEN)
      return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: feature_len %u above %u (127^2 Dp must stay below 2^31)", what, o->feature_len, SA_I8_MAX_FEATURE_LEN);
  }
  return sa_store_create_as(e, o, SA_ELEM_I8, what, out);
}

}  // extern "C"
