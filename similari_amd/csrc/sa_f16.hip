// sa_f16.hip — feature stores whose rows are IEEE binary16 (include/similari_f16.h): the pad kernel that rounds on the way in and the
// counters of the euclidean expansion (sa_store_expand_last).  The creation call and sa_store_get_info are those of sa_bf16.hip, the
// row movers the f32 store's (a 16-bit row of Dp elements is Dp / 2 floats to them, sa_store::row_floats), launch 2 and the BestFit
// launches see f32 cells, and launch 1 is k_search_tile_f16<EU, JOIN, COMPAT> beside k_search_tile_bf16 in sa_gemm.hip.
#include "sa_round.h"   // f16_bits, f16_widen
#include "sa_store.h"

namespace {

constexpr uint32_t PAD_THREADS = 256, PAD_ROWS = PAD_THREADS / 64;

// k_pad_features_bf16 (sa_bf16.hip) for an f16 destination, the same shape: one wave per row, four rows per workgroup; zero-pad
// D -> Dp, round every value, scatter (row r -> slots[r / K] * K + r % K, or r), and the squared norm of the ROUNDED row in f32.
// A lane takes two neighbouring elements per step and stores them as one 32-bit word.  An absent row is zeros with norm 0.
__global__ __launch_bounds__(PAD_THREADS) void k_pad_features_f16(const float* __restrict__ src, uint32_t rows, uint32_t D, uint32_t Dp,
                                                                  uint32_t K, const uint32_t* __restrict__ slots,
                                                                  const uint8_t* __restrict__ present, uint16_t* __restrict__ dst,
                                                                  float* __restrict__ norms) {
  const uint32_t row = blockIdx.x * PAD_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= rows) return;
  const uint32_t drow = slots ? slots[row / K] * K + row % K : row;
  const bool pres = src && (present ? present[row] != 0 : true);
  const float* s = src + (size_t)row * D;
  uint32_t* d = (uint32_t*)(dst + (size_t)drow * Dp);
  float acc = 0.0f;
  for (uint32_t k = 2 * lane; k < Dp; k += 128u) {
    const uint32_t lo = pres && k < D ? f16_bits(s[k]) : 0u, hi = pres && k + 1 < D ? f16_bits(s[k + 1]) : 0u;
    d[k >> 1] = lo | (hi << 16);
    const float x = f16_widen(lo), y = f16_widen(hi);
    acc += x * x + y * y;
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) norms[drow] = acc;
}

}  // namespace

hipError_t sa_launch_pad_features_f16(const float* src, uint32_t rows, uint32_t D, uint32_t Dp, uint32_t K, const uint32_t* slots,
                                      const uint8_t* present, uint16_t* dst, float* norms, hipStream_t st) {
  if (!rows) return hipSuccess;
  hipLaunchKernelGGL(k_pad_features_f16, dim3((rows + PAD_ROWS - 1) / PAD_ROWS), dim3(PAD_THREADS), 0, st, src, rows, D, Dp, K, slots,
                     present, dst, norms);
  return hipGetLastError();
}

extern "C" {

int sa_store_expand_last(sa_store* s, sa_expand_stats* out) {
  if (!s || !out) return SA_ERR_BAD_ARG;
  if (!s->e || s->broken) return sa_store_enter(s, "sa_store_expand_last");
  *out = s->expand_last;
  out->struct_size = sizeof *out;
  out->reserved = 0;
  return SA_OK;
}

}  // extern "C"
