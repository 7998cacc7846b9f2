// sa_bf16.hip — feature stores whose rows are bf16 (include/similari_bf16.h): the creation call with an element type, what a store
// is made of (sa_store_get_info), and the pad kernel that rounds on the way in.  Everything else a bf16 store does is the f32 store's
// code: the row movers (k_gather, k_merge_gather / _scatter / _compact, the removal's device copies) copy 16-byte pieces of a row and
// are handed its length in floats (sa_store::row_floats, half of Dp), launch 2 and the BestFit launches see f32 cells, and launch 1
// is k_search_tile_bf16 beside k_search_tile in sa_gemm.hip, whose epilogue it shares.
#include "sa_round.h"   // bf16_bits
#include "sa_store.h"

namespace {

constexpr uint32_t PAD_THREADS = 256, PAD_ROWS = PAD_THREADS / 64;

// k_pad_features for a bf16 destination.  One wave per row, four rows per workgroup: zero-pad D -> Dp, round every value, scatter
// (row r -> slots[r / K] * K + r % K, or r), and the squared norm of the ROUNDED row in f32.  A lane takes two neighbouring elements
// per step and stores them as one 32-bit word (Dp is even; a row starts 64-byte aligned).  An absent row is zeros with norm 0.
__global__ __launch_bounds__(PAD_THREADS) void k_pad_features_bf16(const float* __restrict__ src, uint32_t rows, uint32_t D, uint32_t Dp,
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
    const uint32_t lo = pres && k < D ? bf16_bits(s[k]) : 0u, hi = pres && k + 1 < D ? bf16_bits(s[k + 1]) : 0u;
    d[k >> 1] = lo | (hi << 16);
    const float x = __uint_as_float(lo << 16), y = __uint_as_float(hi << 16);
    acc += x * x + y * y;
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) norms[drow] = acc;
}

}  // namespace

hipError_t sa_launch_pad_features_bf16(const float* src, uint32_t rows, uint32_t D, uint32_t Dp, uint32_t K, const uint32_t* slots,
                                       const uint8_t* present, uint16_t* dst, float* norms, hipStream_t st) {
  if (!rows) return hipSuccess;
  hipLaunchKernelGGL(k_pad_features_bf16, dim3((rows + PAD_ROWS - 1) / PAD_ROWS), dim3(PAD_THREADS), 0, st, src, rows, D, Dp, K, slots,
                     present, dst, norms);
  return hipGetLastError();
}

extern "C" {

int sa_store_create_elem(sa_engine* e, const sa_store_options* o, int32_t elem, sa_store** out) {
  const char* what = "sa_store_create_elem";
  if (out) *out = nullptr;
  if (elem == SA_ELEM_F32) return sa_store_create(e, o, out);
  // without an engine the answer is about the device, as sa_store_create gives it, whatever else is wrong with the call
  if (e && elem != SA_ELEM_BF16 && elem != SA_ELEM_F16)
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: unknown element type %d (SA_ELEM_F32, SA_ELEM_BF16, SA_ELEM_F16)", what, elem);
  if (e && elem == SA_ELEM_BF16 && o && o->struct_size >= sizeof(sa_store_options) && o->visual_kind == SA_VIS_EUCLIDEAN)
    return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: a bf16 store is cosine only (the euclidean distance is the direct sum on f32 rows)", what);
  return sa_store_create_as(e, o, elem, what, out);
}

int sa_store_get_info(sa_store* s, sa_store_info* out) {
  if (!s || !out) return SA_ERR_BAD_ARG;
  if (!s->e || s->broken) return sa_store_enter(s, "sa_store_get_info");
  out->struct_size = sizeof *out;
  out->elem = s->elem;
  out->Dp = s->Dp;
  out->Kp = s->Kp;
  out->feature_bytes = (uint64_t)s->cap * s->Kp * s->row_bytes();
  return SA_OK;
}

}  // extern "C"
