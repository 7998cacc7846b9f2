// sa_framerows.hip — a frame's feature rows read from device memory (include/similari_framerows.h): the host checks of a descriptor,
// the per-detection row table, and k_widen_rows, the ONE launch per uploaded request set that gathers and widens every such scene's
// rows — f32, f16 or bf16, any stride, any row order — into the slot's own [N][D] f32 buffer (Slot::feat_raw, sa_engine.hip), the seam
// behind which the contraction, the positional tiles, the tail and the upkeep read p_feat_raw and know nothing of the source.
#include "sa_framerows.h"
#include "sa_widen.h"

namespace {

constexpr uint32_t WIDEN_THREADS = 256, WIDEN_ROWS = WIDEN_THREADS / 64;

// One row: a wave.  s: the source row (null for an absent one: zeros, nothing is read), d: its D floats.
// wide (wave-uniform; sa_widen_row_is_wide: the row's address a multiple of 16 and D % 4 == 0, which makes d a multiple of 16 too):
// one 16-byte load per lane and step — 4 f32 elements, or 8 of a 16-bit source; the last step of a 16-bit row with D % 8 == 4 is one
// 8-byte load.  Consecutive lanes read consecutive 16 bytes: a wave-load is 1 KB of one row.  Any other row goes element by element
// (lane l: elements l, l + 64, ...; consecutive lanes, consecutive elements).  No load reaches past element D - 1 of a row, and either
// way d[k] = widen(s[k]): the choice changes no bit.
template <int SRC>
__device__ __forceinline__ void widen_row(const char SA_G* s, bool wide, float SA_G* d, uint32_t D, uint32_t lane) {
  if (wide && SRC == SA_ELEM_F32) {
    for (uint32_t k = 4 * lane; k < D; k += 256u) *(float4 SA_G*)(d + k) = *(const float4 SA_G*)(s + (size_t)k * 4);
  } else if (wide) {
    for (uint32_t k = 8 * lane; k + 8 <= D; k += 512u) {
      const uint4 w = *(const uint4 SA_G*)(s + (size_t)k * 2);
      *(float4 SA_G*)(d + k) = float4{widen16<SRC>(w.x & 0xffffu), widen16<SRC>(w.x >> 16), widen16<SRC>(w.y & 0xffffu), widen16<SRC>(w.y >> 16)};
      *(float4 SA_G*)(d + k + 4) = float4{widen16<SRC>(w.z & 0xffffu), widen16<SRC>(w.z >> 16), widen16<SRC>(w.w & 0xffffu), widen16<SRC>(w.w >> 16)};
    }
    // D % 8 == 4: the row's last four elements, by the lane whose turn they would have been (kept out of the loop: merged into it, the
    // compiler splits the loop's 16-byte load into the part both forms share and the rest)
    const uint32_t k = D - 4u;
    if ((D & 4u) && lane == ((k >> 3) & 63u)) {
      const uint2 w = *(const uint2 SA_G*)(s + (size_t)k * 2);
      *(float4 SA_G*)(d + k) = float4{widen16<SRC>(w.x & 0xffffu), widen16<SRC>(w.x >> 16), widen16<SRC>(w.y & 0xffffu), widen16<SRC>(w.y >> 16)};
    }
  } else {
    for (uint32_t k = lane; k < D; k += 64u) d[k] = s ? load_elem<SRC>((const char*)s, k) : 0.0f;
  }
}

// grid.y = scene (SaWidenSlot), four rows per workgroup, one wave each.  SRC: the element type of every scene of the launch, or -1:
// they differ, and each wave takes its scene's (wave-uniform).
template <int SRC>
__global__ __launch_bounds__(WIDEN_THREADS) void k_widen_rows(const SaWidenSlot* __restrict__ slots, uint32_t D) {
  const SaWidenSlot sl = slots[blockIdx.y];
  const uint32_t row = blockIdx.x * WIDEN_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= sl.n) return;
  const uint32_t t = ((const uint32_t SA_G*)sl.table)[row];
  const int elem = SRC >= 0 ? SRC : sl.elem;
  const char SA_G* s = t != SA_ROW_NONE ? (const char SA_G*)sl.base + (uint64_t)t * sl.row_stride * (elem == SA_ELEM_F32 ? 4u : 2u) : nullptr;
  const bool wide = s && sa_widen_row_is_wide((uint64_t)(uintptr_t)s, D);
  float SA_G* d = (float SA_G*)sl.dst + (size_t)row * D;
  if (elem == SA_ELEM_F32) widen_row<SA_ELEM_F32>(s, wide, d, D, lane);
  else if (elem == SA_ELEM_F16) widen_row<SA_ELEM_F16>(s, wide, d, D, lane);
  else widen_row<SA_ELEM_BF16>(s, wide, d, D, lane);
}

inline bool has_feature(const sa_detections* d, const sa_dev_rows* r, uint32_t i) {
  return (!d->feat_present || d->feat_present[i]) && (!r->index || r->index[i] != SA_ROW_NONE);
}

}  // namespace

hipError_t sa_launch_widen_rows(const SaWidenSlot* slots, uint32_t n_slots, uint32_t max_n, uint32_t D, int elem, hipStream_t st,
                                hipEvent_t start, hipEvent_t done) {
  if (!n_slots || !max_n || !D) return hipSuccess;
  const dim3 grid((max_n + WIDEN_ROWS - 1) / WIDEN_ROWS, n_slots), block(WIDEN_THREADS);
  auto kern = elem == SA_ELEM_F32 ? k_widen_rows<SA_ELEM_F32> : elem == SA_ELEM_F16 ? k_widen_rows<SA_ELEM_F16>
            : elem == SA_ELEM_BF16 ? k_widen_rows<SA_ELEM_BF16> : k_widen_rows<-1>;
  if (start || done) hipExtLaunchKernelGGL(kern, grid, block, 0, st, start, done, 0, slots, D);
  else hipLaunchKernelGGL(kern, grid, block, 0, st, slots, D);
  return hipGetLastError();
}

int sa_framerows_check(sa_engine* e, const char* what, int device, uint32_t D, bool visual, const sa_detections* d, const sa_dev_rows* r,
                       SaFrameRows* out) {
  *out = SaFrameRows{};
  if (!r) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null rows", what);
  if (!visual) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: feature rows for an engine without a visual metric", what);
  if (d->feats) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: detections.feats together with rows (one source of features per scene)", what);
  if (r->struct_size != sizeof(sa_dev_rows))
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: rows.struct_size is %u, sizeof(sa_dev_rows) is %zu", what, r->struct_size, sizeof(sa_dev_rows));
  SA_TRY(sa_dev_rows_layout(e, what, r, D, "feature length"));
  if (!r->n_rows || r->n_rows >= 0xffffffffull)
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: rows.n_rows is %llu (1 .. 2^32 - 2)", what, (unsigned long long)r->n_rows);
  SA_TRY(sa_dev_rows_span(e, what, r, D, device, "this engine runs on"));
  bool all = true;
  for (uint32_t i = 0; i < d->n; ++i) {
    if (!has_feature(d, r, i)) { all = false; out->index_absent = out->index_absent || (r->index && r->index[i] == SA_ROW_NONE); continue; }
    const uint64_t row = r->index ? r->index[i] : i;
    if (row >= r->n_rows) {
      if (r->index) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: rows.index[%u] = %llu is not below n_rows %llu", what, i, (unsigned long long)row, (unsigned long long)r->n_rows);
      return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: detection %u has a feature but rows.n_rows is %llu (and no index)", what, i, (unsigned long long)r->n_rows);
    }
    ++out->present;
  }
  out->in_place = d->n && all && r->elem == SA_ELEM_F32 && r->row_stride == D && !r->index && !((uintptr_t)r->base & 15u);
  return SA_OK;
}

void sa_framerows_table(const sa_detections* d, const sa_dev_rows* r, uint32_t* table, uint8_t* present) {
  for (uint32_t i = 0; i < d->n; ++i) {
    const bool has = has_feature(d, r, i);
    table[i] = has ? (r->index ? r->index[i] : i) : SA_ROW_NONE;
    if (present) present[i] = has ? 1 : 0;
  }
}
