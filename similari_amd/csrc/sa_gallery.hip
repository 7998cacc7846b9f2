// sa_gallery.hip — searches whose queries are stored tracks (include/similari_gallery.h): the gather launch that fills the query
// side of a search from the store's own slots (k_gather), and the entry points.  The
// prologue, the launches of a search, the pool's growth and the copies out are sa_search.hip's (sa_store_search_begin,
// sa_store_search_run); the join's first launch is in sa_gemm.hip (k_search_tile<.., JOIN = true, ..>), its second is k_topn<true>.
//
// Reference: TrackStore::owned_track_distances (src/track/store.rs:471-486), examples/track_merging.rs.
#include "sa_store.h"
#include "../../include/similari_gallery.h"

#include <type_traits>
#include <vector>

namespace {

constexpr uint32_t GATHER_THREADS = 256, GATHER_ROWS = GATHER_THREADS / 64;

// One wave per query observation slot, four slots per workgroup: the padded row (16-byte copies, a wave moves 1 KB a step) and its
// norm move from the stored track's slot to the query's; the first slot of a track also carries its observation count and id, and
// marks the track withdrawn when the call asks for that.  A query the store does not hold (SA_SEARCH_NONE) is a track without
// observations: zero rows, id 0 — no stored track has it.
// ATTRS (k_gather with both attribute tables, the *_compat call): the same lane carries the track's attributes along ({0, 0, 0} for a query the
// store does not hold), so a search under a rule needs no launch of its own for them.
template <bool ATTRS>
__device__ __forceinline__ void gather_body(const uint32_t* __restrict__ slots, const float* __restrict__ s_feat,
                                            const float* __restrict__ s_norm, const uint32_t* __restrict__ s_nobs,
                                            const uint64_t* __restrict__ s_ids, uint32_t T, uint32_t rows, uint32_t Dp, uint32_t lgK,
                                            float* __restrict__ q_feat, float* __restrict__ q_norm, uint32_t* __restrict__ q_nobs,
                                            uint64_t* __restrict__ q_ids, uint8_t* __restrict__ s_out,
                                            const sa_track_attrs* __restrict__ s_attrs = nullptr,
                                            sa_track_attrs* __restrict__ q_attrs = nullptr) {
  const uint32_t row = blockIdx.x * GATHER_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= rows) return;
  const uint32_t q = row >> lgK, k = row & ((1u << lgK) - 1u);
  const uint32_t slot = slots[q];
  const bool held = slot < T;
  float4* dst = (float4*)(q_feat + (size_t)row * Dp);
  const float4* src = (const float4*)(s_feat + (((size_t)(held ? slot : 0u) << lgK) + k) * Dp);
  for (uint32_t i = lane; i < Dp / 4; i += 64u) dst[i] = held ? src[i] : float4{0.f, 0.f, 0.f, 0.f};
  if (lane != 0) return;
  q_norm[row] = held ? s_norm[((size_t)slot << lgK) + k] : 0.f;
  if (k != 0) return;
  q_nobs[q] = held ? s_nobs[slot] : 0u;
  q_ids[q] = held ? s_ids[slot] : 0ull;
  if (ATTRS) q_attrs[q] = held ? s_attrs[slot] : sa_track_attrs{0, 0, 0};
  if (held && s_out) s_out[slot] = 1;
}

// attrs: nothing, or the store's attribute table and the queries' (ATTRS)
template <class... Attrs>
__global__ __launch_bounds__(GATHER_THREADS) void k_gather(const uint32_t* __restrict__ slots, const float* __restrict__ s_feat,
                                                           const float* __restrict__ s_norm, const uint32_t* __restrict__ s_nobs,
                                                           const uint64_t* __restrict__ s_ids, uint32_t T, uint32_t rows, uint32_t Dp,
                                                           uint32_t lgK, float* __restrict__ q_feat, float* __restrict__ q_norm,
                                                           uint32_t* __restrict__ q_nobs, uint64_t* __restrict__ q_ids,
                                                           uint8_t* __restrict__ s_out, Attrs* __restrict__... attrs) {
  static_assert(sizeof...(Attrs) == 0 || sizeof...(Attrs) == 2, "no attributes, or s_attrs and q_attrs");
  gather_body<sizeof...(Attrs) != 0>(slots, s_feat, s_norm, s_nobs, s_ids, T, rows, Dp, lgK, q_feat, q_norm, q_nobs, q_ids, s_out, attrs...);
}

}  // namespace

int sa_store_search_stored_impl(sa_store* s, const char* what, const sa_topn_params* p, bool ruled, const sa_compat* compat, uint32_t flags,
                                uint32_t n, const uint64_t* ids, uint32_t* out_n, uint64_t* out_winner, double* out_weight, float* out_cells,
                                const SaBestFit* fit) {
  SaSearchCall c;
  c.what = what, c.p = p, c.ruled = ruled, c.compat = compat, c.Q = n, c.fit = fit;
  c.bad_flags = flags & ~SA_STORED_WITHDRAW;
  c.null_arg = !ids;
  c.out_n = out_n, c.out_winner = out_winner, c.out_weight = out_weight;
  std::vector<uint32_t> slots;
  bool run;
  SA_TRY(sa_store_search_begin(s, c, [&] {
    slots.resize(n);
    return sa_store_check_ids(s, what, n, ids, slots.data());
  }, &run));
  if (!run) return SA_OK;
  sa_engine* e = s->e;
  const uint32_t T = s->T, Kp = s->Kp, topn = p->topn;
  const bool withdraw = (flags & SA_STORED_WITHDRAW) != 0;
  const size_t rows = (size_t)n * Kp;
  SA_TRY(sa_engine_ensure(e, s->g_slots, (size_t)n * 4));
  SA_TRY(sa_engine_ensure(e, s->q_feat, rows * s->row_bytes()));
  SA_TRY(sa_engine_ensure(e, s->q_norm, rows * 4));
  SA_TRY(sa_engine_ensure(e, s->q_ids, (size_t)n * 8));
  SA_TRY(sa_engine_ensure(e, s->q_nobs, (size_t)n * 4));
  if (withdraw) SA_TRY(sa_engine_ensure(e, s->s_out, T));
  SA_TRY(sa_store_search_buffers(s, n, topn, out_cells != nullptr, false, fit));
  hipStream_t st = s->st;
  SA_HIPCHK(e, hipEventRecord(s->ev[0], st));
  SA_HIPCHK(e, hipMemcpyAsync(s->g_slots.p, slots.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  if (withdraw) SA_HIPCHK(e, hipMemsetAsync(s->s_out.p, 0, T, st));
  const dim3 grid((uint32_t)((rows + GATHER_ROWS - 1) / GATHER_ROWS));
  uint8_t* mark = withdraw ? (uint8_t*)s->s_out.p : nullptr;
  auto gather = [&](auto*... attrs) {
    hipLaunchKernelGGL(k_gather<std::remove_pointer_t<decltype(attrs)>...>, grid, dim3(GATHER_THREADS), 0, st, (const uint32_t*)s->g_slots.p,
                       (const float*)s->feat.p, (const float*)s->norm.p, (const uint32_t*)s->d_nobs.p, (const uint64_t*)s->d_ids.p, T,
                       (uint32_t)rows, s->row_floats(), s->lgK, (float*)s->q_feat.p, (float*)s->q_norm.p, (uint32_t*)s->q_nobs.p,
                       (uint64_t*)s->q_ids.p, mark, attrs...);
  };
  if (compat) {   // the queries' attributes ride in the same launch
    SA_TRY(sa_engine_ensure(e, s->q_attrs, (size_t)n * sizeof(sa_track_attrs)));
    SA_TRY(sa_store_compat_begin(s));
    gather((const sa_track_attrs*)s->d_attrs.p, (sa_track_attrs*)s->q_attrs.p);
  } else {
    gather();
  }
  SA_HIPCHK(e, hipGetLastError());
  return sa_store_search_run(s, p, what, n, false, withdraw ? (const uint8_t*)s->s_out.p : nullptr, out_n, out_winner, out_weight, out_cells,
                             compat, fit);
}

int sa_store_join_topn_impl(sa_store* s, const char* what, const sa_topn_params* p, bool ruled, const sa_compat* compat, uint32_t* out_n,
                            uint64_t* out_winner, double* out_weight, float* out_cells, const SaBestFit* fit) {
  SaSearchCall c;
  c.what = what, c.p = p, c.ruled = ruled, c.compat = compat, c.join = true, c.fit = fit;
  c.out_n = out_n, c.out_winner = out_winner, c.out_weight = out_weight;
  bool run;
  // a consolidation (sa_consolidate.hip): its own refusals behind the join's, its buffers before anything is launched
  const SaAbsorbStep* step = fit ? fit->step : nullptr;
  SA_TRY(sa_store_search_begin(s, c, step ? step->check : std::function<int()>(), &run));
  if (!run) return SA_OK;
  if (step) SA_TRY(step->prepare());
  sa_engine* e = s->e;
  const uint32_t T = s->T;
  SA_TRY(sa_store_search_buffers(s, T, p->topn, out_cells != nullptr, true, fit));
  SA_HIPCHK(e, hipEventRecord(s->ev[0], s->st));
  if (compat) SA_TRY(sa_store_compat_begin(s));
  return sa_store_search_run(s, p, what, T, true, nullptr, out_n, out_winner, out_weight, out_cells, compat, fit);
}

extern "C" {

int sa_store_search_stored(sa_store* s, const sa_topn_params* p, uint32_t flags, uint32_t n, const uint64_t* ids, uint32_t* out_n,
                           uint64_t* out_winner, double* out_weight, float* out_cells) {
  return sa_store_search_stored_impl(s, "sa_store_search_stored", p, false, nullptr, flags, n, ids, out_n, out_winner, out_weight, out_cells);
}

int sa_store_search_stored_compat(sa_store* s, const sa_topn_params* p, const sa_compat* c, uint32_t flags, uint32_t n, const uint64_t* ids,
                                  uint32_t* out_n, uint64_t* out_winner, double* out_weight, float* out_cells) {
  return sa_store_search_stored_impl(s, "sa_store_search_stored_compat", p, true, c, flags, n, ids, out_n, out_winner, out_weight, out_cells);
}

int sa_store_join_topn(sa_store* s, const sa_topn_params* p, uint32_t* out_n, uint64_t* out_winner, double* out_weight, float* out_cells) {
  return sa_store_join_topn_impl(s, "sa_store_join_topn", p, false, nullptr, out_n, out_winner, out_weight, out_cells);
}

int sa_store_join_topn_compat(sa_store* s, const sa_topn_params* p, const sa_compat* c, uint32_t* out_n, uint64_t* out_winner,
                              double* out_weight, float* out_cells) {
  return sa_store_join_topn_impl(s, "sa_store_join_topn_compat", p, true, c, out_n, out_winner, out_weight, out_cells);
}

int sa_store_join_last(sa_store* s, sa_join_stats* out) {
  if (!s || !out) return SA_ERR_BAD_ARG;
  out->tiles = s->join_tiles;
  out->tiles_rect = s->join_tiles_rect;
  out->blocks = s->join_blocks;
  out->reserved = 0;
  return SA_OK;
}

}  // extern "C"
