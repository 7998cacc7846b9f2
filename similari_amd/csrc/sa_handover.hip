// sa_handover.hip — ready tracks handed from one feature store to another (include/similari_handover.h): sa_store_ready (the host's
// filter over the attribute table), sa_store_take (fetch, then the removal), sa_store_hand_over (the taken tracks become the queries
// of one absorb on the other store without their rows leaving the device) and the one-launch removal every call that takes tracks
// out of a store shares, sa_store_remove (sa_search.hip) included.
//
// The hand-over is sa_store_absorb_impl (sa_absorb.hip) handed a third row source, "rows of another store" (SaRowSource::of_store):
// the queries' counts, attributes and qualities come from src's host tables, which are authoritative, and the query side of dst's
// search is filled by the one launch of sa_rows_fill (sa_devrows.hip) over src's banks:
//   k_handover_rows  stores of one element type (Dp is equal then): the padded row and its norm word are copied — the bits the
//                    host route leaves, because re-rounding a rounded row is the identity and the norm of a row does not depend
//                    on which call wrote it;
//   k_pad_rows       (sa_devrows.hip) stores of two types: widen, round to dst's type and sum the norm in dst's order, which is
//                    what the host route does with fetch's widened rows — it runs the same kernel.
// Everything behind the fill — the tiles, the vote, the absorb's step, the host's replay — does not know where the rows came from.
//
// Reference: examples/track_merging.rs:371-481, TrackStore::find_usable, TrackStore::fetch_tracks.
#include "sa_merge_plan.h"
#include "sa_store.h"

#include <unordered_set>
#include <vector>

namespace {

constexpr uint32_t HO_THREADS = 256, HO_ROWS = HO_THREADS / 64;

// One wave per destination row, four rows per workgroup, the grid flat over n * Kp rows of the destination's query side.  A row is
// `pieces` 16-byte pieces in both stores (a padded row is a multiple of 64 bytes and every bank starts on an allocation's boundary, so
// each piece is aligned).  table[row]: the source's observation slot; SA_SEARCH_NONE: an absent row — zeros, norm 0, the source is
// not touched.  The norm travels as the 32-bit word it is, written from lane 0 of the wave.
__global__ __launch_bounds__(HO_THREADS) void k_handover_rows(const uint4* __restrict__ s_feat, const uint32_t* __restrict__ s_norm,
                                                              const uint32_t* __restrict__ table, uint32_t rows, uint32_t pieces,
                                                              uint4* __restrict__ q_feat, uint32_t* __restrict__ q_norm) {
  const uint32_t row = blockIdx.x * HO_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= rows) return;
  const uint32_t t = table[row];
  uint4* to = q_feat + (size_t)row * pieces;
  if (t == SA_SEARCH_NONE) {
    for (uint32_t i = lane; i < pieces; i += 64u) to[i] = uint4{0u, 0u, 0u, 0u};
    if (lane == 0) q_norm[row] = 0u;
    return;
  }
  const uint4* from = s_feat + (size_t)t * pieces;
  for (uint32_t i = lane; i < pieces; i += 64u) to[i] = from[i];
  if (lane == 0) q_norm[row] = s_norm[t];
}

int events(sa_store* s, uint32_t first) {
  for (uint32_t i = first; i < first + 2; ++i)
    if (!s->hev[i]) SA_HIPCHK(s->e, hipEventCreate(&s->hev[i]));
  return SA_OK;
}

}  // namespace

int sa_handover_fill_begin(sa_store* s, const std::vector<uint32_t>& table) {
  for (const uint32_t t : table) s->handover_last.rows += t != SA_SEARCH_NONE ? 1u : 0u;
  SA_TRY(events(s, 0));
  SA_HIPCHK(s->e, hipEventRecord(s->hev[0], s->st));
  return SA_OK;
}

int sa_handover_copy(sa_store* s, const sa_store* from, const uint32_t* d_table, uint32_t rows, void* dst, float* norms) {
  hipLaunchKernelGGL(k_handover_rows, dim3((rows + HO_ROWS - 1) / HO_ROWS), dim3(HO_THREADS), 0, s->st, (const uint4*)from->feat.p,
                     (const uint32_t*)from->norm.p, d_table, rows, (uint32_t)(s->row_bytes() / 16), (uint4*)dst, (uint32_t*)norms);
  SA_HIPCHK(s->e, hipGetLastError());
  return SA_OK;
}

int sa_store_remove_slots(sa_store* s, const std::vector<uint32_t>& slots, bool timed, uint32_t* launches, uint32_t* moved, double* ms) {
  if (slots.empty()) return SA_OK;
  sa_engine* e = s->e;
  std::vector<uint32_t> perm;
  std::vector<SaMergeMove> moves;
  sa_merge_compaction(s->T, slots, perm, moves);
  // whatever can fail without the device comes first: a refusal here leaves the store as it was
  if (!moves.empty()) SA_TRY(sa_engine_ensure(e, s->m_moves, moves.size() * sizeof(SaMergeMove)));
  if (timed) SA_TRY(events(s, 2));
  for (const uint32_t slot : slots) s->slot_of.erase(s->ids[slot]);
  for (const SaMergeMove& m : moves) s->slot_move(m.from, m.to);
  s->slot_truncate((uint32_t)perm.size());
  const int rc = [&]() -> int {
    if (timed) SA_HIPCHK(e, hipEventRecord(s->hev[2], s->st));
    SA_TRY(sa_store_launch_compact(s, moves.data(), moves.size()));
    if (timed) SA_HIPCHK(e, hipEventRecord(s->hev[3], s->st));
    SA_TRY(sa_store_upload_table(s));
    SA_HIPCHK(e, hipStreamSynchronize(s->st));
    if (timed && ms) {
      float t = 0.f;
      SA_HIPCHK(e, hipEventElapsedTime(&t, s->hev[2], s->hev[3]));
      *ms = t;
    }
    return SA_OK;
  }();
  if (rc != SA_OK) {   // the tables have moved and the banks may not have
    s->broken = true;
    return rc;
  }
  if (launches) *launches = moves.empty() ? 0u : 1u;
  if (moved) *moved = (uint32_t)moves.size();
  return SA_OK;
}

extern "C" {

int sa_store_ready(sa_store* s, int64_t ready_at, uint64_t* out_ids, uint32_t cap, uint32_t* out_n) {
  if (!s || !out_n) return SA_ERR_BAD_ARG;
  if (!s->e || s->broken) return sa_store_enter(s, "sa_store_ready");
  uint32_t n = 0;
  for (uint32_t slot = 0; slot < s->T; ++slot)
    if (s->attrs[slot].end <= ready_at) {
      if (out_ids && n < cap) out_ids[n] = s->ids[slot];
      ++n;
    }
  *out_n = n;
  return SA_OK;
}

int sa_store_take(sa_store* s, uint32_t n, const uint64_t* ids, uint32_t* out_n_obs, float* out_feats, float* out_quality,
                  sa_track_attrs* out_attrs) {
  const char* what = "sa_store_take";
  if (!s) return SA_ERR_BAD_ARG;
  SA_TRY(sa_store_enter(s, what));
  if (n == 0) return SA_OK;
  if (!ids || !out_n_obs || !out_feats) return sa_engine_fail(s->e, SA_ERR_BAD_ARG, "%s: null argument", what);
  SA_TRY(sa_store_fetch(s, n, ids, out_n_obs, out_feats, out_quality));
  std::vector<uint32_t> slots;
  std::unordered_set<uint32_t> seen;   // an id's second coming is fetched again and leaves once
  for (uint32_t i = 0; i < n; ++i) {
    const auto it = s->slot_of.find(ids[i]);
    const bool known = it != s->slot_of.end();
    if (out_attrs) out_attrs[i] = known ? s->attrs[it->second] : sa_track_attrs{0, 0, 0};
    if (known && seen.insert(it->second).second) slots.push_back(it->second);
  }
  s->handover_last = sa_handover_stats{};
  return sa_store_remove_slots(s, slots, true, &s->handover_last.launches_compact, &s->handover_last.tracks_moved,
                               &s->handover_last.compact_ms);
}

int sa_store_hand_over(sa_store* src, sa_store* dst, uint32_t keep, const sa_topn_params* p, const sa_compat* c, uint32_t n,
                       const uint64_t* ids, const uint32_t* capacity, uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track,
                       double* out_weight, uint64_t* out_dest) {
  const char* what = "sa_store_hand_over";
  if (!src || !dst) return SA_ERR_BAD_ARG;
  dst->handover_last = sa_handover_stats{};
  dst->absorb_last = sa_absorb_stats{};   // as a refused absorb leaves them
  dst->retain_keep = 0;
  dst->retain_upload = 0;
  SA_TRY(sa_store_enter(dst, what));
  sa_engine* e = dst->e;
  if (src == dst) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: src and dst are one store", what);
  SA_TRY(sa_store_enter(src, what));
  if (src->e != dst->e) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: the stores belong to two engines", what);
  if (src->D != dst->D) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: feature_len %u of src, %u of dst", what, src->D, dst->D);
  if (src->elem == SA_ELEM_I8 && dst->elem != SA_ELEM_I8)
    return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: an i8 source into a store of another element type (codes are directions, not values)", what);
  if (n && !ids) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
  // the queries as src's host tables hold them: counts, attributes, qualities in call order, and the row table of the fill
  std::vector<uint32_t> slots(n), nobs(n), table((size_t)n * dst->Kp, SA_SEARCH_NONE);
  std::vector<sa_track_attrs> attrs(n);
  std::vector<float> quality;
  SA_TRY(sa_store_check_ids(src, what, n, ids, slots.data(), [&](uint32_t i) {
    if (slots[i] == SA_SEARCH_NONE) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: src does not hold id %llu", what, (unsigned long long)ids[i]);
    const uint32_t m = src->nobs[slots[i]];
    if (m > dst->K)
      return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: %u observations for id %llu (max_observations %u of dst)", what, m,
                            (unsigned long long)ids[i], dst->K);
    return (int)SA_OK;
  }));
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t slot = slots[i];
    nobs[i] = src->nobs[slot];
    attrs[i] = src->attrs[slot];
    for (uint32_t k = 0; k < nobs[i]; ++k) {
      table[(size_t)i * dst->Kp + k] = (slot << src->lgK) + k;
      quality.push_back(src->qual[(size_t)slot * src->Kp + k]);
    }
  }
  if (quality.empty()) quality.push_back(0.f);   // (a pointer for the absorb, which reads sum nobs entries)
  const int rc = sa_store_absorb_impl(dst, what, keep, p, c, n, ids, nobs.data(), SaRowSource::of_store(src, &table), c ? attrs.data() : nullptr,
                                      quality.data(), capacity, out_n, out_winner, out_track, out_weight, out_dest);
  if (rc != SA_OK) {
    dst->handover_last = sa_handover_stats{};
    return rc;
  }
  if (n == 0) return SA_OK;
  sa_handover_stats& st = dst->handover_last;
  if (st.launches_fill) {
    float t = 0.f;
    SA_HIPCHK(e, hipEventElapsedTime(&t, dst->hev[0], dst->hev[1]));
    st.fill_ms = t;
  }
  return sa_store_remove_slots(src, slots, true, &st.launches_compact, &st.tracks_moved, &st.compact_ms);
}

int sa_store_handover_last(sa_store* dst, sa_handover_stats* out) {
  if (!dst || !out) return SA_ERR_BAD_ARG;
  *out = dst->handover_last;
  out->struct_size = sizeof *out;
  return SA_OK;
}

}  // extern "C"
