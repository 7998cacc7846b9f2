// sa_merge.hip — bank upkeep on the device (include/similari_merge.h): append, merge, fetch.  The decision which observation lands
// in which slot is the host's (sa_merge_plan.h: ids, counts and qualities suffice); this file moves the rows.  Padded rows travel
// with their norms and are never recomputed, so a search after a merge reads the bits a freshly upserted store holds.
//
// Launches of a call, whatever the number of tracks: [append: the new rows are padded into staging, sa_rows_fill]
// k_merge_gather (every row that changes -> a staging row), k_merge_scatter (staging -> its slot; two launches because a bank may
// permute in place), [merge: k_merge_compact, every net move of the removal at once].
//
// Reference: Track::add_observation (src/track.rs:447-503), Track::merge (src/track.rs:522-588), TrackStore::fetch_tracks.
#include "sa_compat.h"
#include "sa_merge_plan.h"
#include "sa_store.h"

#include <cmath>
#include <cstring>
#include <unordered_set>

namespace {

constexpr uint32_t MERGE_THREADS = 256, MERGE_ROWS = MERGE_THREADS / 64;

// One wave per row, four rows per workgroup, 16-byte copies (Dp is a multiple of 32 floats), as k_gather.
// Gather: staging row j takes the row plan[j].src names — a stored slot, a staged new row, or zeros.
__global__ __launch_bounds__(MERGE_THREADS) void k_merge_gather(const SaMergeRow* __restrict__ plan, uint32_t rows, uint32_t Dp,
                                                                const float* __restrict__ s_feat, const float* __restrict__ s_norm,
                                                                const float* __restrict__ n_feat, const float* __restrict__ n_norm,
                                                                float* __restrict__ m_feat, float* __restrict__ m_norm) {
  const uint32_t row = blockIdx.x * MERGE_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= rows) return;
  const uint32_t src = plan[row].src;
  const bool zero = src == SA_MERGE_ZERO, staged = !zero && (src & SA_MERGE_STAGED);
  const size_t r = zero ? 0 : (src & ~SA_MERGE_STAGED);
  const float4* from = (const float4*)((staged ? n_feat : s_feat) + r * Dp);
  float4* to = (float4*)(m_feat + (size_t)row * Dp);
  for (uint32_t i = lane; i < Dp / 4; i += 64u) to[i] = zero ? float4{0.f, 0.f, 0.f, 0.f} : from[i];
  if (lane == 0) m_norm[row] = zero ? 0.f : (staged ? n_norm : s_norm)[r];
}

// Scatter: staging row j lands in stored slot plan[j].dst.  No two rows of a plan share a slot.
__global__ __launch_bounds__(MERGE_THREADS) void k_merge_scatter(const SaMergeRow* __restrict__ plan, uint32_t rows, uint32_t Dp,
                                                                 const float* __restrict__ m_feat, const float* __restrict__ m_norm,
                                                                 float* __restrict__ s_feat, float* __restrict__ s_norm) {
  const uint32_t row = blockIdx.x * MERGE_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= rows) return;
  const size_t dst = plan[row].dst;
  const float4* from = (const float4*)(m_feat + (size_t)row * Dp);
  float4* to = (float4*)(s_feat + dst * Dp);
  for (uint32_t i = lane; i < Dp / 4; i += 64u) to[i] = from[i];
  if (lane == 0) s_norm[dst] = m_norm[row];
}

// Compaction: row r of move r >> lgK.  Sources lie at or beyond the final track count and targets below it (sa_merge_plan.h), so no
// move reads what another writes and no __restrict__ promise is broken by feat appearing on both sides.
__global__ __launch_bounds__(MERGE_THREADS) void k_merge_compact(const SaMergeMove* __restrict__ moves, uint32_t rows, uint32_t Dp,
                                                                 uint32_t lgK, float* s_feat, float* s_norm) {
  const uint32_t row = blockIdx.x * MERGE_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= rows) return;
  const SaMergeMove m = moves[row >> lgK];
  const uint32_t k = row & ((1u << lgK) - 1u);
  const size_t a = ((size_t)m.from << lgK) + k, b = ((size_t)m.to << lgK) + k;
  const float4* from = (const float4*)(s_feat + a * Dp);
  float4* to = (float4*)(s_feat + b * Dp);
  for (uint32_t i = lane; i < Dp / 4; i += 64u) to[i] = from[i];
  if (lane == 0) s_norm[b] = s_norm[a];
}

uint32_t row_blocks(size_t rows) { return (uint32_t)((rows + MERGE_ROWS - 1) / MERGE_ROWS); }

int check_rule(sa_store* s, uint32_t keep, uint32_t n, const uint32_t* capacity, const char* what) {
  if (keep != SA_KEEP_LATEST && keep != SA_KEEP_BEST) return sa_engine_fail(s->e, SA_ERR_BAD_ARG, "%s: unknown keep %u", what, keep);
  if (capacity)
    for (uint32_t i = 0; i < n; ++i)
      if (capacity[i] < 1 || capacity[i] > s->K)
        return sa_engine_fail(s->e, SA_ERR_BAD_ARG, "%s: capacity %u at %u (1..%u)", what, capacity[i], i, s->K);
  return SA_OK;
}

// The device part of an append or a merge, after the host tables took the result (a failure here leaves the store broken): staged new
// rows (n_new of them, one per observation, read from src where they lie: sa_rows_fill) are padded, the plan's rows gathered and
// scattered, the moves run, the tables uploaded.
int run_plan(sa_store* s, const std::vector<SaMergeRow>& rows, const std::vector<SaMergeMove>& moves, uint32_t n_new, const SaRowSource& src) {
  sa_engine* e = s->e;
  hipStream_t st = s->st;
  const uint32_t Dp = s->row_floats();   // a row as the movers count it (sa_store.h)
  const size_t row_bytes = s->row_bytes() + 4;
  sa_merge_stats& ms = s->merge_last;
  ms = sa_merge_stats{};
  SaRows R;
  SA_TRY(sa_rows_prepare(s, src, 0, nullptr, n_new, false, R));
  if (n_new) {
    SA_TRY(sa_engine_ensure(e, s->m_new_feat, (size_t)n_new * s->row_bytes()));
    SA_TRY(sa_engine_ensure(e, s->m_new_norm, (size_t)n_new * 4));
  }
  if (!rows.empty()) {
    SA_TRY(sa_engine_ensure(e, s->m_rows, rows.size() * sizeof(SaMergeRow)));
    SA_TRY(sa_engine_ensure(e, s->m_feat, rows.size() * s->row_bytes()));
    SA_TRY(sa_engine_ensure(e, s->m_norm, rows.size() * 4));
  }
  SA_HIPCHK(e, hipEventRecord(s->ev[0], st));
  if (n_new) {
    SA_TRY(sa_rows_fill(s, R, 1, nullptr, s->m_new_feat.p, (float*)s->m_new_norm.p));
    ++ms.launches;
    ms.bytes_moved += (uint64_t)n_new * ((size_t)s->D * (R.elem == SA_ELEM_F32 ? 4 : 2) + row_bytes);
  }
  if (!rows.empty()) {
    const uint32_t n = (uint32_t)rows.size();
    SA_HIPCHK(e, hipMemcpyAsync(s->m_rows.p, rows.data(), rows.size() * sizeof(SaMergeRow), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_merge_gather, dim3(row_blocks(n)), dim3(MERGE_THREADS), 0, st, (const SaMergeRow*)s->m_rows.p, n, Dp,
                       (const float*)s->feat.p, (const float*)s->norm.p, (const float*)s->m_new_feat.p, (const float*)s->m_new_norm.p,
                       (float*)s->m_feat.p, (float*)s->m_norm.p);
    SA_HIPCHK(e, hipGetLastError());
    hipLaunchKernelGGL(k_merge_scatter, dim3(row_blocks(n)), dim3(MERGE_THREADS), 0, st, (const SaMergeRow*)s->m_rows.p, n, Dp,
                       (const float*)s->m_feat.p, (const float*)s->m_norm.p, (float*)s->feat.p, (float*)s->norm.p);
    SA_HIPCHK(e, hipGetLastError());
    ms.launches += 2;
    ms.rows_rewritten = n;
    ms.bytes_moved += 4ull * n * row_bytes;   // read + write, twice
  }
  if (!moves.empty()) {
    const size_t n = moves.size() * s->Kp;
    SA_TRY(sa_store_launch_compact(s, moves.data(), moves.size()));
    ++ms.launches;
    ms.tracks_moved = (uint32_t)moves.size();
    ms.bytes_moved += 2ull * n * row_bytes;
  }
  SA_HIPCHK(e, hipEventRecord(s->ev[1], st));
  SA_TRY(sa_store_upload_table(s));
  SA_HIPCHK(e, hipStreamSynchronize(st));
  float t = 0.f;
  SA_HIPCHK(e, hipEventElapsedTime(&t, s->ev[0], s->ev[1]));
  ms.device_ms = t;
  return SA_OK;
}

}  // namespace

int sa_store_launch_compact(sa_store* s, const SaMergeMove* moves, size_t n) {
  if (!n) return SA_OK;
  const size_t rows = n * s->Kp;   // (below 2^31: every move names a stored slot, sa_search_limits.h)
  SA_TRY(sa_engine_ensure(s->e, s->m_moves, n * sizeof(SaMergeMove)));
  SA_HIPCHK(s->e, hipMemcpyAsync(s->m_moves.p, moves, n * sizeof(SaMergeMove), hipMemcpyHostToDevice, s->st));
  hipLaunchKernelGGL(k_merge_compact, dim3(row_blocks(rows)), dim3(MERGE_THREADS), 0, s->st, (const SaMergeMove*)s->m_moves.p, (uint32_t)rows,
                     s->row_floats(), s->lgK, (float*)s->feat.p, (float*)s->norm.p);
  SA_HIPCHK(s->e, hipGetLastError());
  return SA_OK;
}

extern "C" {

int sa_store_append(sa_store* s, uint32_t keep, uint32_t n, const uint64_t* ids, const uint32_t* n_obs, const float* feats,
                    const float* quality, const uint32_t* capacity) {
  return sa_store_append_impl(s, "sa_store_append", keep, n, ids, n_obs, SaRowSource::of_host(feats), quality, capacity);
}

}  // extern "C"

int sa_store_append_impl(sa_store* s, const char* what, uint32_t keep, uint32_t n, const uint64_t* ids, const uint32_t* n_obs,
                         const SaRowSource& src, const float* quality, const uint32_t* capacity) {
  if (!s) return SA_ERR_BAD_ARG;
  SA_TRY(sa_store_enter(s, what));
  sa_engine* e = s->e;
  SA_TRY(check_rule(s, keep, n, capacity, what));
  if (n == 0) return SA_OK;
  if (!ids || !n_obs) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
  size_t total = 0;
  uint32_t fresh = 0;
  std::vector<uint32_t> slots(n);
  SA_TRY(sa_store_check_ids(s, what, n, ids, slots.data(), [&](uint32_t i) {
    if (n_obs[i] > s->K)
      return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: %u observations for id %llu (max_observations %u)", what, n_obs[i],
                            (unsigned long long)ids[i], s->K);
    total += n_obs[i];
    fresh += slots[i] == SA_SEARCH_NONE ? 1u : 0u;
    return (int)SA_OK;
  }));
  SA_TRY(sa_rows_check(s, what, src, total, "feats"));
  if (quality)
    for (size_t r = 0; r < total; ++r)
      if (std::isnan(quality[r])) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: NaN quality at row %zu", what, r);
  const uint64_t T1 = (uint64_t)s->T + fresh;
  if (const int x = sa_search_extent(T1, 0, s->Kp, s->D)) return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: %s", what, sa_search_extent_text(x));
  SA_TRY(sa_store_reserve(s, T1));
  const uint32_t Kp = s->Kp;
  std::vector<SaMergeRow> rows;
  std::vector<SaMergeObs> bank;
  uint32_t off = 0;
  for (uint32_t i = 0; i < n; off += n_obs[i], ++i) {
    const bool is_new = slots[i] == SA_SEARCH_NONE;
    if (!is_new && n_obs[i] == 0) continue;   // nothing added: the bank stays exactly as it is, no rule runs
    const uint32_t slot = is_new ? s->slot_append(ids[i]) : slots[i];
    float* q = s->qual.data() + (size_t)slot * Kp;
    bank.clear();
    for (uint32_t k = 0; k < s->nobs[slot]; ++k) bank.push_back({slot * Kp + k, q[k]});
    for (uint32_t k = 0; k < n_obs[i]; ++k) bank.push_back({SA_MERGE_STAGED | (off + k), quality ? quality[off + k] : 0.f});
    s->nobs[slot] = sa_merge_plan_bank(keep, capacity ? capacity[i] : s->K, Kp, slot, s->nobs[slot], is_new, bank, rows, q);
    s->qual_dirty = true;
  }
  const int rc = run_plan(s, rows, {}, (uint32_t)total, src);
  if (rc != SA_OK) s->broken = true;
  return rc;
}

extern "C" {

int sa_store_merge(sa_store* s, uint32_t keep, uint32_t n_dst, const uint64_t* dst_ids, const uint32_t* n_src, const uint64_t* src_ids,
                   const uint32_t* capacity) {
  return sa_store_merge_impl(s, "sa_store_merge", false, nullptr, keep, n_dst, dst_ids, n_src, src_ids, capacity);
}

int sa_store_merge_compat(sa_store* s, const sa_compat* c, uint32_t keep, uint32_t n_dst, const uint64_t* dst_ids, const uint32_t* n_src,
                          const uint64_t* src_ids, const uint32_t* capacity) {
  return sa_store_merge_impl(s, "sa_store_merge_compat", true, c, keep, n_dst, dst_ids, n_src, src_ids, capacity);
}

}  // extern "C"

// ruled (compat is then the caller's rule, validated here): the attribute merges of Track::merge ride along.  Per destination the
// sources are taken in call order against the destination's attributes as merged so far; the whole call is refused before anything
// changes if a source is not compatible.
int sa_store_merge_impl(sa_store* s, const char* what, bool ruled, const sa_compat* compat, uint32_t keep, uint32_t n_dst,
                        const uint64_t* dst_ids, const uint32_t* n_src, const uint64_t* src_ids, const uint32_t* capacity) {
  if (!s) return SA_ERR_BAD_ARG;
  SA_TRY(sa_store_enter(s, what));
  sa_engine* e = s->e;
  if (ruled) SA_TRY(sa_store_check_compat(s, compat, what, true));
  SA_TRY(check_rule(s, keep, n_dst, capacity, what));
  if (n_dst == 0) return SA_OK;
  if (!dst_ids || !n_src) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
  size_t total = 0;
  for (uint32_t i = 0; i < n_dst; ++i) total += n_src[i];
  if (total && !src_ids) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null src_ids", what);
  if (total > s->T) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: %zu sources in a store of %u tracks", what, total, s->T);
  std::vector<uint32_t> dst_slot(n_dst), src_slot(total);
  {   // the checks of sa_store_check_ids, worded by role ("destination id 0", "unknown source ..."): the messages are this call's own
    std::unordered_set<uint64_t> seen;
    seen.reserve(((size_t)n_dst + total) * 2u);
    auto slot_of = [&](uint64_t id, const char* role, uint32_t* out) {
      if (id == 0) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: %s id 0", what, role);
      if (!seen.insert(id).second) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: id %llu twice in one call", what, (unsigned long long)id);
      const auto it = s->slot_of.find(id);
      if (it == s->slot_of.end()) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: unknown %s %llu", what, role, (unsigned long long)id);
      *out = it->second;
      return (int)SA_OK;
    };
    for (uint32_t i = 0; i < n_dst; ++i) SA_TRY(slot_of(dst_ids[i], "destination", &dst_slot[i]));
    for (size_t j = 0; j < total; ++j) SA_TRY(slot_of(src_ids[j], "source", &src_slot[j]));
  }
  std::vector<sa_track_attrs> merged;
  if (compat) {
    merged.resize(n_dst);
    size_t o = 0;
    for (uint32_t i = 0; i < n_dst; o += n_src[i], ++i) {
      sa_track_attrs run = s->attrs[dst_slot[i]];
      for (uint32_t j = 0; j < n_src[i]; ++j) {
        const sa_track_attrs& src = s->attrs[src_slot[o + j]];
        if (compat->flags && !sa_compat_live(compat->flags, compat->ready_at, run, src))
          return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: source %llu is not compatible with destination %llu (flags 0x%x)", what,
                                (unsigned long long)src_ids[o + j], (unsigned long long)dst_ids[i], compat->flags);
        run = sa_compat_union(run, src);
      }
      merged[i] = run;
    }
    for (uint32_t i = 0; i < n_dst; ++i) s->attrs[dst_slot[i]] = merged[i];
  }
  const uint32_t Kp = s->Kp, T0 = s->T;
  std::vector<SaMergeRow> rows;
  std::vector<SaMergeObs> bank;
  size_t off = 0;
  for (uint32_t i = 0; i < n_dst; off += n_src[i], ++i) {
    const uint32_t slot = dst_slot[i];
    float* q = s->qual.data() + (size_t)slot * Kp;
    bank.clear();
    for (uint32_t k = 0; k < s->nobs[slot]; ++k) bank.push_back({slot * Kp + k, q[k]});
    for (uint32_t j = 0; j < n_src[i]; ++j) {
      const uint32_t ss = src_slot[off + j];
      for (uint32_t k = 0; k < s->nobs[ss]; ++k) bank.push_back({ss * Kp + k, s->qual[(size_t)ss * Kp + k]});
    }
    s->nobs[slot] = sa_merge_plan_bank(keep, capacity ? capacity[i] : s->K, Kp, slot, s->nobs[slot], false, bank, rows, q);
    s->qual_dirty = true;
  }
  // the sources leave: the tables as sa_store_remove(src_ids) would leave them, the device rows in one launch
  std::vector<uint32_t> perm;
  std::vector<SaMergeMove> moves;
  sa_merge_compaction(T0, src_slot, perm, moves);
  for (size_t j = 0; j < total; ++j) s->slot_of.erase(src_ids[j]);
  for (const SaMergeMove& m : moves) s->slot_move(m.from, m.to);
  s->slot_truncate((uint32_t)perm.size());
  const int rc = run_plan(s, rows, moves, 0, SaRowSource{});
  if (rc != SA_OK) s->broken = true;
  return rc;
}

extern "C" {

int sa_store_fetch(sa_store* s, uint32_t n, const uint64_t* ids, uint32_t* out_n_obs, float* out_feats, float* out_quality) {
  const char* what = "sa_store_fetch";
  if (!s) return SA_ERR_BAD_ARG;
  SA_TRY(sa_store_enter(s, what));
  sa_engine* e = s->e;
  if (n == 0) return SA_OK;
  if (!ids || !out_n_obs || !out_feats) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
  const uint32_t K = s->K, Kp = s->Kp, D = s->D, Dp = s->row_floats();
  if ((uint64_t)n * K > SA_STORE_MAX_SLOTS) return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 output rows", what);
  std::vector<SaMergeRow> rows;   // dst: the output row i * K + k
  for (uint32_t i = 0; i < n; ++i) {
    const auto it = s->slot_of.find(ids[i]);
    const uint32_t slot = it == s->slot_of.end() ? 0u : it->second, m = it == s->slot_of.end() ? 0u : s->nobs[slot];
    out_n_obs[i] = m;
    for (uint32_t k = 0; k < m; ++k) rows.push_back({i * K + k, slot * Kp + k});
    if (out_quality)
      for (uint32_t k = 0; k < K; ++k) out_quality[(size_t)i * K + k] = k < m ? s->qual[(size_t)slot * Kp + k] : 0.f;
  }
  std::memset(out_feats, 0, (size_t)n * K * D * 4);
  if (rows.empty()) return SA_OK;
  const uint32_t nr = (uint32_t)rows.size();
  SA_TRY(sa_engine_ensure(e, s->m_rows, rows.size() * sizeof(SaMergeRow)));
  SA_TRY(sa_engine_ensure(e, s->m_feat, rows.size() * s->row_bytes()));
  SA_TRY(sa_engine_ensure(e, s->m_norm, rows.size() * 4));
  hipStream_t st = s->st;
  SA_HIPCHK(e, hipMemcpyAsync(s->m_rows.p, rows.data(), rows.size() * sizeof(SaMergeRow), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_merge_gather, dim3(row_blocks(nr)), dim3(MERGE_THREADS), 0, st, (const SaMergeRow*)s->m_rows.p, nr, Dp,
                     (const float*)s->feat.p, (const float*)s->norm.p, (const float*)nullptr, (const float*)nullptr, (float*)s->m_feat.p,
                     (float*)s->m_norm.p);
  SA_HIPCHK(e, hipGetLastError());
  std::vector<float> padded((size_t)nr * Dp);
  SA_HIPCHK(e, hipMemcpyAsync(padded.data(), s->m_feat.p, padded.size() * 4, hipMemcpyDeviceToHost, st));
  SA_HIPCHK(e, hipStreamSynchronize(st));
  if (s->elem == SA_ELEM_BF16) {   // the 16-bit rows widened on the host: a bf16 value is the upper half of its f32
    const uint16_t* half = (const uint16_t*)padded.data();
    for (uint32_t r = 0; r < nr; ++r)
      for (uint32_t k = 0; k < D; ++k) {
        const uint32_t u = (uint32_t)half[(size_t)r * s->Dp + k] << 16;
        std::memcpy(out_feats + (size_t)rows[r].dst * D + k, &u, 4);
      }
    return SA_OK;
  }
  if (s->elem == SA_ELEM_I8) {   // the codes as they are: integers in -127 .. 127 (include/similari_i8.h)
    const int8_t* code = (const int8_t*)padded.data();
    for (uint32_t r = 0; r < nr; ++r)
      for (uint32_t k = 0; k < D; ++k) out_feats[(size_t)rows[r].dst * D + k] = (float)code[(size_t)r * s->Dp + k];
    return SA_OK;
  }
  if (s->elem == SA_ELEM_F16) {   // binary16 widened exactly: a subnormal is m 2^-24, inf and NaN keep their payload
    const uint16_t* half = (const uint16_t*)padded.data();
    for (uint32_t r = 0; r < nr; ++r)
      for (uint32_t k = 0; k < D; ++k) {
        const uint32_t h = half[(size_t)r * s->Dp + k], sign = (h & 0x8000u) << 16, ex = (h >> 10) & 31u, m = h & 0x3ffu;
        uint32_t u;
        if (ex == 31u) u = sign | 0x7f800000u | (m << 13);
        else if (ex) u = sign | ((ex + 112u) << 23) | (m << 13);
        else {
          const float f = (float)m * 5.9604644775390625e-8f;   // m 2^-24, exact
          std::memcpy(&u, &f, 4);
          u |= sign;
        }
        std::memcpy(out_feats + (size_t)rows[r].dst * D + k, &u, 4);
      }
    return SA_OK;
  }
  for (uint32_t r = 0; r < nr; ++r) std::memcpy(out_feats + (size_t)rows[r].dst * D, padded.data() + (size_t)r * Dp, (size_t)D * 4);
  return SA_OK;
}

int sa_store_merge_last(sa_store* s, sa_merge_stats* out) {
  if (!s || !out) return SA_ERR_BAD_ARG;
  *out = s->merge_last;
  return SA_OK;
}

}  // extern "C"
