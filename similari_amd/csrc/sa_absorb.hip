// sa_absorb.hip — a frame's tracks absorbed in one call (include/similari_absorb.h): the BestFit search of sa_store_search_topn_impl
// with a step queued behind its vote.  The search's body calls back through SaAbsorbStep (sa_store.h): check and prepare before
// anything is launched, queue behind the vote of the run that fits the pool.  The step is three launches whatever the number of
// queries, and nothing it needs crosses the bus: the padded query rows with their norms lie in q_feat / q_norm, the claim's outcome
// in o_n / o_id, the banks' counts in d_nobs.
//   k_absorb_match  one wave per query: the stored slot whose id entry 0 names if it holds the claim, else none
//   k_absorb_rank   one workgroup: an exclusive scan over the unmatched queries; query q's destination slot
//   k_absorb_move   one wave per query: the bank shifts, takes the query rows, zeroes its tail; d_nobs (a created slot: d_ids too)
// After the call's last wait the host replays the same rule on its tables.
// Under SA_KEEP_BEST (include/similari_retain.h) the third launch is k_absorb_move_best instead: the wave ranks the combined bank by
// quality — the bank's from d_qual, the store's device mirror of its quality table, the query's from ab_qual — and permutes the rows
// in place.  The mirror is uploaded ahead of the step only if a call other than a SA_KEEP_BEST absorb wrote the table since.
//
// Reference: examples/incremental_track_build.rs:60-95, benches/feature_tracker.rs:60-90 (merge_external / add_track per new track,
// "keep the last C" as the retention rule); examples/track_merging.rs:279-297 (sort by quality descending, truncate).
#include "sa_bank_move.h"
#include "sa_compat.h"
#include "sa_merge_plan.h"
#include "sa_store.h"

#include <cmath>
#include <vector>

namespace {

constexpr uint32_t AB_THREADS = 256, AB_WAVES = AB_THREADS / 64;
constexpr uint32_t RANK_THREADS = 1024, RANK_WAVES = RANK_THREADS / 64;

// Query q is matched iff its row has an entry and entry 0's winner is not the query itself (similari_bestfit.h, 10b: the winner is
// then the stored id whose claim the entry holds).  The wave walks d_ids for that id (sa_bank_find_slot, sa_bank_move.h):
// SA_SEARCH_NONE if no slot holds it.
__global__ __launch_bounds__(AB_THREADS) void k_absorb_match(const uint32_t* __restrict__ o_n, const uint64_t* __restrict__ o_id,
                                                             const uint64_t* __restrict__ q_ids, const uint64_t* __restrict__ s_ids,
                                                             uint32_t Q, uint32_t T, uint32_t topn, uint32_t* __restrict__ slot_out) {
  const uint32_t q = blockIdx.x * AB_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (q >= Q) return;
  const uint64_t qid = q_ids[q];
  const uint64_t w = o_n[q] ? o_id[(size_t)q * topn] : qid;
  uint32_t found = SA_SEARCH_NONE;
  if (w != qid) found = sa_bank_find_slot(w, s_ids, T, lane);
  if (lane == 0) slot_out[q] = found;
}

// slot[q]: in, the matched slot or SA_SEARCH_NONE; out, the destination slot — an unmatched query takes T + the number of unmatched
// queries before it.  One workgroup walks the queries in chunks of RANK_THREADS with a running carry: a ballot per wave, the waves'
// totals through LDS.  O(Q) work, the same sums in the same order every time.
__global__ __launch_bounds__(RANK_THREADS) void k_absorb_rank(uint32_t* __restrict__ slot, uint32_t Q, uint32_t T) {
  __shared__ uint32_t w_sum[RANK_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t carry = 0;
  for (uint32_t q0 = 0; q0 < Q; q0 += RANK_THREADS) {
    const uint32_t q = q0 + tid;
    const bool fresh = q < Q && slot[q] == SA_SEARCH_NONE;
    const unsigned long long b = __ballot(fresh);
    const uint32_t before = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) w_sum[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t base = carry, total = 0;
    for (uint32_t w = 0; w < RANK_WAVES; ++w) {
      const uint32_t n = w_sum[w];
      base += w < wave ? n : 0u;
      total += n;
    }
    if (fresh) slot[q] = T + base + before;
    carry += total;
    __syncthreads();   // w_sum is rewritten in the next chunk
  }
}

// One wave per query: the destination bank takes the query's n1 rows at capacity C as sa_bank_take_latest (sa_bank_move.h) says.
// A matched query without a row leaves its bank alone, as sa_store_append does.  No other wave touches the bank: BestFit hands a
// stored track to one query, and created slots are distinct.  s_feat / s_norm carry no __restrict__, q_feat / q_norm are only read.
__global__ __launch_bounds__(AB_THREADS) void k_absorb_move(const uint32_t* __restrict__ slot, const uint32_t* __restrict__ q_nobs,
                                                            const uint64_t* __restrict__ q_ids, const uint32_t* __restrict__ cap,
                                                            uint32_t Q, uint32_t T, uint32_t K, uint32_t Kp, uint32_t Dp,
                                                            const float* __restrict__ q_feat, const float* __restrict__ q_norm,
                                                            float* s_feat, float* s_norm, uint32_t* __restrict__ d_nobs,
                                                            uint64_t* __restrict__ d_ids) {
  const uint32_t q = blockIdx.x * AB_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (q >= Q) return;
  const uint32_t dst = slot[q], n1 = q_nobs[q];
  const bool created = dst >= T;
  if (!created && n1 == 0) return;
  const uint32_t n0 = created ? 0u : d_nobs[dst];
  const uint32_t C = cap ? cap[q] : K;
  const uint32_t keep = sa_bank_take_latest(lane, created, n0, n1, C, Kp, Dp, q_feat, q_norm, (size_t)q * Kp, s_feat, s_norm, (size_t)dst * Kp);
  if (lane == 0) {
    d_nobs[dst] = keep;
    if (created) d_ids[dst] = q_ids[q];
  }
}

// The move under SA_KEEP_BEST, one wave per query: the wave ranks the combined bank — the bank's qualities from s_qual, the query's
// from q_qual — and permutes the rows in place as sa_bank_take_best (sa_bank_move.h) says.  A matched query without a row leaves its
// bank alone.  No other wave touches the bank: BestFit hands a stored track to one query, and created slots are distinct.
template <uint32_t KP>
__global__ __launch_bounds__(AB_THREADS) void k_absorb_move_best(const uint32_t* __restrict__ slot, const uint32_t* __restrict__ q_nobs,
                                                                 const uint64_t* __restrict__ q_ids, const uint32_t* __restrict__ cap,
                                                                 uint32_t Q, uint32_t T, uint32_t K, uint32_t Dp,
                                                                 const float* __restrict__ q_feat, const float* __restrict__ q_norm,
                                                                 const float* __restrict__ q_qual, float* s_feat, float* s_norm,
                                                                 float* s_qual, uint32_t* __restrict__ d_nobs, uint64_t* __restrict__ d_ids) {
  // the wave's number is the same in every lane: said to the compiler, so that what follows from it lives in scalar registers and the
  // tests on it are branches, not 2 KP lane masks
  const uint32_t q = blockIdx.x * AB_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (q >= Q) return;
  const uint32_t dst = slot[q], n1 = q_nobs[q];
  const bool created = dst >= T;
  if (!created && n1 == 0) return;
  const uint32_t n0 = created ? 0u : d_nobs[dst];
  const uint32_t C = cap ? cap[q] : K;
  const uint32_t keep = sa_bank_take_best<KP>(lane, created, n0, n1, C, Dp, q_feat, q_norm, q_qual, (size_t)q * KP, s_feat, s_norm, s_qual,
                                              (size_t)dst * KP);
  if (lane == 0) {
    d_nobs[dst] = keep;
    if (created) d_ids[dst] = q_ids[q];
  }
}

using MoveBest = void (*)(const uint32_t*, const uint32_t*, const uint64_t*, const uint32_t*, uint32_t, uint32_t, uint32_t, uint32_t, const float*,
                          const float*, const float*, float*, float*, float*, uint32_t*, uint64_t*);
MoveBest move_best(uint32_t lgK) {   // Kp = 1 << lgK, at most 32 (sa_store_create_as)
  static const MoveBest form[6] = {k_absorb_move_best<1>, k_absorb_move_best<2>, k_absorb_move_best<4>,
                                   k_absorb_move_best<8>, k_absorb_move_best<16>, k_absorb_move_best<32>};
  return lgK < 6 ? form[lgK] : nullptr;
}

uint32_t wave_blocks(uint32_t n) { return (n + AB_WAVES - 1) / AB_WAVES; }

}  // namespace

int sa_store_absorb_impl(sa_store* s, const char* what, uint32_t keep, const sa_topn_params* p, const sa_compat* c, uint32_t nq,
                         const uint64_t* q_ids, const uint32_t* q_n_obs, const SaRowSource& src, const sa_track_attrs* q_attrs,
                         const float* quality, const uint32_t* capacity, uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track,
                         double* out_weight, uint64_t* out_dest) {
  if (!s) return SA_ERR_BAD_ARG;
  s->absorb_last = sa_absorb_stats{};
  s->retain_keep = 0;
  s->retain_upload = 0;
  if (keep != SA_KEEP_LATEST && keep != SA_KEEP_BEST) {   // as sa_store_append: ahead of n_queries == 0
    SA_TRY(sa_store_enter(s, what));
    return sa_engine_fail(s->e, SA_ERR_BAD_ARG, "%s: unknown keep %u", what, keep);
  }
  const bool best = keep == SA_KEEP_BEST;
  bool queued = false, voted = false;
  uint64_t uploaded = 0;
  std::vector<float> padded;   // SA_KEEP_BEST: the qualities of the query rows as ab_qual takes them, [nq][Kp]
  SaAbsorbStep step;
  // behind the search's checks of its query list: ids and counts are valid here
  step.check = [&]() -> int {
    sa_engine* e = s->e;
    if (!out_dest) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
    size_t total = 0;
    for (uint32_t q = 0; q < nq; ++q) {
      if (s->slot_of.count(q_ids[q]))
        return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: query id %llu is a stored track's", what, (unsigned long long)q_ids[q]);
      total += q_n_obs[q];
    }
    if (capacity)
      for (uint32_t q = 0; q < nq; ++q)
        if (capacity[q] < 1 || capacity[q] > s->K)
          return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: capacity %u at %u (1..%u)", what, capacity[q], q, s->K);
    if (quality)
      for (size_t r = 0; r < total; ++r)
        if (std::isnan(quality[r])) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: NaN quality at row %zu", what, r);
    return SA_OK;
  };
  step.prepare = [&]() -> int {
    sa_engine* e = s->e;
    const uint64_t T1 = (uint64_t)s->T + nq;
    if (const int x = sa_search_extent(T1, 0, s->Kp, s->D)) return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: %s", what, sa_search_extent_text(x));
    SA_TRY(sa_store_reserve(s, T1));
    SA_TRY(sa_engine_ensure(e, s->ab_slot, (size_t)nq * 4));
    if (capacity) SA_TRY(sa_engine_ensure(e, s->ab_cap, (size_t)nq * 4));
    if (best) {
      if (!move_best(s->lgK)) return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: no move for %u observations per track", what, s->K);
      SA_TRY(sa_engine_ensure(e, s->d_qual, (size_t)s->cap * s->Kp * 4));   // grows only behind a reservation, which marked it stale
      SA_TRY(sa_engine_ensure(e, s->ab_qual, (size_t)nq * s->Kp * 4));
      padded.assign((size_t)nq * s->Kp, 0.f);
      if (quality) {
        size_t off = 0;
        for (uint32_t q = 0; q < nq; off += q_n_obs[q], ++q) std::copy_n(quality + off, q_n_obs[q], padded.begin() + (size_t)q * s->Kp);
      }
    }
    return SA_OK;
  };
  step.queue = [&](bool after_vote) -> int {
    sa_engine* e = s->e;
    hipStream_t st = s->st;
    queued = true;
    voted = after_vote;
    uint32_t* slot = (uint32_t*)s->ab_slot.p;
    if (capacity) SA_HIPCHK(e, hipMemcpyAsync(s->ab_cap.p, capacity, (size_t)nq * 4, hipMemcpyHostToDevice, st));
    if (best) {
      if (s->qual_dirty && s->T) {   // the table as it stands, ahead of the step; created slots are written whole by the step
        uploaded = (uint64_t)s->T * s->Kp * 4;
        SA_HIPCHK(e, hipMemcpyAsync(s->d_qual.p, s->qual.data(), (size_t)uploaded, hipMemcpyHostToDevice, st));
      }
      SA_HIPCHK(e, hipMemcpyAsync(s->ab_qual.p, padded.data(), padded.size() * 4, hipMemcpyHostToDevice, st));
    }
    SA_HIPCHK(e, hipEventRecord(s->ev[6], st));
    if (after_vote) {
      hipLaunchKernelGGL(k_absorb_match, dim3(wave_blocks(nq)), dim3(AB_THREADS), 0, st, (const uint32_t*)s->o_n.p, (const uint64_t*)s->o_id.p,
                         (const uint64_t*)s->q_ids.p, (const uint64_t*)s->d_ids.p, nq, s->T, p->topn, slot);
      SA_HIPCHK(e, hipGetLastError());
      ++s->absorb_last.launches;
    } else SA_HIPCHK(e, hipMemsetAsync(slot, 0xff, (size_t)nq * 4, st));   // nothing was searched: no query is matched
    hipLaunchKernelGGL(k_absorb_rank, dim3(1), dim3(RANK_THREADS), 0, st, slot, nq, s->T);
    SA_HIPCHK(e, hipGetLastError());
    if (best)
      hipLaunchKernelGGL(move_best(s->lgK), dim3(wave_blocks(nq)), dim3(AB_THREADS), 0, st, (const uint32_t*)slot, (const uint32_t*)s->q_nobs.p,
                         (const uint64_t*)s->q_ids.p, capacity ? (const uint32_t*)s->ab_cap.p : nullptr, nq, s->T, s->K, s->row_floats(),
                         (const float*)s->q_feat.p, (const float*)s->q_norm.p, (const float*)s->ab_qual.p, (float*)s->feat.p, (float*)s->norm.p,
                         (float*)s->d_qual.p, (uint32_t*)s->d_nobs.p, (uint64_t*)s->d_ids.p);
    else
      hipLaunchKernelGGL(k_absorb_move, dim3(wave_blocks(nq)), dim3(AB_THREADS), 0, st, (const uint32_t*)slot, (const uint32_t*)s->q_nobs.p,
                         (const uint64_t*)s->q_ids.p, capacity ? (const uint32_t*)s->ab_cap.p : nullptr, nq, s->T, s->K, s->Kp, s->row_floats(),
                         (const float*)s->q_feat.p, (const float*)s->q_norm.p, (float*)s->feat.p, (float*)s->norm.p, (uint32_t*)s->d_nobs.p,
                         (uint64_t*)s->d_ids.p);
    SA_HIPCHK(e, hipGetLastError());
    s->absorb_last.launches += 2;
    SA_HIPCHK(e, hipEventRecord(s->ev[7], st));
    return SA_OK;
  };
  const SaBestFit fit{out_track, &step};
  const int rc = sa_store_search_topn_impl(s, what, p, c != nullptr, c, nq, q_ids, q_n_obs, src, q_attrs, out_n, out_winner, out_weight,
                                           nullptr, &fit);
  if (rc != SA_OK) {
    if (queued) s->broken = true;   // the banks may have moved while the tables have not
    s->absorb_last = sa_absorb_stats{};
    return rc;
  }
  s->retain_keep = keep;
  if (!queued) return SA_OK;   // n_queries == 0
  // The host tables take the same rule, in query order: an unmatched query's slot_append meets the rank kernel's T + rank.
  sa_absorb_stats& st = s->absorb_last;
  const uint32_t Kp = s->Kp, topn = p->topn;
  std::vector<float> bank;
  std::vector<SaMergeObs> obs;
  size_t off = 0;
  for (uint32_t q = 0; q < nq; off += q_n_obs[q], ++q) {
    const uint32_t n1 = q_n_obs[q];
    const bool matched = out_n[q] >= 1 && out_winner[(size_t)q * topn] != q_ids[q];
    out_dest[q] = matched ? out_winner[(size_t)q * topn] : q_ids[q];
    uint32_t slot;
    if (matched) {
      const auto it = s->slot_of.find(out_dest[q]);
      if (it == s->slot_of.end()) {
        s->broken = true;
        return sa_engine_fail(s->e, SA_ERR_STATE, "%s: the vote named %llu, which the store does not hold", what, (unsigned long long)out_dest[q]);
      }
      slot = it->second;
      ++st.matched;
    } else {
      slot = s->slot_append(q_ids[q]);
      ++st.created;
    }
    if (c) {
      s->attrs[slot] = matched ? sa_compat_union(s->attrs[slot], q_attrs[q]) : q_attrs[q];
      s->attrs_dirty = true;
    }
    if (matched && n1 == 0) continue;
    const uint32_t n0 = s->nobs[slot], C = capacity ? capacity[q] : s->K;
    const uint32_t tot = n0 + n1, keep = tot < C ? tot : C, drop = tot - keep;
    float* ql = s->qual.data() + (size_t)slot * Kp;
    bank.assign(ql, ql + n0);
    for (uint32_t k = 0; k < n1; ++k) bank.push_back(quality ? quality[off + k] : 0.f);
    if (best) {   // the rule as sa_store_append runs it (sa_merge_plan.h); a row whose rank is its own position is not moved
      obs.clear();
      for (uint32_t k = 0; k < tot; ++k) obs.push_back({k, bank[k]});
      const std::vector<uint32_t> sel = sa_merge_select(SA_KEEP_BEST, C, obs);
      uint32_t stay = 0;
      for (uint32_t j = 0; j < keep; ++j) stay += sel[j] == j && j < n0 ? 1u : 0u;
      for (uint32_t j = 0; j < Kp; ++j) ql[j] = j < keep ? bank[sel[j]] : 0.f;
      st.rows_moved += matched ? keep - stay + (n0 > keep ? n0 - keep : 0u) : Kp;
    } else {
      for (uint32_t j = 0; j < Kp; ++j) ql[j] = j < keep ? bank[drop + j] : 0.f;
      st.rows_moved += matched ? (drop ? keep : n1) + (n0 > keep ? n0 - keep : 0u) : Kp;
    }
    s->nobs[slot] = keep;
  }
  s->qual_dirty = !best;   // SA_KEEP_BEST: the step wrote d_qual as the loop above wrote qual; else the table moved on alone
  s->retain_upload = uploaded;
  float ms = 0.f;
  SA_HIPCHK(s->e, hipEventElapsedTime(&ms, s->ev[6], s->ev[7]));
  st.step_ms = ms;
  st.host_waits = voted ? s->last.reruns + 2u : 1u;   // one per run of the search for the pool's cursor, one behind the copies out
  return SA_OK;
}

extern "C" {

int sa_store_absorb(sa_store* s, const sa_topn_params* p, const sa_compat* c, uint32_t n_queries, const uint64_t* q_ids,
                    const uint32_t* q_n_obs, const float* q_feats, const sa_track_attrs* q_attrs, const float* quality,
                    const uint32_t* capacity, uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track, double* out_weight,
                    uint64_t* out_dest) {
  return sa_store_absorb_impl(s, "sa_store_absorb", SA_KEEP_LATEST, p, c, n_queries, q_ids, q_n_obs, SaRowSource::of_host(q_feats), q_attrs, quality, capacity, out_n,
                     out_winner, out_track, out_weight, out_dest);
}

int sa_store_absorb_dev(sa_store* s, const sa_topn_params* p, const sa_compat* c, uint32_t n_queries, const uint64_t* q_ids,
                        const uint32_t* q_n_obs, const sa_dev_rows* rows, const sa_track_attrs* q_attrs, const float* quality,
                        const uint32_t* capacity, uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track, double* out_weight,
                        uint64_t* out_dest) {
  if (!s) return SA_ERR_BAD_ARG;
  s->devrows_last = sa_devrows_stats{};
  return sa_store_absorb_impl(s, "sa_store_absorb_dev", SA_KEEP_LATEST, p, c, n_queries, q_ids, q_n_obs, SaRowSource::of_device(rows), q_attrs, quality, capacity,
                     out_n, out_winner, out_track, out_weight, out_dest);
}

int sa_store_absorb_last(sa_store* s, sa_absorb_stats* out) {
  if (!s || !out) return SA_ERR_BAD_ARG;
  *out = s->absorb_last;
  return SA_OK;
}

int sa_store_absorb_keep(sa_store* s, uint32_t keep, const sa_topn_params* p, const sa_compat* c, uint32_t n_queries, const uint64_t* q_ids,
                         const uint32_t* q_n_obs, const float* q_feats, const sa_track_attrs* q_attrs, const float* quality,
                         const uint32_t* capacity, uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track, double* out_weight,
                         uint64_t* out_dest) {
  return sa_store_absorb_impl(s, "sa_store_absorb_keep", keep, p, c, n_queries, q_ids, q_n_obs, SaRowSource::of_host(q_feats), q_attrs, quality,
                     capacity, out_n, out_winner, out_track, out_weight, out_dest);
}

int sa_store_absorb_keep_dev(sa_store* s, uint32_t keep, const sa_topn_params* p, const sa_compat* c, uint32_t n_queries,
                             const uint64_t* q_ids, const uint32_t* q_n_obs, const sa_dev_rows* rows, const sa_track_attrs* q_attrs,
                             const float* quality, const uint32_t* capacity, uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track,
                             double* out_weight, uint64_t* out_dest) {
  if (!s) return SA_ERR_BAD_ARG;
  s->devrows_last = sa_devrows_stats{};
  return sa_store_absorb_impl(s, "sa_store_absorb_keep_dev", keep, p, c, n_queries, q_ids, q_n_obs, SaRowSource::of_device(rows), q_attrs, quality,
                     capacity, out_n, out_winner, out_track, out_weight, out_dest);
}

int sa_store_retain_last(sa_store* s, sa_retain_stats* out) {
  if (!s || !out) return SA_ERR_BAD_ARG;
  const sa_absorb_stats& a = s->absorb_last;
  *out = sa_retain_stats{a.step_ms, a.matched, a.created, a.rows_moved, a.launches, a.host_waits, s->retain_keep, s->retain_upload};
  return SA_OK;
}

}  // extern "C"
