// sa_absorb.hip — a frame's tracks absorbed in one call (include/similari_absorb.h): the BestFit search of sa_store_search_topn_impl
// with a step queued behind its vote.  The search's body calls back through SaAbsorbStep (sa_store.h): check and prepare before
// anything is launched, queue behind the vote of the run that fits the pool.  The step is three launches whatever the number of
// queries, and nothing it needs crosses the bus: the padded query rows with their norms lie in q_feat / q_norm, the claim's outcome
// in o_n / o_id, the banks' counts in d_nobs.
//   k_absorb_match  one wave per query: the stored slot whose id entry 0 names if it holds the claim, else none
//   k_absorb_rank   one workgroup: an exclusive scan over the unmatched queries; query q's destination slot
//   k_absorb_move   one wave per query: the bank shifts, takes the query rows, zeroes its tail; d_nobs (a created slot: d_ids too)
// After the call's last wait the host replays the same rule on its tables.
//
// Reference: examples/incremental_track_build.rs:60-95, benches/feature_tracker.rs:60-90 (merge_external / add_track per new track,
// "keep the last C" as the retention rule).
#include "sa_compat.h"
#include "sa_store.h"

#include <cmath>
#include <vector>

namespace {

constexpr uint32_t AB_THREADS = 256, AB_WAVES = AB_THREADS / 64;
constexpr uint32_t RANK_THREADS = 1024, RANK_WAVES = RANK_THREADS / 64;

// Query q is matched iff its row has an entry and entry 0's winner is not the query itself (similari_bestfit.h, 10b: the winner is
// then the stored id whose claim the entry holds).  The wave walks d_ids for that id, four loads in flight per lane; ids are unique,
// so at most one lane meets it, and the minimum over the wave is its slot (SA_SEARCH_NONE: no lane did).
__global__ __launch_bounds__(AB_THREADS) void k_absorb_match(const uint32_t* __restrict__ o_n, const uint64_t* __restrict__ o_id,
                                                             const uint64_t* __restrict__ q_ids, const uint64_t* __restrict__ s_ids,
                                                             uint32_t Q, uint32_t T, uint32_t topn, uint32_t* __restrict__ slot_out) {
  constexpr uint32_t U = 4;
  const uint32_t q = blockIdx.x * AB_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (q >= Q) return;
  const uint64_t qid = q_ids[q];
  const uint64_t w = o_n[q] ? o_id[(size_t)q * topn] : qid;
  uint32_t found = SA_SEARCH_NONE;
  if (w != qid) {
    for (uint32_t s0 = lane; s0 < T; s0 += U * 64u) {
      uint64_t id[U];
#pragma unroll
      for (uint32_t u = 0; u < U; ++u) id[u] = s0 + u * 64u < T ? s_ids[s0 + u * 64u] : 0ull;   // 0 is no id
#pragma unroll
      for (uint32_t u = 0; u < U; ++u)
        if (id[u] == w) found = s0 + u * 64u;
    }
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t x = __shfl_xor(found, o);
      found = x < found ? x : found;
    }
  }
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

// One wave per query, 16-byte pieces of a row of Dp floats as the movers of sa_merge.hip count it (sa_store::row_floats).  The
// destination bank holds n0 rows (a created slot: none) and takes the query's n1 at capacity C: keep = min(n0 + n1, C), drop = n0 +
// n1 - keep; position j takes combined row drop + j — the bank's own row drop + j while that is below n0, else row drop + j - n0 of
// the query —, the row's norm moves with it, positions keep .. n0 - 1 (a created slot: keep .. Kp - 1) end zeroed with norm 0.
// A matched query without a row leaves its bank alone, as sa_store_append does.
// The bank shifts onto itself when drop > 0.  The one owning wave moves the rows in ascending j, and piece i of a row is read and
// written by the same lane (i % 64) in every iteration: position j is written in iteration j and read, as row drop + j', only in
// iteration j' = j - drop < j, earlier in that lane's program order.  No other wave touches the bank: BestFit hands a stored track to
// one query, and created slots are distinct.  s_feat / s_norm carry no __restrict__, q_feat / q_norm are only read.
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
  const uint32_t tot = n0 + n1, keep = tot < C ? tot : C, drop = tot - keep;
  const uint32_t end = created ? Kp : (n0 > keep ? n0 : keep);
  const size_t bank = (size_t)dst * Kp, qrow = (size_t)q * Kp;
  for (uint32_t j = 0; j < end; ++j) {
    float4* to = (float4*)(s_feat + (bank + j) * Dp);
    if (j >= keep) {
      for (uint32_t i = lane; i < Dp / 4; i += 64u) to[i] = float4{0.f, 0.f, 0.f, 0.f};
      if (lane == 0) s_norm[bank + j] = 0.f;
      continue;
    }
    const uint32_t r = drop + j;
    if (r < n0) {
      if (drop == 0) continue;   // the row stays where it is
      const float4* from = (const float4*)(s_feat + (bank + r) * Dp);
      for (uint32_t i = lane; i < Dp / 4; i += 64u) to[i] = from[i];
      if (lane == 0) s_norm[bank + j] = s_norm[bank + r];
    } else {
      const float4* from = (const float4*)(q_feat + (qrow + (r - n0)) * Dp);
      for (uint32_t i = lane; i < Dp / 4; i += 64u) to[i] = from[i];
      if (lane == 0) s_norm[bank + j] = q_norm[qrow + (r - n0)];
    }
  }
  if (lane == 0) {
    d_nobs[dst] = keep;
    if (created) d_ids[dst] = q_ids[q];
  }
}

uint32_t wave_blocks(uint32_t n) { return (n + AB_WAVES - 1) / AB_WAVES; }

int absorb_impl(sa_store* s, const char* what, const sa_topn_params* p, const sa_compat* c, uint32_t nq, const uint64_t* q_ids,
                const uint32_t* q_n_obs, const SaRowSource& src, const sa_track_attrs* q_attrs, const float* quality,
                const uint32_t* capacity, uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track, double* out_weight,
                uint64_t* out_dest) {
  if (!s) return SA_ERR_BAD_ARG;
  s->absorb_last = sa_absorb_stats{};
  bool queued = false, voted = false;
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
    return SA_OK;
  };
  step.queue = [&](bool after_vote) -> int {
    sa_engine* e = s->e;
    hipStream_t st = s->st;
    queued = true;
    voted = after_vote;
    uint32_t* slot = (uint32_t*)s->ab_slot.p;
    if (capacity) SA_HIPCHK(e, hipMemcpyAsync(s->ab_cap.p, capacity, (size_t)nq * 4, hipMemcpyHostToDevice, st));
    SA_HIPCHK(e, hipEventRecord(s->ev[6], st));
    if (after_vote) {
      hipLaunchKernelGGL(k_absorb_match, dim3(wave_blocks(nq)), dim3(AB_THREADS), 0, st, (const uint32_t*)s->o_n.p, (const uint64_t*)s->o_id.p,
                         (const uint64_t*)s->q_ids.p, (const uint64_t*)s->d_ids.p, nq, s->T, p->topn, slot);
      SA_HIPCHK(e, hipGetLastError());
      ++s->absorb_last.launches;
    } else SA_HIPCHK(e, hipMemsetAsync(slot, 0xff, (size_t)nq * 4, st));   // nothing was searched: no query is matched
    hipLaunchKernelGGL(k_absorb_rank, dim3(1), dim3(RANK_THREADS), 0, st, slot, nq, s->T);
    SA_HIPCHK(e, hipGetLastError());
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
  if (!queued) return SA_OK;   // n_queries == 0
  // The host tables take the same rule, in query order: an unmatched query's slot_append meets the rank kernel's T + rank.
  sa_absorb_stats& st = s->absorb_last;
  const uint32_t Kp = s->Kp, topn = p->topn;
  std::vector<float> bank;
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
    for (uint32_t j = 0; j < Kp; ++j) ql[j] = j < keep ? bank[drop + j] : 0.f;
    s->nobs[slot] = keep;
    st.rows_moved += matched ? (drop ? keep : n1) + (n0 > keep ? n0 - keep : 0u) : Kp;
  }
  float ms = 0.f;
  SA_HIPCHK(s->e, hipEventElapsedTime(&ms, s->ev[6], s->ev[7]));
  st.step_ms = ms;
  st.host_waits = voted ? s->last.reruns + 2u : 1u;   // one per run of the search for the pool's cursor, one behind the copies out
  return SA_OK;
}

}  // namespace

extern "C" {

int sa_store_absorb(sa_store* s, const sa_topn_params* p, const sa_compat* c, uint32_t n_queries, const uint64_t* q_ids,
                    const uint32_t* q_n_obs, const float* q_feats, const sa_track_attrs* q_attrs, const float* quality,
                    const uint32_t* capacity, uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track, double* out_weight,
                    uint64_t* out_dest) {
  return absorb_impl(s, "sa_store_absorb", p, c, n_queries, q_ids, q_n_obs, SaRowSource::of_host(q_feats), q_attrs, quality, capacity, out_n,
                     out_winner, out_track, out_weight, out_dest);
}

int sa_store_absorb_dev(sa_store* s, const sa_topn_params* p, const sa_compat* c, uint32_t n_queries, const uint64_t* q_ids,
                        const uint32_t* q_n_obs, const sa_dev_rows* rows, const sa_track_attrs* q_attrs, const float* quality,
                        const uint32_t* capacity, uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track, double* out_weight,
                        uint64_t* out_dest) {
  if (!s) return SA_ERR_BAD_ARG;
  s->devrows_last = sa_devrows_stats{};
  return absorb_impl(s, "sa_store_absorb_dev", p, c, n_queries, q_ids, q_n_obs, SaRowSource::of_device(rows), q_attrs, quality, capacity,
                     out_n, out_winner, out_track, out_weight, out_dest);
}

int sa_store_absorb_last(sa_store* s, sa_absorb_stats* out) {
  if (!s || !out) return SA_ERR_BAD_ARG;
  *out = s->absorb_last;
  return SA_OK;
}

}  // extern "C"
