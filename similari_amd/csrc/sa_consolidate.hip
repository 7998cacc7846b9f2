// sa_consolidate.hip — a store's mutual best pairs merged in one call (include/similari_consolidate.h): the BestFit join of
// sa_store_join_topn_impl with a step queued behind its vote.  The join's body calls back through SaAbsorbStep (sa_store.h): check and
// prepare before anything is launched, queue behind the vote of the run that fits the pool.  The step is two launches whatever T is,
// and nothing it needs crosses the bus: the claim's outcome lies in o_n / o_id, the banks with their norms in feat / norm, their
// counts in d_nobs, their qualities in d_qual.
//   k_consolidate_pair        one wave per stored track: the slot of the track entry 0 names if it holds the claim, else none
//   k_consolidate_merge       one wave per stored track: the lower id of a mutual pair takes its partner's bank (SA_KEEP_LATEST)
//   k_consolidate_merge_best  the same under SA_KEEP_BEST
// The moves themselves are the absorb's (sa_bank_move.h).  After the call's wait for its outputs the host derives the pairs from
// them, replays the rule on its tables and removes the sources in one launch (sa_store_remove_slots, sa_handover.hip).
//
// Reference: examples/track_merging.rs (every track's best match inside one store, Track::merge into it).
#include "sa_bank_move.h"
#include "sa_compat.h"
#include "sa_merge_plan.h"
#include "sa_store.h"

#include <vector>

namespace {

constexpr uint32_t CO_THREADS = 256, CO_WAVES = CO_THREADS / 64;

// Track t names a partner iff its row has an entry and entry 0's winner is not t itself: the winner is then the stored id whose claim
// t holds (similari_bestfit.h, 10b).  The walk over d_ids is k_absorb_match's.
__global__ __launch_bounds__(CO_THREADS) void k_consolidate_pair(const uint32_t* __restrict__ o_n, const uint64_t* __restrict__ o_id,
                                                                 const uint64_t* __restrict__ s_ids, uint32_t T, uint32_t topn,
                                                                 uint32_t* __restrict__ partner) {
  const uint32_t t = blockIdx.x * CO_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (t >= T) return;
  const uint64_t own = s_ids[t];
  const uint64_t w = o_n[t] ? o_id[(size_t)t * topn] : own;
  uint32_t found = SA_SEARCH_NONE;
  if (w != own) found = sa_bank_find_slot(w, s_ids, T, lane);
  if (lane == 0) partner[t] = found;
}

// Wave t acts iff t and p = partner[t] name each other and t holds the lower id; *src: p.  Wave-uniform.
// Ownership (sa_bank_move.h asks for it).  partner is a function of the slot, so t's partner p names at most one track back: the
// acting pairs are disjoint.  Bank t is written by wave t alone.  It could be read only by a wave whose partner is t and whom t names
// back — wave p —, and wave p is idle, because id[p] > id[t].  Bank p is written by nobody for the same reason, and read by wave t
// alone.  d_nobs[t] and d_qual of bank t follow their bank.  So the source rows of the absorb's moves may be another bank of the
// same arrays, and the pointers carry no __restrict__.
__device__ __forceinline__ bool consolidate_acts(const uint32_t* __restrict__ partner, const uint64_t* __restrict__ s_ids, uint32_t T,
                                                 uint32_t t, uint32_t* src) {
  const uint32_t p = partner[t];
  if (p >= T) return false;   // SA_SEARCH_NONE among it
  if (partner[p] != t || !(s_ids[t] < s_ids[p])) return false;
  *src = p;
  return true;
}

// SA_KEEP_LATEST: bank t ++ bank p at capacity C, k_absorb_move's shift.  The rule runs whatever the counts are, as sa_store_merge
// runs it.  Rows are 16-byte pieces of row_floats(), so one kernel serves f32, f16, bf16 and i8 stores; norms move with rows.
__global__ __launch_bounds__(CO_THREADS) void k_consolidate_merge(const uint32_t* __restrict__ partner, const uint64_t* __restrict__ s_ids,
                                                                  uint32_t T, uint32_t C, uint32_t Kp, uint32_t Dp, float* s_feat,
                                                                  float* s_norm, uint32_t* d_nobs) {
  const uint32_t t = blockIdx.x * CO_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (t >= T) return;
  uint32_t p;
  if (!consolidate_acts(partner, s_ids, T, t, &p)) return;
  const uint32_t keep = sa_bank_take_latest(lane, false, d_nobs[t], d_nobs[p], C, Kp, Dp, s_feat, s_norm, (size_t)p * Kp, s_feat, s_norm,
                                            (size_t)t * Kp);
  if (lane == 0) d_nobs[t] = keep;
}

// SA_KEEP_BEST: k_absorb_move_best's rank-and-permute, both banks' qualities from d_qual.
template <uint32_t KP>
__global__ __launch_bounds__(CO_THREADS) void k_consolidate_merge_best(const uint32_t* __restrict__ partner, const uint64_t* __restrict__ s_ids,
                                                                       uint32_t T, uint32_t C, uint32_t Dp, float* s_feat, float* s_norm,
                                                                       float* s_qual, uint32_t* d_nobs) {
  // the wave's number is the same in every lane (k_absorb_move_best says why the compiler is told)
  const uint32_t t = blockIdx.x * CO_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (t >= T) return;
  uint32_t p;
  if (!consolidate_acts(partner, s_ids, T, t, &p)) return;
  p = __builtin_amdgcn_readfirstlane(p);
  const uint32_t keep = sa_bank_take_best<KP>(lane, false, d_nobs[t], d_nobs[p], C, Dp, s_feat, s_norm, s_qual, (size_t)p * KP, s_feat, s_norm,
                                              s_qual, (size_t)t * KP);
  if (lane == 0) d_nobs[t] = keep;
}

using MergeBest = void (*)(const uint32_t*, const uint64_t*, uint32_t, uint32_t, uint32_t, float*, float*, float*, uint32_t*);
MergeBest merge_best(uint32_t lgK) {   // Kp = 1 << lgK, at most 32 (sa_store_create_as)
  static const MergeBest form[6] = {k_consolidate_merge_best<1>, k_consolidate_merge_best<2>,  k_consolidate_merge_best<4>,
                                    k_consolidate_merge_best<8>, k_consolidate_merge_best<16>, k_consolidate_merge_best<32>};
  return lgK < 6 ? form[lgK] : nullptr;
}

uint32_t wave_blocks(uint32_t n) { return (n + CO_WAVES - 1) / CO_WAVES; }

}  // namespace

extern "C" {

int sa_store_consolidate(sa_store* s, uint32_t keep, const sa_topn_params* p, const sa_compat* c, uint32_t capacity, uint32_t* out_n,
                         uint64_t* out_winner, uint64_t* out_track, double* out_weight, uint64_t* out_ids, uint64_t* out_dest) {
  const char* what = "sa_store_consolidate";
  if (!s) return SA_ERR_BAD_ARG;
  s->consolidate_last = sa_consolidate_stats{};
  SA_TRY(sa_store_enter(s, what));
  if (keep != SA_KEEP_LATEST && keep != SA_KEEP_BEST) return sa_engine_fail(s->e, SA_ERR_BAD_ARG, "%s: unknown keep %u", what, keep);
  const bool best = keep == SA_KEEP_BEST;
  const uint32_t C = capacity ? capacity : s->K;
  bool queued = false;
  uint64_t uploaded = 0;
  SaAbsorbStep step;
  // behind the join's own checks
  step.check = [&]() -> int {
    sa_engine* e = s->e;
    if (!out_dest) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
    if (capacity > s->K) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: capacity %u (0, or 1..%u)", what, capacity, s->K);
    if (c && (c->flags & SA_COMPAT_QUERY_FIRST))
      return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: SA_COMPAT_QUERY_FIRST is asymmetric, no pair can be mutual under it", what);
    return SA_OK;
  };
  step.prepare = [&]() -> int {
    sa_engine* e = s->e;
    SA_TRY(sa_engine_ensure(e, s->ab_slot, (size_t)s->T * 4));
    if (best) {
      if (!merge_best(s->lgK)) return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: no move for %u observations per track", what, s->K);
      SA_TRY(sa_engine_ensure(e, s->d_qual, (size_t)s->cap * s->Kp * 4));   // grows only behind a reservation, which marked it stale
    }
    return SA_OK;
  };
  step.queue = [&](bool) -> int {   // a join votes or does not run at all
    sa_engine* e = s->e;
    hipStream_t st = s->st;
    queued = true;
    const uint32_t T = s->T;
    uint32_t* partner = (uint32_t*)s->ab_slot.p;
    if (best && s->qual_dirty) {   // the table as it stands, ahead of the step
      uploaded = (uint64_t)T * s->Kp * 4;
      SA_HIPCHK(e, hipMemcpyAsync(s->d_qual.p, s->qual.data(), (size_t)uploaded, hipMemcpyHostToDevice, st));
    }
    SA_HIPCHK(e, hipEventRecord(s->ev[6], st));
    hipLaunchKernelGGL(k_consolidate_pair, dim3(wave_blocks(T)), dim3(CO_THREADS), 0, st, (const uint32_t*)s->o_n.p, (const uint64_t*)s->o_id.p,
                       (const uint64_t*)s->d_ids.p, T, p->topn, partner);
    SA_HIPCHK(e, hipGetLastError());
    if (best)
      hipLaunchKernelGGL(merge_best(s->lgK), dim3(wave_blocks(T)), dim3(CO_THREADS), 0, st, (const uint32_t*)partner, (const uint64_t*)s->d_ids.p,
                         T, C, s->row_floats(), (float*)s->feat.p, (float*)s->norm.p, (float*)s->d_qual.p, (uint32_t*)s->d_nobs.p);
    else
      hipLaunchKernelGGL(k_consolidate_merge, dim3(wave_blocks(T)), dim3(CO_THREADS), 0, st, (const uint32_t*)partner,
                         (const uint64_t*)s->d_ids.p, T, C, s->Kp, s->row_floats(), (float*)s->feat.p, (float*)s->norm.p, (uint32_t*)s->d_nobs.p);
    SA_HIPCHK(e, hipGetLastError());
    SA_HIPCHK(e, hipEventRecord(s->ev[7], st));
    return SA_OK;
  };
  const SaBestFit fit{out_track, &step};
  const int rc = sa_store_join_topn_impl(s, what, p, c != nullptr, c, out_n, out_winner, out_weight, nullptr, &fit);
  if (rc != SA_OK) {
    if (queued) s->broken = true;   // the banks may have moved while the tables have not
    return rc;
  }
  const uint32_t T = s->T, Kp = s->Kp, topn = p->topn;
  const std::vector<uint64_t> ids = s->ids;   // the order of before the call
  if (out_ids) std::copy(ids.begin(), ids.end(), out_ids);
  std::copy(ids.begin(), ids.end(), out_dest);
  if (!queued) return SA_OK;   // an empty store
  // The pairs as the merge kernel found them, from the outputs: partner[] is slot_of here.
  auto names = [&](uint32_t a) { return out_n[a] >= 1 ? out_winner[(size_t)a * topn] : ids[a]; };
  std::vector<uint32_t> dsts, srcs;
  for (uint32_t a = 0; a < T; ++a) {
    const uint64_t w = names(a);
    if (w == ids[a]) continue;
    const auto it = s->slot_of.find(w);
    if (it == s->slot_of.end()) {
      s->broken = true;
      return sa_engine_fail(s->e, SA_ERR_STATE, "%s: the vote named %llu, which the store does not hold", what, (unsigned long long)w);
    }
    const uint32_t b = it->second;
    if (names(b) != ids[a] || !(ids[a] < w)) continue;
    dsts.push_back(a);
    srcs.push_back(b);
    out_dest[b] = ids[a];
  }
  if (dsts.empty()) return SA_OK;   // nothing moved on the device either; the mirror, if it went up, holds the table and stays marked as it was
  // The host tables take the same rule, destination by destination (sa_store_merge_impl's loop for one source each).
  sa_consolidate_stats st{};
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, s->ev[6], s->ev[7]) != hipSuccess) {
    s->broken = true;   // the banks have moved and the tables have not
    return sa_engine_fail(s->e, SA_ERR_HIP, "%s: hipEventElapsedTime failed", what);
  }
  std::vector<float> bank;
  std::vector<SaMergeObs> obs;
  for (size_t i = 0; i < dsts.size(); ++i) {
    const uint32_t a = dsts[i], b = srcs[i];
    if (c) s->attrs[a] = sa_compat_union(s->attrs[a], s->attrs[b]);
    const uint32_t n0 = s->nobs[a], n1 = s->nobs[b];
    const uint32_t tot = n0 + n1, kept = tot < C ? tot : C, drop = tot - kept;
    float* ql = s->qual.data() + (size_t)a * Kp;
    const float* qs = s->qual.data() + (size_t)b * Kp;
    bank.assign(ql, ql + n0);
    bank.insert(bank.end(), qs, qs + n1);
    if (best) {   // a row whose rank is its own position is not moved
      obs.clear();
      for (uint32_t k = 0; k < tot; ++k) obs.push_back({k, bank[k]});
      const std::vector<uint32_t> sel = sa_merge_select(SA_KEEP_BEST, C, obs);
      uint32_t stay = 0;
      for (uint32_t j = 0; j < kept; ++j) stay += sel[j] == j && j < n0 ? 1u : 0u;
      for (uint32_t j = 0; j < Kp; ++j) ql[j] = j < kept ? bank[sel[j]] : 0.f;
      st.rows_moved += kept - stay;
    } else {
      for (uint32_t j = 0; j < Kp; ++j) ql[j] = j < kept ? bank[drop + j] : 0.f;
      st.rows_moved += drop ? kept : n1;
    }
    st.rows_moved += n0 > kept ? n0 - kept : 0u;
    s->nobs[a] = kept;
  }
  s->qual_dirty = true;   // the compaction below moves the table, not the mirror
  if (c) s->attrs_dirty = true;
  st.step_ms = ms;
  st.pairs = (uint32_t)dsts.size();
  st.keep = keep;
  st.qual_upload_bytes = uploaded;
  uint32_t compact = 0;
  SA_TRY(sa_store_remove_slots(s, srcs, true, &compact, &st.tracks_moved, &st.compact_ms));
  if (!compact) st.compact_ms = 0.0;   // no track moved: the two events enclose no launch
  st.launches = 2u + compact;
  st.host_waits = s->last.reruns + 3u;   // one per run of the join for the pool's cursor, one behind the copies out, one behind the compaction
  s->consolidate_last = st;
  return SA_OK;
}

int sa_store_consolidate_last(sa_store* s, sa_consolidate_stats* out) {
  if (!s || !out) return SA_ERR_BAD_ARG;
  *out = s->consolidate_last;
  return SA_OK;
}

}  // extern "C"
