// sa_search.hip — track search (include/similari_search.h): the device-resident feature store, the host side of a search and its
// second launch under the TopN vote (weights + top-N, one workgroup per query; the BestFit vote's second stage is
// sa_bestfit.hip's).  The first launch, the contraction with the group epilogue, lives in
// sa_gemm.hip beside k_cosine_matrix, whose main loops it runs (k_search_tile, sa_launch_search_tiles).  Here too: what every call on
// a store shares — the prologue of the three searches (sa_store_search_begin), the id checks (sa_store_check_ids) and the slot table
// (sa_store::slot_*).  Device buffers, the stream and the error slot are the engine's (sa_engine_ensure, sa_engine_drain,
// sa_engine_fail).
//
// Reference: TrackStore::foreign_track_distances (src/track/store.rs:429-460, worker loop :199-240), Track::distances
// (src/track.rs:604-652), TopNVoting::winners (src/track/voting/topn.rs:82-135).
#include "sa_store.h"
#include "sa_vote_weight.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_set>
#include <vector>

namespace {

constexpr uint32_t TOPN_THREADS = SA_VOTE_THREADS;
constexpr uint32_t TOPN_MAX = SA_TOPN_MAX;
constexpr uint32_t TOPN_LDS_CAND = SA_VOTE_LDS_CAND;   // surviving groups of one query that launch 2 keeps in LDS (40 KB); beyond, it re-reads grp
constexpr uint32_t POOL_BLOCKS0 = 256;     // pool blocks a store starts with

// Launch 2: one workgroup per query.  The query's row of grp is scanned first (eight loads in flight per thread) and its surviving
// groups are gathered into LDS, so that the block sums then run side by side — one group per thread — instead of once per scan step
// in which some lane of a wave happens to meet a group.  Then at most topn rounds of a workgroup arg-max under (weight desc, id asc),
// each over the candidates that rank after the previous pick.  A query with more than TOPN_LDS_CAND groups takes the same steps from
// global memory (weights through wscr).
// JOIN (k_topn<true>): query q is stored track q, and the block of (q, s) holds q's observations as rows when q < s and as columns
// otherwise; a block then serves two queries, whose sums differ in order, so wscr keeps two weights per block.
template <bool JOIN>
__device__ __forceinline__ void topn_body(const uint32_t* __restrict__ grp, const float* __restrict__ pool,
                                          const uint32_t* __restrict__ ctrl, uint32_t pool_cap, const uint64_t* __restrict__ s_ids,
                                          uint32_t T, uint32_t Kp, uint32_t topn, double* __restrict__ wscr,
                                          uint32_t* __restrict__ out_n, uint64_t* __restrict__ out_id, double* __restrict__ out_w) {
  constexpr uint32_t NT = TOPN_THREADS, NW = NT / 64, SCAN_U = 8;
  __shared__ double s_w[NW];
  __shared__ uint64_t s_id[NW];
  __shared__ uint32_t c_b[TOPN_LDS_CAND], c_s[TOPN_LDS_CAND];
  __shared__ double c_w[TOPN_LDS_CAND];
  __shared__ uint64_t c_id[TOPN_LDS_CAND];
  __shared__ uint32_t c_n;
  const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint64_t* oid = out_id + (size_t)q * topn;
  double* ow = out_w + (size_t)q * topn;
  if (ctrl[0] > pool_cap) {   // the pool overflowed and some blocks were not written: the host grows it and searches again
    if (tid == 0) out_n[q] = 0;
    return;
  }
  if (tid == 0) c_n = 0;
  __syncthreads();
  const float M = sa_key_f32(ctrl[1]);
  const uint32_t* g = grp + (size_t)q * T;
  const uint32_t KK = Kp * Kp;
  for (uint32_t s0 = tid; s0 < T; s0 += SCAN_U * NT) {
    uint32_t b[SCAN_U];
#pragma unroll
    for (uint32_t u = 0; u < SCAN_U; ++u) b[u] = s0 + u * NT < T ? g[s0 + u * NT] : SA_SEARCH_NONE;
#pragma unroll
    for (uint32_t u = 0; u < SCAN_U; ++u)
      if (b[u] != SA_SEARCH_NONE) {
        const uint32_t i = atomicAdd(&c_n, 1u);
        if (i < TOPN_LDS_CAND) { c_b[i] = b[u]; c_s[i] = s0 + u * NT; }
      }
  }
  __syncthreads();
  const uint32_t nc = c_n;
  const bool in_lds = nc <= TOPN_LDS_CAND;
  if (in_lds) {
    for (uint32_t i = tid; i < nc; i += NT) {
      if (JOIN && q > c_s[i]) c_w[i] = block_weight_t(pool + (size_t)c_b[i] * KK, Kp, M);
      else c_w[i] = block_weight(pool + (size_t)c_b[i] * KK, KK, M);
      c_id[i] = s_ids[c_s[i]];
    }
  } else {
    for (uint32_t s = tid; s < T; s += NT) {
      const uint32_t b = g[s];
      if (b == SA_SEARCH_NONE) continue;
      if (!JOIN) wscr[b] = block_weight(pool + (size_t)b * KK, KK, M);
      else if (q > s) wscr[2 * (size_t)b + 1] = block_weight_t(pool + (size_t)b * KK, Kp, M);
      else wscr[2 * (size_t)b] = block_weight(pool + (size_t)b * KK, KK, M);
    }
  }
  __syncthreads();
  double pw = 0.0;
  uint64_t pid = 0;
  uint32_t n = 0;
  for (; n < topn; ++n) {
    double bw = 0.0;
    uint64_t bid = 0;   // 0: none (ids are non-zero)
    auto consider = [&](double w, uint64_t id) {
      if (n > 0 && !ranks_before(pw, pid, w, id)) return;   // picked already
      if (bid == 0 || ranks_before(w, id, bw, bid)) { bw = w; bid = id; }
    };
    if (in_lds) {
      for (uint32_t i = tid; i < nc; i += NT) consider(c_w[i], c_id[i]);
    } else {
      for (uint32_t s = tid; s < T; s += NT) {
        const uint32_t b = g[s];
        if (b != SA_SEARCH_NONE) consider(JOIN ? wscr[2 * (size_t)b + (q > s ? 1u : 0u)] : wscr[b], s_ids[s]);
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double xw = __shfl_xor(bw, o);
      const uint64_t xid = __shfl_xor(bid, o);
      if (xid != 0 && (bid == 0 || ranks_before(xw, xid, bw, bid))) { bw = xw; bid = xid; }
    }
    if (lane == 0) { s_w[wave] = bw; s_id[wave] = bid; }
    __syncthreads();
    bw = s_w[0];
    bid = s_id[0];
    for (uint32_t w = 1; w < NW; ++w)
      if (s_id[w] != 0 && (bid == 0 || ranks_before(s_w[w], s_id[w], bw, bid))) { bw = s_w[w]; bid = s_id[w]; }
    __syncthreads();   // s_w / s_id are rewritten in the next round
    if (bid == 0) break;
    if (tid == 0) { oid[n] = bid; ow[n] = bw; }
    pw = bw;
    pid = bid;
  }
  if (tid == 0) {
    out_n[q] = n;
    for (uint32_t r = n; r < topn; ++r) { oid[r] = 0; ow[r] = 0.0; }
  }
}

template <bool JOIN>
__global__ __launch_bounds__(TOPN_THREADS) void k_topn(const uint32_t* __restrict__ grp, const float* __restrict__ pool,
                                                       const uint32_t* __restrict__ ctrl, uint32_t pool_cap,
                                                       const uint64_t* __restrict__ s_ids, uint32_t T, uint32_t Kp, uint32_t topn,
                                                       double* __restrict__ wscr, uint32_t* __restrict__ out_n,
                                                       uint64_t* __restrict__ out_id, double* __restrict__ out_w) {
  topn_body<JOIN>(grp, pool, ctrl, pool_cap, s_ids, T, Kp, topn, wscr, out_n, out_id, out_w);
}

}  // namespace

int sa_store_enter(sa_store* s, const char* what) {
  if (!s->e) return sa_engine_fail(nullptr, SA_ERR_STATE, "%s: the store's engine was destroyed before it", what);
  if (s->broken) return sa_engine_fail(s->e, SA_ERR_STATE, "%s: an earlier device call failed half-way; destroy the store", what);
  return sa_engine_drain(s->e, &s->device, &s->st);
}

int sa_store_check_ids(sa_store* s, const char* what, uint32_t n, const uint64_t* ids, uint32_t* slots,
                       const std::function<int(uint32_t)>& each) {
  std::unordered_set<uint64_t> seen;
  seen.reserve((size_t)n * 2u);
  for (uint32_t i = 0; i < n; ++i) {
    if (ids[i] == 0) return sa_engine_fail(s->e, SA_ERR_BAD_ARG, "%s: id 0 at %u", what, i);
    if (!seen.insert(ids[i]).second)
      return sa_engine_fail(s->e, SA_ERR_BAD_ARG, "%s: id %llu twice in one call", what, (unsigned long long)ids[i]);
    if (slots) {
      const auto it = s->slot_of.find(ids[i]);
      slots[i] = it == s->slot_of.end() ? SA_SEARCH_NONE : it->second;
    }
    if (each) SA_TRY(each(i));
  }
  return SA_OK;
}

// ---- the slot table: ids, nobs, qual, attrs and slot_of change together, here and nowhere else ----
uint32_t sa_store::slot_append(uint64_t id) {
  const uint32_t slot = T++;
  ids.push_back(id);
  nobs.push_back(0);
  qual.resize((size_t)T * Kp, 0.f);
  qual_dirty = true;
  attrs.push_back(sa_track_attrs{0, 0, 0});
  attrs_dirty = true;
  slot_of.emplace(id, slot);
  return slot;
}

void sa_store::slot_move(uint32_t from, uint32_t to) {
  ids[to] = ids[from];
  nobs[to] = nobs[from];
  attrs[to] = attrs[from];
  std::copy_n(qual.begin() + (size_t)from * Kp, Kp, qual.begin() + (size_t)to * Kp);
  qual_dirty = true;
  slot_of[ids[to]] = to;
}

void sa_store::slot_truncate(uint32_t T1) {
  T = T1;
  ids.resize(T);
  nobs.resize(T);
  attrs.resize(T);
  attrs_dirty = true;
  qual.resize((size_t)T * Kp);
  qual_dirty = true;
}

namespace {

// ids with their observation counts, as an upsert and a search take them: the checks every id list gets, at most K observations each
int check_ids(sa_store* s, uint32_t n, const uint64_t* ids, const uint32_t* n_obs, size_t* total, const char* what) {
  *total = 0;
  return sa_store_check_ids(s, what, n, ids, nullptr, [&](uint32_t i) {
    if (n_obs[i] > s->K)
      return sa_engine_fail(s->e, SA_ERR_BAD_ARG, "%s: %u observations for id %llu (max_observations %u)", what, n_obs[i],
                            (unsigned long long)ids[i], s->K);
    *total += n_obs[i];
    return (int)SA_OK;
  });
}

void release(sa_store* s) {
  for (DevBuf* b : {&s->feat, &s->norm, &s->d_ids, &s->d_nobs, &s->stage, &s->up_slots, &s->q_feat,
                    &s->q_norm, &s->q_ids, &s->q_nobs, &s->d_attrs, &s->q_attrs, &s->g_slots, &s->s_out, &s->grp, &s->pool, &s->wscr, &s->ctrl, &s->cells, &s->o_n,
                    &s->o_id, &s->o_w, &s->fit, &s->o_trk, &s->m_new_feat, &s->m_new_norm, &s->m_rows, &s->m_moves, &s->m_feat, &s->m_norm, &s->expand, &s->dr_table, &s->ab_slot, &s->ab_cap, &s->d_qual, &s->ab_qual, &s->w_rows, &s->w_meta, &s->w_table, &s->w_feat})
    sa_engine_free(*b);
  for (auto& ev : s->ev)
    if (ev) { hipEventDestroy(ev); ev = nullptr; }
  for (auto& ev : s->hev)
    if (ev) { hipEventDestroy(ev); ev = nullptr; }
  for (auto& ev : s->wev)
    if (ev) { hipEventDestroy(ev); ev = nullptr; }
}

// the device part of an upsert: after the host tables took the new rows (a failure here leaves the store broken)
int upsert_device(sa_store* s, const SaRows& R, const std::vector<uint32_t>& slots) {
  SA_HIPCHK(s->e, hipMemcpyAsync(s->up_slots.p, slots.data(), slots.size() * 4, hipMemcpyHostToDevice, s->st));
  SA_TRY(sa_rows_fill(s, R, s->Kp, (const uint32_t*)s->up_slots.p, s->feat.p, (float*)s->norm.p));
  SA_TRY(sa_store_upload_table(s));
  SA_HIPCHK(s->e, hipStreamSynchronize(s->st));
  return SA_OK;
}

}  // namespace

int sa_store_upload_table(sa_store* s) {
  if (!s->T) return SA_OK;
  SA_HIPCHK(s->e, hipMemcpyAsync(s->d_ids.p, s->ids.data(), (size_t)s->T * 8, hipMemcpyHostToDevice, s->st));
  SA_HIPCHK(s->e, hipMemcpyAsync(s->d_nobs.p, s->nobs.data(), (size_t)s->T * 4, hipMemcpyHostToDevice, s->st));
  return SA_OK;
}

int sa_store_reserve(sa_store* s, uint64_t T1) {
  if (T1 <= s->cap) return SA_OK;
  const size_t bank_bytes = s->Kp * s->row_bytes();
  uint64_t ncap = s->cap ? (uint64_t)s->cap * 2 : 64;
  while (ncap < T1) ncap *= 2;
  if (ncap > SA_STORE_MAX_SLOTS / s->Kp) ncap = SA_STORE_MAX_SLOTS / s->Kp;
  SA_TRY(sa_engine_ensure(s->e, s->feat, ncap * bank_bytes, true));
  SA_TRY(sa_engine_ensure(s->e, s->norm, ncap * s->Kp * 4, true));
  SA_TRY(sa_engine_ensure(s->e, s->d_ids, ncap * 8, true));
  SA_TRY(sa_engine_ensure(s->e, s->d_nobs, ncap * 4, true));
  s->cap = (uint32_t)ncap;
  s->qual_dirty = true;   // d_qual is sized by cap and does not move along: the next SA_KEEP_BEST absorb uploads the table
  return SA_OK;
}

// ---- what every search shares (sa_store.h): sa_store_search_topn below, the gallery calls in sa_gallery.hip ----
int sa_store_check_params(sa_store* s, const sa_topn_params* p, const char* what) {
  sa_engine* e = s->e;
  if (!p) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null params", what);
  if (p->topn > TOPN_MAX) return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: topn %u > %u", what, p->topn, TOPN_MAX);
  if (p->topn == 0) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: topn must be >= 1", what);
  if (std::isnan(p->max_distance) || std::isnan(p->keep_below))
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: max_distance and keep_below must not be NaN", what);
  return SA_OK;
}

int sa_store_search_buffers(sa_store* s, uint32_t Q, uint32_t topn, bool tap, bool join, const SaBestFit* fit) {
  sa_engine* e = s->e;
  const size_t KK = (size_t)s->Kp * s->Kp;
  SA_TRY(sa_engine_ensure(e, s->grp, (size_t)Q * s->T * 4));
  SA_TRY(sa_engine_ensure(e, s->ctrl, sizeof s->h_ctrl));
  if (s->expands()) SA_TRY(sa_engine_ensure(e, s->expand, sizeof s->h_expand));
  SA_TRY(sa_engine_ensure(e, s->o_n, (size_t)Q * 4));
  SA_TRY(sa_engine_ensure(e, s->o_id, (size_t)Q * topn * 8));
  SA_TRY(sa_engine_ensure(e, s->o_w, (size_t)Q * topn * 8));
  if (tap) SA_TRY(sa_engine_ensure(e, s->cells, (size_t)Q * s->K * s->T * s->K * 4));
  if (fit) SA_TRY(sa_bestfit_buffers(s, Q, topn));
  if (!s->pool_cap) {
    SA_TRY(sa_engine_ensure(e, s->pool, POOL_BLOCKS0 * KK * 4));
    s->pool_cap = POOL_BLOCKS0;
  }
  return sa_engine_ensure(e, s->wscr, (size_t)s->pool_cap * (join ? 16 : 8));   // a join keeps two weights per block (k_topn<true>)
}

int sa_store_search_run(sa_store* s, const sa_topn_params* p, const char* what, uint32_t Q, bool join, const uint8_t* s_out,
                        uint32_t* out_n, uint64_t* out_winner, double* out_weight, float* out_cells, const sa_compat* compat,
                        const SaBestFit* fit) {
  sa_engine* e = s->e;
  const size_t ctrl_bytes = compat ? 12 : 8;   // a compat search also counts the tiles that left early
  hipStream_t st = s->st;
  const uint32_t T = s->T, topn = p->topn, Kp = s->Kp, K = s->K;
  const size_t KK = (size_t)Kp * Kp;
  uint32_t run = 0;
  for (;; ++run) {
    s->h_ctrl[0] = 0;
    s->h_ctrl[1] = sa_f32_key(-1.0f);
    s->h_ctrl[2] = 0;
    SA_HIPCHK(e, hipMemcpyAsync(s->ctrl.p, s->h_ctrl, ctrl_bytes, hipMemcpyHostToDevice, st));
    if (fit) SA_TRY(sa_bestfit_reset(s));
    SaExpandArgs x{};
    if (s->expands()) {   // rho = 5e-3 sqrt(Dp) (include/similari_f16.h); the counters start at zero, in a rerun too
      x.rho = 5e-3f * std::sqrt((float)s->Dp);
      x.ctr = (unsigned long long*)s->expand.p;
      SA_HIPCHK(e, hipMemsetAsync(s->expand.p, 0, sizeof s->h_expand, st));
    }
    SaSearchArgs a{};
    a.q_feat = (const float*)(join ? s->feat.p : s->q_feat.p);
    a.q_norm = (const float*)(join ? s->norm.p : s->q_norm.p);
    a.s_feat = (const float*)s->feat.p;
    a.s_norm = (const float*)s->norm.p;
    a.q_nobs = (const uint32_t*)(join ? s->d_nobs.p : s->q_nobs.p);
    a.q_ids = (const uint64_t*)(join ? s->d_ids.p : s->q_ids.p);
    a.s_nobs = (const uint32_t*)s->d_nobs.p;
    a.s_ids = (const uint64_t*)s->d_ids.p;
    a.Q = Q;
    a.T = T;
    a.Dp = s->Dp;   // in elements
    a.Kp = Kp;
    a.lgK = s->lgK;
    a.K = K;
    a.min_votes = p->min_votes ? p->min_votes : 1u;
    a.max_distance = p->max_distance;
    a.keep_below = p->keep_below;
    a.grp = (uint32_t*)s->grp.p;
    a.pool = (float*)s->pool.p;
    a.pool_cap = s->pool_cap;
    a.ctrl = (uint32_t*)s->ctrl.p;
    a.cells = out_cells ? (float*)s->cells.p : nullptr;
    a.s_out = s_out;
    SA_HIPCHK(e, hipEventRecord(s->ev[1], st));
    SaCompatArgs c{};
    if (compat) {
      c.q_attrs = (const sa_track_attrs*)(join ? s->d_attrs.p : s->q_attrs.p);
      c.s_attrs = (const sa_track_attrs*)s->d_attrs.p;
      c.ready_at = compat->ready_at;
      c.flags = compat->flags;
    }
    SaSearchTiles tiles{};
    const hipError_t h1 = sa_launch_search_tiles(s->kind, join, a, compat ? &c : nullptr, st, &tiles, s->elem, &x);
    if (join) {
      s->join_tiles = tiles.tiles;
      s->join_tiles_rect = tiles.tiles_rect;
    }
    if (compat) s->compat_last.tiles = tiles.tiles;
    SA_HIPCHK(e, h1);
    SA_HIPCHK(e, hipEventRecord(s->ev[2], st));
    if (fit) {   // the BestFit vote: three launches over the same grp, pool and ctrl (sa_bestfit.hip)
      SA_TRY(sa_bestfit_launch(s, join, Q, topn, a.q_ids));
    } else {
      hipLaunchKernelGGL(join ? k_topn<true> : k_topn<false>, dim3(Q), dim3(TOPN_THREADS), 0, st, (const uint32_t*)s->grp.p,
                         (const float*)s->pool.p, (const uint32_t*)s->ctrl.p, s->pool_cap, (const uint64_t*)s->d_ids.p, T, Kp, topn,
                         (double*)s->wscr.p, (uint32_t*)s->o_n.p, (uint64_t*)s->o_id.p, (double*)s->o_w.p);
      SA_HIPCHK(e, hipGetLastError());
    }
    SA_HIPCHK(e, hipEventRecord(s->ev[3], st));
    SA_HIPCHK(e, hipMemcpyAsync(s->h_ctrl, s->ctrl.p, ctrl_bytes, hipMemcpyDeviceToHost, st));
    if (fit) SA_HIPCHK(e, hipMemcpyAsync(s->h_fit, (const uint64_t*)s->fit.p + 2 * (size_t)T, sizeof s->h_fit, hipMemcpyDeviceToHost, st));
    if (x.ctr) SA_HIPCHK(e, hipMemcpyAsync(s->h_expand, s->expand.p, sizeof s->h_expand, hipMemcpyDeviceToHost, st));
    SA_HIPCHK(e, hipStreamSynchronize(st));
    if (compat) s->compat_last.tiles_skipped = s->h_ctrl[2];
    if (s->h_ctrl[0] <= s->pool_cap) break;
    if (run > 0) return sa_engine_fail(e, SA_ERR_STATE, "%s: %u groups after growing the pool to %u", what, s->h_ctrl[0], s->pool_cap);
    // the pool overflowed: the cursor counted every surviving group (at most Q * T < 2^32 - 1, sa_search_limits.h).  Grow with a
    // quarter of slack, as the engine's buffers do, so that searches a little larger than this one fit, and run both launches again.
    const uint64_t want = (uint64_t)s->h_ctrl[0] + s->h_ctrl[0] / 4;
    const uint32_t ncap = (uint32_t)(want < SA_SEARCH_MAX_PAIRS ? want : SA_SEARCH_MAX_PAIRS);
    SA_TRY(sa_engine_ensure(e, s->pool, (size_t)ncap * KK * 4));
    SA_TRY(sa_engine_ensure(e, s->wscr, (size_t)ncap * (join ? 16 : 8)));
    s->pool_cap = ncap;
  }
  float ms1 = 0.f, ms2 = 0.f, msc = 0.f;
  SA_HIPCHK(e, hipEventElapsedTime(&ms1, s->ev[1], s->ev[2]));
  SA_HIPCHK(e, hipEventElapsedTime(&ms2, s->ev[2], s->ev[3]));
  SA_HIPCHK(e, hipEventElapsedTime(&msc, s->ev[0], s->ev[3]));
  if (fit) {   // the three launches of stage 2, whose sum launch2_ms then is
    float w = 0.f, c = 0.f, r = 0.f;
    SA_HIPCHK(e, hipEventElapsedTime(&w, s->ev[2], s->ev[4]));
    SA_HIPCHK(e, hipEventElapsedTime(&c, s->ev[4], s->ev[5]));
    SA_HIPCHK(e, hipEventElapsedTime(&r, s->ev[5], s->ev[3]));
    s->fit_last.weigh_ms = w;
    s->fit_last.claim_ms = c;
    s->fit_last.rank_ms = r;
    s->fit_last.groups = s->h_fit[0];
    s->fit_last.claimed = s->h_fit[1];
    ms2 = w + c + r;
  }
  s->last.launch1_ms = ms1;
  s->last.launch2_ms = ms2;
  s->last.call_ms = msc;
  s->last.groups = s->h_ctrl[0];
  s->last.reruns = run;
  s->last.pool_bytes = s->pool.cap;
  if (join) s->join_blocks = s->h_ctrl[0];
  if (s->expands()) {
    s->expand_last.cells = s->h_expand[0];
    s->expand_last.tiles = s->h_expand[1];
  }
  if (fit && fit->step) SA_TRY(fit->step->queue(true));   // an absorb: its step rides behind the vote of the run that fit, ahead of the last wait
  SA_HIPCHK(e, hipMemcpyAsync(out_n, s->o_n.p, (size_t)Q * 4, hipMemcpyDeviceToHost, st));
  SA_HIPCHK(e, hipMemcpyAsync(out_winner, s->o_id.p, (size_t)Q * topn * 8, hipMemcpyDeviceToHost, st));
  SA_HIPCHK(e, hipMemcpyAsync(out_weight, s->o_w.p, (size_t)Q * topn * 8, hipMemcpyDeviceToHost, st));
  if (fit && fit->out_track) SA_HIPCHK(e, hipMemcpyAsync(fit->out_track, s->o_trk.p, (size_t)Q * topn * 8, hipMemcpyDeviceToHost, st));
  if (out_cells) SA_HIPCHK(e, hipMemcpyAsync(out_cells, s->cells.p, (size_t)Q * K * T * K * 4, hipMemcpyDeviceToHost, st));
  SA_HIPCHK(e, hipStreamSynchronize(st));
  return SA_OK;
}

// sa_engine_destroy: the engine goes first — free what the store holds on its device, refuse every later call
void sa_store_orphan(sa_store* s) {
  release(s);
  s->e = nullptr;
}

extern "C" {

void sa_store_options_default(sa_store_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->struct_size = sizeof *o;
  o->visual_kind = SA_VIS_COSINE;
  o->feature_len = 0;
  o->max_observations = 1;
}

int sa_store_create(sa_engine* e, const sa_store_options* o, sa_store** out) {
  return sa_store_create_as(e, o, SA_ELEM_F32, "sa_store_create", out);
}

}  // extern "C"

int sa_store_create_as(sa_engine* e, const sa_store_options* o, int32_t elem, const char* what, sa_store** out) {
  if (out) *out = nullptr;
  if (!e) {
    // no engine: without a gfx950 device there cannot be one — say so, as sa_engine_create does
    int count = 0;
    const hipError_t h = hipGetDeviceCount(&count);
    if (h != hipSuccess || count <= 0) {
      (void)hipGetLastError();
      return sa_engine_fail(nullptr, SA_ERR_NO_DEVICE, "no HIP device visible; the feature store has no CPU fallback");
    }
    bool gfx950 = false;
    for (int d = 0; d < count && !gfx950; ++d) {
      hipDeviceProp_t prop;
      gfx950 = hipGetDeviceProperties(&prop, d) == hipSuccess && std::strstr(prop.gcnArchName, "gfx950");
    }
    if (!gfx950) return sa_engine_fail(nullptr, SA_ERR_NO_DEVICE, "no gfx950 device; the feature store has no CPU fallback");
    return sa_engine_fail(nullptr, SA_ERR_BAD_ARG, "%s: null engine", what);
  }
  if (!o || !out) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
  if (o->struct_size < sizeof(sa_store_options)) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: struct_size too small", what);
  if (o->visual_kind != SA_VIS_COSINE && o->visual_kind != SA_VIS_EUCLIDEAN)
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: visual_kind must be cosine or euclidean", what);
  if (o->feature_len == 0 || o->max_observations == 0)
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: feature_len and max_observations must be > 0", what);
  if (o->max_observations > 32) return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: at most 32 observations per track", what);
  if (const int x = sa_search_extent(0, 0, 1, o->feature_len))
    return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: %s", what, sa_search_extent_text(x));
  sa_store* s = new sa_store();
  s->e = e;
  int rc = sa_engine_drain(e, &s->device, &s->st);
  if (rc != SA_OK) { delete s; return rc; }
  s->kind = o->visual_kind;
  s->elem = elem;
  s->D = o->feature_len;
  s->Dp = elem == SA_ELEM_I8 ? (o->feature_len + 63u) / 64u * 64u : (o->feature_len + 31u) / 32u * 32u;   // a row is a multiple of 64 bytes
  s->K = o->max_observations;
  while ((1u << s->lgK) < s->K) ++s->lgK;
  s->Kp = 1u << s->lgK;
  for (auto& ev : s->ev)
    if (hipEventCreate(&ev) != hipSuccess) {
      (void)hipGetLastError();
      release(s);
      delete s;
      return sa_engine_fail(e, SA_ERR_HIP, "%s: hipEventCreate failed", what);
    }
  sa_engine_attach_store(e, s);
  *out = s;
  return SA_OK;
}

extern "C" {

void sa_store_destroy(sa_store* s) {
  if (!s) return;
  if (s->e) {
    hipSetDevice(s->device);
    if (s->st) hipStreamSynchronize(s->st);
    release(s);
    sa_engine_detach_store(s->e, s);
  }
  delete s;
}

int sa_store_upsert(sa_store* s, uint32_t n, const uint64_t* ids, const uint32_t* n_obs, const float* feats) {
  return sa_store_upsert_impl(s, "sa_store_upsert", n, ids, n_obs, SaRowSource::of_host(feats));
}

}  // extern "C"

int sa_store_upsert_impl(sa_store* s, const char* what, uint32_t n, const uint64_t* ids, const uint32_t* n_obs, const SaRowSource& src) {
  if (!s) return SA_ERR_BAD_ARG;
  SA_TRY(sa_store_enter(s, what));
  if (n == 0) return SA_OK;
  if (!ids || !n_obs) return sa_engine_fail(s->e, SA_ERR_BAD_ARG, "%s: null argument", what);
  size_t total = 0;
  SA_TRY(check_ids(s, n, ids, n_obs, &total, what));
  SA_TRY(sa_rows_check(s, what, src, total, "feats"));
  uint32_t fresh = 0;
  for (uint32_t i = 0; i < n; ++i) fresh += s->slot_of.count(ids[i]) ? 0u : 1u;
  const uint64_t T1 = (uint64_t)s->T + fresh;
  if (const int x = sa_search_extent(T1, 0, s->Kp, s->D)) return sa_engine_fail(s->e, SA_ERR_UNSUPPORTED, "%s: %s", what, sa_search_extent_text(x));
  SA_TRY(sa_store_reserve(s, T1));
  SaRows R;   // whatever can fail without the device comes first: a refusal here leaves the store as it was
  SA_TRY(sa_rows_prepare(s, src, n, n_obs, total, true, R));
  SA_TRY(sa_engine_ensure(s->e, s->up_slots, (size_t)n * 4));
  std::vector<uint32_t> slots(n);
  for (uint32_t i = 0; i < n; ++i) {
    const auto it = s->slot_of.find(ids[i]);
    const uint32_t slot = it != s->slot_of.end() ? it->second : s->slot_append(ids[i]);
    s->nobs[slot] = n_obs[i];
    s->qual_dirty = true;
    std::fill_n(s->qual.begin() + (size_t)slot * s->Kp, s->Kp, 0.f);   // an upserted bank carries no qualities (similari_merge.h)
    slots[i] = slot;
  }
  const int rc = upsert_device(s, R, slots);
  if (rc != SA_OK) s->broken = true;
  return rc;
}

extern "C" {

int sa_store_remove(sa_store* s, uint32_t n, const uint64_t* ids) {
  if (!s) return SA_ERR_BAD_ARG;
  SA_TRY(sa_store_enter(s, "sa_store_remove"));
  if (n == 0) return SA_OK;
  if (!ids) return sa_engine_fail(s->e, SA_ERR_BAD_ARG, "sa_store_remove: null ids");
  // The slots that leave, in call order: unknown ids are ignored, and so is an id's second coming (it has left by then).  The last
  // track moves into each hole in turn — the net moves of that, in one launch (sa_store_remove_slots, sa_handover.hip).
  std::vector<uint32_t> slots;
  std::unordered_set<uint32_t> seen;
  for (uint32_t i = 0; i < n; ++i) {
    const auto it = s->slot_of.find(ids[i]);
    if (it != s->slot_of.end() && seen.insert(it->second).second) slots.push_back(it->second);
  }
  s->handover_last = sa_handover_stats{};
  return sa_store_remove_slots(s, slots, false, &s->handover_last.launches_compact, &s->handover_last.tracks_moved,
                               nullptr);
}

int sa_store_count(sa_store* s, uint32_t* out_n) {
  if (!s || !out_n) return SA_ERR_BAD_ARG;
  if (!s->e || s->broken) return sa_store_enter(s, "sa_store_count");
  *out_n = s->T;
  return SA_OK;
}

int sa_store_order(sa_store* s, uint64_t* out_ids, uint32_t cap, uint32_t* out_n) {
  if (!s || !out_n) return SA_ERR_BAD_ARG;
  if (!s->e || s->broken) return sa_store_enter(s, "sa_store_order");
  *out_n = s->T;
  if (out_ids) std::memcpy(out_ids, s->ids.data(), (size_t)(cap < s->T ? cap : s->T) * 8);
  return SA_OK;
}

int sa_store_last_stats(sa_store* s, sa_search_stats* out) {
  if (!s || !out) return SA_ERR_BAD_ARG;
  *out = s->last;
  return SA_OK;
}

int sa_store_search_topn(sa_store* s, const sa_topn_params* p, uint32_t nq, const uint64_t* q_ids, const uint32_t* q_n_obs,
                         const float* q_feats, uint32_t* out_n, uint64_t* out_winner, double* out_weight, float* out_cells) {
  return sa_store_search_topn_impl(s, "sa_store_search_topn", p, false, nullptr, nq, q_ids, q_n_obs, SaRowSource::of_host(q_feats), nullptr, out_n,
                                   out_winner, out_weight, out_cells);
}

int sa_store_search_topn_compat(sa_store* s, const sa_topn_params* p, const sa_compat* c, uint32_t nq, const uint64_t* q_ids,
                                const uint32_t* q_n_obs, const float* q_feats, const sa_track_attrs* q_attrs, uint32_t* out_n,
                                uint64_t* out_winner, double* out_weight, float* out_cells) {
  return sa_store_search_topn_impl(s, "sa_store_search_topn_compat", p, true, c, nq, q_ids, q_n_obs, SaRowSource::of_host(q_feats), q_attrs, out_n,
                                   out_winner, out_weight, out_cells);
}

}  // extern "C"

int sa_store_search_begin(sa_store* s, const SaSearchCall& c, const std::function<int()>& queries, bool* run) {
  *run = false;
  if (!s) return SA_ERR_BAD_ARG;
  const char* what = c.what;
  SA_TRY(sa_store_enter(s, what));
  sa_engine* e = s->e;
  if (c.ruled) SA_TRY(sa_store_check_compat(s, c.compat, what, false));
  SA_TRY(sa_store_check_params(s, c.p, what));
  if (c.ruled) s->compat_last = sa_compat_stats{};
  if (c.bad_flags) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: unknown flag bits 0x%x", what, c.bad_flags);
  const uint32_t Q = c.join ? s->T : c.Q;
  if (!c.join && Q == 0) return SA_OK;
  if (c.null_arg || !c.out_n || !c.out_winner || !c.out_weight) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
  if (c.stray_attrs) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: q_attrs without a rule", what);
  if (queries) SA_TRY(queries());
  if (const int x = sa_search_extent(s->T, Q, s->Kp, s->D)) return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: %s", what, sa_search_extent_text(x));
  s->last = sa_search_stats{};
  s->expand_last = sa_expand_stats{};
  s->last.pool_bytes = s->pool.cap;
  if (c.fit) s->fit_last = sa_bestfit_stats{};
  if (c.join) {
    s->join_tiles = s->join_tiles_rect = 0;
    s->join_blocks = 0;
  }
  if (s->T == 0) {   // nothing stored: no pairs, no groups (a join has no query either and leaves the outputs alone)
    if (c.join) return SA_OK;
    std::memset(c.out_n, 0, (size_t)Q * 4);
    std::memset(c.out_winner, 0, (size_t)Q * c.p->topn * 8);
    std::memset(c.out_weight, 0, (size_t)Q * c.p->topn * 8);
    if (c.fit && c.fit->out_track) std::memset(c.fit->out_track, 0, (size_t)Q * c.p->topn * 8);
    return SA_OK;
  }
  *run = true;
  return SA_OK;
}

int sa_store_search_topn_impl(sa_store* s, const char* what, const sa_topn_params* p, bool ruled, const sa_compat* compat, uint32_t nq,
                              const uint64_t* q_ids, const uint32_t* q_n_obs, const SaRowSource& q_src, const sa_track_attrs* q_attrs,
                              uint32_t* out_n, uint64_t* out_winner, double* out_weight, float* out_cells, const SaBestFit* fit) {
  SaSearchCall c;
  c.what = what, c.p = p, c.ruled = ruled, c.compat = compat, c.Q = nq, c.fit = fit;
  c.null_arg = !q_ids || !q_n_obs || (ruled && !q_attrs);
  c.stray_attrs = fit && !ruled && q_attrs;   // a BestFit call takes both forms through one entry point: q_attrs exactly with a rule
  c.out_n = out_n, c.out_winner = out_winner, c.out_weight = out_weight;
  bool run;
  size_t total = 0;
  SA_TRY(sa_store_search_begin(s, c, [&] {
    SA_TRY(check_ids(s, nq, q_ids, q_n_obs, &total, what));
    SA_TRY(sa_rows_check(s, what, q_src, total, "q_feats"));
    if (ruled)
      for (uint32_t i = 0; i < nq; ++i)
        if (q_attrs[i].start > q_attrs[i].end)
          return sa_engine_fail(s->e, SA_ERR_BAD_ARG, "%s: query %llu starts after it ends", what, (unsigned long long)q_ids[i]);
    if (fit && fit->step) SA_TRY(fit->step->check());
    return (int)SA_OK;
  }, &run));
  // An absorb (sa_absorb.hip) into an empty store searches nothing, yet its step needs the padded queries: the query side is filled as
  // ever and the step queued behind it.
  const SaAbsorbStep* step = fit && nq ? fit->step : nullptr;
  if (step) SA_TRY(step->prepare());
  const bool vote = run;
  if (!vote && !step) return SA_OK;
  sa_engine* e = s->e;
  const uint32_t Q = nq, topn = p->topn, Kp = s->Kp;
  const size_t rows = (size_t)Q * Kp;
  SaRows R;
  SA_TRY(sa_rows_prepare(s, q_src, Q, q_n_obs, total, true, R));
  SA_TRY(sa_engine_ensure(e, s->q_feat, rows * s->row_bytes()));
  SA_TRY(sa_engine_ensure(e, s->q_norm, rows * 4));
  SA_TRY(sa_engine_ensure(e, s->q_ids, (size_t)Q * 8));
  SA_TRY(sa_engine_ensure(e, s->q_nobs, (size_t)Q * 4));
  if (vote) SA_TRY(sa_store_search_buffers(s, Q, topn, out_cells != nullptr, false, fit));
  if (vote && compat) SA_TRY(sa_engine_ensure(e, s->q_attrs, (size_t)Q * sizeof(sa_track_attrs)));
  hipStream_t st = s->st;
  SA_HIPCHK(e, hipEventRecord(s->ev[0], st));
  if (vote && compat) {   // the query attributes travel with the query table
    SA_TRY(sa_store_compat_begin(s));
    SA_HIPCHK(e, hipMemcpyAsync(s->q_attrs.p, q_attrs, (size_t)Q * sizeof(sa_track_attrs), hipMemcpyHostToDevice, st));
  }
  // the padded query rows are written once: a pool rerun (sa_store_search_run) runs the launches again over the same q_feat.  The
  // fill goes first: its launch runs while the host queues the two small copies, which only the launches behind it read
  SA_TRY(sa_rows_fill(s, R, Kp, nullptr, s->q_feat.p, (float*)s->q_norm.p));
  SA_HIPCHK(e, hipMemcpyAsync(s->q_ids.p, q_ids, (size_t)Q * 8, hipMemcpyHostToDevice, st));
  SA_HIPCHK(e, hipMemcpyAsync(s->q_nobs.p, q_n_obs, (size_t)Q * 4, hipMemcpyHostToDevice, st));
  if (!vote) {
    SA_TRY(step->queue(false));
    SA_HIPCHK(e, hipStreamSynchronize(st));
    return SA_OK;
  }
  return sa_store_search_run(s, p, what, Q, false, nullptr, out_n, out_winner, out_weight, out_cells, compat, fit);
}
