// sa_bestfit.hip — the BestFit vote of a track search (include/similari_bestfit.h): the second stage of a search in place of k_topn,
// and the three entry points.  Launch 1 (sa_launch_search_tiles), the prologue, the pool's growth with its rerun, the stats and the
// copies out are sa_search.hip's (sa_store_search_begin, sa_store_search_run), the query side is filled by the bodies of the TopN
// calls (sa_store_search_topn_impl, sa_store_search_stored_impl, sa_store_join_topn_impl), which take the vote as their last argument.
//
// Stage 2 is three launches of one workgroup per query row of grp, ordered by their launch boundaries and by nothing else:
//   k_fit_weigh  every surviving group's weight -> wscr, col_key[t] = max over the groups (., t) of the weight's order-preserving key
//   k_fit_claim  col_q[t] = min query id among the groups (., t) whose key is col_key[t]
//   k_fit_rank   the rows: k_topn's selection rounds over the weights in wscr; a group holds the claim iff its key is col_key[t] and
//                its query id is col_q[t]
// Integer atomics whose results do not depend on their order; no thread waits for another workgroup.
//
// Reference: BestFitVoting::winners (src/track/voting/best.rs:52-128).
#include "sa_store.h"
#include "sa_vote_weight.h"

namespace {

typedef unsigned long long u64a;   // the 64-bit type HIP's integer atomics take

constexpr uint32_t FIT_THREADS = SA_VOTE_THREADS;
constexpr uint32_t FIT_LDS_CAND = SA_VOTE_LDS_CAND;   // the threshold between the two regimes is k_topn's
constexpr uint32_t FIT_NO_QUERY_BYTE = 0xff;   // col_q before any claim: all bits set, above every id

// f64 -> u64 that orders as the doubles do (weights are sums of non-negative terms from +0.0, so two equal weights have equal bits
// and equal keys); 0 is below every key: a column without a group
__device__ __forceinline__ uint64_t weight_key(double w) {
  const uint64_t b = (uint64_t)__double_as_longlong(w);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// where wscr keeps the weight of block b as query q sums it against stored track s: a join keeps one weight per direction (k_topn<true>)
template <bool JOIN>
__device__ __forceinline__ size_t weight_slot(uint32_t b, uint32_t q, uint32_t s) {
  return JOIN ? 2 * (size_t)b + (q > s ? 1u : 0u) : (size_t)b;
}

// The surviving groups of one row of grp, gathered into LDS (block and column; arrival order), eight loads in flight per thread as
// k_topn scans.  Returns their number, which may exceed FIT_LDS_CAND: then only the first FIT_LDS_CAND arrivals were kept and the
// caller walks the row itself.  Every thread of the workgroup calls it.
__device__ __forceinline__ uint32_t gather_row(const uint32_t* __restrict__ g, uint32_t T, uint32_t* c_b, uint32_t* c_s, uint32_t* c_n) {
  constexpr uint32_t NT = FIT_THREADS, SCAN_U = 8;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) *c_n = 0;
  __syncthreads();
  for (uint32_t s0 = tid; s0 < T; s0 += SCAN_U * NT) {
    uint32_t b[SCAN_U];
#pragma unroll
    for (uint32_t u = 0; u < SCAN_U; ++u) b[u] = s0 + u * NT < T ? g[s0 + u * NT] : SA_SEARCH_NONE;
#pragma unroll
    for (uint32_t u = 0; u < SCAN_U; ++u)
      if (b[u] != SA_SEARCH_NONE) {
        const uint32_t i = atomicAdd(c_n, 1u);
        if (i < FIT_LDS_CAND) { c_b[i] = b[u]; c_s[i] = s0 + u * NT; }
      }
  }
  __syncthreads();
  return *c_n;
}

// Launch 1 of stage 2.  The block sums run side by side, one group per thread, with block_weight / block_weight_t of k_topn: the bits
// of the TopN call.  cnt[0] takes the row's groups with one atomic per workgroup.
template <bool JOIN>
__global__ __launch_bounds__(FIT_THREADS) void k_fit_weigh(const uint32_t* __restrict__ grp, const float* __restrict__ pool,
                                                           const uint32_t* __restrict__ ctrl, uint32_t pool_cap, uint32_t T, uint32_t Kp,
                                                           double* __restrict__ wscr, uint64_t* __restrict__ col_key,
                                                           uint32_t* __restrict__ cnt) {
  constexpr uint32_t NT = FIT_THREADS;
  __shared__ uint32_t c_b[FIT_LDS_CAND], c_s[FIT_LDS_CAND];
  __shared__ uint32_t c_n;
  if (ctrl[0] > pool_cap) return;   // the pool overflowed: blocks are missing, the host grows it and runs again (nothing to undo)
  const uint32_t q = blockIdx.x, tid = threadIdx.x;
  const float M = sa_key_f32(ctrl[1]);
  const uint32_t* g = grp + (size_t)q * T;
  const uint32_t KK = Kp * Kp;
  auto weigh = [&](uint32_t b, uint32_t s) {
    const double w = JOIN && q > s ? block_weight_t(pool + (size_t)b * KK, Kp, M) : block_weight(pool + (size_t)b * KK, KK, M);
    wscr[weight_slot<JOIN>(b, q, s)] = w;
    atomicMax((u64a*)(col_key + s), (u64a)weight_key(w));
  };
  const uint32_t nc = gather_row(g, T, c_b, c_s, &c_n);
  if (nc <= FIT_LDS_CAND) {
    for (uint32_t i = tid; i < nc; i += NT) weigh(c_b[i], c_s[i]);
  } else {
    for (uint32_t s = tid; s < T; s += NT) {
      const uint32_t b = g[s];
      if (b != SA_SEARCH_NONE) weigh(b, s);
    }
  }
  if (tid == 0 && nc) atomicAdd(cnt, nc);
}

// Launch 2 of stage 2: among the groups that carry a column's best weight, the lowest query id
template <bool JOIN>
__global__ __launch_bounds__(FIT_THREADS) void k_fit_claim(const uint32_t* __restrict__ grp, const uint32_t* __restrict__ ctrl,
                                                           uint32_t pool_cap, const uint64_t* __restrict__ q_ids, uint32_t T,
                                                           const double* __restrict__ wscr, const uint64_t* __restrict__ col_key,
                                                           uint64_t* __restrict__ col_q) {
  constexpr uint32_t NT = FIT_THREADS, SCAN_U = 8;
  if (ctrl[0] > pool_cap) return;
  const uint32_t q = blockIdx.x, tid = threadIdx.x;
  const uint64_t qid = q_ids[q];
  const uint32_t* g = grp + (size_t)q * T;
  for (uint32_t s0 = tid; s0 < T; s0 += SCAN_U * NT) {
    uint32_t b[SCAN_U];
#pragma unroll
    for (uint32_t u = 0; u < SCAN_U; ++u) b[u] = s0 + u * NT < T ? g[s0 + u * NT] : SA_SEARCH_NONE;
#pragma unroll
    for (uint32_t u = 0; u < SCAN_U; ++u) {
      if (b[u] == SA_SEARCH_NONE) continue;
      const uint32_t s = s0 + u * NT;
      if (weight_key(wscr[weight_slot<JOIN>(b[u], q, s)]) == col_key[s]) atomicMin((u64a*)(col_q + s), (u64a)qid);
    }
  }
}

// Launch 3 of stage 2: k_topn's rounds — at most topn times a workgroup arg-max under (weight desc, stored id asc), each over the
// candidates that rank after the previous pick — with the weights read from wscr and the column carried beside the pick, so that the
// entry's winner is decided where it is written.  Up to FIT_LDS_CAND groups are ranked from LDS, more from global memory.  While the
// candidates are loaded every group tests its claim: a claimed column has exactly one holder, so the holders counted are the claimed
// columns (cnt[1], one atomic per workgroup).
template <bool JOIN>
__global__ __launch_bounds__(FIT_THREADS) void k_fit_rank(const uint32_t* __restrict__ grp, const uint32_t* __restrict__ ctrl,
                                                          uint32_t pool_cap, const uint64_t* __restrict__ q_ids,
                                                          const uint64_t* __restrict__ s_ids, uint32_t T, uint32_t topn,
                                                          const double* __restrict__ wscr, const uint64_t* __restrict__ col_key,
                                                          const uint64_t* __restrict__ col_q, uint32_t* __restrict__ cnt,
                                                          uint32_t* __restrict__ out_n, uint64_t* __restrict__ out_winner,
                                                          uint64_t* __restrict__ out_track, double* __restrict__ out_w) {
  constexpr uint32_t NT = FIT_THREADS, NW = NT / 64;
  __shared__ double s_w[NW];
  __shared__ uint64_t s_id[NW];
  __shared__ uint32_t s_s[NW];
  __shared__ uint32_t c_b[FIT_LDS_CAND], c_s[FIT_LDS_CAND];
  __shared__ double c_w[FIT_LDS_CAND];
  __shared__ uint64_t c_id[FIT_LDS_CAND];
  __shared__ uint32_t c_n, c_held;
  const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint64_t* owin = out_winner + (size_t)q * topn;
  uint64_t* otrk = out_track + (size_t)q * topn;
  double* ow = out_w + (size_t)q * topn;
  if (ctrl[0] > pool_cap) {   // as k_topn: the host searches again
    if (tid == 0) out_n[q] = 0;
    return;
  }
  if (tid == 0) c_held = 0;
  const uint64_t qid = q_ids[q];
  const uint32_t* g = grp + (size_t)q * T;
  auto holds = [&](double w, uint32_t s) { return weight_key(w) == col_key[s] && col_q[s] == qid; };
  const uint32_t nc = gather_row(g, T, c_b, c_s, &c_n);   // (its first barrier publishes c_held = 0)
  const bool in_lds = nc <= FIT_LDS_CAND;
  uint32_t held = 0;
  if (in_lds) {
    for (uint32_t i = tid; i < nc; i += NT) {
      const uint32_t s = c_s[i];
      const double w = wscr[weight_slot<JOIN>(c_b[i], q, s)];
      c_w[i] = w;
      c_id[i] = s_ids[s];
      held += holds(w, s) ? 1u : 0u;
    }
  } else {
    for (uint32_t s = tid; s < T; s += NT) {
      const uint32_t b = g[s];
      if (b != SA_SEARCH_NONE) held += holds(wscr[weight_slot<JOIN>(b, q, s)], s) ? 1u : 0u;
    }
  }
  if (held) atomicAdd(&c_held, held);
  __syncthreads();
  if (tid == 0 && c_held) atomicAdd(cnt + 1, c_held);
  double pw = 0.0;
  uint64_t pid = 0;
  uint32_t n = 0;
  for (; n < topn; ++n) {
    double bw = 0.0;
    uint64_t bid = 0;   // 0: none (ids are non-zero)
    uint32_t bs = 0;
    auto consider = [&](double w, uint64_t id, uint32_t s) {
      if (n > 0 && !ranks_before(pw, pid, w, id)) return;   // picked already
      if (bid == 0 || ranks_before(w, id, bw, bid)) { bw = w; bid = id; bs = s; }
    };
    if (in_lds) {
      for (uint32_t i = tid; i < nc; i += NT) consider(c_w[i], c_id[i], c_s[i]);
    } else {
      for (uint32_t s = tid; s < T; s += NT) {
        const uint32_t b = g[s];
        if (b != SA_SEARCH_NONE) consider(wscr[weight_slot<JOIN>(b, q, s)], s_ids[s], s);
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double xw = __shfl_xor(bw, o);
      const uint64_t xid = __shfl_xor(bid, o);
      const uint32_t xs = __shfl_xor(bs, o);
      if (xid != 0 && (bid == 0 || ranks_before(xw, xid, bw, bid))) { bw = xw; bid = xid; bs = xs; }
    }
    if (lane == 0) { s_w[wave] = bw; s_id[wave] = bid; s_s[wave] = bs; }
    __syncthreads();
    bw = s_w[0];
    bid = s_id[0];
    bs = s_s[0];
    for (uint32_t w = 1; w < NW; ++w)
      if (s_id[w] != 0 && (bid == 0 || ranks_before(s_w[w], s_id[w], bw, bid))) { bw = s_w[w]; bid = s_id[w]; bs = s_s[w]; }
    __syncthreads();   // s_w / s_id / s_s are rewritten in the next round
    if (bid == 0) break;
    if (tid == 0) {
      owin[n] = holds(bw, bs) ? bid : qid;
      otrk[n] = bid;
      ow[n] = bw;
    }
    pw = bw;
    pid = bid;
  }
  if (tid == 0) {
    out_n[q] = n;
    for (uint32_t r = n; r < topn; ++r) { owin[r] = 0; otrk[r] = 0; ow[r] = 0.0; }
  }
}

// fit: col_key [T], col_q [T], {groups, claimed}
uint64_t* col_key(const sa_store* s) { return (uint64_t*)s->fit.p; }
uint64_t* col_q(const sa_store* s) { return (uint64_t*)s->fit.p + s->T; }
uint32_t* counters(const sa_store* s) { return (uint32_t*)((uint64_t*)s->fit.p + 2 * (size_t)s->T); }

template <bool JOIN>
int launch(sa_store* s, uint32_t Q, uint32_t topn, const uint64_t* q_ids) {
  sa_engine* e = s->e;
  hipStream_t st = s->st;
  const dim3 grid(Q), block(FIT_THREADS);
  const uint32_t* grp = (const uint32_t*)s->grp.p;
  const uint32_t* ctrl = (const uint32_t*)s->ctrl.p;
  hipLaunchKernelGGL(k_fit_weigh<JOIN>, grid, block, 0, st, grp, (const float*)s->pool.p, ctrl, s->pool_cap, s->T, s->Kp, (double*)s->wscr.p,
                     col_key(s), counters(s));
  SA_HIPCHK(e, hipGetLastError());
  SA_HIPCHK(e, hipEventRecord(s->ev[4], st));
  hipLaunchKernelGGL(k_fit_claim<JOIN>, grid, block, 0, st, grp, ctrl, s->pool_cap, q_ids, s->T, (const double*)s->wscr.p,
                     (const uint64_t*)col_key(s), col_q(s));
  SA_HIPCHK(e, hipGetLastError());
  SA_HIPCHK(e, hipEventRecord(s->ev[5], st));
  hipLaunchKernelGGL(k_fit_rank<JOIN>, grid, block, 0, st, grp, ctrl, s->pool_cap, q_ids, (const uint64_t*)s->d_ids.p, s->T, topn,
                     (const double*)s->wscr.p, (const uint64_t*)col_key(s), (const uint64_t*)col_q(s), counters(s), (uint32_t*)s->o_n.p,
                     (uint64_t*)s->o_id.p, (uint64_t*)s->o_trk.p, (double*)s->o_w.p);
  SA_HIPCHK(e, hipGetLastError());
  return SA_OK;
}

}  // namespace

int sa_bestfit_buffers(sa_store* s, uint32_t Q, uint32_t topn) {
  SA_TRY(sa_engine_ensure(s->e, s->fit, (size_t)s->T * 16 + sizeof s->h_fit));
  return sa_engine_ensure(s->e, s->o_trk, (size_t)Q * topn * 8);
}

int sa_bestfit_reset(sa_store* s) {
  SA_HIPCHK(s->e, hipMemsetAsync(s->fit.p, 0, (size_t)s->T * 16 + sizeof s->h_fit, s->st));
  SA_HIPCHK(s->e, hipMemsetAsync(col_q(s), FIT_NO_QUERY_BYTE, (size_t)s->T * 8, s->st));
  return SA_OK;
}

int sa_bestfit_launch(sa_store* s, bool join, uint32_t Q, uint32_t topn, const uint64_t* q_ids) {
  return join ? launch<true>(s, Q, topn, q_ids) : launch<false>(s, Q, topn, q_ids);
}

extern "C" {

int sa_store_search_bestfit(sa_store* s, const sa_topn_params* p, const sa_compat* c, uint32_t nq, const uint64_t* q_ids,
                            const uint32_t* q_n_obs, const float* q_feats, const sa_track_attrs* q_attrs, uint32_t* out_n,
                            uint64_t* out_winner, uint64_t* out_track, double* out_weight, float* out_cells) {
  const SaBestFit fit{out_track};
  return sa_store_search_topn_impl(s, "sa_store_search_bestfit", p, c != nullptr, c, nq, q_ids, q_n_obs, SaRowSource::of_host(q_feats), q_attrs, out_n,
                                   out_winner,
                                   out_weight, out_cells, &fit);
}

int sa_store_search_stored_bestfit(sa_store* s, const sa_topn_params* p, const sa_compat* c, uint32_t flags, uint32_t n,
                                   const uint64_t* ids, uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track, double* out_weight,
                                   float* out_cells) {
  const SaBestFit fit{out_track};
  return sa_store_search_stored_impl(s, "sa_store_search_stored_bestfit", p, c != nullptr, c, flags, n, ids, out_n, out_winner, out_weight,
                                     out_cells, &fit);
}

int sa_store_join_bestfit(sa_store* s, const sa_topn_params* p, const sa_compat* c, uint32_t* out_n, uint64_t* out_winner,
                          uint64_t* out_track, double* out_weight, float* out_cells) {
  const SaBestFit fit{out_track};
  return sa_store_join_topn_impl(s, "sa_store_join_bestfit", p, c != nullptr, c, out_n, out_winner, out_weight, out_cells, &fit);
}

int sa_store_bestfit_last(sa_store* s, sa_bestfit_stats* out) {
  if (!s || !out) return SA_ERR_BAD_ARG;
  *out = s->fit_last;
  return SA_OK;
}

}  // extern "C"
