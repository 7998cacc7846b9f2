// sa_waste.hip — tracks that leave the engine's table enter a feature store (include/similari_waste.h): sa_tracks_waste (the append),
// sa_tracks_waste_absorb (the absorb) and the stats of both.
//
// A waste is sa_store_append_impl (sa_merge.hip) or sa_store_absorb_impl (sa_absorb.hip) handed a fourth row source, "rows the
// library owns" (SaRowSource::of_own), between two things that exist already: the resolution of (scene, id) to table rows
// (sa_engine_waste_resolve, sa_engine.hip) and sa_tracks_remove_many.  What is new is one kernel, k_waste_capture: it reads the leaving
// rows' present flags and qualities out of the engine's table, compacts the present slots in slot order and copies their feature rows
// into a staging block of the store — the [n][Kp] layout of a search's query side, which k_pad_rows (sa_devrows.hip, through
// sa_rows_fill) then pads, rounds and sums exactly as it does for host rows and for a caller's SA_ELEM_F32 device block.  The counts and the
// qualities come to the host in one copy, because the store's host tables are authoritative; no feature row does.
//
// Reference: TrackStore::wasted / fetch_tracks feeding a second store, examples/middleware_sort_tracker.rs, examples/track_merging.rs.
#include "sa_store.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

constexpr uint32_t WC_THREADS = 256, WC_TRACKS = WC_THREADS / 64;

struct SaWasteSet {   // the scenes of one launch, by value (12 x 32 bytes)
  SaWasteScene t[SA_GATHER_SET];
};

// One wave per leaving track, four tracks per workgroup, blockIdx.y = the scene of the set.  rows[i]: the table row of track i of the
// call.  Lane k < K holds slot k's present flag and quality; the ballot of the flags is the bank's shape: its popcount the number of
// observations, the popcount below lane k where slot k lands.  Outputs, all indexed by the track's place i in the call:
//   w_nobs[i]; w_qual[i][Kp] the qualities of the present slots in slot order, 0 behind them; w_table[i][Kp] the staging row of each,
//   SA_SEARCH_NONE behind them; w_feat[i][Kp][Dp] the present rows themselves, Dp / 4 16-byte pieces each, one load and one store per
//   lane and pass (a bank row is a multiple of 128 bytes and starts on one).  Staging rows behind the last present one are not written
//   and, being SA_SEARCH_NONE in the table, never read.
// No LDS; the listing shows no scratch (the set is read out of the kernel arguments with scalar loads, the loop over the ballot is
// wave-uniform).
__global__ __launch_bounds__(WC_THREADS) void k_waste_capture(const SaWasteSet set, const uint32_t* __restrict__ rows, uint32_t K, uint32_t Kp,
                                                              uint32_t Dp, uint32_t* __restrict__ w_nobs, float* __restrict__ w_qual,
                                                              uint32_t* __restrict__ w_table, float* __restrict__ w_feat) {
  const SaWasteScene& sc = set.t[blockIdx.y];
  const uint32_t j = blockIdx.x * WC_TRACKS + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (j >= sc.count) return;
  const uint32_t i = sc.first + j, r = rows[i];
  bool pres = false;
  float q = 0.f;
  if (lane < K) {
    pres = sc.fpresent[(size_t)r * K + lane] != 0;
    q = sc.fquality[(size_t)r * K + lane];
  }
  const unsigned long long m = __ballot(pres);
  const uint32_t n = (uint32_t)__popcll(m), pos = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  const size_t o = (size_t)i * Kp;
  if (lane < Kp && lane >= n) {
    w_qual[o + lane] = 0.f;
    w_table[o + lane] = SA_SEARCH_NONE;
  }
  if (pres) {
    w_qual[o + pos] = q;
    w_table[o + pos] = (uint32_t)(o + pos);
  }
  if (lane == 0) w_nobs[i] = n;
  const uint32_t pieces = Dp / 4u;
  uint32_t d = 0;
  for (unsigned long long left = m; left; left &= left - 1ull, ++d) {
    const uint32_t k = (uint32_t)__ffsll((long long)left) - 1u;
    const float4* from = (const float4*)(sc.feat + ((size_t)r * K + k) * Dp);
    float4* to = (float4*)(w_feat + (o + d) * Dp);
    for (uint32_t x = lane; x < pieces; x += 64u) to[x] = from[x];
  }
}

// A waste up to the point where its rows lie in the staging block and the host knows their counts and qualities.
struct Captured {
  uint32_t n = 0;
  std::vector<uint64_t> ids;       // [n] flattened in call order
  std::vector<uint32_t> nobs;      // [n]
  std::vector<float> quality;      // [sum nobs], never empty (a pointer for the bodies, which read sum nobs entries)
  std::vector<uint32_t> table;     // [sum nobs] the staging row of each observation: what an append reads
  SaRowSource src;
};

int check_rule(sa_engine* e, const sa_store* s, uint32_t keep, uint32_t n, const uint32_t* capacity, const char* what) {
  if (keep != SA_KEEP_LATEST && keep != SA_KEEP_BEST) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: unknown keep %u", what, keep);
  if (capacity)
    for (uint32_t i = 0; i < n; ++i)
      if (capacity[i] < 1 || capacity[i] > s->K)
        return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: capacity %u at %u (1..%u)", what, capacity[i], i, s->K);
  return SA_OK;
}

// Every check that needs no launch, then the capture.  more(c): the caller's own checks of the flattened ids, behind the shared ones
// and before anything is queued.
int capture(sa_engine* e, sa_store* dst, const char* what, uint32_t keep, uint32_t n_scenes, const uint64_t* scene_ids, const uint32_t* counts,
            const uint64_t* const* ids, const uint32_t* capacity, const std::function<int(const Captured&)>& more, Captured& c) {
  if (n_scenes && (!scene_ids || !counts || !ids)) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
  if (dst->e && dst->e != e) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: dst belongs to another engine", what);
  uint32_t K = 0, D = 0, Dp = 0;
  if (!sa_engine_bank_shape(e, &K, &D, &Dp)) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: the engine is not visual: its tracks have no feature bank", what);
  if (dst->D != D) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: feature_len %u of the engine, %u of dst", what, D, dst->D);
  if (K > dst->K) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: bank depth %u of the engine (max_observations %u of dst)", what, K, dst->K);
  for (uint32_t i = 0; i < n_scenes; ++i)   // (no table holds id 0: the append's refusal, not "unknown track id")
    for (uint32_t j = 0; ids[i] && j < counts[i]; ++j)
      if (ids[i][j] == 0) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: id 0 in the list of scene %llu", what, (unsigned long long)scene_ids[i]);
  std::vector<SaWasteScene> scenes;
  std::vector<uint32_t> rows;
  SA_TRY(sa_engine_waste_resolve(e, what, n_scenes, scene_ids, counts, ids, &scenes, &rows));
  SA_TRY(sa_store_enter(dst, what));
  for (uint32_t i = 0; i < n_scenes; ++i) c.ids.insert(c.ids.end(), ids[i], ids[i] + (counts[i] ? counts[i] : 0u));
  const uint32_t n = c.n = (uint32_t)c.ids.size(), Kp = dst->Kp;
  SA_TRY(check_rule(e, dst, keep, n, capacity, what));
  SA_TRY(sa_store_check_ids(dst, what, n, c.ids.data(), nullptr));
  if ((uint64_t)n * Kp >= SA_SEARCH_NONE) return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: more than 2^32 - 2 staging rows", what);
  if (more) SA_TRY(more(c));
  c.quality.assign(1, 0.f);
  if (!n) return SA_OK;
  const size_t meta = (size_t)n * 4 + (size_t)n * Kp * 4;
  SA_TRY(sa_engine_ensure(e, dst->w_rows, (size_t)n * 4));
  SA_TRY(sa_engine_ensure(e, dst->w_meta, meta));
  SA_TRY(sa_engine_ensure(e, dst->w_table, (size_t)n * Kp * 4));
  SA_TRY(sa_engine_ensure(e, dst->w_feat, (size_t)n * Kp * Dp * 4));
  for (auto& ev : dst->wev)
    if (!ev) SA_HIPCHK(e, hipEventCreate(&ev));
  hipStream_t st = dst->st;
  uint32_t* w_nobs = (uint32_t*)dst->w_meta.p;
  float* w_qual = (float*)(w_nobs + n);
  SA_HIPCHK(e, hipMemcpyAsync(dst->w_rows.p, rows.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  SA_HIPCHK(e, hipEventRecord(dst->wev[0], st));
  uint32_t launches = 0;
  for (size_t at = 0; at < scenes.size(); at += SA_GATHER_SET) {
    SaWasteSet set{};
    const uint32_t ns = (uint32_t)std::min<size_t>(SA_GATHER_SET, scenes.size() - at);
    uint32_t most = 0;
    for (uint32_t k = 0; k < ns; ++k) {
      set.t[k] = scenes[at + k];
      most = std::max(most, set.t[k].count);
    }
    hipLaunchKernelGGL(k_waste_capture, dim3((most + WC_TRACKS - 1) / WC_TRACKS, ns), dim3(WC_THREADS), 0, st, set, (const uint32_t*)dst->w_rows.p, K,
                       Kp, Dp, w_nobs, w_qual, (uint32_t*)dst->w_table.p, (float*)dst->w_feat.p);
    SA_HIPCHK(e, hipGetLastError());
    ++launches;
  }
  SA_HIPCHK(e, hipEventRecord(dst->wev[1], st));
  std::vector<uint32_t> host(meta / 4);
  SA_HIPCHK(e, hipMemcpyAsync(host.data(), dst->w_meta.p, meta, hipMemcpyDeviceToHost, st));
  SA_HIPCHK(e, hipStreamSynchronize(st));
  c.nobs.assign(host.begin(), host.begin() + n);
  c.quality.clear();
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t k = 0; k < c.nobs[i]; ++k) {
      float q;
      std::memcpy(&q, &host[(size_t)n + (size_t)i * Kp + k], 4);
      c.quality.push_back(q);
      c.table.push_back(i * Kp + k);
    }
  sa_waste_stats& ws = dst->waste_last;
  ws.tracks = n;
  ws.rows = c.table.size();
  ws.launches_capture = launches;
  ws.table_bytes_d2h = meta;
  float ms = 0.f;
  SA_HIPCHK(e, hipEventElapsedTime(&ms, dst->wev[0], dst->wev[1]));
  ws.capture_ms = ms;
  if (c.quality.empty()) c.quality.push_back(0.f);
  c.src = SaRowSource::of_own(dst->w_feat.p, Dp, (const uint32_t*)dst->w_table.p, &c.table);
  return SA_OK;
}

}  // namespace

// (the tracker facade, sa_tracker.cpp, checks its capacity against this when a store is attached)
extern "C" __attribute__((visibility("hidden"))) uint32_t sa_store_depth(const sa_store* s) { return s->K; }

extern "C" {

int sa_tracks_waste(sa_engine* e, sa_store* dst, uint32_t keep, uint32_t n_scenes, const uint64_t* scene_ids, const uint32_t* counts,
                    const uint64_t* const* ids, const uint32_t* capacity, uint32_t* out_n_obs) {
  const char* what = "sa_tracks_waste";
  if (!e || !dst) return SA_ERR_BAD_ARG;
  dst->waste_last = sa_waste_stats{};
  Captured c;
  int rc = capture(e, dst, what, keep, n_scenes, scene_ids, counts, ids, capacity, nullptr, c);
  if (rc == SA_OK && c.n)
    rc = sa_store_append_impl(dst, what, keep, c.n, c.ids.data(), c.nobs.data(), c.src, c.quality.data(), capacity);
  if (rc != SA_OK) {
    dst->waste_last = sa_waste_stats{};
    return rc;
  }
  if (out_n_obs) std::copy(c.nobs.begin(), c.nobs.end(), out_n_obs);
  return sa_tracks_remove_many(e, n_scenes, scene_ids, counts, ids);
}

int sa_tracks_waste_absorb(sa_engine* e, sa_store* dst, uint32_t keep, const sa_topn_params* p, const sa_compat* c, uint32_t n_scenes,
                           const uint64_t* scene_ids, const uint32_t* counts, const uint64_t* const* ids, const sa_track_attrs* q_attrs,
                           const uint32_t* capacity, uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track, double* out_weight,
                           uint64_t* out_dest) {
  const char* what = "sa_tracks_waste_absorb";
  if (!e || !dst) return SA_ERR_BAD_ARG;
  dst->waste_last = sa_waste_stats{};
  dst->absorb_last = sa_absorb_stats{};   // as a refused absorb leaves them
  dst->retain_keep = 0;
  dst->retain_upload = 0;
  Captured cap;
  // the absorb's own refusals, ahead of the capture: the rule, the params, the outputs, an id that dst holds already
  int rc = capture(e, dst, what, keep, n_scenes, scene_ids, counts, ids, capacity, [&](const Captured& k) -> int {
    if ((c != nullptr) != (q_attrs != nullptr))
      return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: a rule and q_attrs come together or not at all", what);
    if (c) SA_TRY(sa_store_check_compat(dst, c, what, false));
    SA_TRY(sa_store_check_params(dst, p, what));
    if (!k.n) return (int)SA_OK;
    if (!out_n || !out_winner || !out_weight || !out_dest) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
    for (uint32_t i = 0; i < k.n; ++i) {
      if (dst->slot_of.count(k.ids[i]))
        return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: query id %llu is a stored track's", what, (unsigned long long)k.ids[i]);
      if (c && q_attrs[i].start > q_attrs[i].end)
        return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: query %llu starts after it ends", what, (unsigned long long)k.ids[i]);
    }
    return (int)SA_OK;
  }, cap);
  if (rc == SA_OK)
    rc = sa_store_absorb_impl(dst, what, keep, p, c, cap.n, cap.ids.data(), cap.nobs.data(), cap.src, q_attrs, cap.quality.data(), capacity, out_n,
                              out_winner, out_track, out_weight, out_dest);
  if (rc != SA_OK) {
    dst->waste_last = sa_waste_stats{};
    return rc;
  }
  return sa_tracks_remove_many(e, n_scenes, scene_ids, counts, ids);
}

int sa_store_waste_last(sa_store* dst, sa_waste_stats* out) {
  if (!dst || !out) return SA_ERR_BAD_ARG;
  *out = dst->waste_last;
  out->struct_size = sizeof *out;
  out->reserved = 0;
  return SA_OK;
}

}  // extern "C"
