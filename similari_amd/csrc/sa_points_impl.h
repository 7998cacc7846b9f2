// sa_points_impl.h — what the two sources behind a point bank share: sa_points.hip (include/similari_points.h: the bank, the filter
// calls) and sa_pose.hip (include/similari_pose.h, similari_pose_batch.h: the association of poses to the bank's tracks).  The bank itself and the checks
// every call runs before it launches anything, the growth of the planes, and the load and store of one point's state.  What the points
// of a call are — their check, their staging, the device read of one — is sa_point_rows.h, which pose NMS shares.  Internal: no other
// file includes it.
#pragma once
#include "sa_store.h"
#include "sa_kalman_point.h"
#include "sa_point_rows.h"
#include "../../include/similari_points.h"
#include "../../include/similari_pose.h"
#include "../../include/similari_pose_batch.h"
#include "../../include/similari_pose_track.h"
#include "../../include/similari_pose_oks.h"

#include <algorithm>
#include <unordered_map>
#include <unordered_set>
#include <vector>

struct sa_points {
  sa_engine* e = nullptr;   // nullptr: the engine was destroyed first (sa_points_orphan)
  bool broken = false;      // a device call failed after the host table changed
  int device = 0;
  hipStream_t st = nullptr;
  uint32_t P = 0;
  float pw = 0.f, vw = 0.f;
  uint32_t T = 0, cap = 0;                        // tracks, track capacity of the planes
  std::vector<uint64_t> ids;                      // slot -> id
  std::unordered_map<uint64_t, uint32_t> slot_of;
  DevBuf plane[5], has;                          // [cap * P] float4 each: mean, covariance rows 0..3; [cap * P] u8
  DevBuf d_slots, d_index, d_pts, d_mask, d_out, d_seen, d_moves;
  hipEvent_t ev[2] = {nullptr, nullptr};          // around the launch of a call
  sa_points_stats last{};
  // sa_points_associate (sa_pose.hip): the factors, the gain matrix, the tap, the row words, the results; events around its launches
  DevBuf d_fac4, d_fac1, d_gain, d_tap, d_best, d_res;
  hipEvent_t pev[4] = {nullptr, nullptr, nullptr, nullptr};
  sa_pose_stats last_pose{};
  // sa_points_associate_batch (sa_pose.hip): the call's segment table; the other buffers and the events are the single call's
  DevBuf d_segs;
  sa_pose_batch_stats last_pose_batch{};
  // sa_points_track, sa_points_track_batch (sa_pose.hip): per track the pose that took it, per pose its rank among the unmatched, per
  // scene their number and its prefix; two more events behind the vote's four
  DevBuf d_trk;
  hipEvent_t tev[2] = {nullptr, nullptr};
  sa_pose_track_stats last_track{};
  // the keypoint tracker (sa_pose_sort.hip): the circles of a gated vote and the limit of each listed track (sa_pose.hip); the slots
  // that leave and the staging block their final states are gathered into (sa_points.hip); events around k_pose_circles (0, 1) and
  // k_points_gather (2, 3)
  DevBuf d_circ, d_limit, d_leave, d_stage;
  hipEvent_t gev[4] = {nullptr, nullptr, nullptr, nullptr};
  // the metric of the vote (include/similari_pose_oks.h, sa_pose.hip): under OKS the sigmas as given, var2 [P] on the device, and the
  // areas of a vote's extents [poses + tracks] beside its circles
  uint32_t metric = SA_POSE_METRIC_MAHALANOBIS;
  std::vector<float> sigmas;
  DevBuf d_var2, d_area;
};

struct SaPoseTrackPlan;   // sa_pose_track_plan.h: sort_track hands one out, and this header stays free of it
namespace sa_pt {

inline int enter(sa_points* b, const char* what) {
  if (!b->e) return sa_engine_fail(nullptr, SA_ERR_STATE, "%s: the bank's engine was destroyed before it", what);
  if (b->broken) return sa_engine_fail(b->e, SA_ERR_STATE, "%s: an earlier device call failed half-way; destroy the bank", what);
  return sa_engine_drain(b->e, &b->device, &b->st);
}

// The ids of one call: none is 0, none comes twice.  slots takes each id's slot, SA_SEARCH_NONE for one the bank does not hold;
// known_only: such an id is refused with SA_ERR_NOT_FOUND.
// A call that names the bank's tracks in the bank's own order — the loop that steps every track each frame — costs one comparison per
// id: the leading ids that equal ids[slot] need no look-up and cannot repeat.  Every id behind them goes through one set and one
// look-up; a repeat of a leading id shows as a slot in front of `lead`.
inline int check_ids(sa_points* b, const char* what, uint32_t n, const uint64_t* ids, bool known_only, std::vector<uint32_t>& slots) {
  slots.resize(n);
  uint32_t lead = 0;
  const uint32_t lim = std::min(n, b->T);
  while (lead < lim && ids[lead] == b->ids[lead]) {
    slots[lead] = lead;
    ++lead;
  }
  std::unordered_set<uint64_t> seen;
  seen.reserve((size_t)(n - lead) * 2u);
  for (uint32_t i = lead; i < n; ++i) {
    if (ids[i] == 0) return sa_engine_fail(b->e, SA_ERR_BAD_ARG, "%s: id 0 at %u", what, i);
    const auto it = b->slot_of.find(ids[i]);
    if (!seen.insert(ids[i]).second || (it != b->slot_of.end() && it->second < lead))
      return sa_engine_fail(b->e, SA_ERR_BAD_ARG, "%s: id %llu twice in one call", what, (unsigned long long)ids[i]);
    if (it == b->slot_of.end() && known_only)
      return sa_engine_fail(b->e, SA_ERR_NOT_FOUND, "%s: unknown track id %llu", what, (unsigned long long)ids[i]);
    slots[i] = it == b->slot_of.end() ? SA_SEARCH_NONE : it->second;
  }
  return SA_OK;
}

// the source of a call's points in the bank's words (sa_point_rows_check): its n items are tracks, its block lies on the bank's device
inline int check_rows(sa_points* b, const char* what, uint32_t n, const sa_point_rows* r) {
  return sa_point_rows_check(b->e, what, b->P, n, r, b->device, SaPointRowsWords{"rows", "tracks", "this bank is on"});
}

// the planes hold T1 tracks: capacity doubles, the states stored so far move along (a failed allocation leaves the bank as it was)
inline int reserve(sa_points* b, uint64_t T1) {
  if (T1 <= b->cap) return SA_OK;
  uint64_t ncap = b->cap ? (uint64_t)b->cap * 2 : 64;
  while (ncap < T1) ncap *= 2;
  for (DevBuf& d : b->plane) SA_TRY(sa_engine_ensure(b->e, d, (size_t)ncap * b->P * 16, true));
  SA_TRY(sa_engine_ensure(b->e, b->has, (size_t)ncap * b->P, true));
  b->cap = (uint32_t)ncap;
  return SA_OK;
}

// the state of the point at `at` = slot * P + p out of, and into, the five planes of a kernel's arguments (a.plane[5])
template <class Args>
__device__ __forceinline__ void pt_load(const Args& a, size_t at, sa_pkf& s) {
  const float4 m = a.plane[0][at];
  s.mean[0] = m.x; s.mean[1] = m.y; s.mean[2] = m.z; s.mean[3] = m.w;
  for (int r = 0; r < 4; ++r) {
    const float4 c = a.plane[1 + r][at];
    s.cov[r * 4] = c.x; s.cov[r * 4 + 1] = c.y; s.cov[r * 4 + 2] = c.z; s.cov[r * 4 + 3] = c.w;
  }
}
template <class Args>
__device__ __forceinline__ void pt_store(const Args& a, size_t at, const sa_pkf& s) {
  a.plane[0][at] = make_float4(s.mean[0], s.mean[1], s.mean[2], s.mean[3]);
  for (int r = 0; r < 4; ++r) a.plane[1 + r][at] = make_float4(s.cov[r * 4], s.cov[r * 4 + 1], s.cov[r * 4 + 2], s.cov[r * 4 + 3]);
}

// What ran behind a call of sa_pose.hip (and the traffic of sort_remove): every public stats struct is filled from one of these.  The
// launch counts are set where the launches happen; kernel_ms: factor, tile, assign, scan, step; gate_ms: k_pose_circles.
struct PoseRan {
  uint64_t bytes_h2d = 0, bytes_d2h = 0, src_bytes = 0, refused_pairs = 0;   // refused_pairs: a gated peek with a tap only
  double device_ms = 0, kernel_ms[5] = {0, 0, 0, 0, 0}, gate_ms = 0;
  uint32_t extents_launches = 0, vote_launches = 0, scan_launches = 0, step_launches = 0, roots = 0;   // roots: of all scenes
  std::vector<uint32_t> res;   // [poses] columns, [poses] weights, [scenes] roots
  std::vector<float> circ;     // [poses + tracks][4]: a gated vote whose caller asked for the circles
};
template <class Stats>   // the fields every stats struct of the vote has; kernel_ms: as many as the struct holds
inline void ran_into(Stats& s, const PoseRan& r) {
  s.roots = r.roots;
  s.bytes_h2d = r.bytes_h2d, s.bytes_d2h = r.bytes_d2h, s.src_bytes = r.src_bytes, s.device_ms = r.device_ms;
  for (size_t k = 0; k < sizeof s.kernel_ms / sizeof s.kernel_ms[0]; ++k) s.kernel_ms[k] = r.kernel_ms[k];
}
template <size_t N>   // the events of one of the bank's arrays that do not exist yet
inline int make_events(sa_points* b, hipEvent_t (&evs)[N]) {
  for (auto& ev : evs)
    if (!ev) SA_HIPCHK(b->e, hipEventCreate(&ev));
  return SA_OK;
}
// sa_pose.hip: the options of a vote, and of a tracking call: every refusal, `what` in front
int check_options(sa_engine* e, const char* what, const sa_pose_options* o);
int check_track_options(sa_engine* e, const char* what, const sa_pose_track_options* o);

// ---- what the keypoint tracker (sa_pose_sort.hip, include/similari_pose_sort.h) asks of the two sources --------------------------------
// A frame of the tracker is a sa_points_track_batch whose tracks the tracker names by slot (slots [tracks]: the concatenation of its
// scenes' lists, distinct, below the bank's tracks; no id is looked up), whose new ids are first_id, first_id + 1, ..., and whose vote may
// be gated: limits [tracks] (sa_pose_gate.h), or nullptr when no limit of the call is finite — then the launches of sa_points_track_batch.
// sa_pose.hip.  sort_check: every refusal of sa_points_track_batch that does not concern ids, for a bank of T_after tracks; nothing is
// launched or changed.  sort_track: the call behind them — out_plan: what it did to the table (sa_pose_track_plan.h).  sort_peek: the
// vote alone; out_cols [poses] local columns or -1, out_tap: nullptr or every scene's matrix.
int sort_check(sa_points* b, const char* what, uint32_t n_scenes, const uint32_t* track_counts, const uint32_t* pose_counts,
               const sa_point_rows* poses, uint64_t T_after);
int sort_track(sa_points* b, const char* what, uint32_t n_scenes, const uint32_t* track_counts, const uint32_t* pose_counts,
               const sa_point_rows* poses, const uint32_t* slots, const float* limits, uint64_t first_id, const sa_pose_track_options* o,
               float* out_weight, float* out_xy, SaPoseTrackPlan* out_plan, PoseRan& r);
int sort_peek(sa_points* b, const char* what, uint32_t n_scenes, const uint32_t* track_counts, const uint32_t* pose_counts,
              const sa_point_rows* poses, const uint32_t* slots, const float* limits, const sa_pose_track_options* o, int32_t* out_cols,
              float* out_weight, float* out_tap, PoseRan& r);
// sa_points.hip.  The removal of the tracks at `leaving` (in this order, the rule of sa_points_remove: the last track moves into each
// hole in turn; what_is [tracks left]: the slot, as the planes hold it now, whose state ends in each slot — sa_pose_sort_plan.h works
// it out) QUEUED, not waited for: k_points_gather copies the leaving states into the staging block, k_points_move compacts, the block is
// copied into stage [leaving * P * 81 bytes: mean, cov, has] by the time the stream is next waited for.
int sort_remove(sa_points* b, const std::vector<uint32_t>& leaving, const std::vector<uint32_t>& what_is, uint8_t* stage, PoseRan& r);
// after the wait: the gather's time by device events
int sort_remove_ms(sa_points* b, double* ms);

}  // namespace sa_pt
