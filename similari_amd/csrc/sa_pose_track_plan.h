// sa_pose_track_plan.h — what one sa_points_track / sa_points_track_batch call (include/similari_pose_track.h) did to the bank's table,
// worked out on the host from what the vote returns.  Host arithmetic only: sa_pose.hip runs it after the call's one wait, to append the
// created ids in the order the device gave them slots, and tests/test_pose_track_plan.py compiles this header on the host.
//
// The device's rule (k_pose_step): a matched pose steps the slot of its track; an unmatched pose of scene s takes slot
// T_old + base[s] + rank, base[s] the unmatched poses of the scenes in front of s and rank its place among the unmatched poses of its
// own scene.  That is the pose's place among ALL unmatched poses in call order — scene after scene, then pose order —, which is the order
// in which the call hands out new_ids.
#pragma once
#include <stdint.h>

#include <vector>

#define SA_POSE_TRACK_NONE 0xffffffffu

struct SaPoseTrackPlan {
  std::vector<uint32_t> slot;       // [poses] the slot every pose stepped
  std::vector<uint32_t> rank;       // [poses] an unmatched pose's place in call order = its entry of new_ids; SA_POSE_TRACK_NONE: matched
  std::vector<uint32_t> unmatched;  // [scenes] the unmatched poses of each scene (the device's counts)
  std::vector<uint32_t> coasted;    // the listed tracks nobody matched, as positions in the call's track list, ascending
  uint32_t matched = 0, created = 0;
};

// track_counts[s], pose_counts[s]: the tracks and poses of scene s, back to back in the call's lists.  cols [poses]: the column the
// vote gave each pose, LOCAL to its scene, negative = none (a column at or beyond the scene's tracks counts as none, as in give_out).
// slots [tracks]: the slot of each listed track, or nullptr: 0, 1, 2, ...  T_old: the tracks of the bank before the call.
static inline void sa_pose_track_plan(uint32_t n_scenes, const uint32_t* track_counts, const uint32_t* pose_counts, const int32_t* cols,
                                      const uint32_t* slots, uint32_t T_old, SaPoseTrackPlan* out) {
  *out = SaPoseTrackPlan();
  uint64_t poses = 0, tracks = 0;
  for (uint32_t s = 0; s < n_scenes; ++s) {
    poses += pose_counts[s];
    tracks += track_counts[s];
  }
  out->slot.resize((size_t)poses);
  out->rank.resize((size_t)poses);
  out->unmatched.resize(n_scenes);
  std::vector<uint8_t> taken((size_t)tracks, 0);
  size_t pose0 = 0, track0 = 0;
  for (uint32_t s = 0; s < n_scenes; ++s) {
    const uint32_t m = pose_counts[s], n = track_counts[s];
    uint32_t left = 0;
    for (uint32_t i = 0; i < m; ++i) {
      const int32_t c = cols[pose0 + i];
      if (c >= 0 && (uint32_t)c < n) {
        const size_t j = track0 + (uint32_t)c;
        taken[j] = 1;
        out->slot[pose0 + i] = slots ? slots[j] : (uint32_t)j;
        out->rank[pose0 + i] = SA_POSE_TRACK_NONE;
        ++out->matched;
      } else {
        out->slot[pose0 + i] = T_old + out->created;
        out->rank[pose0 + i] = out->created++;
        ++left;
      }
    }
    out->unmatched[s] = left;
    pose0 += m;
    track0 += n;
  }
  for (size_t j = 0; j < taken.size(); ++j)
    if (!taken[j]) out->coasted.push_back((uint32_t)j);
}
