// sa_pose_sort_plan.h — the host's half of the keypoint tracker (include/similari_pose_sort.h): the scenes' epochs and track lists, the
// per-slot records, the id counter, and what one frame does to them.  Host arithmetic only: sa_pose_sort.hip runs it around the device
// calls, and tests/test_pose_sort_plan.py compiles this header with the host compiler and compares it with tests/pose_sort_ref.py.
//
// A frame in three steps.  sa_pose_sort_frame works out, changing nothing, what the frame will do: the named scenes' new epochs, the
// tracks that expire (scenes in call order, then list order), the compaction of the bank (sa_points_remove's rule: the last track moves
// into each hole in turn), the remaining tracks of every named scene as slots AFTER the compaction, and each one's limit
// (sa_pose_gate.h: validate()'s rule resolved per track, because the limit depends on the track alone).  The caller refuses or goes on.
// sa_pose_sort_expire applies the epochs and the removal; sa_pose_sort_absorb applies what the vote returned (sa_pose_track_plan.h).
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <unordered_map>
#include <utility>
#include <vector>

#include "sa_pose_track_plan.h"

#define SA_POSE_SORT_MAX_CONSTRAINTS 8
#define SA_POSE_SORT_NONE 0xffffffffu

enum SaPoseSortFit { SA_POSE_SORT_FITS = 0, SA_POSE_SORT_SCENE_TWICE, SA_POSE_SORT_SCENE_TOO_LARGE };

struct SaPoseSortSlot {
  uint64_t id;
  uint32_t scene;   // index into the scene table
  uint32_t first, last, length;
};
struct SaPoseSortState {
  uint32_t max_idle = 0;
  std::vector<std::pair<uint32_t, float>> cons;          // sorted by delta, one per delta
  std::unordered_map<uint64_t, uint32_t> scene_of;       // scene id -> index
  std::vector<uint64_t> scene_id;
  std::vector<uint32_t> epoch;
  std::vector<std::vector<uint32_t>> list;               // per scene: its tracks' slots in creation order
  std::vector<SaPoseSortSlot> slot;                      // per slot of the bank
  uint64_t next_id = 1;
};

// add_constraints (src/trackers/spatio_temporal_constraints.rs:36-46): a stable sort by delta, then of equal deltas the first stays
static inline void sa_pose_sort_constraints(uint32_t n, const uint32_t* delta, const float* max_dist, std::vector<std::pair<uint32_t, float>>* out) {
  out->clear();
  for (uint32_t i = 0; i < n; ++i) out->push_back({delta[i], max_dist[i]});
  std::stable_sort(out->begin(), out->end(), [](const std::pair<uint32_t, float>& a, const std::pair<uint32_t, float>& b) { return a.first < b.first; });
  out->erase(std::unique(out->begin(), out->end(), [](const std::pair<uint32_t, float>& a, const std::pair<uint32_t, float>& b) { return a.first == b.first; }),
             out->end());
}
// validate()'s choice: the max_dist of the first constraint whose delta is >= epoch_delta, +inf: none (sa_pose_limit of sa_pose_gate.h on
// the tracker's own table)
static inline float sa_pose_sort_limit(const std::vector<std::pair<uint32_t, float>>& cons, uint64_t epoch_delta) {
  for (const auto& c : cons)
    if ((uint64_t)c.first >= epoch_delta) return c.second;
  return INFINITY;
}

// The compaction of a removal by slots: `leaving` in call order, each the slot a track has BEFORE the call; T0 tracks.
// -> what_is [T0 - leaving]: the old slot whose track ends in each slot; new_of [T0]: where each old slot's track ends, NONE: it left.
static inline void sa_pose_sort_compact(uint32_t T0, const std::vector<uint32_t>& leaving, std::vector<uint32_t>* what_is, std::vector<uint32_t>* new_of) {
  std::vector<uint32_t> at(T0), is(T0);   // at[old]: where the old slot's track is now; is[s]: the old slot of the track now in s
  for (uint32_t s = 0; s < T0; ++s) at[s] = is[s] = s;
  uint32_t T = T0;
  for (uint32_t old : leaving) {
    const uint32_t hole = at[old], last = T - 1;
    if (hole != last) {
      is[hole] = is[last];
      at[is[hole]] = hole;
    }
    at[old] = SA_POSE_SORT_NONE;
    --T;
  }
  is.resize(T);
  *what_is = is;
  *new_of = at;
}

struct SaPoseSortFrame {
  std::vector<uint32_t> scene;          // [named] index into the scene table; an unseen scene gets the next free index
  std::vector<uint32_t> epoch;          // [named] the scene's epoch in this frame
  std::vector<uint32_t> leaving;        // the expired tracks' slots as they are before the frame
  std::vector<uint32_t> what_is, new_of;
  std::vector<uint32_t> track_counts;   // [named] the remaining tracks of each scene
  std::vector<uint32_t> slots;          // their slots after the compaction, scene after scene in list order
  std::vector<uint32_t> old_slots;      // and before it (a peek removes nothing)
  std::vector<float> limits;            // and their limits
  bool gated = false;                   // at least one limit is finite
  uint32_t new_scenes = 0;
};

// -> SA_POSE_SORT_FITS, or the refusal with *bad = the position of the scene in the call
static inline SaPoseSortFit sa_pose_sort_frame(const SaPoseSortState& t, uint32_t n_scenes, const uint64_t* scene_ids, uint32_t max_tracks,
                                               SaPoseSortFrame* f, uint32_t* bad) {
  *f = SaPoseSortFrame();
  std::unordered_map<uint64_t, uint32_t> named;
  named.reserve((size_t)n_scenes * 2u);
  for (uint32_t k = 0; k < n_scenes; ++k) {
    if (!named.emplace(scene_ids[k], k).second) { *bad = k; return SA_POSE_SORT_SCENE_TWICE; }
    const auto it = t.scene_of.find(scene_ids[k]);
    const bool known = it != t.scene_of.end();
    f->scene.push_back(known ? it->second : (uint32_t)t.scene_id.size() + f->new_scenes++);
    f->epoch.push_back(known ? t.epoch[it->second] + 1u : 1u);
  }
  for (uint32_t k = 0; k < n_scenes; ++k) {
    if (f->scene[k] >= t.list.size()) continue;
    for (uint32_t s : t.list[f->scene[k]])
      if ((uint64_t)f->epoch[k] - t.slot[s].last > t.max_idle) f->leaving.push_back(s);
  }
  sa_pose_sort_compact((uint32_t)t.slot.size(), f->leaving, &f->what_is, &f->new_of);
  for (uint32_t k = 0; k < n_scenes; ++k) {
    uint32_t n = 0;
    if (f->scene[k] < t.list.size())
      for (uint32_t s : t.list[f->scene[k]]) {
        if (f->new_of[s] == SA_POSE_SORT_NONE) continue;
        const float lim = sa_pose_sort_limit(t.cons, (uint64_t)f->epoch[k] - t.slot[s].last);
        f->slots.push_back(f->new_of[s]);
        f->old_slots.push_back(s);
        f->limits.push_back(lim);
        f->gated = f->gated || lim != INFINITY;
        ++n;
      }
    f->track_counts.push_back(n);
    if (n > max_tracks) { *bad = k; return SA_POSE_SORT_SCENE_TOO_LARGE; }
  }
  return SA_POSE_SORT_FITS;
}

// the frame's epochs and its removal -> the records of the tracks that left, in `leaving` order
static inline void sa_pose_sort_expire(SaPoseSortState* t, uint32_t n_scenes, const uint64_t* scene_ids, const SaPoseSortFrame& f,
                                       std::vector<SaPoseSortSlot>* left) {
  left->clear();
  for (uint32_t k = 0; k < n_scenes; ++k) {
    if (f.scene[k] >= t->scene_id.size()) {   // (new scenes take their indices in call order, as the frame numbered them)
      t->scene_of.emplace(scene_ids[k], (uint32_t)t->scene_id.size());
      t->scene_id.push_back(scene_ids[k]);
      t->epoch.push_back(0u);
      t->list.emplace_back();
    }
    t->epoch[f.scene[k]] = f.epoch[k];
  }
  if (f.leaving.empty()) return;
  for (uint32_t s : f.leaving) left->push_back(t->slot[s]);
  for (auto& l : t->list) {   // every list: a moved track may belong to a scene the frame does not name
    size_t w = 0;
    for (uint32_t s : l)
      if (f.new_of[s] != SA_POSE_SORT_NONE) l[w++] = f.new_of[s];
    l.resize(w);
  }
  std::vector<SaPoseSortSlot> slot(f.what_is.size());
  for (size_t s = 0; s < slot.size(); ++s) slot[s] = t->slot[f.what_is[s]];
  t->slot.swap(slot);
}

// what the vote did (p: sa_pose_track_plan over the frame's scenes, T_old = the slots before it): a matched track was seen in this
// epoch, a created one joins its scene's list; the counter advances by the created count
static inline void sa_pose_sort_absorb(SaPoseSortState* t, const SaPoseSortFrame& f, const uint32_t* pose_counts, const SaPoseTrackPlan& p) {
  size_t i = 0;
  for (size_t k = 0; k < f.scene.size(); ++k)
    for (uint32_t q = 0; q < pose_counts[k]; ++q, ++i) {
      if (p.rank[i] == SA_POSE_TRACK_NONE) {
        SaPoseSortSlot& s = t->slot[p.slot[i]];
        s.last = f.epoch[k];
        s.length += 1u;
      } else {   // (slots are handed out in call order: this one is the next)
        t->slot.push_back(SaPoseSortSlot{t->next_id + p.rank[i], f.scene[k], f.epoch[k], f.epoch[k], 1u});
        t->list[f.scene[k]].push_back(p.slot[i]);
      }
    }
  t->next_id += p.created;
}

// a scene's epoch moves on by n without a frame; an unseen scene starts at n
static inline void sa_pose_sort_skip(SaPoseSortState* t, uint64_t scene_id, uint32_t n) {
  const auto it = t->scene_of.find(scene_id);
  if (it != t->scene_of.end()) { t->epoch[it->second] += n; return; }
  t->scene_of.emplace(scene_id, (uint32_t)t->scene_id.size());
  t->scene_id.push_back(scene_id);
  t->epoch.push_back(n);
  t->list.emplace_back();
}
