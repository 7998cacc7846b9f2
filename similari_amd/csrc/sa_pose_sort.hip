// sa_pose_sort.hip — the keypoint tracker (include/similari_pose_sort.h): Sort's life cycle around the frame loop of sa_pose.hip.
//
// What is here: the object, its refusals and the order of a frame.  The life cycle itself — epochs, expiry, the compaction's slot
// arithmetic, the limits, what the vote's answer does to the lists — is sa_pose_sort_plan.h, host arithmetic that a test compiles on its
// own.  The device work is in the two sources that own the bank: the gated vote, the step and the circles in sa_pose.hip (sort_track,
// sort_peek), the gather in front of the compaction in sa_points.hip (sort_remove); sa_points_impl.h declares them.
//
// A predict: sa_pose_sort_frame (nothing changes) -> every refusal -> sort_remove (queued: gather, move, the staging block's copy) ->
// sort_track (uploads, the launches, the copy back, the ONE wait) -> sa_pose_sort_absorb.  The staging block lands in host memory that
// lives until the wait; the wasted records are cut from it afterwards.  A frame that expires tracks and has neither a pose nor a track
// to coast launches nothing behind the removal, so it waits for the stream itself.
#include "sa_points_impl.h"
#include "sa_pose_sort_plan.h"
#include "../../include/similari_pose_sort.h"

#include <cstring>
#include <deque>

struct sa_pose_sort_wasted {
  SaPoseSortSlot rec;
  uint64_t scene_id;
  std::vector<uint8_t> has;
  std::vector<float> mean, cov;
};

struct sa_pose_sort {
  sa_points* b = nullptr;
  sa_pose_track_options opt{};
  SaPoseSortState s;
  std::deque<sa_pose_sort_wasted> wasted;
  sa_pose_sort_stats last{};
};

namespace {

using namespace sa_pt;

static_assert(SA_POSE_SORT_CONSTRAINTS == SA_POSE_SORT_MAX_CONSTRAINTS, "sa_pose_sort_plan.h states the limit of the public header");
static_assert(sizeof(sa_pose_sort_options) == 104 && sizeof(sa_pose_sort_track) == 32 && sizeof(sa_pose_sort_stats) == 144, "the layouts the header states");

// the frame of a call, or its refusal; m: the poses of the call
int plan_frame(sa_pose_sort* t, const char* what, uint32_t n_scenes, const uint64_t* scene_ids, const uint32_t* pose_counts, const sa_point_rows* poses,
               SaPoseSortFrame& f, uint64_t& m) {
  sa_engine* e = t->b->e;
  if (n_scenes && (!scene_ids || !pose_counts)) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null scene ids or pose counts", what);
  uint32_t bad = 0;
  switch (sa_pose_sort_frame(t->s, n_scenes, scene_ids, SA_POSE_MAX, &f, &bad)) {
    case SA_POSE_SORT_FITS: break;
    case SA_POSE_SORT_SCENE_TWICE:
      return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: scene %llu twice in one call (at %u)", what, (unsigned long long)scene_ids[bad], bad);
    case SA_POSE_SORT_SCENE_TOO_LARGE:
      return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: scene %llu has %u tracks; a scene takes at most %u", what, (unsigned long long)scene_ids[bad],
                            f.track_counts[bad], SA_POSE_MAX);
  }
  m = 0;
  for (uint32_t k = 0; k < n_scenes; ++k) m += pose_counts[k];
  if (n_scenes) SA_TRY(sort_check(t->b, what, n_scenes, f.track_counts.data(), pose_counts, poses, f.what_is.size()));
  return SA_OK;
}

// the tracker reports the extents launch as its gate launch: vote_launches is 3 whenever there was a vote
void stats_of(sa_pose_sort_stats& s, const PoseRan& r) {
  ran_into(s, r);
  s.vote_launches = r.vote_launches, s.step_launches = r.scan_launches + r.step_launches, s.gate_launches = r.extents_launches;
  s.gate_ms = r.gate_ms, s.refused_pairs = r.refused_pairs;
}

}  // namespace

extern "C" {

void sa_pose_sort_options_default(sa_pose_sort_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->struct_size = sizeof *o;
  sa_points_options po;
  sa_points_options_default(&po);
  o->points = po.points, o->position_weight = po.position_weight, o->velocity_weight = po.velocity_weight;
  o->max_idle_epochs = 5;
  o->min_common = 1;
  o->threshold = 1.0f;
  o->coast = 1;
}

int sa_pose_sort_create(sa_engine* e, const sa_pose_sort_options* o, sa_pose_sort** out) {
  const char* what = "sa_pose_sort_create";
  if (out) *out = nullptr;
  sa_points_options po;
  sa_points_options_default(&po);
  if (!e) {   // the bank's own answer: no device, or a null engine
    sa_points* none = nullptr;
    return sa_points_create(nullptr, &po, &none);
  }
  if (!o || !out) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
  if (o->struct_size != sizeof(sa_pose_sort_options)) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: struct_size %u (%zu)", what, o->struct_size, sizeof(sa_pose_sort_options));
  const sa_pose_track_options to{(uint32_t)sizeof(sa_pose_track_options), o->min_common, o->threshold, o->coast};
  SA_TRY(check_track_options(e, what, &to));
  if (o->n_constraints > SA_POSE_SORT_CONSTRAINTS)
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: %u constraints; a tracker takes at most %u", what, o->n_constraints, SA_POSE_SORT_CONSTRAINTS);
  for (uint32_t i = 0; i < o->n_constraints; ++i)
    if (!(o->max_dist[i] > 0.0f)) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: constraint %u: max_dist %g must be > 0", what, i, (double)o->max_dist[i]);
  po.points = o->points, po.position_weight = o->position_weight, po.velocity_weight = o->velocity_weight;
  sa_points* b = nullptr;
  SA_TRY(sa_points_create(e, &po, &b));
  sa_pose_sort* t = new sa_pose_sort();
  t->b = b;
  t->opt = to;
  t->s.max_idle = o->max_idle_epochs;
  sa_pose_sort_constraints(o->n_constraints, o->epoch_delta, o->max_dist, &t->s.cons);
  *out = t;
  return SA_OK;
}

void sa_pose_sort_destroy(sa_pose_sort* t) {
  if (!t) return;
  sa_points_destroy(t->b);
  delete t;
}

sa_points* sa_pose_sort_bank(sa_pose_sort* t) { return t ? t->b : nullptr; }

int sa_pose_sort_predict(sa_pose_sort* t, uint32_t n_scenes, const uint64_t* scene_ids, const uint32_t* pose_counts, const sa_point_rows* poses,
                         sa_pose_sort_track* out, float* out_xy) {
  const char* what = "sa_pose_sort_predict";
  if (!t) return SA_ERR_BAD_ARG;
  sa_points* b = t->b;
  SA_TRY(enter(b, what));
  t->last = sa_pose_sort_stats{};
  SaPoseSortFrame f;
  uint64_t m64 = 0;
  SA_TRY(plan_frame(t, what, n_scenes, scene_ids, pose_counts, poses, f, m64));
  const uint32_t m = (uint32_t)m64;
  if (m && !out) return sa_engine_fail(b->e, SA_ERR_BAD_ARG, "%s: null out", what);
  if (n_scenes == 0) return SA_OK;
  // nothing is refused from here on
  std::vector<SaPoseSortSlot> left;
  sa_pose_sort_expire(&t->s, n_scenes, scene_ids, f, &left);
  PoseRan gone, r;   // the removal's traffic, the frame loop's
  const size_t lp = left.size() * b->P;
  std::vector<uint8_t> stage(lp * 81);
  if (!left.empty()) SA_TRY(sort_remove(b, f.leaving, f.what_is, stage.data(), gone));
  const uint32_t n = (uint32_t)f.slots.size();
  std::vector<float> w((size_t)m + 1);
  SaPoseTrackPlan tp;
  SA_TRY(sort_track(b, what, n_scenes, f.track_counts.data(), pose_counts, poses, f.slots.data(), f.gated ? f.limits.data() : nullptr, t->s.next_id, &t->opt,
                    w.data(), out_xy, &tp, r));
  if (!left.empty() && r.step_launches == 0) {   // nothing ran behind the removal: its copy is still in flight
    SA_HIPCHK(b->e, hipStreamSynchronize(b->st));
  }
  sa_pose_sort_absorb(&t->s, f, pose_counts, tp);
  size_t i = 0;
  for (uint32_t k = 0; k < n_scenes; ++k)
    for (uint32_t q = 0; q < pose_counts[k]; ++q, ++i) {
      const SaPoseSortSlot& s = t->s.slot[tp.slot[i]];
      const bool made = tp.rank[i] != SA_POSE_TRACK_NONE;
      out[i] = sa_pose_sort_track{s.id, scene_ids[k], f.epoch[k], s.length, made ? NAN : w[i], made ? 1u : 0u};
    }
  for (size_t k = 0; k < left.size(); ++k) {   // the staging block: mean [n][P][4], cov [n][P][16], has [n][P]
    sa_pose_sort_wasted rec;
    rec.rec = left[k], rec.scene_id = t->s.scene_id[left[k].scene];
    const size_t P = b->P;
    const float* mean = (const float*)stage.data() + k * P * 4;
    const float* cov = (const float*)stage.data() + lp * 4 + k * P * 16;
    const uint8_t* has = stage.data() + lp * 80 + k * P;
    rec.has.assign(has, has + P);
    rec.mean.assign(mean, mean + P * 4);
    rec.cov.assign(cov, cov + P * 16);
    for (size_t p = 0; p < P; ++p)
      if (!rec.has[p]) {
        std::fill(rec.mean.begin() + p * 4, rec.mean.begin() + p * 4 + 4, NAN);
        std::fill(rec.cov.begin() + p * 16, rec.cov.begin() + p * 16 + 16, NAN);
      }
    t->wasted.push_back(std::move(rec));
  }
  sa_pose_sort_stats s{};
  s.scenes = n_scenes, s.poses = m, s.tracks = n;
  stats_of(s, r);
  s.bytes_h2d += gone.bytes_h2d, s.bytes_d2h += gone.bytes_d2h;
  s.matched = tp.matched, s.created = tp.created, s.coasted = t->opt.coast ? (uint32_t)tp.coasted.size() : 0u;
  s.expired = (uint32_t)left.size();
  if (!left.empty()) SA_TRY(sort_remove_ms(b, &s.gather_ms));
  t->last = s;
  return SA_OK;
}

uint64_t sa_pose_sort_peek_cells(sa_pose_sort* t, uint32_t n_scenes, const uint64_t* scene_ids, const uint32_t* pose_counts) {
  if (!t || !n_scenes || !scene_ids || !pose_counts) return 0;
  SaPoseSortFrame f;
  uint32_t bad = 0;
  if (sa_pose_sort_frame(t->s, n_scenes, scene_ids, SA_POSE_MAX, &f, &bad) != SA_POSE_SORT_FITS) return 0;
  uint64_t cells = 0;
  for (uint32_t k = 0; k < n_scenes; ++k) cells += (uint64_t)pose_counts[k] * f.track_counts[k];
  return cells;
}

int sa_pose_sort_peek(sa_pose_sort* t, uint32_t n_scenes, const uint64_t* scene_ids, const uint32_t* pose_counts, const sa_point_rows* poses,
                      uint64_t* out_track, float* out_weight, uint32_t* out_track_counts, float* out_tap) {
  const char* what = "sa_pose_sort_peek";
  if (!t) return SA_ERR_BAD_ARG;
  sa_points* b = t->b;
  SA_TRY(enter(b, what));
  t->last = sa_pose_sort_stats{};
  SaPoseSortFrame f;
  uint64_t m64 = 0;
  SA_TRY(plan_frame(t, what, n_scenes, scene_ids, pose_counts, poses, f, m64));
  const uint32_t m = (uint32_t)m64;
  if (m && (!out_track || !out_weight)) return sa_engine_fail(b->e, SA_ERR_BAD_ARG, "%s: null argument", what);
  if (n_scenes == 0) return SA_OK;
  if (out_track_counts) std::copy(f.track_counts.begin(), f.track_counts.end(), out_track_counts);
  std::vector<int32_t> cols((size_t)m + 1);
  PoseRan r;   // nothing is removed: the slots as they are
  SA_TRY(sort_peek(b, what, n_scenes, f.track_counts.data(), pose_counts, poses, f.old_slots.data(), f.gated ? f.limits.data() : nullptr, &t->opt, cols.data(),
                   out_weight, out_tap, r));
  sa_pose_sort_stats s{};
  size_t i = 0, track0 = 0;
  for (uint32_t k = 0; k < n_scenes; ++k) {
    for (uint32_t q = 0; q < pose_counts[k]; ++q, ++i) {
      out_track[i] = cols[i] >= 0 ? t->s.slot[f.old_slots[track0 + (uint32_t)cols[i]]].id : 0;
      s.matched += cols[i] >= 0;
    }
    track0 += f.track_counts[k];
  }
  s.scenes = n_scenes, s.poses = m, s.tracks = (uint32_t)f.slots.size(), s.expired = (uint32_t)f.leaving.size();
  stats_of(s, r);
  t->last = s;
  return SA_OK;
}

int sa_pose_sort_wasted_count(sa_pose_sort* t, uint32_t* out_n) {
  if (!t || !out_n) return SA_ERR_BAD_ARG;
  *out_n = (uint32_t)t->wasted.size();
  return SA_OK;
}

int sa_pose_sort_wasted_take(sa_pose_sort* t, uint32_t cap, uint64_t* ids, uint64_t* scenes, uint32_t* first, uint32_t* last, uint32_t* length,
                             uint8_t* has, float* mean, float* cov, uint32_t* out_n) {
  if (!t || !out_n) return SA_ERR_BAD_ARG;
  *out_n = 0;
  if (cap && (!ids || !scenes || !first || !last || !length || !has || !mean || !cov)) return SA_ERR_BAD_ARG;
  const size_t P = t->b->P;
  uint32_t k = 0;
  for (; k < cap && !t->wasted.empty(); ++k) {
    const sa_pose_sort_wasted& w = t->wasted.front();
    ids[k] = w.rec.id, scenes[k] = w.scene_id, first[k] = w.rec.first, last[k] = w.rec.last, length[k] = w.rec.length;
    std::memcpy(has + k * P, w.has.data(), P);
    std::memcpy(mean + k * P * 4, w.mean.data(), P * 16);
    std::memcpy(cov + k * P * 16, w.cov.data(), P * 64);
    t->wasted.pop_front();
  }
  *out_n = k;
  return SA_OK;
}

int sa_pose_sort_skip_epochs(sa_pose_sort* t, uint64_t scene, uint32_t n) {
  if (!t) return SA_ERR_BAD_ARG;
  sa_pose_sort_skip(&t->s, scene, n);
  return SA_OK;
}

int sa_pose_sort_epoch(sa_pose_sort* t, uint64_t scene, uint32_t* out_epoch) {
  if (!t || !out_epoch) return SA_ERR_BAD_ARG;
  const auto it = t->s.scene_of.find(scene);
  *out_epoch = it == t->s.scene_of.end() ? 0u : t->s.epoch[it->second];
  return SA_OK;
}

int sa_pose_sort_active(sa_pose_sort* t, uint64_t scene, uint32_t* out_n) {
  if (!t || !out_n) return SA_ERR_BAD_ARG;
  if (scene == SA_POSE_SORT_ALL_SCENES) { *out_n = (uint32_t)t->s.slot.size(); return SA_OK; }
  const auto it = t->s.scene_of.find(scene);
  *out_n = it == t->s.scene_of.end() ? 0u : (uint32_t)t->s.list[it->second].size();
  return SA_OK;
}

int sa_pose_sort_last(sa_pose_sort* t, sa_pose_sort_stats* out) {
  if (!t || !out) return SA_ERR_BAD_ARG;
  *out = t->last;
  out->struct_size = sizeof *out;
  return SA_OK;
}

}  // extern "C"
