// sa_pose_gate.h — the spatio-temporal gate of the keypoint tracker (include/similari_pose_sort.h), written once for the kernels of
// sa_pose.hip and for the host (tests/test_pose_sort_emu.py compiles this file with g++).
//
// The reference's trackers refuse a (candidate, track) pair in compatible() (src/trackers/sort.rs:250-270) before the metric is asked:
// SpatioTemporalConstraints::validate(epoch_delta, dist_in_2r) must hold, dist_in_2r being the distance of the two boxes' centres in
// units of the sum of their bounding circles' radii.  A pose has no box; its circle is the one around the bounding rectangle of the
// points that count — centre the rectangle's, radius half its diagonal, the shape of Universal2DBox::get_radius.  Minimum and maximum
// are exact, so the order in which the points are walked cannot change a bit.  All f32; build with -ffp-contract=off, as sa_device.h.
#pragma once
#include "sa_device.h"

// The running rectangle of a circle: empty until the first point.
struct sa_pose_rect {
  float xmin, xmax, ymin, ymax;
  uint32_t n;
};
SA_HD void sa_pose_rect_clear(sa_pose_rect& q) { q.xmin = q.xmax = q.ymin = q.ymax = 0.f; q.n = 0u; }
// one point that counts (finite: the presence rule of similari_points.h, or a stored mean)
SA_HD void sa_pose_rect_add(sa_pose_rect& q, float x, float y) {
  if (q.n == 0u) { q.xmin = q.xmax = x; q.ymin = q.ymax = y; }
  else {
    q.xmin = x < q.xmin ? x : q.xmin; q.xmax = x > q.xmax ? x : q.xmax;
    q.ymin = y < q.ymin ? y : q.ymin; q.ymax = y > q.ymax ? y : q.ymax;
  }
  q.n += 1u;
}
// -> (xc, yc, r) in a sa_geo (hha unused: 0) and whether there is a circle at all; one point gives r = 0, which sa_dist_in_2r allows
// (SA_EPS under its root)
SA_HD bool sa_pose_circle(const sa_pose_rect& q, sa_geo& c) {
  c.xc = c.yc = c.r = c.hha = 0.f;
  if (q.n == 0u) return false;
  c.xc = 0.5f * (q.xmin + q.xmax);
  c.yc = 0.5f * (q.ymin + q.ymax);
  const float hw = 0.5f * (q.xmax - q.xmin), hh = 0.5f * (q.ymax - q.ymin);
  c.r = sqrtf(hw * hw + hh * hh);
  return true;
}
// validate()'s rule as one number per track: the max_dist of the first of the n constraints (sorted by delta, deduplicated — as
// add_constraints leaves them) whose delta is >= epoch_delta; +inf: no constraint applies
SA_HD float sa_pose_limit(uint32_t n, const uint32_t* delta, const float* max_dist, uint64_t epoch_delta) {
  for (uint32_t i = 0; i < n; ++i)
    if ((uint64_t)delta[i] >= epoch_delta) return max_dist[i];
  return INFINITY;
}
// Is the pair refused?  An infinite limit refuses nothing; a side without a circle refuses nothing (such a pair has no common point
// and does not exist anyway); otherwise validate(): the pair stays iff dist_in_2r <= limit.
SA_HD bool sa_pose_refused(bool has_pose, const sa_geo& pose, bool has_track, const sa_geo& track, float limit) {
  if (limit == INFINITY || !has_pose || !has_track) return false;
  return !(sa_dist_in_2r(pose, track) <= limit);
}
