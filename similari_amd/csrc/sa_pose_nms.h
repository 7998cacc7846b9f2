// sa_pose_nms.h — pose NMS by OKS (include/similari_pose_nms.h), written once for the kernels of sa_pose_nms.hip and for the host
// (tests/emu_pose_nms compiles this file with g++).  Nothing numeric is new here: the presence rule is sa_point_present
// (sa_kalman_point.h), the extent sa_pose_rect (sa_pose_gate.h), the cell sa_oks_acc over sa_oks_scale / sa_oks_refused (sa_pose_oks.h) and
// the weight rule sa_pose_weight (sa_pose.h).  What is here: a pose point as the pair loop takes it, the pair loop with the EARLIER pose
// where the track stands, the strict comparison, and the host's part — filter, stable rank, greedy pass.  All f32; build with
// -ffp-contract=off, as sa_pose.h.
#pragma once
#include "sa_pose.h"
#include "sa_pose_oks.h"

#include <algorithm>
#include <vector>

// one point of a pose: x = NaN for an absent one (the shape k_pose_tile stages).  sa_pose_nms_point is the host's form of it
// (tests/emu_pose_nms); the kernels read theirs through sa_point_at<SRC> (sa_point_rows.h), the same rule over a device row.
struct alignas(8) sa_xy {
  float x, y;
};
SA_HD sa_xy sa_pose_nms_point(float x, float y, bool scored, float score, float min_score, bool masked_in) {
  return sa_point_present(x, y, scored, score, min_score, masked_in) ? sa_xy{x, y} : sa_xy{NAN, 0.f};
}
// the area of the extent of a pose whose P points lie at z[0], z[stride], ...; NaN: no point is present
SA_HD float sa_pose_nms_area(const sa_xy* z, size_t stride, uint32_t P) {
  sa_pose_rect q;
  sa_pose_rect_clear(q);
  for (uint32_t p = 0; p < P; ++p) {
    const sa_xy v = z[(size_t)p * stride];
    if (v.x == v.x) sa_pose_rect_add(q, v.x, v.y);
  }
  return sa_oks_area(q);
}
// one point of a pair: (sum, k) take point p of the earlier pose (where sa_oks_acc has the track) and of the later one
SA_HD void sa_pose_nms_acc(float& sum, uint32_t& k, sa_xy earlier, sa_xy later, float s2, float var2) {
  sa_oks_acc(sum, k, earlier.x == earlier.x, earlier.x, earlier.y, later.x == later.x, later.x, later.y, s2, var2);
}
// the weight of the pair, NaN: it does not exist (k < min_common) or is refused by its scale
SA_HD float sa_pose_nms_weight(float sum, uint32_t k, uint32_t min_common, float s2) {
  const float w = sa_pose_weight(sum, k, min_common);
  return sa_oks_refused(s2) ? NAN : w;
}
// nms.rs:63: strictly above; a NaN on either side suppresses nothing
SA_HD bool sa_pose_nms_suppresses(float w, float nms_threshold) { return w > nms_threshold; }
// the whole pair: points p ascending, both poses strided
SA_HD float sa_pose_nms_pair(uint32_t P, const float* var2, uint32_t min_common, const sa_xy* earlier, size_t stride_e, float area_e,
                             const sa_xy* later, size_t stride_l, float area_l) {
  const float s2 = sa_oks_scale(area_e, area_l);
  float sum = 0.f;
  uint32_t k = 0;
  for (uint32_t p = 0; p < P; ++p) sa_pose_nms_acc(sum, k, earlier[(size_t)p * stride_e], later[(size_t)p * stride_l], s2, var2[p]);
  return sa_pose_nms_weight(sum, k, min_common, s2);
}

// ---- the host's part --------------------------------------------------------------------------------------------------------------
// nms.rs:36-56 from the scores alone: the poses with score > score_threshold (NaN: f32::MIN; a NaN score never passes) as indices
// into the scene, by score descending, stable in the caller's order — nms_rank of sa_engine.hip without the box tests.
static inline void sa_pose_nms_rank(uint32_t m, const float* scores, float score_threshold, std::vector<uint32_t>& src) {
  const float thr = score_threshold == score_threshold ? score_threshold : -3.4028234663852886e38f;
  src.clear();
  src.reserve(m);
  for (uint32_t i = 0; i < m; ++i)
    if (scores[i] > thr) src.push_back(i);
  std::stable_sort(src.begin(), src.end(), [scores](uint32_t a, uint32_t b) { return scores[a] > scores[b]; });
}
// nms.rs:58-70 over the pairs of n ranked poses; w(i, j), i < j: the pair's weight.  keep [n]: 1 = survives.
template <class W>
static inline void sa_pose_nms_greedy(uint32_t n, float nms_threshold, W w, uint8_t* keep) {
  std::fill(keep, keep + n, (uint8_t)1);
  for (uint32_t i = 0; i < n; ++i) {
    if (!keep[i]) continue;
    for (uint32_t j = i + 1; j < n; ++j)
      if (keep[j] && sa_pose_nms_suppresses(w(i, j), nms_threshold)) keep[j] = 0;
  }
}
