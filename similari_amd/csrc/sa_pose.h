// sa_pose.h — the pair weight of the keypoint association (include/similari_pose.h), written once for the kernels of sa_pose.hip and for
// the host (tests/emu_pose compiles this file with g++).
//
// Pose i against track j, points p ascending: point p is COMMON iff it is present in the pose, the track's point has a state whose
// factor exists (sa_pkf_factor) and the distance is not NaN; c_p = calculate_cost(d2, inverted = true); w = (c_p1 + c_p2 + ...) / (f32)k,
// an f32 sum in ascending p seeded by the first term; the pair exists iff k >= min_common.  The vote is SortVoting::winners
// (sort/voting.rs): weight sa_quantise(w) against the diagonal threshold_q; a pair is a usable edge iff its gain is positive.
// Build with -ffp-contract=off, as sa_kalman_point.h.
#pragma once
#include "sa_kalman_point.h"

// one point of a cell: (sum, k) take point p, whose factor is f (ok: the track's point has a state and both pivots held)
SA_HD void sa_pose_acc(float& sum, uint32_t& k, bool ok, const sa_pkf_fac& f, bool present, float zx, float zy) {
  if (!ok || !present) return;
  const float d2 = sa_pkf_distance_factored(f, zx, zy);
  if (d2 != d2) return;
  const float c = sa_pkf_cost(d2, true);
  sum = k ? sum + c : c;
  k += 1u;
}
// the weight of the cell, NaN = no pair
SA_HD float sa_pose_weight(float sum, uint32_t k, uint32_t min_common) { return k >= min_common && k ? sum / (float)k : NAN; }
// the diagonal of SortVoting's matrix: (threshold * 1e6f) as i64
SA_HD int64_t sa_pose_threshold_q(float threshold) { return sa_quantise(threshold); }
// the gain of the cell over the diagonal, 0 = no usable edge
SA_HD int64_t sa_pose_gain(float w, int64_t threshold_q) {
  if (w != w) return 0;
  const int64_t g = sa_quantise(w) - threshold_q;
  return g > 0 ? g : 0;
}
// A row's bid: (gain << 16) | (0xffff - column) — the unsigned maximum is the heaviest gain and, on ties, the lowest column.  Gains are
// at most 1e8 (w <= 100, threshold >= 0) and columns at most 2047, so nothing is lost; 0 = the row has no usable edge.
SA_HD unsigned long long sa_pose_word(int64_t gain, uint32_t col) { return ((unsigned long long)gain << 16) | (unsigned long long)(0xffffu - col); }
SA_HD int64_t sa_pose_word_gain(unsigned long long w) { return (int64_t)(w >> 16); }
SA_HD uint32_t sa_pose_word_col(unsigned long long w) { return 0xffffu - (uint32_t)(w & 0xffffu); }
