// sa_pose_oks.h — object keypoint similarity, the overlap metric of the keypoint association (include/similari_pose_oks.h), written
// once for the kernels of sa_pose.hip and for the host (tests/emu_oks compiles this file with g++).
//
// Pose i against track j.  Each side has an EXTENT: the bounding rectangle (sa_pose_rect, sa_pose_gate.h) of the pose's present points,
// or of the stored means of the track's points that have a state, and its area a = (xmax - xmin) * (ymax - ymin); a side without a
// point has no area (NaN).  The SCALE of the pair is s2 = 0.5f * (a_pose + a_track), the mean of the two areas — the common choice
// where no ground-truth area exists.  The pair is REFUSED iff !(s2 > 0), NaN included: no weight (NaN in the tap), no gain, no match.
// Two single-point sides, collinear (axis-parallel) points on both sides and every P = 1 bank have s2 = 0 and are refused: OKS needs
// a body size, and such a pair has none.
//
// Points p ascending: point p is COMMON iff it is present in the pose, the track's point has a state and e is not NaN, with
//   dx = zx - mx; dy = zy - my; d2 = dx * dx + dy * dy; e = d2 / (s2 * var2_p);   var2_p = 2 (2 sigma_p)^2 (sa_oks_var2, the host)
// c_p = sa_oks_exp(e); w = (c_p1 + c_p2 + ...) / (f32)k, an f32 sum in ascending p seeded by the first term; the pair exists iff
// k >= min_common: sa_pose.h's rule, and sa_pose_weight, sa_pose_gain and sa_pose_word are reused as they are.  Weights lie in [0, 1],
// so gains stay at or below 1e6 and fit the bid word.
//
// sa_oks_exp(e) = exp(-e) is DEFINED here, by f32 + - *, rintf, one float-to-int conversion and a power of two assembled from exponent
// bits: expf, __expf and exp2f give other bits in libm than on the device, and the bits are the contract.  All f32; build with
// -ffp-contract=off, as sa_pose.h.
#pragma once
#include "sa_pose_gate.h"

// exp(-e) for e >= 0.  Exactly 1 at 0; exactly 0 for every e with !(e < 32) (NaN included): exp(-32) ~ 1.3e-14 is far under the vote's
// 1e-6 quantum — the cut plays the part of calculate_cost's 11.070 — and it keeps 2^n a normal number (n >= -47), so no denormal mode
// matters.  Cody-Waite: n = rint(x log2 e), r = x - n ln2_hi - n ln2_lo with |r| <= 0.3466 (n * ln2_hi is exact: ln2_hi is 355 / 512,
// nine significant bits, and n has six), then the degree-6 Taylor form by Horner.  For n = 0, r <= 0 and the form is <= 1; for n <= -1 it is below
// 1.42 / 2: every result lies in [0, 1].
SA_HD float sa_oks_exp(float e) {
  if (!(e < 32.f)) return 0.f;
  const float x = -e;
  const float n = rintf(x * 1.44269504f);
  float r = x - n * 0.693359375f;
  r = r - n * -2.12194440e-4f;
  float p = 1.f / 720.f;
  p = p * r + 1.f / 120.f;
  p = p * r + 1.f / 24.f;
  p = p * r + 1.f / 6.f;
  p = p * r + 0.5f;
  p = p * r + 1.f;
  p = p * r + 1.f;
  union { uint32_t u; float f; } s;
  s.u = (uint32_t)((int32_t)n + 127) << 23;
  return p * s.f;
}
// the per-point constant from the caller's sigma: 2 (2 sigma)^2
SA_HD float sa_oks_var2(float sigma) {
  const float k = 2.f * sigma;
  return 2.f * (k * k);
}
// the area of a side's extent, NaN: the side has no point
SA_HD float sa_oks_area(const sa_pose_rect& q) { return q.n ? (q.xmax - q.xmin) * (q.ymax - q.ymin) : NAN; }
// the scale of a pair, and whether it refuses the pair
SA_HD float sa_oks_scale(float a_pose, float a_track) { return 0.5f * (a_pose + a_track); }
SA_HD bool sa_oks_refused(float s2) { return !(s2 > 0.f); }
// one point of a cell: (sum, k) take point p, whose stored mean is (mx, my) (has: the track's point has a state)
SA_HD void sa_oks_acc(float& sum, uint32_t& k, bool has, float mx, float my, bool present, float zx, float zy, float s2, float var2) {
  if (!has || !present) return;
  const float dx = zx - mx, dy = zy - my;
  const float d2 = dx * dx + dy * dy;
  const float e = d2 / (s2 * var2);
  if (e != e) return;
  const float c = sa_oks_exp(e);
  sum = k ? sum + c : c;
  k += 1u;
}
