// sa_kalman_point.h — the 4-state / 2-measurement point Kalman filter of the reference, written once for the device-side point bank
// (sa_points.hip) and for the host (tests/emu_points compiles this file with g++).
//
//   Point2DKalmanFilter::{initiate, predict, project, update, distance, calculate_cost}   src/utils/kalman/kalman_2d_point.rs:51-151
//   Vec2DKalmanFilter: the same filter applied to every point of a vector                   src/utils/kalman/kalman_2d_point_vec.rs
//   make_prediction                                                                          src/trackers/kalman_prediction.rs:13-32
//
// Written like sa_kalman.h against the filter's structure (motion = I + shift, update matrix = [I 0]): the multiplications by the
// constant 0 / 1 entries of those matrices are skipped, every remaining f32 operation keeps the reference's order (nalgebra's
// k-ascending sums seeded by the first product, its column-oriented forward substitution), so host and device produce the bits of the
// dense restatement tests/points_ref.py, which tests/test_points_ref.py pins to the oracle's box filter.  The covariance is a general
// 4 x 4 matrix: nothing assumes that the x and y blocks stay decoupled.  Build with -ffp-contract=off (rustc never fuses a*b+c).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/similari_assoc.h"
#include "sa_device.h"

#define SA_POINT_CHI2INV95_2 5.9915f   // CHI2INV95[1]  src/utils/kalman.rs:18-20

struct sa_pkf {
  float mean[4];   // x, y, vx, vy
  float cov[16];   // row-major
};

SA_HD bool sa_point_finite(float v) { return (v - v) == 0.0f; }

// Is a point of a call there?  Its coordinates are finite, its score (comps == 3) reaches min_score — a NaN score does not —, and the
// caller's mask, where there is one, says so.
SA_HD bool sa_point_present(float x, float y, bool scored, float score, float min_score, bool masked_in) {
  return masked_in && sa_point_finite(x) && sa_point_finite(y) && (!scored || score >= min_score);
}

SA_HD void sa_pkf_initiate(float pw, float vw, float x, float y, sa_pkf& s) {  // kalman_2d_point.rs:51-65
  const float sp = 2.0f * pw, sv = 10.0f * vw;
  s.mean[0] = x; s.mean[1] = y; s.mean[2] = 0.0f; s.mean[3] = 0.0f;
  for (int i = 0; i < 16; ++i) s.cov[i] = 0.0f;
  s.cov[0] = sp * sp; s.cov[5] = sp * sp; s.cov[10] = sv * sv; s.cov[15] = sv * sv;
}

SA_HD void sa_pkf_predict(float pw, float vw, sa_pkf& s) {  // kalman_2d_point.rs:67-84
  const float q[4] = {pw * pw, pw * pw, vw * vw, vw * vw};
  for (int i = 0; i < 2; ++i) s.mean[i] = s.mean[i] + s.mean[i + 2];
  float mc[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) mc[i * 4 + j] = i < 2 ? s.cov[i * 4 + j] + s.cov[(i + 2) * 4 + j] : s.cov[i * 4 + j];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      const float v = j < 2 ? mc[i * 4 + j] + mc[i * 4 + j + 2] : mc[i * 4 + j];
      s.cov[i * 4 + j] = v + (i == j ? q[i] : 0.0f);
    }
}

// project()  kalman_2d_point.rs:86-101 : the projected mean is mean[0..2], this is the projected covariance
SA_HD void sa_pkf_project(float pw, const sa_pkf& s, float* pc4) {
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) pc4[i * 2 + j] = s.cov[i * 4 + j] + (i == j ? pw * pw : 0.0f);
}

SA_HD void sa_pkf_update(float pw, sa_pkf& s, float zx, float zy) {  // kalman_2d_point.rs:103-121
  float P[4];
  sa_pkf_project(pw, s, P);
  // kalman_gain = projected_cov.solve_lower_triangular(B), B[r][c] = cov[c][r]: the UN-factorised covariance is used as the
  // triangular matrix — the reference's formula, kept as is (sa_kalman.h does the same with five rows)
  float G[8];
  for (int r = 0; r < 2; ++r)
    for (int c = 0; c < 4; ++c) G[r * 4 + c] = s.cov[c * 4 + r];
  for (int c = 0; c < 4; ++c)
    for (int i = 0; i < 2; ++i) {
      const float coeff = G[i * 4 + c] / P[i * 2 + i];
      G[i * 4 + c] = coeff;
      const float nc = -coeff;
      for (int r = i + 1; r < 2; ++r) G[r * 4 + c] = nc * P[r * 2 + i] + G[r * 4 + c];
    }
  const float innov[2] = {zx - s.mean[0], zy - s.mean[1]};
  float nm[4];
  for (int c = 0; c < 4; ++c) {
    float acc = innov[0] * G[c];
    acc = innov[1] * G[4 + c] + acc;
    nm[c] = s.mean[c] + acc;
  }
  float gtp[8];  // 4 x 2
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 2; ++j) {
      float acc = G[i] * P[j];
      acc = G[4 + i] * P[2 + j] + acc;
      gtp[i * 2 + j] = acc;
    }
  float nc[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      float acc = gtp[i * 2] * G[j];
      acc = gtp[i * 2 + 1] * G[4 + j] + acc;
      nc[i * 4 + j] = s.cov[i * 4 + j] - acc;
    }
  for (int i = 0; i < 4; ++i) s.mean[i] = nm[i];
  for (int i = 0; i < 16; ++i) s.cov[i] = nc[i];
}

// distance()  kalman_2d_point.rs:123-137 : the squared Mahalanobis distance through nalgebra's Cholesky factor of the projected
// covariance.  A failed pivot (the reference unwraps a None there) answers NaN, never a trap.
// In two parts, because the factor depends on the state alone: a caller that measures many points against one state (the pose
// association, sa_pose.hip) factors once.  sa_pkf_factor: the projected mean and the Cholesky factor; false = a pivot failed (the
// fields behind the failed pivot are not written).  sa_pkf_distance_factored: the forward substitution and the squared norm.
struct sa_pkf_fac {
  float mx, my, l00, l10, l11;
};
SA_HD bool sa_pkf_factor(float pw, const sa_pkf& s, sa_pkf_fac& f) {
  float P[4];
  sa_pkf_project(pw, s, P);
  f.mx = s.mean[0];
  f.my = s.mean[1];
  if (P[0] == 0.0f || !(P[0] >= 0.0f)) return false;
  f.l00 = sqrtf(P[0]);
  f.l10 = P[2] / f.l00;
  const float d1 = (-f.l10) * f.l10 + P[3];
  if (d1 == 0.0f || !(d1 >= 0.0f)) return false;
  f.l11 = sqrtf(d1);
  return true;
}
SA_HD float sa_pkf_distance_factored(const sa_pkf_fac& f, float zx, float zy) {
  const float r0 = zx - f.mx, r1 = zy - f.my;
  const float y0 = r0 / f.l00;
  const float y1 = ((-y0) * f.l10 + r1) / f.l11;
  return y0 * y0 + y1 * y1;
}
SA_HD float sa_pkf_distance(float pw, const sa_pkf& s, float zx, float zy) {
  sa_pkf_fac f;
  if (!sa_pkf_factor(pw, s, f)) return NAN;
  return sa_pkf_distance_factored(f, zx, zy);
}

// calculate_cost()  kalman_2d_point.rs:139-151 : a NaN falls through both comparisons and stays NaN
SA_HD float sa_pkf_cost(float d2, bool inverted) {
  if (!inverted) return d2 > SA_POINT_CHI2INV95_2 ? SA_CHI2_UPPER_BOUND : d2;
  return d2 > SA_CHI2INV95_4 ? 0.0f : SA_CHI2_UPPER_BOUND - d2;
}

// make_prediction  kalman_prediction.rs:13-32 for one point that may be absent: a present point without a state is initiated; a point
// that has a state is predicted; a present one is then updated.  Returns whether the point has a state afterwards.
SA_HD bool sa_pkf_step(float pw, float vw, bool has, sa_pkf& s, bool present, float zx, float zy) {
  if (present && !has) {
    sa_pkf_initiate(pw, vw, zx, zy, s);
    has = true;
  }
  if (has) sa_pkf_predict(pw, vw, s);
  if (has && present) sa_pkf_update(pw, s, zx, zy);
  return has;
}
