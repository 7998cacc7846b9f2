/*
 * similari_points.h — point banks: the 2D point-vector Kalman filter for the keypoints of many tracks, on the device
 * (beside similari_framerows.h and similari_waste.h).
 *
 * The reference has three filters: the box filter, which the trackers of similari_tracker.h run, the 2D point filter
 * (src/utils/kalman/kalman_2d_point.rs, Point2DKalmanFilter) and the 2D point-vector filter (kalman_2d_point_vec.rs,
 * Vec2DKalmanFilter: "predicts the vector of independent 2D points motion, used in the Keypoint Tracker"), which is the point filter
 * applied to every point of a vector.  A pose network beside the detector leaves P keypoints per person in device memory; a point
 * bank keeps the Kalman states of T tracks x P points on the engine's GPU, keyed by track id, and steps them in one launch per call.
 *
 * A state is mean[4] = (x, y, vx, vy) and cov[16], row-major, a general 4 x 4 matrix.  A point of a track either has a state or has
 * none (it was never sighted).  The arithmetic is sa_kalman_point.h, the reference's f32 operations in the reference's order, so every
 * call returns and leaves the bits of the reference's filter fed the same values:
 *
 *   initiate(z)  mean = (z.x, z.y, 0, 0), cov = diag((2 pw)^2, (2 pw)^2, (10 vw)^2, (10 vw)^2)
 *   predict      mean = F mean, cov = F cov F^T + diag(pw^2, pw^2, vw^2, vw^2), F = I with F[0][2] = F[1][3] = 1
 *   update(z)    the reference's update, its solve_lower_triangular on the un-factorised projected covariance included
 *   distance(z)  d^2 = |L^-1 (z - mean[0..2])|^2, L the Cholesky factor of cov[0..2][0..2] + diag(pw^2, pw^2); NaN if a pivot fails
 *   cost         SA_POINT_COST: d^2 > 5.9915 ? 100 : d^2;  SA_POINT_COST_INVERTED: d^2 > 11.070 ? 0 : 100 - d^2;  NaN stays NaN
 *
 * Where the points of a call lie (sa_point_rows): in host memory, [n][P][comps] f32, or in device memory, described by an sa_dev_rows
 * of similari_devrows.h whose rows hold P * comps elements — f32, f16 or bf16, strided, gathered by index[n] (NULL = 0, 1, 2, ...),
 * SA_ROW_NONE = every point of that track is absent.  Exactly one of host / dev is given.  A 16-bit element is widened exactly
 * (similari_devrows.h), so a call fed from the device leaves the bits of the call fed the widened values from the host.  A point is
 * PRESENT iff its x and y are finite, AND comps == 2 or its score >= min_score (a NaN score is absent), AND present == NULL or
 * present[i][p] != 0.  The device span must lie inside one block registered with sa_device_block_register on the bank's device; the
 * rows must be final at the call; every call is synchronous, so they are free again when it returns.
 *
 * A bank belongs to an engine: it lives on the engine's device and works on its stream, behind whatever the engine has queued, and
 * touches none of the engine's tables.  Lifetime and errors are a store's (similari_search.h): destroy the bank before the engine or
 * after it; once the engine is gone every call answers SA_ERR_STATE; a refusal's text is in sa_last_error(engine).  ids are non-zero
 * and distinct within a call.
 *
 * Refusals run before anything is launched and leave the bank as it was.  SA_ERR_BAD_ARG: a null argument, id 0, an id twice, a wrong
 * struct_size, comps not 2 or 3, both or neither of host / dev, points == 0, an unknown mode, a dev span outside one registered block
 * or on another device (the checks of similari_devrows.h).  SA_ERR_NOT_FOUND: an unknown id in predict, update, distance, get_state
 * or set_state.  SA_ERR_UNSUPPORTED: tracks x points >= 2^31.
 *
 * Device path.  The states lie as struct-of-arrays planes over capacity * P: five planes of 16 bytes per point (the mean and the four
 * covariance rows) and one byte plane (has a state), so consecutive lanes read consecutive 16-byte pieces.  Every state-changing call
 * is ONE launch whatever n and P are, one thread per (track of the call, point); the host resolves ids to slots and uploads one u32
 * slot table, plus the points when they come from the host.  With a dev source only the slot table and the index cross the bus on
 * the way in.  Capacity doubles.  sa_points_remove compacts in one launch whatever n is.
 */
#ifndef SIMILARI_POINTS_H
#define SIMILARI_POINTS_H

#include "similari_devrows.h"
#include "similari_framerows.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sa_points sa_points;

typedef struct sa_points_options {
  uint32_t struct_size, points;            /* points: P >= 1 */
  float position_weight, velocity_weight;  /* pw, vw: 1/20 and 1/160 by default */
} sa_points_options; /* 16 B */

typedef struct sa_point_rows {             /* where the points of a call lie: exactly one of host / dev */
  uint32_t struct_size, comps;             /* comps 2: x, y    3: x, y, score */
  float min_score; uint32_t reserved;      /* comps == 3: present iff score >= min_score (a NaN score is absent) */
  const float* host;                       /* [n][P][comps] f32 */
  const uint8_t* present;                  /* host [n][P] or NULL = all; ANDed with the score test, for either source */
  const sa_dev_rows* dev;                  /* rows of P * comps elements in a registered block; index[n], SA_ROW_NONE = every point of that track absent */
} sa_point_rows; /* 40 B */

/* mode of sa_points_distance */
#define SA_POINT_D2 0u
#define SA_POINT_COST 1u
#define SA_POINT_COST_INVERTED 2u

void sa_points_options_default(sa_points_options* o);
/* e == NULL without a gfx950 device: SA_ERR_NO_DEVICE (there is no CPU fallback) */
int sa_points_create(sa_engine* e, const sa_points_options* o, sa_points** out);
void sa_points_destroy(sa_points* b);

/* An unknown id is created with no point state.  A present point gets initiate(z); an absent one keeps what it has. */
int sa_points_initiate(sa_points* b, uint32_t n, const uint64_t* ids, const sa_point_rows* rows);
/* Every point that has a state gets predict.  ids == NULL: every track, in sa_points_order order (n is ignored).  out_xy [n][P][2]
 * (or NULL): the new mean x, y; NaN where there is no state. */
int sa_points_predict(sa_points* b, uint32_t n, const uint64_t* ids, float* out_xy);
/* A point that is present and has a state gets update(z); everything else is unchanged.  out_xy as for predict. */
int sa_points_update(sa_points* b, uint32_t n, const uint64_t* ids, const sa_point_rows* rows, float* out_xy);
/* Changes no state.  out [n][P]: d^2, or calculate_cost of it; NaN where the point is absent or has no state. */
int sa_points_distance(sa_points* b, uint32_t n, const uint64_t* ids, const sa_point_rows* rows, uint32_t mode, float* out);
/* make_prediction (src/trackers/kalman_prediction.rs:13-32), the loop a tracker runs: an unknown id is created; per point: present
 * and without a state: initiate(z); then, if it has a state, predict; then, if present, update(z).  Exactly the bits of
 * sa_points_initiate (first-sighted points only) + sa_points_predict + sa_points_update. */
int sa_points_step(sa_points* b, uint32_t n, const uint64_t* ids, const sa_point_rows* rows, float* out_xy);
/* Unknown ids are ignored.  The last tracks move into the holes, one after the other in call order, as in sa_store_remove. */
int sa_points_remove(sa_points* b, uint32_t n, const uint64_t* ids);
int sa_points_count(sa_points* b, uint32_t* out_n);
int sa_points_order(sa_points* b, uint64_t* out_ids, uint32_t cap, uint32_t* out_n);
/* For parity tests and seeding, like sa_tracks_get_state / sa_tracks_set_state: has [P] (0 / 1), mean [P][4], cov [P][16]; a get
 * leaves mean and cov of a point without a state as NaN; a set with has[p] == 0 leaves point p without a state, whatever mean and cov
 * say there (its stored values are unspecified and never read). */
int sa_points_get_state(sa_points* b, uint64_t id, uint8_t* has, float* mean, float* cov);
int sa_points_set_state(sa_points* b, uint64_t id, const uint8_t* has, const float* mean, const float* cov);

/* The last call that launched (zeros before the first one, and after a refused one): tracks = n of the call, launches (1),
 * capacity = tracks the planes hold, points = n * P, present = points of the call that were present (0 for predict and remove),
 * bytes_h2d / bytes_d2h = everything the call sent over the bus, src_bytes = bytes read from the caller's device memory,
 * device_ms = device events around the launch.  struct_size: written by the call, sizeof(sa_points_stats). */
typedef struct sa_points_stats {
  uint32_t struct_size, tracks, launches, capacity;
  uint64_t points, present, bytes_h2d, bytes_d2h, src_bytes;
  double device_ms;
} sa_points_stats; /* 64 B */
int sa_points_last(sa_points* b, sa_points_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_POINTS_H */
