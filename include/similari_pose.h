/*
 * similari_pose.h — keypoint association: the poses of a frame matched to the tracks of a point bank, on the device
 * (beside similari_points.h).
 *
 * A point bank (similari_points.h) steps the Kalman states of T tracks x P keypoints for a caller who knows which pose belongs to
 * which track.  This call finds that out: the M x T matrix "how well does pose i continue track j" from the reference's
 * Vec2DKalmanFilter::distance and calculate_cost (src/utils/kalman/kalman_2d_point_vec.rs, kalman_2d_point.rs:123-151), and the
 * assignment over it by the reference's vote, SortVoting::winners (src/trackers/sort/voting.rs).
 *
 * The pair weight, reference arithmetic in the reference's order.  Pose i of the call against track j of the call, points p ascending:
 *   point p is COMMON iff it is present in pose i (the presence rule of similari_points.h: finite x and y, score >= min_score, mask),
 *     track j's point p has a state, and d2 = distance(state, z) is not NaN (a failed pivot makes the point not common; it does not
 *     poison the pair);
 *   c_p = calculate_cost(d2, inverted = true): 100 - d2, or 0 beyond 11.070;
 *   k = the number of common points;  w = (c_p1 + c_p2 + ...) / (float)k, an f32 sum in ascending p seeded by the first term;
 *   the pair EXISTS iff k >= min_common.
 * The vote: rows are poses, columns are tracks, the weight of a pair is (w * 1e6f) as i64, the diagonal ("a new track") is
 * (threshold * 1e6f) as i64; a pair is a usable edge iff its weight exceeds the diagonal.  The assignment is the exact maximum of the
 * reference's dense M x (M + T) matrix (kuhn_munkres there; here a greedy start and shortest augmenting paths over the dense gains).
 * Where several assignments reach that maximum the call returns one of them.
 *
 * The call changes no state: as in the reference's trackers, a track's stored state is matched as it is (not predicted first).
 *
 * Device path: three launches whatever M, T and P are.  k_pose_factor, one thread per (track, point): the Cholesky factor of the
 * projected covariance, once per track point instead of once per cell.  k_pose_tile, one block per 16 poses x 64 tracks: the cells,
 * the dense i64 gain matrix, one 64-bit atomic maximum per row and wave for the row's heaviest gain.  k_pose_assign, one workgroup:
 * the greedy start from those words, then the dense solver over the rows that lost their bid.  The two are the kernels of
 * similari_pose_batch.h run on one scene, which travels in the kernel arguments.  The poses are read where they lie
 * (sa_point_rows: host f32, or f32 / f16 / bf16 rows in a registered device block).
 *
 * Limits: m <= 2048 poses and n_tracks <= 2048 tracks in one call (SA_POSE_MAX); beyond: SA_ERR_UNSUPPORTED.
 */
#ifndef SIMILARI_POSE_H
#define SIMILARI_POSE_H

#include "similari_points.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_POSE_MAX 2048u

typedef struct sa_pose_options {
  uint32_t struct_size, min_common;  /* min_common: the pair exists iff that many points are common; >= 1 (default 1) */
  float threshold; uint32_t reserved; /* the diagonal of the vote, finite and >= 0; default 1.0 (MAHALANOBIS_NEW_TRACK_THRESHOLD) */
} sa_pose_options; /* 16 B */

void sa_pose_options_default(sa_pose_options* o);

/* Poses `poses` (m rows: host or device, index / SA_ROW_NONE as in similari_points.h; a pose with SA_ROW_NONE has no common point)
 * against the tracks track_ids[n_tracks] of the bank; track_ids == NULL: every track, in sa_points_order order (n_tracks is ignored).
 * out_track [m]: the id of the track the pose continues, 0 = none: a new track.  out_weight [m]: w of that pair, NaN if none.
 * out_matrix: NULL, or [m][n_tracks] w of every pair, NaN = no pair (a parity tap: the only output that costs m x n_tracks on the bus).
 *
 * Refusals run before anything is launched and leave everything as it was: those of similari_points.h (a null argument, id 0, an id
 * twice, an unknown id: SA_ERR_NOT_FOUND, a wrong struct_size, bad rows), min_common == 0, a threshold that is not finite or negative
 * (SA_ERR_BAD_ARG); m or n_tracks beyond SA_POSE_MAX (SA_ERR_UNSUPPORTED).  m == 0: SA_OK, nothing is read or written.  No tracks:
 * SA_OK without a launch, out_track all 0, out_weight all NaN. */
int sa_points_associate(sa_points* b, uint32_t n_tracks, const uint64_t* track_ids, uint32_t m, const sa_point_rows* poses,
                        const sa_pose_options* o, uint64_t* out_track, float* out_weight, float* out_matrix);

/* The last sa_points_associate (zeros after a refused one): launches is 3, or 0 when there was nothing to match; roots = the rows
 * that lost their greedy bid, i.e. the searches the dense solver ran; matched = poses that got a track; bytes_h2d: the slot table, the
 * poses when host-fed, the mask, the index; bytes_d2h: 8 * m of results and 4 for `roots`, plus the tap; src_bytes: the pose rows the
 * call names in the caller's device memory, each counted once; device_ms: device events around the three launches, kernel_ms: around
 * each (factor, tile, assign).  sa_points_last is not touched. */
typedef struct sa_pose_stats {
  uint32_t struct_size, poses, tracks, launches;
  uint32_t roots, matched;
  uint64_t bytes_h2d, bytes_d2h, src_bytes;
  double device_ms;
  double kernel_ms[3];
} sa_pose_stats; /* 80 B */
int sa_points_associate_last(sa_points* b, sa_pose_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_POSE_H */
