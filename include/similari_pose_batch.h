/*
 * similari_pose_batch.h — keypoint association for a batch of scenes: the poses of S cameras matched to the tracks of ONE point bank in
 * one call (beside similari_pose.h, as sa_associate_batch stands beside sa_associate).
 *
 * Scene s has m_s poses and n_s tracks of the bank.  It returns exactly what sa_points_associate returns for those poses against those
 * tracks with the same options: the tap is bit for bit the single call's, out_track and out_weight are equal to the single call's (the
 * route is deterministic: the bid words are atomic maxima, the column claim is an LDS atomic minimum, the dense solver has no atomics,
 * the roots are taken in ascending order).  A pose is never given a track of another scene: scenes are independent components, as
 * compatible() is false across scene ids in the reference.  The call changes no state.
 *
 * Device path: three launches whatever S is.  k_pose_factor over the concatenation of the scenes' tracks; k_pose_tile, a 1-D grid
 * over the 16 x 64 tiles of all scenes, a block finding its scene in the tile prefix of the call's segment table; k_pose_assign,
 * one workgroup per scene.  They are the single call's kernels: that call is one scene, carried in the kernel arguments without a table.
 *
 * Limits: every scene within SA_POSE_MAX either way, at most SA_POSE_BATCH_SCENES scenes, at most SA_POSE_BATCH_CELLS pairs in all.
 */
#ifndef SIMILARI_POSE_BATCH_H
#define SIMILARI_POSE_BATCH_H

#include "similari_pose.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_POSE_BATCH_SCENES 65535u
#define SA_POSE_BATCH_CELLS (1u << 27) /* the sum of m_s * n_s: 1 GiB of gains at 8 B per cell, thirty-two 2048 x 2048 scenes */

/* Scene s: its n_s = track_counts[s] tracks are the next n_s ids of track_ids, its m_s = pose_counts[s] poses the next m_s rows of
 * `poses` (host: [sum m][P][comps] and present [sum m][P]; device: row i, or index[i], of the descriptor, i counting over the whole
 * call, SA_ROW_NONE as in the single call).  out_track / out_weight [sum m], scene after scene: as the single call's.  out_roots: NULL,
 * or [n_scenes] the search roots of each scene.  out_matrix: NULL, or the taps back to back: scene s is [m_s][n_s] at offset
 * sum over r < s of m_r * n_r.
 *
 * Allowed: a scene without poses (it writes nothing); a scene without tracks (its poses get 0 / NaN, 0 roots).  n_scenes == 0, or poses
 * that sum to 0: SA_OK, nothing is launched, only out_roots (when given) is written: zeros.  Poses but no track in the whole call: SA_OK
 * without a launch, out_track all 0, out_weight all NaN.
 *
 * Refusals run before anything is launched and leave everything as it was: those of sa_points_associate, the rules for ids over the
 * whole concatenation (an id named in two scenes is "an id twice"); null counts or null track_ids with n_scenes > 0 (SA_ERR_BAD_ARG);
 * SA_ERR_UNSUPPORTED, the message naming the scene: a scene beyond SA_POSE_MAX either way, n_scenes > SA_POSE_BATCH_SCENES, a pose sum
 * or a track sum that does not fit 32 bits, more than SA_POSE_BATCH_CELLS pairs. */
int sa_points_associate_batch(sa_points* b, uint32_t n_scenes, const uint32_t* track_counts, const uint64_t* track_ids,
                              const uint32_t* pose_counts, const sa_point_rows* poses, const sa_pose_options* o, uint64_t* out_track,
                              float* out_weight, uint32_t* out_roots, float* out_matrix);

/* The last sa_points_associate_batch (zeros after a refused one).  launches is 3 whatever n_scenes is, or 0 when there was nothing to
 * match; tiles = the blocks of the tile launch; roots = the sum over the scenes; matched = poses that got a track.
 * bytes_h2d: the segment table (32 B per scene), the slot table (4 B per track), the poses when host-fed, the mask, the index.
 * bytes_d2h: 8 B per pose of results and 4 B per scene of roots, plus the taps (4 B per pair).  src_bytes, device_ms, kernel_ms: as
 * sa_pose_stats.  The records of sa_points_associate_last and sa_points_last are not touched. */
typedef struct sa_pose_batch_stats {
  uint32_t struct_size, scenes, poses, tracks;
  uint32_t tiles, launches, roots, matched;
  uint64_t bytes_h2d, bytes_d2h, src_bytes;
  double device_ms;
  double kernel_ms[3];
} sa_pose_batch_stats; /* 88 B */
int sa_points_associate_batch_last(sa_points* b, sa_pose_batch_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_POSE_BATCH_H */
