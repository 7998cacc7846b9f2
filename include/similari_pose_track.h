/*
 * similari_pose_track.h — the keypoint frame loop in one call: associate the poses of a frame to the tracks of a point bank, step the
 * matched and the new tracks, let the others coast, all on the device (beside similari_pose.h and similari_pose_batch.h, as
 * sa_store_absorb stands beside sa_store_search).
 *
 * The call returns, and leaves in the bank, exactly the bits of this sequence:
 *   1. sa_points_associate (sa_points_associate_batch) on the same tracks, poses and options;
 *   2. every pose without a track takes the next unused entry of new_ids, in call order: scene after scene, then pose order;
 *   3. ONE sa_points_step over all m poses under those ids, with the poses' own rows, mask and score rule;
 *   4. if options.coast: ONE sa_points_predict over the listed tracks that no pose was matched to.
 * The keypoint states never leave the device between the vote and the filter update, the poses are uploaded once, the ids of the
 * listed tracks are resolved once, and the host waits for the stream once.
 *
 * sa_points_order afterwards is the old order followed by the created ids in call order.  Tracks of the bank the call does not list are
 * untouched.  The records of sa_points_last, sa_points_associate_last and sa_points_associate_batch_last are not touched.  The one thing
 * that may differ from the sequence is the capacity of the planes: the call reserves room for T + m tracks before it knows how many it
 * creates.
 *
 * Device path.  The vote is the three launches of similari_pose.h; its assignment additionally leaves, per track, the pose that took
 * it, per unmatched pose its rank among the unmatched poses of its scene, and per scene their number.  A batch then runs one workgroup
 * that turns the scenes' numbers into their exclusive prefix.  k_pose_step, ONE launch, one thread per (item, point), the items being the
 * m poses followed by the listed tracks: a pose's thread steps the state of its track — the matched one, or slot T + prefix + rank, taken
 * as fresh —, a track's thread predicts it if nobody took the track.  One copy back: 8 B per pose, 4 B per scene, and out_xy if asked.
 */
#ifndef SIMILARI_POSE_TRACK_H
#define SIMILARI_POSE_TRACK_H

#include "similari_pose_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sa_pose_track_options {
  uint32_t struct_size, min_common;  /* as sa_pose_options */
  float threshold; uint32_t coast;   /* threshold: as sa_pose_options; coast: 0 / 1 (default 1): predict the listed tracks nobody matched */
} sa_pose_track_options; /* 16 B */

void sa_pose_track_options_default(sa_pose_track_options* o);

/* One frame of one scene.  track_ids[n_tracks]: the tracks the poses may continue; NULL: every track, in sa_points_order order
 * (n_tracks is ignored).  poses: m rows as sa_points_associate takes them.  new_ids[n_new]: the ids offered to created tracks,
 * n_new >= m.  out_track [m]: the id every pose ended up with, never 0.  out_weight [m]: the association's w, NaN for a created track.
 * out_xy: NULL, or [m][P][2], sa_points_step's out_xy.  *out_created: the entries of new_ids that were used (new_ids[0 .. created)).
 *
 * A pose the vote leaves alone — also an absent one (SA_ROW_NONE), one with no present point, one against failed pivots — creates a
 * track; with no present point that track has no point state.  m == 0: with coast set, a predict over the listed tracks.  No listed
 * tracks: every pose creates a track and no vote is launched.
 *
 * Refusals run before anything is launched and leave everything as it was: those of sa_points_associate and sa_points_step; a coast
 * that is neither 0 nor 1; n_new < m, a null new_ids with m > 0, a new id that is 0, that comes twice, or that the bank or track_ids
 * already holds (SA_ERR_BAD_ARG); (T + m) * P >= 2^31, T the tracks of the bank (SA_ERR_UNSUPPORTED). */
int sa_points_track(sa_points* b, uint32_t n_tracks, const uint64_t* track_ids, uint32_t m, const sa_point_rows* poses, uint32_t n_new,
                    const uint64_t* new_ids, const sa_pose_track_options* o, uint64_t* out_track, float* out_weight, float* out_xy,
                    uint32_t* out_created);

/* One frame of n_scenes scenes, laid out as sa_points_associate_batch takes them; m is the sum of pose_counts.  out_track, out_weight,
 * out_xy: scene after scene.  out_roots: NULL, or [n_scenes] the search roots of each scene's vote.  Refusals: those of
 * sa_points_associate_batch, and those above. */
int sa_points_track_batch(sa_points* b, uint32_t n_scenes, const uint32_t* track_counts, const uint64_t* track_ids,
                          const uint32_t* pose_counts, const sa_point_rows* poses, uint32_t n_new, const uint64_t* new_ids,
                          const sa_pose_track_options* o, uint64_t* out_track, float* out_weight, float* out_xy, uint32_t* out_roots,
                          uint32_t* out_created);

/* The last sa_points_track or sa_points_track_batch (zeros after a refused one).  scenes: 1 for the single call.  vote_launches: 3, or
 * 0 when no pose had a track to be matched to.  step_launches: 1, and 2 for a batch that voted (the scene scan); 0 when there was
 * neither a pose nor a track to coast.  roots, matched: the vote's.  created: poses that created a track.  coasted: listed tracks nobody
 * matched, 0 without coast.  bytes_h2d: the segment table (a batch), the slot table, the poses when host-fed, the mask, the index.
 * bytes_d2h: 8 B per pose, 4 B per scene, and out_xy.  src_bytes: as sa_pose_stats.  device_ms: device events around all launches;
 * kernel_ms: factor, tile, assign, scan, step. */
typedef struct sa_pose_track_stats {
  uint32_t struct_size, scenes, poses, tracks;
  uint32_t vote_launches, step_launches, roots, matched;
  uint32_t created, coasted;
  uint64_t bytes_h2d, bytes_d2h, src_bytes;
  double device_ms;
  double kernel_ms[5];
} sa_pose_track_stats; /* 112 B */
int sa_points_track_last(sa_points* b, sa_pose_track_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_POSE_TRACK_H */
