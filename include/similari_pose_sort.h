/*
 * similari_pose_sort.h — the keypoint tracker: Sort's life cycle and compatible() for poses as one object.  The tracker owns a point bank
 * (similari_points.h), the track ids, the scenes' epochs and the per-scene track lists; per frame the caller hands over scene ids and
 * poses, and nothing else (beside similari_pose_track.h, as a Sort tracker stands beside its metric).
 *
 * The tracker keeps: per scene an epoch and the list of its tracks in creation order (a removal closes the gap, the order is kept); per
 * track its id, scene, first epoch, last epoch and length; an id counter that starts at 1.
 *
 * sa_pose_sort_predict returns, and leaves in the bank, exactly the bits of this sequence:
 *   1. every named scene's epoch advances by 1 (a scene never seen starts at 1; a scene not named keeps its epoch);
 *   2. a track of a named scene with epoch - last_epoch > max_idle_epochs is expired: ONE sa_points_remove over all expired tracks,
 *      scenes in call order, then list order; their final states go to the wasted list;
 *   3. ONE sa_points_track_batch over the named scenes with their remaining tracks in list order, the counter's next ids as new_ids and
 *      the tracker's min_common, threshold and coast — and, the one addition, the spatio-temporal gate below;
 *   4. a matched track gets last_epoch = epoch and length + 1; a created one joins its scene's list with first = last = epoch and
 *      length = 1; the counter advances by the created count.
 *
 * The gate.  The reference's trackers refuse a (candidate, track) pair in compatible() (src/trackers/sort.rs:250-270) before the metric
 * is asked: SpatioTemporalConstraints::validate(epoch_delta, dist_in_2r).  For poses: the circle around a set of points is the circle
 * around their bounding rectangle (centre the rectangle's, radius half its diagonal, the shape of Universal2DBox::get_radius), all f32;
 * a pose's points are its present points, a track's the stored means (x, y) of its points that have a state, as they are at the time
 * of the vote; dist_in_2r is the box path's (the distance of the centres over the root of (r1 + r2)^2 + 1e-5).  A track's limit is the
 * max_dist of the first constraint whose epoch_delta is >= the track's epoch - last_epoch (constraints sorted and deduplicated as
 * add_constraints does), +inf when none applies.  A pair is refused iff the limit is finite, both sides have a circle and
 * !(dist_in_2r <= limit).  A refused pair does not exist: it has no weight (NaN in the tap), no gain and is never matched.
 *
 * Cost of one predict: ONE wait, ONE upload of the poses (none when they are in device memory), ONE copy back — 8 B per pose, 4 B per
 * scene, out_xy if asked, and the staging block (81 B per point of an expired track) when anything expired.  No id is looked up per
 * track: the slot table of the call is the concatenation of the scenes' lists.
 *
 * Device path.  Without a finite limit in the call: exactly the launches of sa_points_track_batch.  With one: k_pose_circles, ONE launch
 * (one thread per pose and per listed track) in front of the vote, and the vote's tile in its GATE form.  When anything expired:
 * k_points_gather, ONE launch whatever the number of leaving tracks, copies their states into a staging block in front of the bank's
 * compaction (k_points_move).
 */
#ifndef SIMILARI_POSE_SORT_H
#define SIMILARI_POSE_SORT_H

#include "similari_pose_track.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_POSE_SORT_CONSTRAINTS 8
#define SA_POSE_SORT_ALL_SCENES 0xffffffffffffffffull

typedef struct sa_pose_sort sa_pose_sort;

typedef struct sa_pose_sort_options {
  uint32_t struct_size, points;                       /* points: as sa_points_options (default 17) */
  float position_weight, velocity_weight;             /* as sa_points_options */
  uint32_t max_idle_epochs, min_common;               /* default 5; min_common as sa_pose_options */
  float threshold; uint32_t coast;                    /* as sa_pose_track_options */
  uint32_t n_constraints, reserved;                   /* at most SA_POSE_SORT_CONSTRAINTS; reserved: 0 */
  uint32_t epoch_delta[SA_POSE_SORT_CONSTRAINTS];
  float max_dist[SA_POSE_SORT_CONSTRAINTS];           /* each > 0 */
} sa_pose_sort_options; /* 104 B */

void sa_pose_sort_options_default(sa_pose_sort_options* o);

/* Refusals: those of sa_points_create and of sa_pose_track_options; more than SA_POSE_SORT_CONSTRAINTS constraints, or a max_dist that
 * is not > 0 (SA_ERR_BAD_ARG). */
int sa_pose_sort_create(sa_engine* e, const sa_pose_sort_options* o, sa_pose_sort** out);
void sa_pose_sort_destroy(sa_pose_sort* t);

/* The tracker's bank, for sa_points_get_state, sa_points_order, sa_points_count and sa_points_last.  Calls that change it break the
 * tracker's records.  sa_points_set_metric (similari_pose_oks.h) is allowed: it changes no track and none of the records, and every
 * later predict and peek votes with the new metric. */
sa_points* sa_pose_sort_bank(sa_pose_sort* t);

typedef struct sa_pose_sort_track {
  uint64_t id, scene;
  uint32_t epoch, length;   /* the scene's epoch in this frame; the track's length after it */
  float weight;             /* the association's w, NaN for a created track */
  uint32_t created;         /* 1: the pose created the track */
} sa_pose_sort_track; /* 32 B */

/* One frame.  scene_ids [n_scenes], pose_counts [n_scenes], poses: m = the sum of pose_counts rows as sa_points_track_batch takes them,
 * scene after scene.  out [m]; out_xy: NULL or [m][P][2], the step's means.
 *
 * Refusals run before anything is launched and leave epochs, lists, counter, bank and wasted list untouched: everything
 * sa_points_track_batch refuses; a scene id that comes twice (SA_ERR_BAD_ARG); a scene whose remaining tracks exceed SA_POSE_MAX
 * (SA_ERR_UNSUPPORTED, the scene is named in the message). */
int sa_pose_sort_predict(sa_pose_sort* t, uint32_t n_scenes, const uint64_t* scene_ids, const uint32_t* pose_counts, const sa_point_rows* poses,
                         sa_pose_sort_track* out, float* out_xy);

/* The vote of the predict that would come next: the same expiry view, the same limits, the epochs as they would be.  It changes
 * nothing: no epoch, no state, no id, no wasted entry.  out_track [m]: the id of the track each pose would continue, 0: it would
 * create one.  out_weight [m].  out_tap: NULL, or the f32 weight matrix of every scene back to back ([pose_counts[s]][tracks of s],
 * the scene's remaining tracks in list order); out_track_counts: NULL or [n_scenes] those numbers of tracks.  Refusals: as predict. */
int sa_pose_sort_peek(sa_pose_sort* t, uint32_t n_scenes, const uint64_t* scene_ids, const uint32_t* pose_counts, const sa_point_rows* poses,
                      uint64_t* out_track, float* out_weight, uint32_t* out_track_counts, float* out_tap);
/* the floats out_tap needs for the same scenes and counts (0 when the call would be refused) */
uint64_t sa_pose_sort_peek_cells(sa_pose_sort* t, uint32_t n_scenes, const uint64_t* scene_ids, const uint32_t* pose_counts);

/* The tracks that expired, oldest first.  take: up to cap records — ids, scenes, first, last, length [cap]; has [cap][P]; mean
 * [cap][P][4]; cov [cap][P][16], per track as sa_points_get_state returns them (NaN where has is 0) — are handed over and leave the
 * list; *out_n: how many. */
int sa_pose_sort_wasted_count(sa_pose_sort* t, uint32_t* out_n);
int sa_pose_sort_wasted_take(sa_pose_sort* t, uint32_t cap, uint64_t* ids, uint64_t* scenes, uint32_t* first, uint32_t* last, uint32_t* length,
                             uint8_t* has, float* mean, float* cov, uint32_t* out_n);

/* A scene's epoch moves on by n without a frame (an unseen scene starts at n); its idle tracks expire at the next predict that names it. */
int sa_pose_sort_skip_epochs(sa_pose_sort* t, uint64_t scene, uint32_t n);
/* 0 for a scene never seen */
int sa_pose_sort_epoch(sa_pose_sort* t, uint64_t scene, uint32_t* out_epoch);
/* the tracks of a scene, or of all scenes (SA_POSE_SORT_ALL_SCENES) */
int sa_pose_sort_active(sa_pose_sort* t, uint64_t scene, uint32_t* out_n);

/* The last predict or peek (zeros after a refused one).  The first fields are those of sa_pose_track_stats.  expired: tracks the call
 * removed (a peek: would remove).  gate_launches: 1 when k_pose_circles and the GATE tile ran, else 0.  refused_pairs: only after a
 * peek with a tap — the (pose, track) pairs of the call that the rule above refused; the timed path counts nothing.  gate_ms, gather_ms:
 * k_pose_circles and k_points_gather by device events. */
typedef struct sa_pose_sort_stats {
  uint32_t struct_size, scenes, poses, tracks;
  uint32_t vote_launches, step_launches, roots, matched;
  uint32_t created, coasted;
  uint64_t bytes_h2d, bytes_d2h, src_bytes;
  double device_ms;
  double kernel_ms[5];
  uint32_t expired, gate_launches;
  uint64_t refused_pairs;
  double gate_ms, gather_ms;
} sa_pose_sort_stats; /* 144 B */
int sa_pose_sort_last(sa_pose_sort* t, sa_pose_sort_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_POSE_SORT_H */
