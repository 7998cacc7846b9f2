/*
 * similari_pose_nms.h — non-maximum suppression of poses by object keypoint similarity (OKS), on the device: one scene or a whole
 * batch of scenes in one call.  What sa_nms / sa_nms_batch (similari_assoc.h, similari_frames.h) are for boxes in front of the box
 * trackers, this is for poses in front of the keypoint tracker (similari_pose_sort.h): every pose network emits duplicates — two
 * skeletons on one person, a half body beside a full one — and a tracker fed with them keeps two tracks per person.
 *
 * Semantics: src/utils/nms.rs:32-72 with poses in place of boxes and OKS in place of intersection / area.
 *   filter   pose i is dropped iff !(scores[i] > score_threshold): a NaN score is dropped; score_threshold NaN means none (f32::MIN),
 *            as in sa_nms.  scores is a host array and is required — a pose has no height to rank by, and the host ranks: 4 bytes per
 *            pose are the whole input traffic of a call fed from device memory.  Nothing else filters: a pose with few or no present
 *            points is kept, and can neither suppress nor be suppressed (the pair rule below)
 *   rank     the surviving poses are stable-sorted by score, descending: equal scores keep the caller's order
 *   pair     w(i, j) for i before j in rank order is the OKS cell of similari_pose_oks.h with the EARLIER pose where the track stands:
 *            each side's extent is the bounding rectangle of its present points, its area a = (xmax - xmin) * (ymax - ymin), a side
 *            without a present point has none; s2 = 0.5f * (a_i + a_j), the pair is REFUSED iff !(s2 > 0); point p is common iff it
 *            is present on both sides and e = ((x_j - x_i)^2 + (y_j - y_i)^2) / (s2 * var2_p) is not NaN, var2_p = 2 (2 sigma_p)^2;
 *            w = (c_p1 + c_p2 + ...) / k over the k common points, p ascending, an f32 sum seeded by the first term, c_p = exp(-e) by
 *            the polynomial of similari_amd/csrc/sa_pose_oks.h; the pair EXISTS iff k >= min_common.  A point is present by the rule
 *            of similari_points.h: finite x and y, score >= min_score when comps == 3, and the present mask.  All f32, no fused
 *            multiply-add.  w is SYMMETRIC in value, bit for bit: s2 is a sum of two terms and each distance a sum of two squares,
 *            neither of which changes when the sides are exchanged.  Two exact duplicates with a body size have w == 1
 *   greedy   the poses are visited in rank order; a visited pose that is still alive suppresses every later alive pose j with
 *            w(i, j) > nms_threshold — strictly, as the reference compares.  A pair that does not exist or is refused suppresses
 *            nothing (single-point and collinear poses, every call with points == 1).  A NaN nms_threshold suppresses nothing
 *   result   out_keep[0 .. *out_n) are the survivors as indices into the caller's poses, in rank order — the reference's output
 *            order, and what sa_nms returns
 *
 * A batch runs every scene by these rules: scene s returns exactly what the single call on scene s returns, and poses of different
 * scenes never see each other, whatever their coordinates.  There is one implementation: the single call is the batch of its one
 * scene, on the same host path and the same kernels.
 *
 * Where the poses lie: an sa_point_rows of similari_points.h over the rows of the whole call — host [m][P][comps] f32 or an sa_dev_rows
 * of P * comps elements per row (f32, f16 or bf16, strided, gathered by index[m], SA_ROW_NONE = a pose without a point), present
 * [m][P] or NULL.  In a batch the rows of the scenes follow each other, scene after scene, as sa_points_track_batch takes them, and so
 * do the scores.  A call fed from device memory leaves the bits of the call fed the widened values from the host.
 *
 * The calls belong to the engine and need no point bank.  They drain the engine first and return with the results in the caller's
 * arrays, like sa_nms.
 *
 * Refusals run before anything is queued and leave every output untouched; sa_last_error(engine) has the text, and a batch names the
 * scene where one is at fault.
 *   SA_ERR_BAD_ARG      a null argument (the engine, the options, the poses, the scores, an output; in a batch counts, and out_keep[s]
 *                       of a scene that has poses); a wrong struct_size; points == 0; n_sigmas != points; a null sigmas; a sigma that
 *                       is not finite or not > 0; min_common == 0; the sa_point_rows / sa_dev_rows checks of similari_points.h
 *   SA_ERR_UNSUPPORTED  more than 65535 scenes; more than 16384 poses of one scene pass the filter; more than 2^32 - 2 poses in one
 *                       call; sa_pose_nms_matrix: more than SA_POSE_NMS_TAP_MAX poses pass the filter
 * m == 0, counts[s] == 0 anywhere in a batch and n_scenes == 0 are legal and return SA_OK with nothing kept.
 *
 * Device path.  The host filters and ranks each scene from the scores alone and lays the scenes out (sa_frames_plan.h).  ONE upload
 * carries the segment table, var2 [P], the rank table — one u32 per surviving pose: the row it reads, the caller's index composed
 * into it — the present flags of the surviving poses when there is a mask, and the surviving poses themselves only when they come from
 * the host.  Three launches, however many scenes: k_pose_nms_lay (one thread per surviving pose: its points, point-major in rank
 * order, and the area of its extent), k_pose_nms_mask (one block per 16 rows x 64 columns of a scene's pair matrix: one 64-bit mask
 * word per row, by a ballot) and k_nms_sweep, the greedy pass the box path runs.  One byte per surviving pose comes back; the call
 * waits once.
 */
#ifndef SIMILARI_POSE_NMS_H
#define SIMILARI_POSE_NMS_H

#include "similari_points.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_POSE_NMS_MAX_SCENES 65535u   /* scenes of one call */
#define SA_POSE_NMS_MAX        16384u   /* poses of one scene that may pass the filter (SA_FRAMES_NMS_MAX) */
#define SA_POSE_NMS_TAP_MAX    2048u    /* sa_pose_nms_matrix: poses that may pass the filter (a 16 MiB matrix) */

typedef struct sa_pose_nms_options {
  uint32_t struct_size, points;          /* points: P >= 1 */
  uint32_t min_common, n_sigmas;         /* min_common >= 1; n_sigmas == points */
  const float* sigmas;                   /* [P], each finite and > 0 */
  float nms_threshold, score_threshold;  /* score_threshold NaN: none */
} sa_pose_nms_options; /* 32 B */

/* struct_size, points 17, min_common 1, n_sigmas 0 and no sigmas (the caller sets both), nms_threshold 0.9, score_threshold NaN */
void sa_pose_nms_options_default(sa_pose_nms_options* o);

/* One scene of m poses.  out_keep: room for m indices; *out_n: how many were written. */
int sa_pose_nms(sa_engine* e, const sa_pose_nms_options* o, uint32_t m, const sa_point_rows* poses, const float* scores,
                uint32_t* out_keep, uint32_t* out_n);

/* n_scenes scenes of counts[s] poses with one set of options.  poses: the sum of counts rows, scene after scene; scores: the same
 * order.  out_keep[s]: room for counts[s] indices INTO SCENE s (0 .. counts[s] - 1), not read when counts[s] == 0; out_n[s]: how many
 * were written. */
int sa_pose_nms_batch(sa_engine* e, const sa_pose_nms_options* o, uint32_t n_scenes, const uint32_t* counts, const sa_point_rows* poses,
                      const float* scores, uint32_t* const* out_keep, uint32_t* out_n);

/* Parity tap: the pairs of ONE scene.  *out_m = m', the poses that pass the filter; out_order [m']: the caller's indices in rank order;
 * out_w [m'][m'], rank order on both axes: w for i < j, NaN for a pair that does not exist or is refused, NaN on and below the
 * diagonal.  Room for min(m, SA_POSE_NMS_TAP_MAX) entries and their square is enough.  Nothing is suppressed. */
int sa_pose_nms_matrix(sa_engine* e, const sa_pose_nms_options* o, uint32_t m, const sa_point_rows* poses, const float* scores,
                       uint32_t* out_order, float* out_w, uint32_t* out_m);

/* The last of the three calls on e; zeros before the first and after a refused one.  struct_size: written by the call,
 * sizeof(sa_pose_nms_stats). */
typedef struct sa_pose_nms_stats {
  uint32_t struct_size, scenes;
  uint32_t poses;                  /* poses that reached the device: those that passed the filter, of all scenes */
  uint32_t launches;               /* kernel launches of the call: 3, the tap 2, 0 when no pose passed */
  uint32_t host_waits;             /* times the call waited for the stream behind what it queued: 1 */
  uint32_t reserved;
  uint64_t bytes_h2d, bytes_d2h;   /* everything the call sent over the bus */
  uint64_t src_bytes;              /* bytes read from the caller's device memory */
  double device_ms;                /* first launch to last, device events */
} sa_pose_nms_stats; /* 56 B */
int sa_pose_nms_last(sa_engine* e, sa_pose_nms_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_POSE_NMS_H */
