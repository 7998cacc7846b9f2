/*
 * similari_pose_oks.h — a second metric for the keypoint association: object keypoint similarity (OKS), the overlap measure of poses,
 * beside the mean inverted Mahalanobis cost of similari_pose.h — as PositionalMetricType::IoU stands beside ::Mahalanobis for boxes
 * (src/trackers/sort.rs, sort/metric.rs).  Unlike the Mahalanobis cost it does not depend on how much covariance a track has grown:
 * "the same pose, scaled by body size, with a tolerance per joint".
 *
 * The metric is a property of the BANK: sa_points_associate, _associate_batch, _track, _track_batch, sa_pose_sort_predict and _peek
 * all vote with the metric of the bank they run on.  The default is Mahalanobis: a bank that never switches runs exactly the launches
 * and leaves exactly the bits it did before this header existed, and so does a bank that switched back.
 *
 * The weight of pose i against track j under OKS, all f32 without fused multiply-add:
 *   extent of a side   the bounding rectangle of the pose's present points / of the stored means (x, y) of the track's points that
 *                      have a state, as they are at the time of the vote; its area a = (xmax - xmin) * (ymax - ymin); a side without
 *                      a point has no area
 *   scale of the pair  s2 = 0.5f * (a_pose + a_track); the pair is REFUSED iff !(s2 > 0): no weight (NaN in the tap), no gain, no
 *                      match.  Two single-point sides, collinear (axis-parallel) points on both sides and every bank of one point
 *                      have s2 = 0: OKS needs a body size
 *   per point          var2_p = 2 * (2 sigma_p)^2;  e = ((zx - mx)^2 + (zy - my)^2) / (s2 * var2_p);  c_p = exp(-e), by a polynomial
 *                      defined in similari_amd/csrc/sa_pose_oks.h (exactly 1 at 0, exactly 0 from e = 32 on, relative error below 1e-5);
 *                      point p is common iff it is present in the pose, the track's point has a state and e is not NaN
 *   the pair           w = (c_p1 + c_p2 + ...) / k over the k common points, p ascending; it exists iff k >= min_common.  0 <= w <= 1
 *
 * The diagonal.  `threshold` of sa_pose_options, sa_pose_track_options and sa_pose_sort_options is the diagonal of the vote under either
 * metric.  Its default of 1.0 matches NOTHING under OKS, because w <= 1: set it — the reference's DEFAULT_SORT_IOU_THRESHOLD is 0.3
 * (src/trackers/sort.rs:31).
 *
 * Device path under OKS.  In front of every vote the extents launch — the one the keypoint tracker's gate runs (similari_pose_sort.h),
 * one thread per pose and per listed track, here also writing each item's area — so sa_points_associate takes four launches (extents,
 * factor, tile, assign; sa_pose_stats.launches and sa_pose_batch_stats.launches say 4, sa_pose_track_stats.vote_launches 4), and its
 * device_ms begins in front of the extents.  In the tracker that ONE launch serves the gate and the metric: sa_pose_sort_stats reports
 * it as gate_launches = 1 and gate_ms, with or without a finite limit in the call, and vote_launches stays 3.  The factor launch
 * reads no covariance.
 */
#ifndef SIMILARI_POSE_OKS_H
#define SIMILARI_POSE_OKS_H

#include "similari_pose_sort.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_POSE_METRIC_MAHALANOBIS 0u   /* the default: everything as it is without this header */
#define SA_POSE_METRIC_OKS         1u

typedef struct sa_pose_metric {
  uint32_t struct_size, kind;
  uint32_t n_sigmas, reserved;      /* n_sigmas == the bank's P under OKS, 0 otherwise; reserved: 0 */
  const float* sigmas;              /* [n_sigmas], each finite and > 0 (COCO's per-joint constants, for instance) */
} sa_pose_metric; /* 24 B */

/* struct_size, Mahalanobis, no sigmas */
void sa_pose_metric_default(sa_pose_metric* m);

/* The metric of every later vote on this bank.  Uploads var2 [P] once; changes no track state.  Allowed on a tracker's bank
 * (sa_pose_sort_bank): it changes none of the tracker's records.  Switching back to Mahalanobis restores the launches and the bits
 * of a bank that never switched.
 * Refusals (SA_ERR_BAD_ARG; the previous metric stays): a null argument, a wrong struct_size, an unknown kind, n_sigmas != P under
 * OKS or != 0 under Mahalanobis, a sigma that is not finite or not > 0, reserved != 0. */
int sa_points_set_metric(sa_points* b, const sa_pose_metric* m);

/* out_kind: the bank's metric; out_sigmas: NULL, or [P] — the sigmas as they were given under OKS, untouched otherwise. */
int sa_points_get_metric(sa_points* b, uint32_t* out_kind, float* out_sigmas);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_POSE_OKS_H */
