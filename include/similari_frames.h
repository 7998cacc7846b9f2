/*
 * similari_frames.h — frame preprocessing for a whole batch of scenes: sa_nms and sa_own_areas (similari_assoc.h) over many
 * scenes in one call.
 *
 * The single calls take one scene each, and each one drains the engine, uploads, launches, copies back and waits.  A batch call
 * does that once: the boxes of every scene lie back to back in one staging block, a small table tells the device where each scene
 * begins, and the scene is a grid dimension of the launches.  The number of launches does not depend on the number of scenes.
 * There is one implementation: a single call runs the same host path and the same kernels as a batch of its one scene (its
 * refusals name no scene, and sa_frames_last does not see it).
 *
 * Semantics.  Scene s of a batch call returns what the single call on scene s returns: sa_nms_batch exactly the same indices in the
 * same order; sa_own_areas_batch the same arithmetic per box with the neighbours scanned in the scene's own order (the covered
 * stretches of an edge are summed in the order the neighbours arrive in the device's list, as in the single call: shares agree to
 * 1e-6).  Boxes of different scenes never see each other, whatever their coordinates.  counts[s] == 0 is legal anywhere in the list
 * and produces nothing (boxes[s], out_share[s], out_keep[s] are not read then and may be NULL); n_scenes == 0 returns SA_OK.
 *
 * Refusals.  Every refusal but the last runs before anything is queued; all leave every output untouched and name the scene in
 * sa_last_error:
 *   SA_ERR_BAD_ARG      a null argument; own areas: a box whose aspect, height or confidence sa_own_areas refuses
 *   SA_ERR_UNSUPPORTED  more than 65535 scenes in one call; NMS: more than 16384 boxes of one scene pass its host filter
 *   SA_ERR_UNSUPPORTED  own areas, after the spill path ran: more than 512 disjoint stretches of one box edge are covered
 *
 * Like every synchronous call of similari_assoc.h these drain the engine first and return with the results in the caller's arrays.
 */
#ifndef SIMILARI_FRAMES_H
#define SIMILARI_FRAMES_H

#include "similari_assoc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sa_own_areas over n_scenes scenes: out_share[s][i] = the share of box i of scene s that no other box of scene s covers. */
int sa_own_areas_batch(sa_engine* e, uint32_t n_scenes, const uint32_t* counts, const sa_box* const* boxes, float* const* out_share);

/* sa_nms over n_scenes scenes with one pair of thresholds.  scores: NULL, or one pointer per scene of which any may be NULL (the
 * scene ranks by height).  out_keep[s]: room for counts[s] indices; out_n[s]: how many were written. */
int sa_nms_batch(sa_engine* e, uint32_t n_scenes, const uint32_t* counts, const sa_box* const* boxes, const float* const* scores,
                 float nms_threshold, float score_threshold, uint32_t* const* out_keep, uint32_t* out_n);

/* The last *_batch call on e; zeros before the first and after a refused one.  struct_size: written by the call,
 * sizeof(sa_frames_stats). */
typedef struct sa_frames_stats {
  uint32_t struct_size, scenes;
  uint32_t boxes;                  /* boxes that reached the device (NMS: after the host filter) */
  uint32_t launches;               /* kernel launches of the call */
  uint32_t spilled;                /* own areas: boxes that took the spill path */
  uint32_t host_waits;             /* times the call waited for the stream behind what it queued: 1, or 2 when something spilled */
  uint64_t bytes_h2d, bytes_d2h;
  double device_ms;                /* first launch to last, device events */
} sa_frames_stats;                 /* 48 B */
int sa_frames_last(sa_engine* e, sa_frames_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_FRAMES_H */
