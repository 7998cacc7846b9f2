/*
 * similari_framerows.h — a frame's feature rows read from device memory, f32, f16 or bf16, strided and optionally gathered
 * (beside similari_devrows.h, which does the same for the track search).
 *
 * The per-frame association (similari_assoc.h: sa_associate, sa_batch_*, sa_pipe_*) and the tracker facade (similari_tracker.h) take
 * sa_detections.feats as N x D contiguous f32 rows.  The calls here take a descriptor of similari_devrows.h instead: the output of a
 * ReID head where it lies — a [B, W] batch of any of the three element types, of which a scene owns some rows and perhaps a column
 * slice.  One launch per uploaded request set widens every such scene's rows into the engine's own f32 buffer; nothing behind that
 * buffer knows where the rows came from.
 *
 * Semantics.  A *_dev call returns, and leaves in the engine's track tables, exactly the bits of the corresponding call of
 * similari_assoc.h / similari_tracker.h fed widen(x) as host f32 for every source element x — widen is the exact conversion of
 * similari_devrows.h; "every source element" is row index[i] (or i) of the descriptor for detection i, with the same feat_present,
 * qualities, own areas and boxes.  This holds for ids, vote types and winner columns, under SA_FLAG_TAP for every tap, after
 * sa_tracks_apply* / sa_batch_run_apply for the banks and the Kalman state; for all three source types, both visual metrics,
 * D == Dp and D != Dp.
 *
 * Presence.  Detection i has a feature iff feat_present is NULL or feat_present[i] != 0, AND index is NULL or index[i] != SA_ROW_NONE.
 * For a detection without a feature the index entry is never validated and no source byte is read; its widened row is zeros.
 * sa_dev_rows.index is a HOST array of d->n entries here, one per detection; a row may be named more than once.
 *
 * Where the rows may lie.  As in similari_devrows.h the span must sit inside one block registered with sa_device_block_register, and
 * that block's device must be the engine's (a multi-device tracker: the device of the scene's shard).  Every check runs on the host
 * before anything is staged.  The rows must be final at the call and stay untouched until that frame's results have been fetched
 * (the contract of detection features read in place).  The descriptor and its index are read during the call only.
 *
 * A source that is f32, contiguous (row_stride == D), without an index, with every detection present and a 16-byte aligned base is
 * read in place, without a launch, like sa_detections.feats inside a registered block.
 *
 * Refusals are SA_ERR_BAD_ARG (sa_last_error names the cause) and leave nothing staged, so the same request set can be added to
 * again: a null rows; a wrong struct_size; an unknown elem; a null base or one not aligned to its element; row_stride < D; n_rows of 0
 * or >= 2^32 - 1; a span that is not inside one registered block; a block of another device; an index entry (or, without an index, a
 * detection number) >= n_rows for a detection that has a feature; d->feats != NULL together with rows (the facade: any
 * obs[i].feature != NULL); an engine or tracker that is not visual.  The facade calls need sa_tracker_options.device_upkeep = 1:
 * host upkeep keeps the feature values on the host, so the call is refused with SA_ERR_UNSUPPORTED.
 */
#ifndef SIMILARI_FRAMEROWS_H
#define SIMILARI_FRAMEROWS_H

#include "similari_devrows.h"
#include "similari_tracker.h"

#ifdef __cplusplus
extern "C" {
#endif

/* An entry of sa_dev_rows.index: the detection has no feature. */
#define SA_ROW_NONE 0xFFFFFFFFu

/* sa_associate, sa_batch_add and sa_batch_add_deferred (filled by sa_batch_fill like any deferred slot) with the detections'
 * features described by rows; d->feats must be NULL.  Everything else that works on a slot — sa_batch_run, sa_batch_run_apply,
 * sa_batch_fetch, sa_batch_results, the taps, sa_tracks_apply* — works on it whatever staged it. */
int sa_associate_dev(sa_engine* e, uint64_t scene_id, uint64_t epoch, const sa_detections* d, const sa_dev_rows* rows,
                     uint64_t* out_track_id, uint8_t* out_voting_type);
int sa_batch_add_dev(sa_engine* e, uint64_t scene_id, uint64_t epoch, const sa_detections* d, const sa_dev_rows* rows, uint32_t* out_slot);
int sa_batch_add_deferred_dev(sa_engine* e, uint64_t scene_id, uint64_t epoch, const sa_detections* d, const sa_dev_rows* rows, uint32_t* out_slot);

/* sa_associate_batch, sa_pipe_stage and sa_pipe_submit with one descriptor pointer per scene; rows == NULL or rows[i] == NULL: scene i
 * is staged exactly as by the call without _dev.  sa_pipe_launch / sa_pipe_wait take the ticket as ever. */
int sa_associate_batch_dev(sa_engine* e, uint32_t n_scenes, const sa_scene_request* req, const sa_dev_rows* const* rows, const sa_scene_result* res);
int sa_pipe_stage_dev(sa_engine* e, uint32_t n_scenes, const sa_scene_request* req, const sa_dev_rows* const* rows, uint64_t* out_ticket);
int sa_pipe_submit_dev(sa_engine* e, uint32_t n_scenes, const sa_scene_request* req, const sa_dev_rows* const* rows, uint64_t* out_ticket);

/* sa_tracker_predict and sa_tracker_predict_batch_begin of a VisualSort / BatchVisualSort tracker with device_upkeep = 1: the
 * observations' features come from rows (one descriptor per scene in the batch form, none NULL; index entry i belongs to observation
 * i), every obs[i].feature must be NULL. */
int sa_tracker_predict_dev(sa_tracker* t, uint64_t scene_id, uint32_t n, const sa_observation* obs, const sa_dev_rows* rows, sa_sort_track* out);
int sa_tracker_predict_batch_begin_dev(sa_tracker* t, uint32_t n_scenes, const uint64_t* scene_ids, const uint32_t* counts,
                                       const sa_observation* const* obs, const sa_dev_rows* const* rows, sa_batch_result** out_result);

/* The last request-set upload of the engine that had a *_dev slot: launches = widen launches it made (0 or 1, whatever the number of
 * scenes), rows = source rows read (detections with a feature, over the scenes that were widened; a scene read in place counts none),
 * wide_rows = how many of them were read with one 16-byte load per lane and step (a row whose address is a multiple of 16, with
 * D % 4 == 0; every other row is read element by element — the choice is per row and changes no bit), src_bytes = bytes read from the
 * caller's memory.  Zeros before the first such upload.  struct_size: written by the call, sizeof(sa_framerows_stats). */
typedef struct sa_framerows_stats { uint32_t struct_size, launches; uint64_t rows, wide_rows, src_bytes; } sa_framerows_stats; /* 32 B */
int sa_framerows_last(sa_engine* e, sa_framerows_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_FRAMEROWS_H */
