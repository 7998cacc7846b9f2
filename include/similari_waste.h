/*
 * similari_waste.h — wasted tracker tracks enter a feature store on the device (beside similari_consolidate.h).
 *
 * In the reference a tracker and the track search are joined by wasted(): it returns whole tracks, observations and feature vectors
 * included, and examples/middleware_sort_tracker.rs and examples/track_merging.rs feed exactly those tracks to the temporary and the
 * merge store.  Here a VisualSORT track's feature bank lives in the engine's table in HBM (t_feat[T][K][Dp] with t_fpresent and
 * t_fquality), under device upkeep it never exists on the host, and sa_tracks_remove* throw it away.  The calls of this header are
 * the removal that keeps the bank: the leaving tracks' rows go from the engine's table into a store of the same engine without
 * crossing the bus.
 *
 * Semantics of sa_tracks_waste.  The call returns, and leaves in dst and in the engine, exactly the bits of this sequence, the ids
 * flattened in call order (scene after scene):
 *
 *     for every id:  sa_tracks_get_state(e, scene, id, NULL, NULL, quality[K], present[K], feats[K][D]);
 *                    rows(id) = the slots with present == 1, in slot order (slot 0 first), each with its quality; n_obs = their number
 *     sa_store_append(dst, keep, n, ids, n_obs, rows, quality, capacity);      similari_merge.h: an unknown id is created, a known one joined
 *     sa_tracks_remove_many(e, n_scenes, scene_ids, counts, ids);
 *
 * A slot with present == 0 contributes nothing: the newest observation that came without a usable feature, and an empty slot.  A
 * track with no feature row becomes a track of 0 observations, as sa_store_append makes one.  Rounding, int8 coding and norm
 * summation are dst's own, the same as in the host-fed call, for f32, f16, bf16 and i8 stores: the engine's bank is an f32 source,
 * like a SA_ELEM_F32 device block.  out_n_obs, unless NULL, takes n_obs.  A scene with counts[i] == 0 is skipped, as the removal
 * skips it.
 *
 * Refusals.  Every refusal runs before anything is launched and leaves the engine and the store untouched.  SA_ERR_BAD_ARG: a null
 * argument, an engine that is not visual, dst of another engine, dst's feature_len differing from the engine's, the engine's bank
 * depth K greater than dst's max_observations (a static check: no refusal depends on device data), whatever sa_store_append refuses
 * for these ids, keep and capacities (id 0, an id twice across the whole call), a scene twice.  SA_ERR_NOT_FOUND: an unknown scene
 * or id.  Upkeep steps that were begun are finished first, as in sa_tracks_remove_many.  One refusal does depend on device data and
 * comes behind the capture launch, which writes staging memory only: a NaN quality among the leaving rows (sa_store_append refuses
 * it); engine and store are untouched then too.  If the append fails after it was queued, the store is marked broken as ever and the
 * tables are NOT removed.
 *
 * Device path.  k_waste_capture, one wave per leaving track, ceil(scenes / 12) launches whatever the number of tracks (the
 * arguments of up to 12 scenes travel by value): the wave reads its row's present flags and qualities, compacts the present slots in
 * slot order, and copies the present rows into a staging block of the store, 16 bytes per lane and pass.  One small copy brings the
 * counts and qualities to the host — the store's host tables need them — and one wait follows.  Then sa_store_append's own body
 * runs, handed a row source "rows the library owns", then sa_tracks_remove_many.  Feature-row bytes over the bus: 0.
 *
 * sa_tracks_waste_absorb.  The leaving tracks become the queries of one sa_store_absorb_keep on dst in place of the append
 * (middleware_sort_tracker.rs's loop: a wasted track is searched in the gallery, then merged or added).  The arguments are those of
 * sa_store_hand_over with the engine, the scenes and the ids in place of src and ids, and q_attrs [sum counts], which comes exactly
 * with a rule c (both or neither).  It returns the bits of get_state + compact + sa_store_absorb_keep + sa_tracks_remove_many.
 * Refusals: those above plus the absorb's (an id that dst holds already among them).
 *
 * sa_tracker_waste_into.  While a store is attached to a VisualSORT or BatchVisualSORT tracker, every row that leaves the engine's
 * table goes through sa_tracks_waste in place of sa_tracks_remove*: the periodic waste and the eviction of expired rows (which then
 * takes the serial call for the scenes of the set).  An evicted track can never match again, so retiring it at eviction loses
 * nothing.  The guarantee: a track's bank is in dst no later than the wasted() call that reports it.  Each created track's attributes
 * are set to {key = scene_id, start = the epoch of the track's first observation, end = last_updated_epoch}.  predict() results,
 * ids, epochs and the wasted() / idle_tracks outputs are bit for bit those of the same tracker without a store.  dst must lie on
 * sa_tracker_engine(t); dst == NULL detaches.  capacity: 0 = dst's max_observations.  A tracker that is not visual is refused with
 * SA_ERR_BAD_ARG, a device group (n_devices > 1) with SA_ERR_UNSUPPORTED: one store per shard is a follow-up.  The qualities of the
 * stored rows are the engine's (t_fquality), which only device upkeep writes: under host upkeep (device_upkeep = 0) the facade writes
 * each leaving track's qualities into the table before the call.
 */
#ifndef SIMILARI_WASTE_H
#define SIMILARI_WASTE_H

#include "similari_consolidate.h"
#include "similari_tracker.h"

#ifdef __cplusplus
extern "C" {
#endif

int sa_tracks_waste(sa_engine* e, sa_store* dst, uint32_t keep, uint32_t n_scenes, const uint64_t* scene_ids, const uint32_t* counts,
                    const uint64_t* const* ids, const uint32_t* capacity /* [sum counts] or NULL */,
                    uint32_t* out_n_obs /* [sum counts] or NULL */);

/* out_n, out_dest: [sum counts]; out_winner, out_track, out_weight: [sum counts][topn] (out_track may be NULL). */
int sa_tracks_waste_absorb(sa_engine* e, sa_store* dst, uint32_t keep, const sa_topn_params* p, const sa_compat* c, uint32_t n_scenes,
                           const uint64_t* scene_ids, const uint32_t* counts, const uint64_t* const* ids, const sa_track_attrs* q_attrs,
                           const uint32_t* capacity, uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track, double* out_weight,
                           uint64_t* out_dest);

int sa_tracker_waste_into(sa_tracker* t, sa_store* dst, uint32_t keep, uint32_t capacity); /* dst == NULL detaches */

typedef struct sa_waste_stats {
  uint32_t struct_size, tracks;       /* leaving tracks of the call */
  uint32_t launches_capture;          /* launches in front of the append or the absorb: ceil(scenes / 12) */
  uint32_t reserved;
  uint64_t rows;                      /* present rows copied out of the engine's banks */
  uint64_t feature_bytes_h2d;         /* feature-row bytes this call sent over the bus: 0 */
  uint64_t feature_bytes_d2h;         /* likewise the other way: 0 */
  uint64_t table_bytes_d2h;           /* the counts and qualities the host tables need */
  double capture_ms;                  /* device events around the capture launches */
} sa_waste_stats; /* 56 B */

/* The last sa_tracks_waste or sa_tracks_waste_absorb into dst (zeros before the first one, and after a refused one). */
int sa_store_waste_last(sa_store* dst, sa_waste_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_WASTE_H */
