/*
 * similari_handover.h — ready tracks handed from one feature store to another on the device (beside similari_i8.h).
 *
 * The reference's track search is a pipeline of two stores (examples/track_merging.rs:371-481; the same shape in
 * incremental_track_build.rs:162-164, middleware_sort_tracker.rs:86-88 and simple.rs:35):
 *
 *     baked = temp_store.find_usable()                        tracks whose attributes say Ready
 *     for id in baked:
 *         track = temp_store.fetch_tracks(&[id])              leaves temp_store
 *         winners = voting.winners(merge_store.foreign_track_distances([track]))
 *         winners.is_empty() ? merge_store.add_track(track) : merge_store.merge_external(winner, &track)
 *
 * sa_store_ready is find_usable, sa_store_take is fetch_tracks, and sa_store_hand_over is the loop: both stores lie on one GPU and
 * one stream, so the feature rows never leave the device.
 *
 * Semantics of sa_store_hand_over.  It returns, and leaves in both stores, exactly the bits of
 *
 *     sa_store_fetch(src, n, ids, nobs, feats, quality);  sa_store_get_attrs(src, n, ids, attrs, known);
 *     sa_store_absorb_keep(dst, keep, p, c, n, ids, nobs, compact(feats), c ? attrs : NULL, compact(quality), capacity, out_...);
 *     sa_store_remove(src, n, ids);
 *
 * where compact drops the unfilled rows of fetch's [n][K][D] layout.  Everything similari_absorb.h, similari_retain.h and
 * similari_merge.h document carries over.  Fetch returns the stored values — f16 and bf16 widened exactly, the codes of an i8 store —,
 * so dst rounds, encodes and sums norms exactly as the host call does.  A transfer between stores of one element type reproduces the
 * source rows: re-rounding a rounded row is the identity, and a non-zero i8 row holds a +-127 code, so its scale is 1.  src's order
 * afterwards is what sa_store_remove(ids) in call order leaves; dst's absorb, retain, BestFit and search stats are those of the absorb.
 * The queries' counts, attributes and qualities are src's host tables; with c == NULL no attribute of dst changes.
 *
 * Refusals.  Every check runs before anything is launched, and a refused call leaves both stores untouched, the state of the quality
 * mirror included.  SA_ERR_BAD_ARG: src == dst, stores of two engines, feature_len differing, an id that src does not hold, id 0 or an
 * id twice, a taken track with more observations than dst's max_observations, and whatever sa_store_absorb_keep refuses (an id that
 * dst holds already among it).  SA_ERR_UNSUPPORTED, with a message: an i8 source into a store of another element type — codes are
 * directions, not values.  i8 into i8 is allowed, and so is any of f32, f16 or bf16 into any of the four store types; visual_kind may
 * differ between the stores: rows are rows.  A failure after dst's step was queued marks dst broken and leaves src as it was; a
 * failure inside src's compaction marks src broken.  n == 0 does nothing.  An empty dst creates every track.
 *
 * Device path.  One launch fills the query side of dst's search from src's banks whatever n is (a copy of the padded rows with their
 * norm words between stores of one element type; widen, round and sum as dst's pad kernel does otherwise), then the absorb's own
 * launches, then one launch moves src's last tracks into the holes (the net moves of the removal, planned on the host).
 * sa_store_remove takes the same single launch.
 */
#ifndef SIMILARI_HANDOVER_H
#define SIMILARI_HANDOVER_H

#include "similari_i8.h"

#ifdef __cplusplus
extern "C" {
#endif

/* find_usable: the ids whose stored attributes satisfy end <= ready_at, in sa_store_order() order ({0, 0, 0} until
 * sa_store_set_attrs).  *out_n takes their number; out_ids, unless NULL, the first min(cap, *out_n) of them.  Host only, no launch. */
int sa_store_ready(sa_store* s, int64_t ready_at, uint64_t* out_ids, uint32_t cap, uint32_t* out_n);

/* fetch_tracks: sa_store_fetch(s, n, ids, out_n_obs, out_feats, out_quality) + sa_store_get_attrs (out_attrs may be NULL),
 * then sa_store_remove(s, n, ids).  An unknown id returns 0 observations, as fetch does, and is ignored by the removal.
 * The removal is one launch whatever n is. */
int sa_store_take(sa_store* s, uint32_t n, const uint64_t* ids, uint32_t* out_n_obs, float* out_feats, float* out_quality,
                  sa_track_attrs* out_attrs);

/* The loop above for n tracks of src: they become the queries of one sa_store_absorb_keep on dst and leave src. */
int sa_store_hand_over(sa_store* src, sa_store* dst, uint32_t keep, const sa_topn_params* p, const sa_compat* c, uint32_t n,
                       const uint64_t* ids, const uint32_t* capacity, uint32_t* out_n, uint64_t* out_winner,
                       uint64_t* out_track, double* out_weight, uint64_t* out_dest);

typedef struct sa_handover_stats {
  uint32_t struct_size, launches_fill;  /* launches that fill dst's query side: the same for any n */
  uint32_t launches_compact;            /* launches of src's compaction: 0 or 1 */
  uint32_t tracks_moved;                /* net moves of src's compaction */
  uint64_t rows;                        /* observation rows read from src's banks */
  uint64_t feature_bytes_h2d;           /* feature-row bytes this call sent over the bus: 0 */
  uint64_t feature_bytes_d2h;           /* likewise the other way: 0 */
  double fill_ms, compact_ms;           /* device events */
} sa_handover_stats; /* 56 B */

/* The last sa_store_hand_over into dst (zeros before the first one, and after a refused one).  A store that was the subject of
 * sa_store_take or sa_store_remove since answers with that call's compaction: launches_compact and tracks_moved (sa_store_take:
 * compact_ms too), the other fields zero. */
int sa_store_handover_last(sa_store* dst, sa_handover_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_HANDOVER_H */
