/*
 * similari_merge.h — bank upkeep on the device for the feature store of similari_search.h: append observations, merge tracks, read
 * banks back (beside similari_gallery.h, whose searches find the pairs these calls act on).
 *
 * In the reference this is the statement that follows the voting:
 *
 *     store.add(track_id, feature_class, attr, feature, ..)        Track::add_observation   src/track.rs:447-503
 *     store.merge_external(dst, &src, ..) after fetch_tracks(src)  Track::merge             src/track.rs:522-588
 *     store.fetch_tracks(ids)                                      as a read
 *
 * each followed by the metric's optimize(), which decides what a bank keeps (examples/track_merging.rs:279-297,
 * examples/incremental_track_build.rs:76-78, benches/feature_tracker.rs:72-74, VisualSORT's optimize_observations).
 *
 * A bank is the ORDERED list of a track's observations — steps 2 and 7 of similari_search.h sum in bank order — and every observation
 * carries an f32 quality, the reference's Observation::attr().  Rows written by sa_store_upsert have quality 0.  Two retention rules,
 * with a capacity C in 1..K (one per destination track; a NULL array means K for all):
 *
 *   SA_KEEP_LATEST  the last min(len, C) observations, in their order                        (reverse; truncate(C); reverse)
 *   SA_KEEP_BEST    stable sort by quality descending, then the first min(len, C); the bank's order becomes the sorted order, equal
 *                   qualities keep their earlier-first order, -0.0 == 0.0                    (sort_by(r.partial_cmp(l)); truncate(C))
 *
 * A NaN quality is refused (the reference panics on it).
 *
 * Device path: which observation lands in which slot is decided on the host from ids, counts and qualities alone
 * (similari_amd/csrc/sa_merge_plan.h); the device then moves padded rows WITH their norms — a search after a merge returns the bits a
 * freshly upserted store returns — in a fixed number of launches per call: the appended rows are padded into staging, the rows that
 * change are gathered into staging and scattered back (a bank may permute in place), and one launch runs every move of the
 * compaction.  Only ids, counts, qualities and appended rows cross the bus.
 *
 * All calls are synchronous, ordered behind the engine's queue, report through sa_last_error(engine), and follow the lifetime rules
 * of the store.  A refused call leaves the store as it was; a failure after device work began leaves it broken, as in sa_store_upsert.
 */
#ifndef SIMILARI_MERGE_H
#define SIMILARI_MERGE_H

#include "similari_gallery.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_KEEP_LATEST 0u
#define SA_KEEP_BEST 1u

/* TrackStore::add for n tracks: bank = old bank ++ the n_obs[i] (0..K) rows of feats[sum n_obs][D] in the given order, then the
 * rule runs once (equal to running it after every single observation).  quality: [sum n_obs] or NULL (all 0); capacity: [n] or NULL
 * (all K).  An unknown id creates the track, with growth and limits as in sa_store_upsert.  n_obs[i] == 0 leaves an existing bank
 * exactly as it is — no rule runs.
 * Refused with SA_ERR_BAD_ARG: id 0, an id twice, n_obs > K, a NaN quality, a capacity outside 1..K, an unknown keep. */
int sa_store_append(sa_store* s, uint32_t keep, uint32_t n, const uint64_t* ids, const uint32_t* n_obs, const float* feats,
                    const float* quality, const uint32_t* capacity);

/* fetch_tracks(src) + merge_external(dst, &src) for n_dst destinations: bank = dst ++ src0 ++ src1 .. in the order of src_ids
 * (flat, n_src[i] per destination), then the rule ALWAYS runs, also without sources.  Afterwards every source track is gone and the
 * store's order is exactly what sa_store_remove(src_ids) in call order leaves.  No merge history is kept.
 * Refused with SA_ERR_BAD_ARG: an unknown destination or source, id 0, an id twice in the call (as destination or source), a
 * capacity outside 1..K, an unknown keep. */
int sa_store_merge(sa_store* s, uint32_t keep, uint32_t n_dst, const uint64_t* dst_ids, const uint32_t* n_src,
                   const uint64_t* src_ids, const uint32_t* capacity);

/* The banks of n tracks as they lie in the store: out_n_obs[n], out_feats [n][K][D] (the bits that were put in, in bank order;
 * unfilled rows zero), out_quality NULL or [n][K].  An unknown id returns 0 observations. */
int sa_store_fetch(sa_store* s, uint32_t n, const uint64_t* ids, uint32_t* out_n_obs, float* out_feats, float* out_quality);

typedef struct sa_merge_stats { /* what the last sa_store_append or sa_store_merge did */
  double device_ms;        /* first upload to last launch, device events */
  uint64_t bytes_moved;    /* bytes the launches read and wrote */
  uint64_t rows_rewritten; /* padded rows that changed inside destination banks */
  uint32_t tracks_moved;   /* net moves of the compaction */
  uint32_t launches;       /* kernel launches: the same for any number of tracks */
} sa_merge_stats;

int sa_store_merge_last(sa_store* s, sa_merge_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_MERGE_H */
