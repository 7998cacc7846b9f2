/*
 * similari_absorb.h — absorb a frame's tracks in one call: the BestFit search and the append it decides, the step taken on the device
 * (beside similari_devrows.h).
 *
 * The reference's incremental loop (examples/incremental_track_build.rs, benches/feature_tracker.rs, examples/middleware_sort_tracker.rs)
 * runs on every frame
 *
 *     (dists, _) = store.foreign_track_distances(new_tracks, FEAT0, false)
 *     winners    = voting.winners(dists)
 *     for t in new_tracks:  winner ? store.merge_external(winner, &t) : store.add_track(t)
 *
 * sa_store_absorb is that loop for one batch of new tracks, with the retention rule those loops use (keep the last C observations).
 *
 * Semantics.  A call returns, and leaves in the store, exactly the bits of this sequence on the same store:
 *
 *   1. sa_store_search_bestfit(s, p, c, n_queries, q_ids, q_n_obs, q_feats, q_attrs, out_n, out_winner, out_track, out_weight, NULL).
 *   2. Query q is MATCHED iff out_n[q] >= 1 and out_winner[q * topn] != q_ids[q].  Only entry 0 acts, as winners[..][0] does in the
 *      examples; topn stays the caller's choice for what is reported.  out_dest[q] = out_winner[q * topn] if q is matched, else
 *      q_ids[q].
 *   3. One sa_store_append(s, SA_KEEP_LATEST, n_queries, out_dest, q_n_obs, q_feats, quality, capacity): matched rows join the
 *      winner's bank; every other query becomes a track under its own id, in query order, empty ones included, exactly as append
 *      treats an unknown id.  (A matched query without observations leaves its winner's bank alone, as append does.)
 *   4. If c != NULL: a created track takes q_attrs[q]; a matched destination becomes {dst.key, min(start), max(end)}, the union of
 *      sa_store_merge_compat.  With c == NULL, q_attrs must be NULL and no attribute is touched.
 *
 * BestFit is the vote because a batch must not hand one stored track to two queries: step 3's id list is duplicate-free by
 * construction.
 *
 * Refusals.  Everything sa_store_search_bestfit and sa_store_append refuse is refused with the same code (a NaN quality, a capacity
 * outside 1..max_observations among them).  In addition a query id that the store already holds is refused with SA_ERR_BAD_ARG: the
 * reference uses fresh ids, and a query that is also a destination would make step 3 ambiguous.  The extent and the capacity
 * reservation are checked for T + n_queries tracks.  Every check and the reservation run before anything is launched, and a refused
 * call leaves the store as it was; a failure after the step was queued marks the store broken, as in sa_store_upsert.
 * An empty store: every query is created.  n_queries == 0: nothing happens.
 *
 * Known follow-up: SA_KEEP_BEST is not offered here.  It needs the qualities on the device, and the store keeps them on the host only.
 *
 * Device path.  The search's launches up to and including the vote are those of sa_store_search_bestfit.  Behind the vote of the run
 * that fits the pool, three launches whatever n_queries is — match (the stored slot of entry 0 if it holds the claim), rank (an
 * exclusive scan: an unmatched query's new slot is T + the unmatched queries before it) and move (one wave per query shifts the bank
 * and takes the padded query rows with their norms from where the search left them) — then the output copies and the call's last
 * wait.  No plan crosses the bus and the call adds no wait of its own.
 */
#ifndef SIMILARI_ABSORB_H
#define SIMILARI_ABSORB_H

#include "similari_devrows.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sa_absorb_stats {
  double step_ms;       /* the launches behind the vote, device events */
  uint32_t matched;     /* queries whose rows went into a stored track */
  uint32_t created;     /* queries that became tracks */
  uint32_t rows_moved;  /* padded rows written into banks (copied or zeroed) */
  uint32_t launches;    /* kernel launches behind the vote: the same for any n_queries */
  uint32_t host_waits;  /* times the call waited for the stream */
} sa_absorb_stats; /* 32 B */

/* quality: one f32 per observation in call order, or NULL (zeros); capacity: one per query (1..max_observations), or NULL
 * (max_observations): the arguments of sa_store_append.  out_track may be NULL; out_dest is [n_queries]. */
int sa_store_absorb(sa_store* s, const sa_topn_params* p, const sa_compat* c, uint32_t n_queries, const uint64_t* q_ids,
                    const uint32_t* q_n_obs, const float* q_feats, const sa_track_attrs* q_attrs, const float* quality,
                    const uint32_t* capacity, uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track, double* out_weight,
                    uint64_t* out_dest);
/* The same with the query rows in device memory: sa_store_search_dev (SA_VOTE_BESTFIT) followed by sa_store_append_dev. */
int sa_store_absorb_dev(sa_store* s, const sa_topn_params* p, const sa_compat* c, uint32_t n_queries, const uint64_t* q_ids,
                        const uint32_t* q_n_obs, const sa_dev_rows* rows, const sa_track_attrs* q_attrs, const float* quality,
                        const uint32_t* capacity, uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track, double* out_weight,
                        uint64_t* out_dest);
/* The last absorb of a store (zeros before the first one, and after a refused one). */
int sa_store_absorb_last(sa_store* s, sa_absorb_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_ABSORB_H */
