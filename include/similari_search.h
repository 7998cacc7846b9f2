/*
 * similari_search.h — track search on the MI355X: TopN voting over a device-resident feature store.
 *
 * In the reference this is the pair of statements
 *
 *     store.foreign_track_distances(query_tracks, feature_class, false);  TopNVoting::winners(dists)
 *
 *     TrackStore::foreign_track_distances   src/track/store.rs:429-460 (worker loop :199-240)
 *     Track::distances                      src/track.rs:604-652
 *     TopNVoting::winners                   src/track/voting/topn.rs:82-135
 *
 * used for re-identification and track merging (examples/track_merging.rs, incremental_track_build.rs,
 * middleware_sort_tracker.rs, simple.rs).  A store holds the feature banks of T tracks on the engine's device; a
 * search pairs every query track with every stored track of another id, computes all observation distances of each
 * pair (cosine or euclidean, src/distance.rs) and votes them as TopNVoting does:
 *
 *   1. pairs: every query track x every stored track except the one with the SAME id (store.rs:206);
 *   2. distances: all observation pairs of a pair, query observation outer, stored observation inner (track.rs:617-640);
 *      cosine is the similarity a.b / sqrt(|a|^2 |b|^2), as the reference names it;
 *   3. keep_below: a distance d >= keep_below is dropped (+inf: nothing is, the identity postprocess of track.rs:191-196);
 *   4. M = max(-1, max of every remaining distance of the CALL) — all queries, all pairs, kept or not;
 *   5. kept cells: d <= max_distance (a NaN distance, cosine of a zero vector, neither raises M nor is kept);
 *   6. groups: (query, stored track) pairs with at least max(1, min_votes) kept cells;
 *   7. weight: sequential f64 sum, in the order of step 2, of f64(f32(M - d)) over the group's kept cells;
 *   8. ranking per query: weight descending, then winner id ascending (the reference breaks ties in HashMap order);
 *      truncated to topn.  A query without a group gets 0 winners.
 *
 * Device path: the store keeps T tracks x Kp slots (Kp = the next power of two >= max_observations) of rows padded to
 * a multiple of 32 floats, with norms, per-track observation counts and ids; removal compacts by moving the last
 * tracks into the holes; capacity doubles.  A search is two launches on the engine's stream: the contraction with a
 * group epilogue (votes counted inside the tile, the cells of surviving groups written to a pool) and one workgroup
 * per query that sums the weights and selects the top-N.  Device memory per search: 4 B per (query, stored track)
 * pair, plus 4 Kp^2 + 8 B per block of the group pool (the pool keeps its size between searches; a search with more
 * surviving groups than it holds grows it to a quarter more than that search needs and runs once more).
 *
 * Limits (SA_ERR_UNSUPPORTED): feature_len up to 2^24; at most 2^31 - 1 stored observation slots (tracks x Kp); per
 * search at most 65535 x 32 query observation slots (queries x Kp) and fewer than 2^32 - 1 (query, stored track)
 * pairs.  Feature rows are addressed with 64-bit offsets, so a store may hold any number of floats the device has
 * memory for within those counts.
 *
 * Lifetime: a store belongs to its engine.  Destroy stores before their engine; an engine destroyed first frees its
 * stores' device memory, and every later call on such a store but sa_store_destroy fails with SA_ERR_STATE (message:
 * sa_last_error(NULL)).  If a device call fails half-way through sa_store_upsert or sa_store_remove, the store fails
 * every later call with SA_ERR_STATE too: destroy it and build it again.
 *
 * Every call is synchronous and ordered behind whatever the engine has queued.  The store touches none of the
 * engine's scene tables, taps or captured graphs.  Errors go to sa_last_error(engine).  No CPU fallback.
 */
#ifndef SIMILARI_SEARCH_H
#define SIMILARI_SEARCH_H

#include "similari_assoc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sa_store sa_store;

typedef struct sa_store_options {
  uint32_t struct_size;       /* sizeof(sa_store_options) */
  int32_t visual_kind;        /* SA_VIS_COSINE | SA_VIS_EUCLIDEAN */
  uint32_t feature_len;       /* D > 0 */
  uint32_t max_observations;  /* K, 1..32: observations per track, for the store and for queries */
} sa_store_options;

typedef struct sa_topn_params {
  uint32_t topn;        /* 1..64 */
  uint32_t min_votes;   /* 0 counts as 1 */
  float max_distance;   /* kept cells: d <= max_distance */
  float keep_below;     /* dropped cells: d >= keep_below (+inf: none) */
} sa_topn_params;

typedef struct sa_search_stats {  /* what the last sa_store_search_topn did */
  double launch1_ms;      /* contraction + group epilogue (its last run), device events */
  double launch2_ms;      /* weights + top-N (its last run), device events */
  double call_ms;         /* every launch of the call, device events */
  uint32_t groups;        /* surviving groups */
  uint32_t reruns;        /* 1: the pool overflowed and the search ran once more */
  uint64_t pool_bytes;    /* the group pool's size after the call */
} sa_search_stats;

/* Defaults: cosine, feature_len 0 (must be set), max_observations 1. */
void sa_store_options_default(sa_store_options* o);
/* Lives on e's device and stream.  e == NULL without a gfx950 device: SA_ERR_NO_DEVICE.  max_observations > 32:
 * SA_ERR_UNSUPPORTED. */
int sa_store_create(sa_engine* e, const sa_store_options* o, sa_store** out);
void sa_store_destroy(sa_store* s);
/* Inserts or replaces the whole bank of each track: n_obs[i] (0..K) rows of feats[sum n_obs][D], in track order.
 * Ids must be non-zero and distinct within the call. */
int sa_store_upsert(sa_store* s, uint32_t n, const uint64_t* ids, const uint32_t* n_obs, const float* feats);
/* Unknown ids are ignored (as sa_tracks_remove). */
int sa_store_remove(sa_store* s, uint32_t n, const uint64_t* ids);
int sa_store_count(sa_store* s, uint32_t* out_n);
/* Ids in column order of out_cells (out_ids may be NULL to ask for the count). */
int sa_store_order(sa_store* s, uint64_t* out_ids, uint32_t cap, uint32_t* out_n);
/* One search.  q_feats: [sum q_n_obs][D] in query order.  Per query q: out_n[q] winners in out_winner[q * topn ...]
 * and out_weight[q * topn ...] (the rest of the row is zero).
 * out_cells (NULL, or [n_queries][K][count][K] f32): every distance of the call before steps 1 and 3 — self pairs and
 * distances >= keep_below included — NaN where an observation is absent; columns in sa_store_order order.
 * Refused with SA_ERR_BAD_ARG: duplicate query ids, id 0, q_n_obs > K, null pointers, a NaN max_distance or
 * keep_below; SA_ERR_UNSUPPORTED: topn > 64, a search beyond the limits above.  A refused call leaves the store as it
 * was. */
int sa_store_search_topn(sa_store* s, const sa_topn_params* p, uint32_t n_queries, const uint64_t* q_ids,
                         const uint32_t* q_n_obs, const float* q_feats, uint32_t* out_n, uint64_t* out_winner,
                         double* out_weight, float* out_cells);
int sa_store_last_stats(sa_store* s, sa_search_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_SEARCH_H */
