/*
 * similari_attrs.h — track attributes and the compatibility rule of a track search (beside similari_gallery.h and similari_merge.h).
 *
 * In the reference this is the first statement of Track::distances (src/track.rs:609):
 *
 *     if !self.attributes.compatible(&other.attributes) { Err(IncompatibleAttributes) }
 *
 * whose pairs TrackStore drops silently (src/track/store.rs:217-219): they yield no distances, form no group and never reach the
 * maximum TopNVoting subtracts from.  The same worker loop holds the only_baked gate (store.rs:222-238): a stored track that is not
 * Ready is not searched.  The rules below are the ones the reference's users write: examples/track_merging.rs:222-225 (same camera,
 * disjoint time spans), src/track/store/store_tests.rs:44-46 and src/track.rs:856-858 (the query ended before the stored track began).
 *
 * Every stored track carries sa_track_attrs.  A track created by sa_store_upsert / sa_store_append has {0, 0, 0}; replacing its bank
 * keeps them, sa_store_remove drops them, and they follow their track through every compaction.  Nothing is special-cased for
 * attributes that were never set: the rule is applied to whatever is stored.  Plain sa_store_merge leaves the destination's as they are.
 *
 * Semantics of the *_compat searches: steps 2-8 of similari_search.h, and
 *
 *   1'. pairs: every query track x every stored track, except the one with the same id, a withdrawn one, and every pair for which
 *       live(q, t) is false.
 *
 * live(q, t) is the conjunction of the flagged tests (q: the query's attributes, t: the stored track's).  All tests are integer
 * comparisons — no arithmetic on times, no overflow at the int64 extremes.  A dead pair forms no group and does not raise M.
 * out_cells keeps its meaning (every distance, before steps 1 and 3), so it still holds the cells of dead pairs.  With flags 0 a
 * *_compat call returns the bits of the plain call.
 *
 * Device path: liveness is a property of a (query track, stored track) group, and a group never straddles a tile of launch 1.  The
 * tile evaluates it once per group; a tile none of whose groups is live leaves before it reads a feature row (not when out_cells is
 * asked for).  sa_store_compat_last tells how many did.
 */
#ifndef SIMILARI_ATTRS_H
#define SIMILARI_ATTRS_H

#include "similari_merge.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sa_track_attrs { uint64_t key; int64_t start; int64_t end; } sa_track_attrs; /* 24 B; start <= end */

#define SA_COMPAT_SAME_KEY 1u    /* q.key == t.key                                   track_merging.rs:224 */
#define SA_COMPAT_DISJOINT 2u    /* q.start >= t.end || q.end <= t.start             track_merging.rs:223 */
#define SA_COMPAT_QUERY_FIRST 4u /* q.end <= t.start (asymmetric)                    store_tests.rs:45, track.rs:857 */
#define SA_COMPAT_ONLY_READY 8u  /* stored track searched only if t.end <= ready_at  store.rs:222-238 (only_baked) */

typedef struct sa_compat { uint32_t struct_size; uint32_t flags; int64_t ready_at; } sa_compat; /* 16 B */

/* launch 1 of the last *_compat search (its last run): the tiles launched, and those that left before their main loop */
typedef struct sa_compat_stats { uint64_t tiles; uint64_t tiles_skipped; } sa_compat_stats;

/* flags 0, ready_at INT64_MAX */
void sa_compat_default(sa_compat* c);

/* Attributes of n stored tracks.  Refused with SA_ERR_BAD_ARG (store untouched): a null pointer, id 0, an id twice, an id the store
 * does not hold, start > end. */
int sa_store_set_attrs(sa_store* s, uint32_t n, const uint64_t* ids, const sa_track_attrs* attrs);
/* out[n], out_known[n] (1: the store holds the id; 0: out[i] is {0, 0, 0}) */
int sa_store_get_attrs(sa_store* s, uint32_t n, const uint64_t* ids, sa_track_attrs* out, uint8_t* out_known);

/* The three searches under a rule.  Everything the plain call refuses is refused the same way; besides, with SA_ERR_BAD_ARG: a null
 * sa_compat, a struct_size that is not sizeof(sa_compat), unknown flag bits, DISJOINT together with QUERY_FIRST, start > end in
 * q_attrs.
 * sa_store_search_topn_compat: q_attrs[n_queries] are the queries' attributes.  sa_store_search_stored_compat and
 * sa_store_join_topn_compat: the stored attributes of the queried tracks (an unknown id stays a query without observations);
 * SA_STORED_WITHDRAW works as before.  Under an asymmetric rule (QUERY_FIRST, ONLY_READY) live(a, b) and live(b, a) differ: the join
 * returns, direction by direction, what sa_store_search_stored_compat over sa_store_order() returns.  After a compat join,
 * sa_join_stats.blocks and sa_search_stats.groups count the unordered pairs with at least one live surviving direction. */
int sa_store_search_topn_compat(sa_store* s, const sa_topn_params* p, const sa_compat* c, uint32_t n_queries, const uint64_t* q_ids,
                                const uint32_t* q_n_obs, const float* q_feats, const sa_track_attrs* q_attrs, uint32_t* out_n,
                                uint64_t* out_winner, double* out_weight, float* out_cells);
int sa_store_search_stored_compat(sa_store* s, const sa_topn_params* p, const sa_compat* c, uint32_t flags, uint32_t n,
                                  const uint64_t* ids, uint32_t* out_n, uint64_t* out_winner, double* out_weight, float* out_cells);
int sa_store_join_topn_compat(sa_store* s, const sa_topn_params* p, const sa_compat* c, uint32_t* out_n, uint64_t* out_winner,
                              double* out_weight, float* out_cells);

/* sa_store_merge with the reference's attribute merges (Track::merge, src/track.rs:522-527).  For each destination the sources are
 * taken in call order; with rule bits set live(dst, src) must hold — the destination plays self, with its attributes as merged so
 * far — and the destination becomes {dst.key, min(start), max(end)}.  Flags 0: the union without a test (TimeAttrs::merge); flags
 * set: CamTrackingAttributes::merge.  An incompatible source refuses the WHOLE call with SA_ERR_BAD_ARG (sa_last_error names the
 * pair) and the store stays as it was.  SA_COMPAT_ONLY_READY is refused here.  Banks, retention and order are sa_store_merge's. */
int sa_store_merge_compat(sa_store* s, const sa_compat* c, uint32_t keep, uint32_t n_dst, const uint64_t* dst_ids,
                          const uint32_t* n_src, const uint64_t* src_ids, const uint32_t* capacity);

int sa_store_compat_last(sa_store* s, sa_compat_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_ATTRS_H */
