/*
 * similari_bestfit.h — track search under the BestFit vote: one claimant per stored track (beside similari_attrs.h).
 *
 * The reference has two voting engines over TrackStore::foreign_track_distances: TopNVoting (src/track/voting/topn.rs), which the
 * searches of similari_search.h, similari_gallery.h and similari_attrs.h answer, and BestFitVoting (src/track/voting/best.rs:52-128),
 * which these answer.  TopN ranks every query on its own, so ten queries may all name one stored track as their winner; BestFit puts
 * every surviving group of the call into one ranked list and lets a stored track be claimed once.
 *
 * Semantics: steps 1-7 of similari_search.h — under a rule, step 1' of similari_attrs.h; SA_STORED_WITHDRAW as in similari_gallery.h.
 * M, the kept cells, the groups and their f64 weights are those of the TopN call with the same arguments, bit for bit.  Then
 *
 *   8b. ranking: all surviving groups of the call form ONE list ranked by weight descending, then query id ascending, then stored id
 *       ascending.  (The reference stable-sorts the order of a HashMap, so its ties are unspecified; this is the engine's rule.)
 *       Within one query this is TopN's order.
 *   9b. claim: walking that list, a stored track is claimed by the first group that names it — column t belongs to the best-ranked
 *       group among all groups (., t).  The claim runs over ALL surviving groups of the call, whatever topn is.
 *  10b. result: query q's row lists its first topn groups in list order.  Entry r: out_track[q][r] = the stored id the group names,
 *       out_weight[q][r] its weight, out_winner[q][r] = that stored id if the group holds the claim, else q's own id
 *       (best.rs:112-119).  A self pair never forms a group, so "winner == query id" is unambiguous.  out_n[q] = entries written;
 *       the rest of the row is zero.  The reference returns a query's whole list; the engine truncates it at topn <= 64.
 *
 * So (out_n, out_track, out_weight) of a call equal (out_n, out_winner, out_weight) of the corresponding TopN call, and a stored id
 * appears as out_winner at most once in the whole call.  The result cannot be computed from the TopN call's output: the claim runs
 * over the groups that call does not return, and it crosses queries.
 *
 * Device path: launch 1 is the one of the TopN call.  Stage 2 is three launches of one workgroup per query — weights and the best
 * weight per column, the lowest query id among a column's best, the ranked rows — ordered by their launch boundaries alone (integer
 * atomics, no waiting), so the result does not depend on arrival order.
 */
#ifndef SIMILARI_BESTFIT_H
#define SIMILARI_BESTFIT_H

#include "similari_attrs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* stage 2 of the last BestFit call (its last run): the three launches; groups = ordered surviving groups of the call (in a join
 * each live direction counts), claimed = stored tracks with a claimant.  Groups that lost their track: groups - claimed. */
typedef struct sa_bestfit_stats { double weigh_ms, claim_ms, rank_ms; uint32_t groups; uint32_t claimed; } sa_bestfit_stats; /* 32 B */

/* The three searches under the BestFit vote.  c == NULL: no rule — the plain path, which neither uploads nor reads attributes; c != NULL:
 * the rule of the *_compat call.  q_attrs must be non-NULL exactly when c is (SA_ERR_BAD_ARG otherwise).  out_track and out_cells may
 * be NULL; out_winner, out_track, out_weight are [n][topn], out_cells as in the TopN call.  Everything the corresponding TopN call —
 * sa_store_search_topn / _stored / sa_store_join_topn, or its *_compat twin when c != NULL — refuses is refused with the same code:
 * SA_ERR_BAD_ARG for a null store, null params, topn 0, a NaN max_distance or keep_below, a null q_ids / q_n_obs / ids / out_n /
 * out_winner / out_weight, id 0, an id twice in one call, more than max_observations observations, null q_feats with observations,
 * unknown flag bits, a struct_size that is not sizeof(sa_compat), unknown rule bits, DISJOINT together with QUERY_FIRST, start > end
 * in q_attrs; SA_ERR_UNSUPPORTED for topn > 64 and an extent beyond the search's limits.  A refused call leaves the store unchanged.
 * Afterwards sa_store_last_stats is filled as ever (launch1_ms: launch 1; launch2_ms: the sum of the stage-2 launches; groups: pool
 * blocks), sa_store_join_last and sa_store_compat_last where they apply. */
int sa_store_search_bestfit(sa_store* s, const sa_topn_params* p, const sa_compat* c, uint32_t n_queries, const uint64_t* q_ids,
                            const uint32_t* q_n_obs, const float* q_feats, const sa_track_attrs* q_attrs, uint32_t* out_n,
                            uint64_t* out_winner, uint64_t* out_track, double* out_weight, float* out_cells);
int sa_store_search_stored_bestfit(sa_store* s, const sa_topn_params* p, const sa_compat* c, uint32_t flags, uint32_t n,
                                   const uint64_t* ids, uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track, double* out_weight,
                                   float* out_cells);
int sa_store_join_bestfit(sa_store* s, const sa_topn_params* p, const sa_compat* c, uint32_t* out_n, uint64_t* out_winner,
                          uint64_t* out_track, double* out_weight, float* out_cells);

int sa_store_bestfit_last(sa_store* s, sa_bestfit_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_BESTFIT_H */
