/*
 * similari_gallery.h — track search whose queries are tracks the store already holds (beside similari_search.h, whose store,
 * parameters, steps 1-8, limits and lifetime rules it shares).
 *
 * In the reference:
 *
 *     store.owned_track_distances(ids, feature_class, false)     src/track/store.rs:471-486
 *         the named tracks are taken out of the store (fetch_tracks), searched against what is left, and put back;
 *     the loop of examples/track_merging.rs run over a whole store: every stored track searched against every other one,
 *         the job that merges tracklets and de-duplicates a gallery.
 *
 * Both read the banks where they lie on the device — padded, with norms, in the layout the contraction reads.  No feature crosses
 * the bus: sa_store_search_stored sends the list of queried slots, sa_store_join_topn sends nothing.
 *
 * sa_store_search_stored(ids) answers exactly what sa_store_search_topn answers when each named track's bank is handed to it as a
 * query under its own id: one M for the call, the self pair skipped, ranking by weight descending then id ascending.  An id the
 * store does not hold is a query without observations (0 winners, NaN cells), as fetch_tracks skips it.  With SA_STORED_WITHDRAW
 * the queried tracks are out of the store for the call: a pair of two queried tracks is no pair — it forms no group and does not
 * raise M.  That is owned_track_distances.
 *
 * sa_store_join_topn is sa_store_search_stored without flags over sa_store_order's ids in that order, computed once per unordered
 * pair: d(a, b) and d(b, a) are the same bits (symmetric terms, the same order of accumulation), so the contraction runs only the
 * tiles that reach the diagonal or lie above it, a (query, stored track) group is voted once for both directions and keeps ONE pool
 * block, and the second launch reads that block row by row for the lower slot and column by column for the higher one — each
 * query's weight is the sequential sum in ITS order of step 2.
 *
 * Counting: after either call sa_search_stats.groups counts pool blocks.  For sa_store_search_stored that is the surviving (query,
 * stored track) groups, as for sa_store_search_topn; for a join it is the surviving UNORDERED pairs (sa_join_stats.blocks), half
 * the ordered groups.  Device memory of a join: 4 B per ordered pair (T * T), 4 Kp^2 + 16 B per block.
 *
 * Limits are those of a search of T stored tracks by n (or T) queries (sa_search_extent): a join needs T * Kp <= 65535 * 32 and
 * T * T < 2^32 - 1.  Both calls are synchronous, ordered behind the engine's queue, leave the store unchanged when they refuse, fill
 * sa_store_last_stats, and report errors through sa_last_error(engine).  No CPU fallback.
 */
#ifndef SIMILARI_GALLERY_H
#define SIMILARI_GALLERY_H

#include "similari_search.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_STORED_WITHDRAW 1u   /* queried tracks are out of the store for the call: owned_track_distances */

/* Search with n stored tracks as queries, named by id.  Outputs as sa_store_search_topn: out_n[n], out_winner / out_weight
 * [n][topn], out_cells NULL or [n][K][count][K] (every distance, self pairs and withdrawn pairs included).
 * Refused with SA_ERR_BAD_ARG: id 0, an id given twice, null pointers, NaN parameters, unknown flag bits. */
int sa_store_search_stored(sa_store* s, const sa_topn_params* p, uint32_t flags, uint32_t n, const uint64_t* ids,
                           uint32_t* out_n, uint64_t* out_winner, double* out_weight, float* out_cells);

/* Every stored track as a query, rows in sa_store_order order: out_n[T], out_winner / out_weight [T][topn], out_cells NULL or
 * [T][K][T][K]. */
int sa_store_join_topn(sa_store* s, const sa_topn_params* p,
                       uint32_t* out_n, uint64_t* out_winner, double* out_weight, float* out_cells);

typedef struct sa_join_stats {
  uint64_t tiles;       /* workgroups launch 1 of the last join ran */
  uint64_t tiles_rect;  /* what sa_store_search_topn's grid would be for the same rows */
  uint32_t blocks;      /* pool blocks = surviving unordered pairs */
  uint32_t reserved;
} sa_join_stats;

int sa_store_join_last(sa_store* s, sa_join_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_GALLERY_H */
