/*
 * similari_retain.h — absorb a frame's tracks under either retention rule: the follow-up similari_absorb.h names ("SA_KEEP_BEST is
 * not offered here").  The store now mirrors its qualities on the device, so the one-call form of the incremental loop serves the
 * rule of examples/track_merging.rs:279-297 and of VisualSORT's feature banks (stable sort by quality descending, truncate) as well
 * as "keep the last C".
 *
 * Semantics.  sa_store_absorb_keep(s, keep, ...) returns, and leaves in the store, exactly the bits of steps 1-4 of
 * similari_absorb.h with step 3 being
 *
 *     sa_store_append(s, keep, n_queries, out_dest, q_n_obs, q_feats, quality, capacity)
 *
 * and everything similari_merge.h documents for that rule carries over.  Under SA_KEEP_BEST: the combined bank — the destination's
 * rows in bank order, then the query's rows in call order — is sorted by quality descending, stably (-0.0 == 0.0 in the compare), and
 * the first min(len, C) observations stay in sorted order; each row moves with its norm and its quality; positions past the new count
 * are zero, with norm 0 and quality +0.0.  A bank that was not in quality order before (after an upsert, after SA_KEEP_LATEST calls)
 * is fully reordered.  A matched query without rows leaves its bank exactly as it is: no rule runs, and an unsorted bank stays
 * unsorted.  A created track's own rows are sorted and cut to C.
 * keep == SA_KEEP_LATEST is the body of sa_store_absorb itself: the same launches, the same bits.
 *
 * Refusals.  Everything sa_store_absorb refuses, with the same codes; an unknown keep is SA_ERR_BAD_ARG.  Every check runs before
 * anything is launched, and a refused call leaves the store as it was, the state of the quality mirror included.
 *
 * The quality mirror.  The host table stays authoritative.  Every call that changes it (upsert, append, merge, remove, a
 * SA_KEEP_LATEST absorb, a reservation that reallocates) marks the mirror stale on the host and costs nothing else.  A SA_KEEP_BEST
 * absorb that finds it stale uploads the whole table once, queued on the store's stream ahead of the step (qual_upload_bytes); the
 * step then writes the mirror itself and the call leaves it valid, so in a loop of SA_KEEP_BEST absorbs only the call's own qualities
 * cross the bus ([n_queries][Kp] f32).
 *
 * Device path.  Still three launches behind the vote whatever n_queries is: match and rank as in similari_absorb.h, then a move in
 * which one wave per query ranks the combined bank (at most 64 observations, one per lane) and permutes the rows in place.
 */
#ifndef SIMILARI_RETAIN_H
#define SIMILARI_RETAIN_H

#include "similari_absorb.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sa_retain_stats {
  double step_ms;             /* as sa_absorb_stats: the launches behind the vote, device events */
  uint32_t matched;           /* queries whose rows went into a stored track */
  uint32_t created;           /* queries that became tracks */
  uint32_t rows_moved;        /* padded rows written into banks (copied or zeroed) */
  uint32_t launches;          /* kernel launches behind the vote: the same for any n_queries */
  uint32_t host_waits;        /* times the call waited for the stream */
  uint32_t keep;              /* the rule of the call: SA_KEEP_LATEST or SA_KEEP_BEST */
  uint64_t qual_upload_bytes; /* bytes of the quality mirror this call uploaded; 0: the mirror was valid, or the rule does not read it */
} sa_retain_stats; /* 40 B */

/* sa_store_absorb with the retention rule as an argument: keep is SA_KEEP_LATEST or SA_KEEP_BEST (similari_merge.h). */
int sa_store_absorb_keep(sa_store* s, uint32_t keep, const sa_topn_params* p, const sa_compat* c, uint32_t n_queries,
                         const uint64_t* q_ids, const uint32_t* q_n_obs, const float* q_feats, const sa_track_attrs* q_attrs,
                         const float* quality, const uint32_t* capacity, uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track,
                         double* out_weight, uint64_t* out_dest);
/* The same with the query rows in device memory, as sa_store_absorb_dev. */
int sa_store_absorb_keep_dev(sa_store* s, uint32_t keep, const sa_topn_params* p, const sa_compat* c, uint32_t n_queries,
                             const uint64_t* q_ids, const uint32_t* q_n_obs, const sa_dev_rows* rows, const sa_track_attrs* q_attrs,
                             const float* quality, const uint32_t* capacity, uint32_t* out_n, uint64_t* out_winner,
                             uint64_t* out_track, double* out_weight, uint64_t* out_dest);
/* The last absorb of a store through any of the four entry points (zeros before the first one, and after a refused one). */
int sa_store_retain_last(sa_store* s, sa_retain_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_RETAIN_H */
