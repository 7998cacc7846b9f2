/*
 * similari_consolidate.h — a store's mutual best pairs merged in one call on the device (beside similari_handover.h).
 *
 * The pass inside one store — tracklets of one identity merged, a gallery de-duplicated — is what similari_gallery.h names as the
 * purpose of the join (examples/track_merging.rs: every track asks the store for its best match and merges into it).  Through the
 * calls before this header it is a join, Python between, and a merge:
 *
 *     sa_store_join_bestfit(s, p, c, out_n, out_winner, out_track, out_weight, NULL);
 *     pairs (a, b) with winner(a) == b and winner(b) == a
 *     sa_store_merge(s, keep, n_pairs, dst_ids, ones, src_ids, capacity);
 *
 * sa_store_consolidate is that sequence as one call whose merge runs on the device behind the vote: no plan and no feature row
 * crosses the bus, only the join's outputs and the move list of the compaction.
 *
 * Semantics.  A call returns, and leaves in the store, exactly the bits of this sequence on the same store:
 *   1. sa_store_order gives out_ids; sa_store_join_bestfit(s, p, c, out_n, out_winner, out_track, out_weight, NULL), topn as given.
 *   2. Only entry 0 acts, as in the absorb.  w(a) = out_winner[a][0] if out_n[a] >= 1, else a's own id.  Tracks a and b are a mutual
 *      pair iff w(a) == b, w(b) == a and a != b.  w is a function, so mutual pairs are disjoint.  The destination is the lower id,
 *      the source the higher.  out_dest[i] is the destination's id for a source, out_ids[i] for every other track.
 *   3. One sa_store_merge(s, keep, n_pairs, dst_ids, n_src = all 1, src_ids, capacity per destination), destinations in out_ids
 *      order — with c != NULL sa_store_merge_compat under c with SA_COMPAT_ONLY_READY cleared (merge refuses that bit; both tracks of
 *      a pair were ready, or they would not be a pair).  The bank is dst ++ src and the rule always runs; the source leaves, and the
 *      store's order is what sa_store_remove(src_ids) in that order leaves.  Under a rule the destination's attributes become the
 *      union; with c == NULL no attribute is touched.
 *   4. With no pair the store stays exactly as it was, the state of the quality mirror included.
 * One call merges pairs, not clusters: four tracklets of one identity take two calls (similari_amd.consolidate.consolidate_all
 * repeats until a call merges nothing).
 *
 * Every array is sized for T, the store's count BEFORE the call (out_n, out_ids, out_dest: [T]; out_winner, out_track, out_weight:
 * [T][topn]); rows are in the sa_store_order() order of before the call, which out_ids returns.  out_track and out_ids may be NULL,
 * out_dest may not.  capacity: 0 means max_observations, otherwise 1 .. max_observations.
 *
 * Refusals run before anything is launched and leave the store untouched: whatever sa_store_join_bestfit refuses, with the same
 * code; SA_ERR_BAD_ARG for an unknown keep, a capacity above max_observations or a null out_dest; SA_ERR_BAD_ARG with a message for
 * SA_COMPAT_QUERY_FIRST — that rule is asymmetric, so no pair can be mutual under it.  An empty store does nothing and a store of one
 * track merges nothing; both return SA_OK.  A failure after the step was queued marks the store broken, as in the absorb.
 *
 * Device path.  The launches up to and including the vote are sa_store_join_bestfit's.  Behind the vote of the run that fits the
 * pool two launches follow whatever T is: one wave per stored track resolves entry 0's winner to a slot, then one wave per stored
 * track, if it is the lower id of a mutual pair, combines its bank with its partner's under the rule — the moves of the absorb's
 * step, with another bank of the store in place of the query rows.  After the wait the call makes for its outputs the host replays
 * the rule on its tables and removes the sources as sa_store_remove does: one more launch unless every source already lies behind
 * the tracks that stay, and one more wait.
 * Quality mirror (similari_retain.h).  Under SA_KEEP_BEST the table is uploaded ahead of the step if it is stale, as
 * sa_store_absorb_keep does, and the bytes are reported.  A call that merged a pair leaves the mirror stale — the compaction moves
 * the host table, not the mirror —; a call that merged none leaves its state as it found it.
 */
#ifndef SIMILARI_CONSOLIDATE_H
#define SIMILARI_CONSOLIDATE_H

#include "similari_handover.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sa_consolidate_stats {
  double step_ms;             /* the pair and merge launches behind the vote, device events */
  double compact_ms;          /* the compaction launch, device events; 0 without a pair */
  uint32_t pairs;             /* mutual pairs merged = tracks that left the store */
  uint32_t rows_moved;        /* padded rows written into destination banks (copied or zeroed) */
  uint32_t tracks_moved;      /* net moves of the compaction */
  uint32_t launches;          /* kernel launches behind the vote, compaction included: the same for any T (2, and the compaction's 1 if a track moves) */
  uint32_t host_waits;        /* times the call waited for the stream: the join's, and one for the compaction */
  uint32_t keep;              /* SA_KEEP_LATEST or SA_KEEP_BEST */
  uint64_t qual_upload_bytes; /* quality-mirror bytes this call uploaded (similari_retain.h) */
} sa_consolidate_stats; /* 48 B */

int sa_store_consolidate(sa_store* s, uint32_t keep, const sa_topn_params* p, const sa_compat* c, uint32_t capacity,
                         uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track, double* out_weight,
                         uint64_t* out_ids, uint64_t* out_dest);

/* The last sa_store_consolidate on s that merged a pair counts what it did; zeros before the first call, after a refused one and
 * after one that merged no pair (the store is then as it was).  sa_store_last_stats, sa_store_bestfit_last, sa_store_join_last and
 * sa_store_compat_last answer as after sa_store_join_bestfit. */
int sa_store_consolidate_last(sa_store* s, sa_consolidate_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_CONSOLIDATE_H */
