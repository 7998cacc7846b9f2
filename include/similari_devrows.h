/*
 * similari_devrows.h — feature rows read from device memory (beside similari_f16.h).
 *
 * A ReID network leaves its embeddings in device memory, as f32, f16 or bf16.  Every call of similari_search.h .. similari_bestfit.h
 * that takes feature rows takes them as host f32; the calls here take them where they lie: only the id tables and one small row
 * table cross the bus.
 *
 * Semantics.  A *_dev call returns, and leaves in the store, exactly the bits that the corresponding host call returns and leaves
 * when it is fed widen(x) as f32 for every source element x.  widen is the exact conversion to f32: the identity for an f32 source;
 * for f16 and bf16 sources every value is representable, subnormals, +-inf and NaN (sign and payload kept, payload in the upper
 * mantissa bits) included.  Everything in similari_search.h .. similari_f16.h holds unchanged from there: the eight steps, rounding
 * to the store's element type, norms of the rounded row, rho, the rule that runs once after an append.  All three store element
 * types accept all three source types.
 *
 * Where the rows may lie.  The span [base, base + ((n_rows - 1) * row_stride + D) * elem_size) must lie inside one block registered
 * with sa_device_block_register (similari_assoc.h), and that block's device must be the store's.  The contract is that of detection
 * features read in place: rows are final when the call is made (the engine's stream does not know the producer's), and the calls
 * are synchronous, so the rows are free again when the call returns.  Every check runs on the host before any launch; a refused
 * call (SA_ERR_BAD_ARG, sa_last_error names the cause) leaves the store as it was.  Everything the host calls refuse, these refuse
 * with the same code.
 */
#ifndef SIMILARI_DEVROWS_H
#define SIMILARI_DEVROWS_H

#include "similari_f16.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The vote of sa_store_search_dev. */
#define SA_VOTE_TOPN    0u
#define SA_VOTE_BESTFIT 1u

typedef struct sa_dev_rows {
  uint32_t struct_size;   /* sizeof(sa_dev_rows) = 40 */
  int32_t  elem;          /* SA_ELEM_F32 | SA_ELEM_BF16 | SA_ELEM_F16: the type of the elements in device memory */
  const void* base;       /* device address of element 0 of row 0; aligned to the element size */
  uint64_t n_rows;        /* rows addressable from base, < 2^32 - 1 */
  uint64_t row_stride;    /* ELEMENTS from one row to the next, >= D */
  const uint32_t* index;  /* HOST array [sum n_obs], the source row of each observation in call order; NULL = 0, 1, 2, ... ; a row may be named more than once */
} sa_dev_rows;

/* sa_store_upsert (similari_search.h) and sa_store_append (similari_merge.h) with rows from device memory. */
int sa_store_upsert_dev(sa_store* s, uint32_t n, const uint64_t* ids, const uint32_t* n_obs, const sa_dev_rows* rows);
int sa_store_append_dev(sa_store* s, uint32_t keep, uint32_t n, const uint64_t* ids, const uint32_t* n_obs,
                        const sa_dev_rows* rows, const float* quality, const uint32_t* capacity);
/* sa_store_search_topn, sa_store_search_topn_compat and sa_store_search_bestfit with query rows from device memory.
 * vote: SA_VOTE_TOPN (out_track must be NULL) | SA_VOTE_BESTFIT.  c / q_attrs: both NULL (the plain call) or both given (the *_compat call). */
int sa_store_search_dev(sa_store* s, const sa_topn_params* p, uint32_t vote, const sa_compat* c, uint32_t n_queries,
                        const uint64_t* q_ids, const uint32_t* q_n_obs, const sa_dev_rows* q_rows, const sa_track_attrs* q_attrs,
                        uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track, double* out_weight, float* out_cells);

/* The last *_dev call of a store: rows = source rows read, wide_rows = how many of them were read with one wide load per lane and
 * step (4 B for a 16-bit source into a 16-bit store; 8 B for f32 into a 16-bit store, or for a 16-bit source into an f32 store with
 * D % 4 == 0; 16 B for f32 into an f32 store with D % 4 == 0; every other row is read element by element — the choice is per row,
 * by its address, and changes no result bit), src_bytes = bytes read from the caller's memory.  Zeros for a store that never made
 * such a call.  struct_size: written by the call, sizeof(sa_devrows_stats). */
typedef struct sa_devrows_stats { uint32_t struct_size, reserved; uint64_t rows, wide_rows, src_bytes; } sa_devrows_stats; /* 32 B */
int sa_store_devrows_last(sa_store* s, sa_devrows_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_DEVROWS_H */
