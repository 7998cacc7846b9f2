/*
 * similari_bf16.h — feature stores whose rows are bf16 (beside similari_bestfit.h).
 *
 * A store created by sa_store_create holds f32 rows and contracts them on the f32-input matrix instruction.  A bf16 store holds
 * half-width rows — half the memory, so twice the gallery per GPU — and contracts them on the bf16 matrix instruction
 * (v_mfma_f32_32x32x16_bf16) with f32 accumulators.
 *
 * Semantics.  A bf16 store behaves as an f32 store whose every feature value x — of stored rows and of query rows alike — was
 * replaced by bf16(x) before anything else happened.  bf16(x) is round-to-nearest-even on the f32 bit pattern u:
 *
 *       bf16(x) = the upper 16 bits of  u + 0x7fff + ((u >> 16) & 1)
 *
 * for finite x whose rounding is finite (a NaN stays a NaN).  A product of two bf16 values is exact in f32, so a bf16 store is the
 * reference's algorithm run on features rounded once to bf16, accumulated in f32: not an approximation of its own kind.  From there
 *
 *   - squared norms are those of the ROUNDED row, accumulated in f32;
 *   - distances are f32 cells: the dot product of the rounded rows with f32 accumulation, over sqrt(|a|^2 |b|^2);
 *   - the eight steps of similari_search.h hold unchanged (pairs, keep_below, M, kept cells, groups, f64 weights, ranking), and so
 *     do similari_gallery.h, similari_merge.h, similari_attrs.h and similari_bestfit.h: every call that takes a sa_store* works on
 *     a bf16 store;
 *   - rounding is idempotent: feeding back what sa_store_fetch returned changes no bit.
 *
 * The ABI keeps taking and returning f32 rows (upsert, append, queries, fetch, out_cells): rounding happens on the device on the
 * way in, and sa_store_fetch returns the stored values widened, exactly.  The limits of a store (slots, pairs) are those of an f32
 * store.
 *
 * Cosine only.  The euclidean distance of the engine is the direct sum (a - b)^2 on the vector pipe; the |a|^2 + |b|^2 - 2ab form
 * that would run on the matrix cores loses near-duplicates — the re-identification case — to cancellation.  A bf16 store with
 * SA_VIS_EUCLIDEAN is refused.
 */
#ifndef SIMILARI_BF16_H
#define SIMILARI_BF16_H

#include "similari_bestfit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_ELEM_F32  0
#define SA_ELEM_BF16 1

/* As sa_store_create, with the element type of the stored and query rows.  SA_ELEM_F32 is sa_store_create itself.  Refused beyond
 * what sa_store_create refuses: an unknown elem (SA_ERR_BAD_ARG), SA_ELEM_BF16 with SA_VIS_EUCLIDEAN (SA_ERR_UNSUPPORTED).
 * e == NULL without a gfx950 device: SA_ERR_NO_DEVICE, as sa_store_create. */
int sa_store_create_elem(sa_engine* e, const sa_store_options* o, int32_t elem, sa_store** out);

/* What a store is made of.  Dp: the padded row length in elements (a multiple of 32); Kp: observation slots per track (a power of
 * two); feature_bytes: the feature array as allocated (capacity * Kp * Dp * element size; 0 before the first row); struct_size: written
 * by the call, sizeof(sa_store_info). */
typedef struct sa_store_info { uint32_t struct_size; int32_t elem; uint32_t Dp, Kp; uint64_t feature_bytes; } sa_store_info; /* 24 B */
int sa_store_get_info(sa_store* s, sa_store_info* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_BF16_H */
