/*
 * similari_f16.h — feature stores whose rows are IEEE binary16 (beside similari_bf16.h).
 *
 * ReID networks on a GPU emit fp16 embeddings.  A bf16 store rounds them to 8 significant bits, an f32 store spends twice the memory
 * on bits that are not there; an f16 store takes such rows unchanged, at half the memory of an f32 store, and contracts them on the
 * f16 matrix instruction (v_mfma_f32_32x32x16_f16) with f32 accumulators — for BOTH metrics, euclidean included.
 *
 * Semantics.  An f16 store behaves as an f32 store whose every feature value x — of stored rows and of query rows alike — was
 * replaced by f16(x) before anything else happened.  f16(x) is the IEEE binary16 conversion, round-to-nearest-even: overflow goes to
 * +-inf (|x| >= 65520), a NaN stays a NaN, subnormals are kept (the f16 matrix instruction of gfx950 takes subnormal inputs as
 * they are).  A row that is already f16-representable is stored without loss.  A product of two f16 values
 * (11 x 11 significant bits) is exact in f32, so an f16 store is the reference's algorithm run on features rounded once to f16,
 * accumulated in f32: not an approximation of its own kind.  From there
 *
 *   - squared norms are those of the ROUNDED row, accumulated in f32;
 *   - cosine cells: the dot product of the rounded rows with f32 accumulation, over sqrt(|a|^2 |b|^2), as in a bf16 store;
 *   - euclidean cells: with s = |a|^2 + |b|^2 and d2 = s - 2 a.b (the dot product from the matrix cores),
 *         sqrt(max(d2, 0))                                           unless d2 < rho * s,
 *         sqrt(sum over k of (a_k - b_k)^2), f32 differences of the widened rows, f32 sum        for such a FLAGGED cell:
 *     the expansion cancels on near-identical rows — the re-identification case — so a cell it cannot be trusted with to 1e-5
 *     relative is recomputed directly.  rho = 5e-3 sqrt(Dp), Dp the padded row length; a NaN never flags and stays NaN; an exact
 *     duplicate pair comes out as exactly 0.0; cell (i, j) and cell (j, i) have the same bits.  A store whose rho reaches 1
 *     (Dp >= 40000) recomputes every cell and is merely slow;
 *   - the eight steps of similari_search.h hold unchanged (pairs, keep_below, M, kept cells, groups, f64 weights, ranking), and so
 *     do similari_gallery.h, similari_merge.h, similari_attrs.h, similari_bestfit.h and similari_bf16.h: every call that takes a
 *     sa_store* works on an f16 store, sa_store_get_info answers elem == SA_ELEM_F16;
 *   - rounding is idempotent: sa_store_fetch returns the stored values widened, exactly, and feeding them back changes no bit.
 *
 * The ABI keeps taking and returning f32 rows (upsert, append, queries, fetch, out_cells): rounding happens on the device on the
 * way in.  The limits of a store (slots, pairs) are those of an f32 store.
 */
#ifndef SIMILARI_F16_H
#define SIMILARI_F16_H

#include "similari_bf16.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The third element type of sa_store_create_elem (similari_bf16.h): accepted with SA_VIS_COSINE and with SA_VIS_EUCLIDEAN. */
#define SA_ELEM_F16 2

/* Launch 1 of the last search, stored search or join of an f16 euclidean store: cells = the flagged cells it recomputed directly,
 * tiles = the tiles that recomputed any (of a rerun after the pool grew: the rerun's).  Zeros for every other store and before
 * the first search.  struct_size: written by the call, sizeof(sa_expand_stats). */
typedef struct sa_expand_stats { uint32_t struct_size; uint32_t reserved; uint64_t cells, tiles; } sa_expand_stats; /* 24 B */
int sa_store_expand_last(sa_store* s, sa_expand_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_F16_H */
