/*
 * similari_i8.h — feature stores whose rows are int8 codes (beside similari_bf16.h and similari_f16.h).
 *
 * An int8 store holds a row in a quarter of the bytes of an f32 store — four times the gallery per GPU — and contracts the codes on
 * the int8 matrix instruction (v_mfma_i32_32x32x32_i8) with i32 accumulators.  A per-row scale cancels in the cosine
 * a.b / sqrt(|a|^2 |b|^2), so the store keeps no scale at all: dot products and squared norms are exact integers.
 *
 * Semantics.  An i8 store behaves as an f32 store whose every row x — stored rows and query rows alike — was replaced by codes(x)
 * before anything else happened:
 *
 *       m   = max over k of |x_k|                                   (f32)
 *       ZERO ROW if m == 0, or m is not finite (a NaN or an inf anywhere in the row), or m < 2^-100
 *       inv = 127.0f / m                                            (one correctly rounded f32 division)
 *       q_k = clamp(rintf(x_k * inv), -127, 127)                    (one f32 product, round half to even); a ZERO ROW: all q_k = 0
 *
 * The 2^-100 floor guarantees that no subnormal product can round to a non-zero code, whatever the denormal mode.  A non-zero row
 * always holds a +-127.  From there
 *
 *   - the squared norm of a row is the exact integer n = sum q_k^2, summed and reduced in integers; the norm array holds f32(n),
 *     converted once, round-to-nearest-even: no summation order is involved;
 *   - a cell is f32(dot) / sqrtf(f32(na) * f32(nb)), dot the exact i32 dot product of the codes from the matrix cores.  A zero row
 *     gives 0 / 0 = NaN — the reference's zero-vector cosine, which neither raises M nor is kept.  Cell (i, j) and cell (j, i) have
 *     the same bits; a pair of rows with equal codes gives exactly 1.0f (sqrtf(x * x) == x);
 *   - the eight steps of similari_search.h hold unchanged (pairs, keep_below, M, kept cells, groups, f64 weights, ranking), and so do
 *     similari_gallery.h, similari_merge.h, similari_attrs.h, similari_bestfit.h, similari_devrows.h, similari_absorb.h and
 *     similari_retain.h: every call that takes a sa_store* works on an i8 store, sa_store_get_info answers elem == SA_ELEM_I8;
 *   - directions, not lengths: sa_store_fetch returns each row as its codes widened to f32 (integers in -127 .. 127), the stored row
 *     up to a positive factor.  Feeding it back changes no bit: a non-zero row holds a +-127, so m = 127 and inv = 1.
 *
 * The ABI keeps taking and returning f32 rows (upsert, append, queries, fetch, out_cells): the codes are taken on the device on the
 * way in.  Rows in device memory (similari_devrows.h) are f32, f16 or bf16 as before, widened exactly and then coded; source rows of
 * int8 are not offered.  Dp, the padded row length, is a multiple of 64 elements (64 bytes); feature_bytes = capacity * Kp * Dp.
 *
 * Cosine only.  With per-row scales the expansion sa^2 na + sb^2 nb - 2 sa sb dot cancels for near-proportional rows even in f64, and
 * a per-store scale wastes the code range on normalised features: an i8 store with SA_VIS_EUCLIDEAN is refused.  The f16 store is the
 * compact euclidean store.
 *
 * Limit.  feature_len <= 131072: then 127^2 Dp < 2^31 and neither an accumulator nor a norm can overflow.
 */
#ifndef SIMILARI_I8_H
#define SIMILARI_I8_H

#include "similari_retain.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The element type sa_store_get_info reports for an i8 store.  sa_store_create_elem does not take it: an i8 store has a limit and a
 * padding of its own and is created by sa_store_create_i8. */
#define SA_ELEM_I8 8
#define SA_I8_MAX_FEATURE_LEN 131072u

/* As sa_store_create, for a store of int8 codes.  Refused beyond what sa_store_create refuses: SA_VIS_EUCLIDEAN and a feature_len
 * above SA_I8_MAX_FEATURE_LEN (SA_ERR_UNSUPPORTED, each with a message).  e == NULL without a gfx950 device: SA_ERR_NO_DEVICE, as
 * sa_store_create. */
int sa_store_create_i8(sa_engine* e, const sa_store_options* o, sa_store** out);

#ifdef __cplusplus
}
#endif
#endif /* SIMILARI_I8_H */
