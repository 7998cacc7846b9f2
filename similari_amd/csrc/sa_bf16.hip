// sa_bf16.hip — feature stores whose rows are bf16 (include/similari_bf16.h): the creation call with an element type, what a store
// is made of (sa_store_get_info).  Rows are rounded on the way in by the pad kernel of every store, k_pad_rows<source, SA_ELEM_BF16>
// (sa_devrows.hip: bf16_bits of sa_round.h, the norm of the ROUNDED row).  Everything else a bf16 store does is the f32 store's
// code: the row movers (k_gather, k_merge_gather / _scatter / _compact, the removal's device copies) copy 16-byte pieces of a row and
// are handed its length in floats (sa_store::row_floats, half of Dp), launch 2 and the BestFit launches see f32 cells, and launch 1
// is k_search_tile_bf16 beside k_search_tile in sa_gemm.hip, whose epilogue it shares.
#include "sa_store.h"

extern "C" {

int sa_store_create_elem(sa_engine* e, const sa_store_options* o, int32_t elem, sa_store** out) {
  const char* what = "sa_store_create_elem";
  if (out) *out = nullptr;
  if (elem == SA_ELEM_F32) return sa_store_create(e, o, out);
  // without an engine the answer is about the device, as sa_store_create gives it, whatever else is wrong with the call
  if (e && elem != SA_ELEM_BF16 && elem != SA_ELEM_F16)
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: unknown element type %d (SA_ELEM_F32, SA_ELEM_BF16, SA_ELEM_F16)", what, elem);
  if (e && elem == SA_ELEM_BF16 && o && o->struct_size >= sizeof(sa_store_options) && o->visual_kind == SA_VIS_EUCLIDEAN)
    return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: a bf16 store is cosine only (the euclidean distance is the direct sum on f32 rows)", what);
  return sa_store_create_as(e, o, elem, what, out);
}

int sa_store_get_info(sa_store* s, sa_store_info* out) {
  if (!s || !out) return SA_ERR_BAD_ARG;
  if (!s->e || s->broken) return sa_store_enter(s, "sa_store_get_info");
  out->struct_size = sizeof *out;
  out->elem = s->elem;
  out->Dp = s->Dp;
  out->Kp = s->Kp;
  out->feature_bytes = (uint64_t)s->cap * s->Kp * s->row_bytes();
  return SA_OK;
}

}  // extern "C"
