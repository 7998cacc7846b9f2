// sa_f16.hip — feature stores whose rows are IEEE binary16 (include/similari_f16.h): the counters of the euclidean expansion
// (sa_store_expand_last).  Rows are rounded on the way in by the pad kernel of every store, k_pad_rows<source, SA_ELEM_F16>
// (sa_devrows.hip: f16_bits and f16_widen of sa_round.h, the norm of the ROUNDED row).  The creation call and sa_store_get_info are those of sa_bf16.hip, the
// row movers the f32 store's (a 16-bit row of Dp elements is Dp / 2 floats to them, sa_store::row_floats), launch 2 and the BestFit
// launches see f32 cells, and launch 1 is k_search_tile_f16<EU, JOIN, COMPAT> beside k_search_tile_bf16 in sa_gemm.hip.
#include "sa_store.h"

extern "C" {

int sa_store_expand_last(sa_store* s, sa_expand_stats* out) {
  if (!s || !out) return SA_ERR_BAD_ARG;
  if (!s->e || s->broken) return sa_store_enter(s, "sa_store_expand_last");
  *out = s->expand_last;
  out->struct_size = sizeof *out;
  out->reserved = 0;
  return SA_OK;
}

}  // extern "C"
