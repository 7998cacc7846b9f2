// sa_i8.hip — feature stores whose rows are int8 codes (include/similari_i8.h): the creation call.  Rows become their codes on the
// way in in the pad kernel of every store, k_pad_rows<source, SA_ELEM_I8> (sa_devrows.hip: two passes over the row — the unsigned
// maximum of |x_k|'s bits, then i8_code of sa_round.h — and the norm as the integer sum of the squared codes, converted once).
// sa_store_get_info is that of sa_bf16.hip, the row movers the f32 store's (an i8 row of Dp elements is Dp / 4
// floats to them, sa_store::row_floats), launch 2 and the BestFit launches see f32 cells, and launch 1 is k_search_tile_i8<JOIN, COMPAT>
// beside k_search_tile_bf16 in sa_gemm.hip.
#include "sa_store.h"

extern "C" {

int sa_store_create_i8(sa_engine* e, const sa_store_options* o, sa_store** out) {
  const char* what = "sa_store_create_i8";
  if (out) *out = nullptr;
  // without an engine the answer is about the device, as sa_store_create gives it, whatever else is wrong with the call
  if (e && o && o->struct_size >= sizeof(sa_store_options)) {
    if (o->visual_kind == SA_VIS_EUCLIDEAN)
      return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: an i8 store is cosine only (per-row scales cancel in the cosine alone; the f16 store is the compact euclidean store)", what);
    if (o->feature_len > SA_I8_MAX_FEATURE_LEN)
      return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: feature_len %u above %u (127^2 Dp must stay below 2^31)", what, o->feature_len, SA_I8_MAX_FEATURE_LEN);
  }
  return sa_store_create_as(e, o, SA_ELEM_I8, what, out);
}

}  // extern "C"
