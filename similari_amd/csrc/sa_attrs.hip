// sa_attrs.hip — track attributes of the feature store (include/similari_attrs.h): the table beside ids / nobs / qual, its device
// mirror, and what the *_compat calls share.  The searches themselves are sa_search.hip's and sa_gallery.hip's with one more
// argument, the merge is sa_merge.hip's; the rule is sa_compat.h.
//
// Reference: Track::distances (src/track.rs:609), TrackStore's worker loop (src/track/store.rs:217-238).
#include "sa_compat.h"
#include "sa_store.h"

#include <vector>

int sa_store_check_compat(sa_store* s, const sa_compat* c, const char* what, bool merge) {
  sa_engine* e = s->e;
  if (!c) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null sa_compat", what);
  if (c->struct_size != sizeof(sa_compat))
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: sa_compat.struct_size %u (expected %zu)", what, c->struct_size, sizeof(sa_compat));
  if (c->flags & ~SA_COMPAT_ALL) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: unknown rule bits 0x%x", what, c->flags & ~SA_COMPAT_ALL);
  if ((c->flags & SA_COMPAT_DISJOINT) && (c->flags & SA_COMPAT_QUERY_FIRST))
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: SA_COMPAT_DISJOINT and SA_COMPAT_QUERY_FIRST exclude each other", what);
  if (merge && (c->flags & SA_COMPAT_ONLY_READY))
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: SA_COMPAT_ONLY_READY is a rule of searches", what);
  return SA_OK;
}

int sa_store_compat_begin(sa_store* s) {
  s->compat_last = sa_compat_stats{};
  const size_t bytes = (size_t)s->cap * sizeof(sa_track_attrs);
  if (!s->attrs_dirty && s->d_attrs.cap >= bytes) return SA_OK;
  SA_TRY(sa_engine_ensure(s->e, s->d_attrs, bytes));
  if (s->T) SA_HIPCHK(s->e, hipMemcpyAsync(s->d_attrs.p, s->attrs.data(), (size_t)s->T * sizeof(sa_track_attrs), hipMemcpyHostToDevice, s->st));
  s->attrs_dirty = false;
  return SA_OK;
}

extern "C" {

void sa_compat_default(sa_compat* c) {
  if (!c) return;
  c->struct_size = sizeof *c;
  c->flags = 0;
  c->ready_at = INT64_MAX;
}

int sa_store_set_attrs(sa_store* s, uint32_t n, const uint64_t* ids, const sa_track_attrs* attrs) {
  const char* what = "sa_store_set_attrs";
  if (!s) return SA_ERR_BAD_ARG;
  SA_TRY(sa_store_enter(s, what));
  sa_engine* e = s->e;
  if (n == 0) return SA_OK;
  if (!ids || !attrs) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
  std::vector<uint32_t> slots(n);
  SA_TRY(sa_store_check_ids(s, what, n, ids, slots.data(), [&](uint32_t i) {
    if (slots[i] == SA_SEARCH_NONE) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: unknown id %llu", what, (unsigned long long)ids[i]);
    if (attrs[i].start > attrs[i].end)
      return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: id %llu starts after it ends", what, (unsigned long long)ids[i]);
    return (int)SA_OK;
  }));
  for (uint32_t i = 0; i < n; ++i) s->attrs[slots[i]] = attrs[i];
  s->attrs_dirty = true;
  return SA_OK;
}

int sa_store_get_attrs(sa_store* s, uint32_t n, const uint64_t* ids, sa_track_attrs* out, uint8_t* out_known) {
  const char* what = "sa_store_get_attrs";
  if (!s) return SA_ERR_BAD_ARG;
  SA_TRY(sa_store_enter(s, what));
  if (n == 0) return SA_OK;
  if (!ids || !out || !out_known) return sa_engine_fail(s->e, SA_ERR_BAD_ARG, "%s: null argument", what);
  for (uint32_t i = 0; i < n; ++i) {
    const auto it = s->slot_of.find(ids[i]);
    out_known[i] = it != s->slot_of.end();
    out[i] = out_known[i] ? s->attrs[it->second] : sa_track_attrs{0, 0, 0};
  }
  return SA_OK;
}

int sa_store_compat_last(sa_store* s, sa_compat_stats* out) {
  if (!s || !out) return SA_ERR_BAD_ARG;
  *out = s->compat_last;
  return SA_OK;
}

}  // extern "C"
