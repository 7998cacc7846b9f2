// sa_compat.h — the compatibility rule of include/similari_attrs.h, once: the tiles of launch 1 (sa_gemm.hip), sa_store_merge_compat
// (sa_merge.hip) and tests/test_compat_ref.py (host compiler, behind a driver) all call this function.  No HIP in here.
//
// Reference: Track::distances' first statement (src/track.rs:609), examples/track_merging.rs:222-225 (same camera, disjoint spans),
// src/track/store/store_tests.rs:44-46 (the query ended first), the only_baked gate of TrackStore (src/track/store.rs:222-238).
#pragma once
#include <stdint.h>

#include "../../include/similari_attrs.h"

#ifndef SA_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SA_HD __host__ __device__ __forceinline__
#else
#define SA_HD inline
#endif
#endif

#define SA_COMPAT_ALL (SA_COMPAT_SAME_KEY | SA_COMPAT_DISJOINT | SA_COMPAT_QUERY_FIRST | SA_COMPAT_ONLY_READY)

// q: the query's attributes (self in self.compatible(other)), t: the stored track's.  Comparisons only: the int64 extremes are times
// like any other.
SA_HD bool sa_compat_live(uint32_t flags, int64_t ready_at, const sa_track_attrs& q, const sa_track_attrs& t) {
  bool live = true;
  if (flags & SA_COMPAT_SAME_KEY) live = live && q.key == t.key;
  if (flags & SA_COMPAT_DISJOINT) live = live && (q.start >= t.end || q.end <= t.start);
  if (flags & SA_COMPAT_QUERY_FIRST) live = live && q.end <= t.start;
  if (flags & SA_COMPAT_ONLY_READY) live = live && t.end <= ready_at;
  return live;
}

// the two attribute merges of Track::merge: the destination keeps its key and spans both
SA_HD sa_track_attrs sa_compat_union(const sa_track_attrs& dst, const sa_track_attrs& src) {
  return sa_track_attrs{dst.key, src.start < dst.start ? src.start : dst.start, src.end > dst.end ? src.end : dst.end};
}
