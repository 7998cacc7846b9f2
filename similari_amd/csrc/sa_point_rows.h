// sa_point_rows.h — the points of a keypoint call (sa_point_rows of include/similari_points.h), written once for the three sources that
// take them: sa_points.hip (the bank's filter calls), sa_pose.hip (the vote, the frame loop, the tracker's gate) and sa_pose_nms.hip
// (pose NMS).  The device view of a call's points and the read of ONE point under the presence rule, the walk of a pose's present
// points into its extent, the host's check of the descriptor, the staging of host rows, index and mask, and the dispatch on the element
// type.  The shape of the store side's SaRowSource / sa_rows_check / sa_rows_prepare (sa_store.h).  Internal: sa_points_impl.h and
// sa_pose_nms.hip include it, no other file.
#pragma once
#include "sa_store.h"
#include "sa_kalman_point.h"
#include "sa_pose_gate.h"
#include "sa_widen.h"
#include "../../include/similari_points.h"

#include <algorithm>
#include <type_traits>

// The device view of a call's points: item i of the call (a track of a filter call, a pose of a vote, a ranked pose of NMS) has its P
// points, comps elements each, in ONE row.
// Bounds, stated here for every kernel that reads through it: the row of item i is index[i] (or i), which the host checked to lie below
// n_rows of a span inside one registered block (sa_point_rows_check) or below the items of the staged host rows; SA_ROW_NONE is never
// dereferenced.  The mask byte of point p of item i is mask[i * P + p] — by ITEM, whatever row the item reads —, below items * P.
struct SaPointSrc {
  const char* base;        // row r at base + r * row_stride elements (f32, f16 or bf16: the kernel's SRC)
  uint64_t row_stride;     // elements
  const uint32_t* index;   // [items] the row of each item, SA_ROW_NONE: every point absent; nullptr: 0, 1, 2, ...
  const uint8_t* mask;     // [items][P] or nullptr
  uint32_t comps;          // 2: x, y; 3: x, y, score
  float min_score;
};

// the row of item i, SA_ROW_NONE: none
__device__ __forceinline__ uint32_t sa_point_row(const SaPointSrc& s, uint32_t i) { return s.index ? s.index[i] : i; }

// point p < P of item i, whose row is r = sa_point_row(s, i), as every consumer takes it: (x, y) widened exactly, x = NaN for an absent
// one (sa_point_present: the rule of include/similari_points.h).  base is not tested: a call without rows (a predict) does not come here.
template <int SRC>
__device__ __forceinline__ float2 sa_point_of(const SaPointSrc& s, uint32_t r, uint32_t i, uint32_t P, uint32_t p) {
  if (r == SA_ROW_NONE) return make_float2(NAN, 0.f);
  const char* row = s.base + (size_t)r * s.row_stride * (SRC == SA_ELEM_F32 ? 4u : 2u);
  const uint32_t k = p * s.comps;
  const float zx = load_elem<SRC>(row, k);
  const float zy = load_elem<SRC>(row, k + 1u);
  const float score = s.comps == 3u ? load_elem<SRC>(row, k + 2u) : 0.f;
  const bool present = sa_point_present(zx, zy, s.comps == 3u, score, s.min_score, !s.mask || s.mask[(size_t)i * P + p] != 0);
  return present ? make_float2(zx, zy) : make_float2(NAN, 0.f);
}
// ... for a thread that reads ONE point of the item; a thread that walks the item's points looks the row up once, in front of its loop
template <int SRC>
__device__ __forceinline__ float2 sa_point_at(const SaPointSrc& s, uint32_t i, uint32_t P, uint32_t p) {
  return sa_point_of<SRC>(s, sa_point_row(s, i), i, P, p);
}

// the present points of item i into q (sa_pose_gate.h), p ascending
template <int SRC>
__device__ __forceinline__ void sa_pose_extent(const SaPointSrc& s, uint32_t i, uint32_t P, sa_pose_rect& q) {
  const uint32_t r = sa_point_row(s, i);
  for (uint32_t p = 0; p < P; ++p) {
    const float2 z = sa_point_of<SRC>(s, r, i, P, p);
    if (z.x == z.x) sa_pose_rect_add(q, z.x, z.y);
  }
}

// f(std::integral_constant<int, SA_ELEM_*>) for the element type of a call's rows: the one place that decides which SRC instance runs
template <class F>
inline auto sa_point_elem(int32_t elem, F&& f) {
  if (elem == SA_ELEM_F16) return f(std::integral_constant<int, SA_ELEM_F16>{});
  if (elem == SA_ELEM_BF16) return f(std::integral_constant<int, SA_ELEM_BF16>{});
  return f(std::integral_constant<int, SA_ELEM_F32>{});
}

inline uint32_t sa_point_elem_size(int32_t elem) { return elem == SA_ELEM_F32 ? 4u : 2u; }

// The words in which the callers' refusals differ: what the rows are called when they are null, what the call's n items are called,
// and whose device the block must be on (sa_dev_rows_span's `owner`).
struct SaPointRowsWords {
  const char *rows, *items, *owner;
};
// The source of a call's points: the struct itself, then — for a descriptor — the checks of similari_devrows.h (sa_dev_rows_layout,
// sa_dev_rows_span: shared with the track search and a frame's rows) for rows of P * comps elements, of which the call reads row
// index[i] (or i) for each of its n items, SA_ROW_NONE excepted.
inline int sa_point_rows_check(sa_engine* e, const char* what, uint32_t P, uint64_t n, const sa_point_rows* r, int device, const SaPointRowsWords& w) {
  if (!r) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null %s", what, w.rows);
  if (r->struct_size != sizeof(sa_point_rows)) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: rows.struct_size %u (%zu)", what, r->struct_size, sizeof(sa_point_rows));
  if (r->comps != 2u && r->comps != 3u) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: rows.comps %u (2: x, y; 3: x, y, score)", what, r->comps);
  if ((r->host != nullptr) == (r->dev != nullptr)) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: exactly one of rows.host and rows.dev", what);
  const sa_dev_rows* d = r->dev;
  if (!d) return SA_OK;
  const uint64_t len = (uint64_t)P * r->comps;
  if (d->struct_size < sizeof(sa_dev_rows)) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: rows.struct_size too small", what);
  SA_TRY(sa_dev_rows_layout(e, what, d, len, "row length"));
  if (d->n_rows == 0 || d->n_rows >= 0xffffffffull) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: rows.n_rows must be in 1 .. 2^32 - 2", what);
  if (d->index) {
    for (uint64_t i = 0; i < n; ++i)
      if (d->index[i] != SA_ROW_NONE && d->index[i] >= d->n_rows)
        return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: rows.index[%llu] = %u is not below n_rows %llu", what, (unsigned long long)i, d->index[i],
                              (unsigned long long)d->n_rows);
  } else if (n > d->n_rows)
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: %llu %s but rows.n_rows is %llu (and no index)", what, (unsigned long long)n, w.items,
                          (unsigned long long)d->n_rows);
  return sa_dev_rows_span(e, what, d, len, device, w.owner);
}

// The n items of a checked call where the kernels read them: host rows go up into `pts`, the index into `index`, the mask into `mask`,
// in this order; rows in device memory stay where they are.  out: the view; elem: the rows' element type (host rows: f32); bytes_h2d
// grows by what was uploaded, src_bytes is set to what the kernels read of the caller's device memory (a descriptor only).
inline int sa_point_rows_stage(sa_engine* e, hipStream_t st, uint32_t P, uint32_t n, const sa_point_rows* rows, DevBuf& pts, DevBuf& index, DevBuf& mask,
                               SaPointSrc& out, int32_t& elem, uint64_t& bytes_h2d, uint64_t& src_bytes) {
  const uint64_t np = (uint64_t)n * P;
  out.comps = rows->comps, out.min_score = rows->min_score;
  elem = SA_ELEM_F32;
  if (rows->host) {
    const size_t bytes = (size_t)np * rows->comps * 4;
    SA_TRY(sa_engine_ensure(e, pts, bytes));
    SA_HIPCHK(e, hipMemcpyAsync(pts.p, rows->host, bytes, hipMemcpyHostToDevice, st));
    bytes_h2d += bytes;
    out.base = (const char*)pts.p;
    out.row_stride = (uint64_t)P * rows->comps;
  } else {
    const sa_dev_rows* d = rows->dev;
    elem = d->elem;
    out.base = (const char*)d->base;
    out.row_stride = d->row_stride;
    uint64_t read = n;
    if (d->index) {
      SA_TRY(sa_engine_ensure(e, index, (size_t)n * 4));
      SA_HIPCHK(e, hipMemcpyAsync(index.p, d->index, (size_t)n * 4, hipMemcpyHostToDevice, st));
      bytes_h2d += (uint64_t)n * 4;
      out.index = (const uint32_t*)index.p;
      read = (uint64_t)(n - std::count(d->index, d->index + n, SA_ROW_NONE));
    }
    src_bytes = read * P * rows->comps * sa_point_elem_size(elem);
  }
  if (rows->present) {
    SA_TRY(sa_engine_ensure(e, mask, (size_t)np));
    SA_HIPCHK(e, hipMemcpyAsync(mask.p, rows->present, (size_t)np, hipMemcpyHostToDevice, st));
    bytes_h2d += np;
    out.mask = (const uint8_t*)mask.p;
  }
  return SA_OK;
}
