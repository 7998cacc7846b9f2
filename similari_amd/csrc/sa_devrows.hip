// sa_devrows.hip — the one way a feature store fills padded rows, and feature rows read from device memory
// (include/similari_devrows.h).  Whatever a call's rows come from (SaRowSource, sa_store.h: the caller's host memory, the caller's
// device block, another store, a block the library owns), the source resolves to (element type, base, stride in elements, row table)
// and ONE launch of k_pad_rows pads, converts and sums — the int8 codes of include/similari_i8.h included.  Host rows go up as the
// caller passed them and are then an f32 block the library owns.  The only other route is the same-type hand-over copy
// k_handover_rows (sa_handover.hip), which moves norms as words.  Here too: the host checks of a descriptor, the row table, and the
// three *_dev calls, which are the bodies of sa_store_upsert, sa_store_append and the host-fed searches (sa_search.hip, sa_merge.hip,
// sa_bestfit.hip) handed another row source.
// Launch 1, launch 2, the BestFit launches, the pool and the merge plan do not know where the padded rows came from.
// A new element type of stores adds a DST branch to k_pad_rows and nothing else on this side.
#include "sa_round.h"
#include "sa_store.h"
#include "sa_widen.h"

namespace {

constexpr uint32_t PAD_THREADS = 256, PAD_ROWS = PAD_THREADS / 64;

__host__ __device__ inline uint32_t elem_bytes(int elem) { return elem == SA_ELEM_F32 ? 4u : 2u; }

// Bytes of the one load per lane and step that a row of `src` elements takes into a store of `dst` elements when its address is a
// multiple of it; 0: no wide route (an f32 store whose D is no multiple of 4 sums one element per lane).  An i8 store takes four
// neighbouring elements per lane and step, whatever D is.
__host__ __device__ inline uint32_t wide_bytes(int src, int dst, uint32_t D) {
  const bool s16 = src != SA_ELEM_F32;
  if (dst == SA_ELEM_I8) return s16 ? 8u : 16u;
  if (dst != SA_ELEM_F32) return s16 ? 4u : 8u;
  if (D & 3u) return 0u;
  return s16 ? 8u : 16u;
}
__host__ __device__ inline bool row_is_wide(uint64_t addr, uint32_t w) { return w && (addr & (uint64_t)(w - 1u)) == 0; }

// the store's rounding of a 16-bit store (sa_round.h: to nearest, ties to even) and the value the rounded element stands for
template <int DST>
__device__ __forceinline__ uint32_t round16(float x) { return DST == SA_ELEM_BF16 ? bf16_bits(x) : f16_bits(x); }
template <int DST>
__device__ __forceinline__ float stored16(uint32_t b) { return DST == SA_ELEM_BF16 ? __uint_as_float(b << 16) : f16_widen(b); }

// The pad kernel of every store.  One wave per destination row, four rows per workgroup: zero-pad D -> Dp, convert to the store's
// element type, scatter (row r -> slots[r / K] * K + r % K, or r), and the squared norm of the STORED row in f32.  table[row]: the
// source row, at base + table[row] * row_stride elements (64-bit arithmetic); SA_SEARCH_NONE: an absent row — zeros, norm 0, base is
// not touched.
// The order of the norm's f32 sum is a property of the store and D alone — the bits of a stored norm do not depend on the source's
// type, stride or alignment, nor on which call wrote the row — and it is defined here (tests/golden/store_rows_parent.npz pins it):
//   a 16-bit store: lane l owns elements 2l, 2l + 1, stepping by 128, and adds x * x + y * y of the ROUNDED values per step;
//   an f32 store, D % 4 == 0: lane l owns 4l .. 4l + 3, stepping by 256, and adds the four squares in one expression, left to right;
//   an f32 store, any other D: lane l owns element l, stepping by 64, one square per step;
//   an i8 store: no order at all — the row is read twice (the absmax, then the codes of include/similari_i8.h, lane l owning elements
//     4l .. 4l + 3, stepping by 256) and the norm is an integer sum, converted once;
//   then, for the f32 sums, the wave's butterfly: acc += shfl_xor(acc, o) for o = 32, 16, .. 1.  An absent row sums zeros: norm +0.
// A row whose address is a multiple of wide_bytes takes one load of that width per lane and step, any other row one load per
// element: the choice is wave-uniform and changes no bit.  No load reaches past element D - 1 of a row: a wide load is taken only
// where all its elements lie below D.
template <int SRC, int DST>
__global__ __launch_bounds__(PAD_THREADS) void k_pad_rows(const char* __restrict__ base, uint64_t row_stride,
                                                          const uint32_t* __restrict__ table, uint32_t rows, uint32_t D, uint32_t Dp,
                                                          uint32_t K, const uint32_t* __restrict__ slots, void* __restrict__ dst,
                                                          float* __restrict__ norms) {
  const uint32_t row = blockIdx.x * PAD_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= rows) return;
  const uint32_t drow = slots ? slots[row / K] * K + row % K : row;
  const uint32_t t = table[row];
  const bool pres = t != SA_SEARCH_NONE;
  const char* s = base + (pres ? (uint64_t)t * row_stride * elem_bytes(SRC) : 0ull);
  const bool wide = pres && row_is_wide((uint64_t)(uintptr_t)s, wide_bytes(SRC, DST, D));
  float acc = 0.0f;
  if (DST == SA_ELEM_I8) {
    uint32_t* d = (uint32_t*)((uint8_t*)dst + (size_t)drow * Dp);
    // elements k .. k + 3 of the source row, widened; zeros past D and of an absent row
    auto load4 = [&](uint32_t k) {
      float4 x = float4{0.f, 0.f, 0.f, 0.f};
      if (wide && k + 3 < D) {
        if (SRC == SA_ELEM_F32) x = *(const float4*)(s + (size_t)k * 4);
        else {
          const uint2 w = *(const uint2*)(s + (size_t)k * 2);
          x = float4{widen16<SRC>(w.x & 0xffffu), widen16<SRC>(w.x >> 16), widen16<SRC>(w.y & 0xffffu), widen16<SRC>(w.y >> 16)};
        }
      } else if (pres) {
        if (k < D) x.x = load_elem<SRC>(s, k);
        if (k + 1 < D) x.y = load_elem<SRC>(s, k + 1);
        if (k + 2 < D) x.z = load_elem<SRC>(s, k + 2);
        if (k + 3 < D) x.w = load_elem<SRC>(s, k + 3);
      }
      return x;
    };
    uint32_t mb = 0;
    for (uint32_t k = 4 * lane; k < D; k += 256u) {
      const float4 x = load4(k);
      const uint32_t b0 = i8_abs_bits(x.x), b1 = i8_abs_bits(x.y), b2 = i8_abs_bits(x.z), b3 = i8_abs_bits(x.w);
      const uint32_t b01 = b0 > b1 ? b0 : b1, b23 = b2 > b3 ? b2 : b3, b = b01 > b23 ? b01 : b23;
      mb = b > mb ? b : mb;
    }
    const float inv = i8_inv(i8_wave_max(mb));
    uint32_t n = 0;
    for (uint32_t k = 4 * lane; k < Dp; k += 256u) {
      const float4 x = k < D ? load4(k) : float4{0.f, 0.f, 0.f, 0.f};
      const uint32_t c0 = i8_code(x.x, inv), c1 = i8_code(x.y, inv), c2 = i8_code(x.z, inv), c3 = i8_code(x.w, inv);
      d[k >> 2] = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
      const int q0 = i8_value(c0), q1 = i8_value(c1), q2 = i8_value(c2), q3 = i8_value(c3);
      n += (uint32_t)(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    }
    for (int o = 32; o > 0; o >>= 1) n += (uint32_t)__shfl_xor((int)n, o);
    if (lane == 0) norms[drow] = (float)n;
    return;
  } else if (DST != SA_ELEM_F32) {
    uint32_t* d = (uint32_t*)((uint16_t*)dst + (size_t)drow * Dp);
    for (uint32_t k = 2 * lane; k < Dp; k += 128u) {
      float a = 0.0f, b = 0.0f;
      if (wide && k + 1 < D) {
        if (SRC == SA_ELEM_F32) {
          const float2 v = *(const float2*)(s + (size_t)k * 4);
          a = v.x, b = v.y;
        } else {
          const uint32_t w = *(const uint32_t*)(s + (size_t)k * 2);
          a = widen16<SRC>(w & 0xffffu), b = widen16<SRC>(w >> 16);
        }
      } else if (pres) {
        if (k < D) a = load_elem<SRC>(s, k);
        if (k + 1 < D) b = load_elem<SRC>(s, k + 1);
      }
      const uint32_t lo = pres && k < D ? round16<DST>(a) : 0u, hi = pres && k + 1 < D ? round16<DST>(b) : 0u;
      d[k >> 1] = lo | (hi << 16);
      const float x = stored16<DST>(lo), y = stored16<DST>(hi);
      acc += x * x + y * y;
    }
  } else {
    float* d = (float*)dst + (size_t)drow * Dp;
    if (pres && (D & 3u) == 0) {
      for (uint32_t k = lane * 4; k < Dp; k += 256u) {
        float4 x = float4{0.f, 0.f, 0.f, 0.f};
        if (k < D) {   // D % 4 == 0: all four lie below D
          if (wide && SRC == SA_ELEM_F32) x = *(const float4*)(s + (size_t)k * 4);
          else if (wide) {
            const uint2 w = *(const uint2*)(s + (size_t)k * 2);
            x = float4{widen16<SRC>(w.x & 0xffffu), widen16<SRC>(w.x >> 16), widen16<SRC>(w.y & 0xffffu), widen16<SRC>(w.y >> 16)};
          } else x = float4{load_elem<SRC>(s, k), load_elem<SRC>(s, k + 1), load_elem<SRC>(s, k + 2), load_elem<SRC>(s, k + 3)};
        }
        *(float4*)(d + k) = x;
        acc += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
      }
    } else {
      for (uint32_t k = lane; k < Dp; k += 64u) {
        const float x = (pres && k < D) ? load_elem<SRC>(s, k) : 0.0f;
        d[k] = x;
        acc += x * x;
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) norms[drow] = acc;
}

using PadRows = void (*)(const char*, uint64_t, const uint32_t*, uint32_t, uint32_t, uint32_t, uint32_t, const uint32_t*, void*, float*);
template <int SRC>
PadRows pad_rows_to(int dst) {
  return dst == SA_ELEM_BF16 ? k_pad_rows<SRC, SA_ELEM_BF16> : dst == SA_ELEM_F16 ? k_pad_rows<SRC, SA_ELEM_F16>
       : dst == SA_ELEM_I8 ? k_pad_rows<SRC, SA_ELEM_I8> : k_pad_rows<SRC, SA_ELEM_F32>;
}
PadRows pad_rows_kernel(int src, int dst) {
  return src == SA_ELEM_BF16 ? pad_rows_to<SA_ELEM_BF16>(dst) : src == SA_ELEM_F16 ? pad_rows_to<SA_ELEM_F16>(dst) : pad_rows_to<SA_ELEM_F32>(dst);
}

// k_pad_rows over a resolved source (SaRows, sa_store.h: elem rows of `stride` elements from `base`, d_table on the device): one launch
int sa_devrows_pad_own(sa_store* s, const SaRows& R, uint32_t K, const uint32_t* slots, void* dst, float* norms) {
  hipLaunchKernelGGL(pad_rows_kernel(R.elem, s->elem), dim3((R.rows + PAD_ROWS - 1) / PAD_ROWS), dim3(PAD_THREADS), 0, s->st, (const char*)R.base,
                     R.stride, R.d_table, R.rows, s->D, s->Dp, K, slots, dst, norms);
  SA_HIPCHK(s->e, hipGetLastError());
  return SA_OK;
}

const char* elem_name(int elem) { return elem == SA_ELEM_F32 ? "f32" : elem == SA_ELEM_BF16 ? "bf16" : "f16"; }

}  // namespace

// ---- what every reader of a caller's device rows checks (sa_engine.h): the track search here, a frame's rows (sa_framerows.hip), a
// point bank's points (sa_points.hip) ----
int sa_dev_rows_layout(sa_engine* e, const char* what, const sa_dev_rows* r, uint64_t len, const char* length_name) {
  if (r->elem != SA_ELEM_F32 && r->elem != SA_ELEM_BF16 && r->elem != SA_ELEM_F16)
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: unknown element type %d of rows (SA_ELEM_F32, SA_ELEM_BF16, SA_ELEM_F16)", what, r->elem);
  if (!r->base) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null rows.base", what);
  const uint32_t eb = elem_bytes(r->elem);
  if ((uintptr_t)r->base & (eb - 1u))
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: rows.base is not aligned to its %s elements (%u bytes)", what, elem_name(r->elem), eb);
  if (r->row_stride < len)
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: rows.row_stride %llu is below the %s %llu", what, (unsigned long long)r->row_stride, length_name,
                          (unsigned long long)len);
  return SA_OK;
}

int sa_dev_rows_span(sa_engine* e, const char* what, const sa_dev_rows* r, uint64_t len, int device, const char* owner) {
  // ((n_rows - 1) * row_stride + len) * elem bytes: n_rows >= 1 here; 128-bit, so that no stride wraps the span into a small one
  const unsigned __int128 span = ((unsigned __int128)(r->n_rows - 1) * r->row_stride + len) * elem_bytes(r->elem);
  int on = -1;
  if (span > ((unsigned __int128)1 << 48) || !sa_in_device_block(r->base, (size_t)span, &on))
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: the rows' span is not inside one block registered with sa_device_block_register", what);
  if (on != device)
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: the rows lie in a block registered for device %d, %s device %d", what, on, owner, device);
  return SA_OK;
}

int sa_devrows_check(sa_store* s, const char* what, const sa_dev_rows* r, size_t total) {
  sa_engine* e = s->e;
  if (!total) return SA_OK;
  if (!r) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null rows", what);
  if (r->struct_size < sizeof(sa_dev_rows)) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: rows.struct_size too small", what);
  SA_TRY(sa_dev_rows_layout(e, what, r, s->D, "feature length"));
  if (r->n_rows >= 0xffffffffull) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: rows.n_rows must be below 2^32 - 1", what);
  if (r->index) {
    for (size_t j = 0; j < total; ++j)
      if (r->index[j] >= r->n_rows)
        return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: rows.index[%zu] = %u is not below n_rows %llu", what, j, r->index[j], (unsigned long long)r->n_rows);
  } else if (total > r->n_rows)
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: %zu observations but rows.n_rows is %llu (and no index)", what, total, (unsigned long long)r->n_rows);
  return sa_dev_rows_span(e, what, r, s->D, s->device, "this store is on");
}

void sa_devrows_table(uint32_t n, const uint32_t* n_obs, const uint32_t* index, uint32_t Kp, std::vector<uint32_t>& table) {
  table.assign((size_t)n * Kp, SA_SEARCH_NONE);
  uint32_t off = 0;
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t k = 0; k < n_obs[i]; ++k, ++off) table[(size_t)i * Kp + k] = index ? index[off] : off;
}

int sa_rows_check(sa_store* s, const char* what, const SaRowSource& src, size_t total, const char* name) {
  if (src.kind == SaRowSource::DEVICE) return sa_devrows_check(s, what, src.dev, total);
  if (src.kind == SaRowSource::HOST && total && !src.base) return sa_engine_fail(s->e, SA_ERR_BAD_ARG, "%s: null %s", what, name);
  return SA_OK;
}

int sa_rows_prepare(sa_store* s, const SaRowSource& src, uint32_t n, const uint32_t* n_obs, size_t total, bool banked, SaRows& R) {
  sa_engine* e = s->e;
  R = SaRows{};
  R.src = &src;
  R.total = total;
  R.rows = banked ? n * s->Kp : (uint32_t)total;
  if (!R.rows) return SA_OK;
  const bool host = src.kind == SaRowSource::HOST, dev = src.kind == SaRowSource::DEVICE;
  if (host || dev) {   // the call's rows in order, or as the descriptor's index names them
    const uint32_t* index = dev && total ? src.dev->index : nullptr;
    if (banked) sa_devrows_table(n, n_obs, index, s->Kp, R.built);
    else {
      R.built.resize(total);
      for (uint32_t j = 0; j < R.rows; ++j) R.built[j] = index ? index[j] : j;
    }
    R.table = &R.built;
  } else if (src.kind == SaRowSource::STORE || !banked) R.table = src.table;
  if (R.table) {
    SA_TRY(sa_engine_ensure(e, s->dr_table, (size_t)R.rows * 4));
    R.d_table = (const uint32_t*)s->dr_table.p;
  } else R.d_table = src.d_table;
  // without a row to read a descriptor was not checked and host rows may be null: the kernel gets no address at all (every table
  // entry is SA_SEARCH_NONE)
  if (host && total) {
    SA_TRY(sa_engine_ensure(e, s->stage, total * s->D * 4));
    R.base = s->stage.p, R.stride = s->D;
  } else if (dev && total) R.elem = src.dev->elem, R.base = src.dev->base, R.stride = src.dev->row_stride;
  else if (src.kind == SaRowSource::STORE) R.elem = src.store->elem, R.base = src.store->feat.p, R.stride = src.store->Dp;   // row t lies Dp elements after row t - 1, and the first D of them are read
  else if (src.kind == SaRowSource::OWN) R.base = src.base, R.stride = src.stride;
  return SA_OK;
}

int sa_rows_fill(sa_store* s, const SaRows& R, uint32_t K, const uint32_t* slots, void* dst, float* norms) {
  sa_engine* e = s->e;
  if (!R.rows) return SA_OK;
  const SaRowSource& src = *R.src;
  if (src.kind == SaRowSource::DEVICE) {
    const uint32_t eb = elem_bytes(R.elem), w = wide_bytes(R.elem, s->elem, s->D);
    sa_devrows_stats& st = s->devrows_last;
    for (const uint32_t t : R.built)
      if (t != SA_SEARCH_NONE) {
        ++st.rows;
        st.wide_rows += row_is_wide((uint64_t)(uintptr_t)R.base + (uint64_t)t * R.stride * eb, w) ? 1u : 0u;   // the kernel's own test
      }
    st.src_bytes = st.rows * s->D * eb;
  }
  if (src.kind == SaRowSource::HOST && R.total)
    SA_HIPCHK(e, hipMemcpyAsync(s->stage.p, src.base, R.total * s->D * 4, hipMemcpyHostToDevice, s->st));
  if (R.table) SA_HIPCHK(e, hipMemcpyAsync(s->dr_table.p, R.table->data(), (size_t)R.rows * 4, hipMemcpyHostToDevice, s->st));
  const bool handed = src.kind == SaRowSource::STORE;
  if (handed) SA_TRY(sa_handover_fill_begin(s, *R.table));
  if (handed && R.elem == s->elem) SA_TRY(sa_handover_copy(s, src.store, R.d_table, R.rows, dst, norms));   // Dp is equal: both pad the same feature_len by the same rule
  else SA_TRY(sa_devrows_pad_own(s, R, K, slots, dst, norms));
  if (handed) {
    ++s->handover_last.launches_fill;
    SA_HIPCHK(e, hipEventRecord(s->hev[1], s->st));
  }
  return SA_OK;
}

extern "C" {

int sa_store_upsert_dev(sa_store* s, uint32_t n, const uint64_t* ids, const uint32_t* n_obs, const sa_dev_rows* rows) {
  if (!s) return SA_ERR_BAD_ARG;
  s->devrows_last = sa_devrows_stats{};
  return sa_store_upsert_impl(s, "sa_store_upsert_dev", n, ids, n_obs, SaRowSource::of_device(rows));
}

int sa_store_append_dev(sa_store* s, uint32_t keep, uint32_t n, const uint64_t* ids, const uint32_t* n_obs, const sa_dev_rows* rows,
                        const float* quality, const uint32_t* capacity) {
  if (!s) return SA_ERR_BAD_ARG;
  s->devrows_last = sa_devrows_stats{};
  return sa_store_append_impl(s, "sa_store_append_dev", keep, n, ids, n_obs, SaRowSource::of_device(rows), quality, capacity);
}

int sa_store_search_dev(sa_store* s, const sa_topn_params* p, uint32_t vote, const sa_compat* c, uint32_t n_queries,
                        const uint64_t* q_ids, const uint32_t* q_n_obs, const sa_dev_rows* q_rows, const sa_track_attrs* q_attrs,
                        uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track, double* out_weight, float* out_cells) {
  const char* what = "sa_store_search_dev";
  if (!s) return SA_ERR_BAD_ARG;
  s->devrows_last = sa_devrows_stats{};
  SA_TRY(sa_store_enter(s, what));
  if (vote != SA_VOTE_TOPN && vote != SA_VOTE_BESTFIT)
    return sa_engine_fail(s->e, SA_ERR_BAD_ARG, "%s: unknown vote %u (SA_VOTE_TOPN, SA_VOTE_BESTFIT)", what, vote);
  if (vote == SA_VOTE_TOPN && out_track) return sa_engine_fail(s->e, SA_ERR_BAD_ARG, "%s: out_track with SA_VOTE_TOPN", what);
  if ((c != nullptr) != (q_attrs != nullptr))
    return sa_engine_fail(s->e, SA_ERR_BAD_ARG, "%s: a rule and q_attrs come together or not at all", what);
  const SaRowSource src = SaRowSource::of_device(q_rows);
  if (vote == SA_VOTE_TOPN)
    return sa_store_search_topn_impl(s, what, p, c != nullptr, c, n_queries, q_ids, q_n_obs, src, q_attrs, out_n, out_winner, out_weight, out_cells);
  const SaBestFit fit{out_track};
  return sa_store_search_topn_impl(s, what, p, c != nullptr, c, n_queries, q_ids, q_n_obs, src, q_attrs, out_n, out_winner, out_weight, out_cells, &fit);
}

int sa_store_devrows_last(sa_store* s, sa_devrows_stats* out) {
  if (!s || !out) return SA_ERR_BAD_ARG;
  *out = s->devrows_last;
  out->struct_size = sizeof *out;
  out->reserved = 0;
  return SA_OK;
}

}  // extern "C"
