// sa_pose.hip — keypoint association (include/similari_pose.h): the poses of a call against the tracks of a point bank, the M x T weight
// matrix and the vote over it, in three launches whatever M, T and P are.
//
// The arithmetic is sa_pose.h over sa_kalman_point.h, shared with the host build of tests/emu_pose; the assignment is sa_dense.h, shared
// with tests/emu.  What is here: the call and its refusals, and three kernels.
//
//   k_pose_factor    one thread per (track j of the call, point p), t = j * P + p like k_points, so the five plane reads of a wave are
//                    consecutive 16-byte pieces: slot table -> has byte -> state -> sa_pkf_factor.  The factor goes out POINT-MAJOR, at
//                    [p * T + j]: one 16-byte piece (mean x, y, l00, l10) and one f32 (l11; NaN: no state or a failed pivot), so that a
//                    wave of the tile kernel, whose lanes are consecutive tracks, reads consecutive memory for each point.  The first
//                    M threads arm the rows' 64-bit bid words to 0.
//   k_pose_tile<SRC> 256 threads, one tile of 16 poses x 64 tracks: lane = track, wave w owns pose rows 4 w .. 4 w + 3 (the shape of
//                    positional_tile, sa_frame.h).  The tile's pose points are staged in LDS, (x, y) as one 8-byte piece with x = NaN for
//                    an absent point, at most 64 points at a time: 8 KiB whatever P is.  Every read of them is a broadcast — all lanes
//                    of a wave read the address of (row, point) — so no bank is asked for two addresses.  Each thread walks p ascending
//                    and keeps (sum, k) of its four cells in registers; per cell it writes the gain (i64, 0 = no usable edge) and,
//                    for the tap only, w; per row the wave's heaviest (gain, lowest column) goes into the row's word by ONE 64-bit
//                    atomic maximum at agent scope.
//   k_pose_assign<SRC> one workgroup of 256 threads, the scheme at the top of sa_tail.h with the whole scene as one component: greedy
//                    start from the words (u = -(heaviest gain); a column goes to the lowest row that bids for it: LDS atomic minimum),
//                    the rows that lost their bid compacted in ascending order by wave 0, sa_assign_component_dense<256, 8, false> (the
//                    64-bit variant: gains reach 1e8), then per pose the matched column and w of that cell, which the row's thread
//                    computes again from the factor and the pose with the tile's own functions: the f32 matrix is only written for
//                    the tap.  u, the matches, pred and the roots live in LDS: 48 KiB + 68 B.
//
// Bounds.  M, T <= SA_POSE_MAX = 2048 (checked by the call): every LDS table has SA_POSE_MAX entries, a bid word's column fits 16 bits,
// T <= NT * CPT.  Plane reads: slot < cap (the bank's table), p < P.  Pose reads: index[i] < n_rows of a span inside one registered
// block (check_rows) or i < M of the staged rows; mask at i * P + p < M * P.  Matrix accesses: i < M and j < T, leading dimension T.
//
// Reference: src/utils/kalman/kalman_2d_point_vec.rs (distance, calculate_cost), src/trackers/sort/voting.rs (SortVoting::winners).
#include "sa_points_impl.h"
#include "sa_pose.h"
#include "sa_dense.h"
#include "sa_widen.h"

#include <cstring>

namespace {

using namespace sa_pt;

constexpr uint32_t PF_THREADS = 256;
constexpr uint32_t TILE_M = 16, TILE_T = 64, TILE_THREADS = 256, TILE_CHUNK = 64, TILE_ROWS = TILE_M / (TILE_THREADS / 64);
constexpr int AS_NT = 256, AS_CPT = 8;
static_assert((uint32_t)AS_NT * AS_CPT >= SA_POSE_MAX, "every column needs an owner");
static_assert(SA_POSE_MAX <= 0xffffu, "a bid word keeps the column in 16 bits");

struct PoseArgs {
  uint32_t M, T, P, comps, min_common;
  float pw, min_score;
  int64_t threshold_q;
  const uint32_t* slots;     // [T] the slot of each track of the call; nullptr: 0, 1, 2, ...
  const char* base;          // the poses: row r at base + r * row_stride elements
  uint64_t row_stride;
  const uint32_t* index;     // [M] the row of each pose, SA_ROW_NONE: every point absent; nullptr: 0, 1, 2, ...
  const uint8_t* mask;       // [M][P] or nullptr
  const float4* plane[5];
  const uint8_t* has;
  float4* fac4;              // [P][T] mean x, y, l00, l10
  float* fac1;               // [P][T] l11, NaN = no factor
  int64_t* gain;             // [M][T]
  float* tap;                // [M][T] or nullptr
  unsigned long long* best;  // [M] the rows' bid words
  int32_t* out_col;          // [M] the matched column or -1
  float* out_w;              // [M] w of the matched cell, NaN
  uint32_t* out_roots;       // [1]
};

__global__ __launch_bounds__(PF_THREADS) void k_pose_factor(const PoseArgs a) {
  const uint32_t t = blockIdx.x * PF_THREADS + threadIdx.x;
  if (t < a.M) a.best[t] = 0ull;
  if (t >= a.T * a.P) return;   // (T * P < 2^31: the bank's own limit)
  const uint32_t j = t / a.P, p = t - j * a.P;
  const uint32_t slot = a.slots ? a.slots[j] : j;
  const size_t at = (size_t)slot * a.P + p;
  sa_pkf_fac f{0.f, 0.f, 0.f, 0.f, 0.f};
  bool ok = a.has[at] != 0;
  if (ok) {
    sa_pkf s;
    const float4 m = a.plane[0][at];
    s.mean[0] = m.x; s.mean[1] = m.y; s.mean[2] = m.z; s.mean[3] = m.w;
    for (int r = 0; r < 4; ++r) {
      const float4 c = a.plane[1 + r][at];
      s.cov[r * 4] = c.x; s.cov[r * 4 + 1] = c.y; s.cov[r * 4 + 2] = c.z; s.cov[r * 4 + 3] = c.w;
    }
    ok = sa_pkf_factor(a.pw, s, f);
  }
  const size_t o = (size_t)p * a.T + j;
  a.fac4[o] = make_float4(f.mx, f.my, f.l00, f.l10);
  a.fac1[o] = ok ? f.l11 : NAN;   // (a factor's l11 is the root of a positive number: never NaN)
}

// point p of pose i as the cell functions take it: x = NaN for an absent one
template <int SRC>
__device__ __forceinline__ float2 pose_point(const PoseArgs& a, uint32_t i, uint32_t p) {
  const uint32_t r = a.index ? a.index[i] : i;
  if (r == SA_ROW_NONE) return make_float2(NAN, 0.f);
  const char* row = a.base + (size_t)r * a.row_stride * (SRC == SA_ELEM_F32 ? 4u : 2u);
  const uint32_t k = p * a.comps;
  const float zx = load_elem<SRC>(row, k);
  const float zy = load_elem<SRC>(row, k + 1u);
  const float score = a.comps == 3u ? load_elem<SRC>(row, k + 2u) : 0.f;
  const bool present = sa_point_present(zx, zy, a.comps == 3u, score, a.min_score, !a.mask || a.mask[(size_t)i * a.P + p] != 0);
  return present ? make_float2(zx, zy) : make_float2(NAN, 0.f);
}
__device__ __forceinline__ bool pose_factor_at(const PoseArgs& a, uint32_t p, uint32_t j, sa_pkf_fac& f) {
  const size_t o = (size_t)p * a.T + j;
  const float4 q = a.fac4[o];
  f.mx = q.x; f.my = q.y; f.l00 = q.z; f.l10 = q.w;
  f.l11 = a.fac1[o];
  return f.l11 == f.l11;
}

template <int SRC>
__global__ __launch_bounds__(TILE_THREADS) void k_pose_tile(const PoseArgs a) {
  __shared__ float2 s_z[TILE_M][TILE_CHUNK];
  const uint32_t i0 = blockIdx.y * TILE_M, j0 = blockIdx.x * TILE_T;
  if (i0 >= a.M || j0 >= a.T) return;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t j = j0 + lane;
  const bool col = j < a.T;
  float sum[TILE_ROWS];
  uint32_t k[TILE_ROWS];
#pragma unroll
  for (uint32_t r = 0; r < TILE_ROWS; ++r) { sum[r] = 0.f; k[r] = 0u; }
  for (uint32_t p0 = 0; p0 < a.P; p0 += TILE_CHUNK) {
    const uint32_t cn = a.P - p0 < TILE_CHUNK ? a.P - p0 : TILE_CHUNK;
    if (p0) __syncthreads();   // the chunk before has been read
    for (uint32_t e = tid; e < TILE_M * cn; e += TILE_THREADS) {
      const uint32_t r = e / cn, pp = e - r * cn;
      s_z[r][pp] = i0 + r < a.M ? pose_point<SRC>(a, i0 + r, p0 + pp) : make_float2(NAN, 0.f);
    }
    __syncthreads();
    for (uint32_t pp = 0; pp < cn; ++pp) {
      sa_pkf_fac f{0.f, 0.f, 0.f, 0.f, 0.f};
      const bool ok = col && pose_factor_at(a, p0 + pp, j, f);
#pragma unroll
      for (uint32_t r = 0; r < TILE_ROWS; ++r) {
        const float2 z = s_z[wave * TILE_ROWS + r][pp];
        sa_pose_acc(sum[r], k[r], ok, f, z.x == z.x, z.x, z.y);
      }
    }
  }
#pragma unroll
  for (uint32_t r = 0; r < TILE_ROWS; ++r) {
    const uint32_t i = i0 + wave * TILE_ROWS + r;
    if (i >= a.M) break;   // (wave-uniform)
    const float w = sa_pose_weight(sum[r], k[r], a.min_common);
    const int64_t g = col ? sa_pose_gain(w, a.threshold_q) : 0;
    if (col) {
      const size_t at = (size_t)i * a.T + j;
      a.gain[at] = g;
      if (a.tap) a.tap[at] = w;
    }
    unsigned long long word = g > 0 ? sa_pose_word(g, j) : 0ull;
#pragma unroll
    for (int o = 32; o; o >>= 1) {
      const unsigned long long other = __shfl_xor(word, o);
      word = other > word ? other : word;
    }
    if (lane == 0 && word) __hip_atomic_fetch_max(a.best + i, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <int SRC>
__global__ __launch_bounds__(AS_NT) void k_pose_assign(const PoseArgs a) {
  __shared__ int64_t s_u[SA_POSE_MAX];
  __shared__ int32_t s_rmatch[SA_POSE_MAX], s_cmatch[SA_POSE_MAX], s_pred[SA_POSE_MAX];
  __shared__ uint32_t s_roots[SA_POSE_MAX];
  __shared__ unsigned long long s_part[2 * AS_NT / 64];
  __shared__ uint32_t s_n;
  const uint32_t q = threadIdx.x, lane = q & 63u;
  const uint32_t M = a.M, T = a.T;
  for (uint32_t j = q; j < T; j += AS_NT) s_cmatch[j] = -1;   // (as u32: above every row)
  __syncthreads();
  // greedy start: every row bids for the column of its heaviest gain, a column goes to the lowest row that bids for it
  for (uint32_t i = q; i < M; i += AS_NT) {
    const unsigned long long word = a.best[i];
    s_u[i] = -sa_pose_word_gain(word);
    const int32_t bc = word ? (int32_t)sa_pose_word_col(word) : -1;
    s_rmatch[i] = bc;
    if (bc >= 0) atomicMin((uint32_t*)&s_cmatch[bc], i);
  }
  __syncthreads();
  if (q < 64) {  // the rows that lost their bid are the search roots, ascending
    uint32_t n = 0;
    for (uint32_t i0 = 0; i0 < M; i0 += 64) {
      const uint32_t i = i0 + lane;
      bool pend = false;
      if (i < M) {
        const int32_t bc = s_rmatch[i];
        if (bc >= 0 && s_cmatch[bc] != (int32_t)i) {
          pend = true;
          s_rmatch[i] = -1;
        }
      }
      const unsigned long long m = __ballot(pend);
      if (pend) s_roots[n + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
      n += (uint32_t)__popcll(m);
    }
    if (lane == 0) s_n = n;
  }
  __syncthreads();
  const uint32_t n_roots = s_n;
  sa_dense_ws w;
  w.gain = a.gain; w.ld = T; w.T = T;
  w.u = s_u; w.rmatch = s_rmatch; w.cmatch = s_cmatch; w.pred = s_pred; w.part = s_part;
  sa_assign_component_dense<AS_NT, AS_CPT, false>(w, s_roots, n_roots);
  __syncthreads();
  // results: the matched column, and w of that cell by the tile's own arithmetic
  for (uint32_t i = q; i < M; i += AS_NT) {
    const int32_t c = s_rmatch[i];
    float wv = NAN;
    if (c >= 0) {
      float sum = 0.f;
      uint32_t k = 0;
      for (uint32_t p = 0; p < a.P; ++p) {
        sa_pkf_fac f;
        const bool ok = pose_factor_at(a, p, (uint32_t)c, f);
        const float2 z = pose_point<SRC>(a, i, p);
        sa_pose_acc(sum, k, ok, f, z.x == z.x, z.x, z.y);
      }
      wv = sa_pose_weight(sum, k, a.min_common);
    }
    a.out_col[i] = c;
    a.out_w[i] = wv;
  }
  if (q == 0) a.out_roots[0] = n_roots;
}

hipError_t launch(const PoseArgs& a, int32_t elem, hipStream_t st, hipEvent_t* ev) {
  const uint64_t cells = (uint64_t)a.T * a.P;
  const uint32_t fb = (uint32_t)(((cells > a.M ? cells : a.M) + PF_THREADS - 1) / PF_THREADS);
  const dim3 tiles((a.T + TILE_T - 1) / TILE_T, (a.M + TILE_M - 1) / TILE_M);
  hipError_t h;
  if ((h = hipEventRecord(ev[0], st)) != hipSuccess) return h;
  hipLaunchKernelGGL(k_pose_factor, dim3(fb), dim3(PF_THREADS), 0, st, a);
  if ((h = hipGetLastError()) != hipSuccess) return h;
  if ((h = hipEventRecord(ev[1], st)) != hipSuccess) return h;
  if (elem == SA_ELEM_F16) hipLaunchKernelGGL(k_pose_tile<SA_ELEM_F16>, tiles, dim3(TILE_THREADS), 0, st, a);
  else if (elem == SA_ELEM_BF16) hipLaunchKernelGGL(k_pose_tile<SA_ELEM_BF16>, tiles, dim3(TILE_THREADS), 0, st, a);
  else hipLaunchKernelGGL(k_pose_tile<SA_ELEM_F32>, tiles, dim3(TILE_THREADS), 0, st, a);
  if ((h = hipGetLastError()) != hipSuccess) return h;
  if ((h = hipEventRecord(ev[2], st)) != hipSuccess) return h;
  if (elem == SA_ELEM_F16) hipLaunchKernelGGL(k_pose_assign<SA_ELEM_F16>, dim3(1), dim3(AS_NT), 0, st, a);
  else if (elem == SA_ELEM_BF16) hipLaunchKernelGGL(k_pose_assign<SA_ELEM_BF16>, dim3(1), dim3(AS_NT), 0, st, a);
  else hipLaunchKernelGGL(k_pose_assign<SA_ELEM_F32>, dim3(1), dim3(AS_NT), 0, st, a);
  if ((h = hipGetLastError()) != hipSuccess) return h;
  return hipEventRecord(ev[3], st);
}

// Everything behind the refusals: the uploads, the three launches, the copies out, the wait, the stats.  slots: [n] or empty (0, 1, ...).
int run(sa_points* b, uint32_t n, const std::vector<uint32_t>& slots, const uint64_t* track_ids, uint32_t m, const sa_point_rows* rows,
        const sa_pose_options* o, uint64_t* out_track, float* out_weight, float* out_matrix) {
  sa_engine* e = b->e;
  hipStream_t st = b->st;
  for (auto& ev : b->pev)
    if (!ev) SA_HIPCHK(e, hipEventCreate(&ev));
  const uint64_t mp = (uint64_t)m * b->P, np = (uint64_t)n * b->P, cells = (uint64_t)m * n;
  sa_pose_stats s{};
  PoseArgs a{};
  a.M = m, a.T = n, a.P = b->P, a.comps = rows->comps, a.min_common = o->min_common;
  a.pw = b->pw, a.min_score = rows->min_score;
  a.threshold_q = sa_pose_threshold_q(o->threshold);
  int32_t elem = SA_ELEM_F32;
  if (!slots.empty()) {
    SA_TRY(sa_engine_ensure(e, b->d_slots, (size_t)n * 4));
    SA_HIPCHK(e, hipMemcpyAsync(b->d_slots.p, slots.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    s.bytes_h2d += (uint64_t)n * 4;
    a.slots = (const uint32_t*)b->d_slots.p;
  }
  if (rows->host) {
    const size_t bytes = (size_t)mp * rows->comps * 4;
    SA_TRY(sa_engine_ensure(e, b->d_pts, bytes));
    SA_HIPCHK(e, hipMemcpyAsync(b->d_pts.p, rows->host, bytes, hipMemcpyHostToDevice, st));
    s.bytes_h2d += bytes;
    a.base = (const char*)b->d_pts.p;
    a.row_stride = (uint64_t)b->P * rows->comps;
  } else {
    const sa_dev_rows* d = rows->dev;
    elem = d->elem;
    a.base = (const char*)d->base;
    a.row_stride = d->row_stride;
    uint64_t read = m;
    if (d->index) {
      SA_TRY(sa_engine_ensure(e, b->d_index, (size_t)m * 4));
      SA_HIPCHK(e, hipMemcpyAsync(b->d_index.p, d->index, (size_t)m * 4, hipMemcpyHostToDevice, st));
      s.bytes_h2d += (uint64_t)m * 4;
      a.index = (const uint32_t*)b->d_index.p;
      read = (uint64_t)(m - std::count(d->index, d->index + m, SA_ROW_NONE));
    }
    s.src_bytes = read * b->P * rows->comps * elem_size(elem);
  }
  if (rows->present) {
    SA_TRY(sa_engine_ensure(e, b->d_mask, (size_t)mp));
    SA_HIPCHK(e, hipMemcpyAsync(b->d_mask.p, rows->present, (size_t)mp, hipMemcpyHostToDevice, st));
    s.bytes_h2d += mp;
    a.mask = (const uint8_t*)b->d_mask.p;
  }
  SA_TRY(sa_engine_ensure(e, b->d_fac4, (size_t)np * 16));
  SA_TRY(sa_engine_ensure(e, b->d_fac1, (size_t)np * 4));
  SA_TRY(sa_engine_ensure(e, b->d_gain, (size_t)cells * 8));
  SA_TRY(sa_engine_ensure(e, b->d_best, (size_t)m * 8));
  SA_TRY(sa_engine_ensure(e, b->d_res, (size_t)m * 8 + 4));
  if (out_matrix) {
    SA_TRY(sa_engine_ensure(e, b->d_tap, (size_t)cells * 4));
    a.tap = (float*)b->d_tap.p;
  }
  for (int k = 0; k < 5; ++k) a.plane[k] = (const float4*)b->plane[k].p;
  a.has = (const uint8_t*)b->has.p;
  a.fac4 = (float4*)b->d_fac4.p, a.fac1 = (float*)b->d_fac1.p, a.gain = (int64_t*)b->d_gain.p, a.best = (unsigned long long*)b->d_best.p;
  a.out_col = (int32_t*)b->d_res.p, a.out_w = (float*)b->d_res.p + m, a.out_roots = (uint32_t*)b->d_res.p + 2 * (size_t)m;
  SA_HIPCHK(e, launch(a, elem, st, b->pev));
  std::vector<uint32_t> res((size_t)m * 2 + 1);
  SA_HIPCHK(e, hipMemcpyAsync(res.data(), b->d_res.p, res.size() * 4, hipMemcpyDeviceToHost, st));
  s.bytes_d2h += res.size() * 4;
  if (out_matrix) {
    SA_HIPCHK(e, hipMemcpyAsync(out_matrix, b->d_tap.p, (size_t)cells * 4, hipMemcpyDeviceToHost, st));
    s.bytes_d2h += cells * 4;
  }
  SA_HIPCHK(e, hipStreamSynchronize(st));
  float ms = 0.f;
  SA_HIPCHK(e, hipEventElapsedTime(&ms, b->pev[0], b->pev[3]));
  s.device_ms = ms;
  for (int k = 0; k < 3; ++k) {
    SA_HIPCHK(e, hipEventElapsedTime(&ms, b->pev[k], b->pev[k + 1]));
    s.kernel_ms[k] = ms;
  }
  for (uint32_t i = 0; i < m; ++i) {
    const int32_t c = (int32_t)res[i];
    const bool hit = c >= 0 && (uint32_t)c < n;
    out_track[i] = hit ? (track_ids ? track_ids[c] : b->ids[c]) : 0;
    std::memcpy(out_weight + i, &res[(size_t)m + i], 4);
    s.matched += hit;
  }
  s.poses = m, s.tracks = n, s.launches = 3, s.roots = res[(size_t)m * 2];
  b->last_pose = s;
  return SA_OK;
}

}  // namespace

extern "C" {

void sa_pose_options_default(sa_pose_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->struct_size = sizeof *o;
  o->min_common = 1;
  o->threshold = 1.0f;
}

int sa_points_associate(sa_points* b, uint32_t n_tracks, const uint64_t* track_ids, uint32_t m, const sa_point_rows* poses,
                        const sa_pose_options* o, uint64_t* out_track, float* out_weight, float* out_matrix) {
  const char* what = "sa_points_associate";
  if (!b) return SA_ERR_BAD_ARG;
  SA_TRY(enter(b, what));
  b->last_pose = sa_pose_stats{};
  sa_engine* e = b->e;
  if (!o) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null options", what);
  if (o->struct_size != sizeof(sa_pose_options)) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: options.struct_size %u (%zu)", what, o->struct_size, sizeof(sa_pose_options));
  if (o->min_common == 0) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: min_common must be >= 1", what);
  if (!sa_point_finite(o->threshold) || o->threshold < 0.0f) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: threshold %g must be finite and >= 0", what, (double)o->threshold);
  if (m == 0) return SA_OK;
  if (!out_track || !out_weight) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
  SA_TRY(check_rows(b, what, m, poses));
  const uint32_t n = track_ids ? n_tracks : b->T;
  std::vector<uint32_t> slots;
  if (track_ids) SA_TRY(check_ids(b, what, n, track_ids, true, slots));
  if (m > SA_POSE_MAX || n > SA_POSE_MAX)
    return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: %u poses x %u tracks; one call takes at most %u of either", what, m, n, SA_POSE_MAX);
  if (n == 0) {
    for (uint32_t i = 0; i < m; ++i) { out_track[i] = 0; out_weight[i] = NAN; }
    b->last_pose.poses = m;
    return SA_OK;
  }
  return run(b, n, slots, track_ids, m, poses, o, out_track, out_weight, out_matrix);
}

int sa_points_associate_last(sa_points* b, sa_pose_stats* out) {
  if (!b || !out) return SA_ERR_BAD_ARG;
  *out = b->last_pose;
  out->struct_size = sizeof *out;
  return SA_OK;
}

}  // extern "C"
