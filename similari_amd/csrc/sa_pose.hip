// sa_pose.hip — keypoint association (include/similari_pose.h): the poses of a call against the tracks of a point bank, the M x T weight
// matrix and the vote over it, in three launches whatever M, T and P are; and the same for a batch of scenes
// (include/similari_pose_batch.h): S independent matrices and votes, still in three launches.
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
// Scenes.  Every call is a plan of scenes (sa_pose_plan.h).  The cell loop (pose_tile) and the assignment (pose_assign) take a PoseView:
// a scene's M and T, its first column in the call's factor and the factor's leading dimension, its gains and tap, its first pose.
// k_pose_tile is a 1-D grid over the tiles of all scenes, the scene found by bisection in the tile prefix of the segment table;
// k_pose_assign is one workgroup per scene.  A batch uploads the table; the single calls are the plan of ONE scene, which travels by value
// in the kernel arguments (PoseArgs::one, pose_seg): no table, and the grid is the tiles of the matrix, row-major.  k_pose_factor works
// on the call: T = the sum of the scenes' tracks, the slot table their concatenation, M = the sum of the poses.  The host: an entry point
// describes its call in a PoseCall, run() / track_call() do what it says, a PoseRan (sa_points_impl.h) records what ran.  The poses themselves — the check of their
// descriptor, the staging of host rows, index and mask, the read of one point under the presence rule (sa_point_at<SRC>), the walk of
// a pose's extent and the choice of the SRC instance — are sa_point_rows.h, shared with sa_points.hip and sa_pose_nms.hip.
//
// The frame loop (include/similari_pose_track.h): sa_points_track / sa_points_track_batch run the same three launches with TRACK set —
// the factor also arms one word per track, the assignment also leaves who took each track, each unmatched pose's rank in its scene and
// the scene's count —, then k_pose_scan (a call with a table: the exclusive prefix of the counts, one workgroup) and k_pose_step (one thread per
// (pose or listed track, point): step, create, coast), and come back with ONE copy and ONE wait.  The existing calls instantiate
// TRACK = false: their kernels are what they were.  The host's part of it is sa_pose_track_plan.h.
//
// The keypoint tracker (include/similari_pose_sort.h, sa_pose_sort.hip): sort_track / sort_peek run the frame loop and the vote on tracks
// named by slot.  When the call has a finite limit, k_pose_circles — ONE launch, one thread per pose and per listed track — writes the
// circles of sa_pose_gate.h and the tile runs its GATE instantiation, where a refused cell's w is NaN before the gain; otherwise the
// launches are those above and the GATE = false tiles are what they were.
//
// The OKS metric (include/similari_pose_oks.h, arithmetic in sa_pose_oks.h): a bank whose metric is OKS runs the OKS instantiations of
// the four kernels of a vote — k_pose_circles also writes each item's area and runs in front of EVERY vote (one launch, shared with the
// gate when the call has limits), k_pose_factor reads the mean plane alone, the tile and the assignment call sa_oks_acc with the cell's
// scale.  The OKS = false instantiations are what they were; a bank on the Mahalanobis metric launches nothing else.
//
// Bounds.  A scene's poses are [pose0, pose0 + m) of the call's M, its columns [track0, track0 + n) of the call's T, its cells
// [cell0, cell0 + m * n) of the call's gains — back to back by the plan, so what holds for a scene's own i < m and j < n holds in the
// call's arrays; a block of the tile launch lands in a scene that has tiles because the grid is the plan's tile total; the table has S
// entries and the assignment's grid is S; with S == 1 and no table neither kernel reads one.  Per scene:
// M, T <= SA_POSE_MAX = 2048 (checked by the call): every LDS table has SA_POSE_MAX entries, a bid word's column fits 16 bits,
// T <= NT * CPT.  Plane reads: slot < cap (the bank's table), p < P.  Pose reads: item i < M of the call's SaPointSrc
// (sa_point_rows.h states the row and the mask byte it reads, and what the host checked of them).  Matrix accesses: i < M and j < T, leading dimension T.
//
// Reference: src/utils/kalman/kalman_2d_point_vec.rs (distance, calculate_cost), src/trackers/sort/voting.rs (SortVoting::winners).
#include "sa_points_impl.h"
#include "sa_pose.h"
#include "sa_pose_gate.h"
#include "sa_pose_oks.h"
#include "sa_pose_plan.h"
#include "sa_pose_track_plan.h"
#include "sa_dense.h"

#include <cstring>

namespace {

using namespace sa_pt;

constexpr uint32_t PF_THREADS = 256;
constexpr uint32_t TILE_M = 16, TILE_T = 64, TILE_THREADS = 256, TILE_CHUNK = 64, TILE_ROWS = TILE_M / (TILE_THREADS / 64);
constexpr int AS_NT = 256, AS_CPT = 8;
static_assert((uint32_t)AS_NT * AS_CPT >= SA_POSE_MAX, "every column needs an owner");
static_assert(SA_POSE_MAX <= 0xffffu, "a bid word keeps the column in 16 bits");

struct PoseArgs {
  uint32_t M, T, P, min_common;
  float pw;
  int64_t threshold_q;
  const uint32_t* slots;     // [T] the slot of each track of the call; nullptr: 0, 1, 2, ...
  SaPointSrc src;            // the points of the M poses (sa_point_rows.h)
  const float4* plane[5];
  const uint8_t* has;
  float4* fac4;              // [P][T] mean x, y, l00, l10
  float* fac1;               // [P][T] l11, NaN = no factor
  int64_t* gain;             // [M][T]
  float* tap;                // [M][T] or nullptr
  unsigned long long* best;  // [M] the rows' bid words
  int32_t* out_col;          // [M] the matched column or -1
  float* out_w;              // [M] w of the matched cell, NaN
  uint32_t* out_roots;       // [1]; a batch: [S]
  const SaPoseSeg* segs;     // a batch: the S scenes of the call (sa_pose_plan.h); M and T are then the sums over them
  uint32_t S;
  SaPoseSeg one;             // segs == nullptr, the single calls: S == 1 and this is the scene, the whole call, no table is uploaded
  // sa_points_track (the TRACK instantiations only): what the assignment leaves for k_pose_step
  uint32_t* col_row;         // [T] the pose that took the track, POSE_NOBODY: none
  uint32_t* rank;            // [M] an unmatched pose's place among the unmatched poses of its scene
  uint32_t* unmatched;       // [1]; a batch: [S] the unmatched poses of each scene
  uint32_t* scene_base;      // a batch: [S] the exclusive prefix of `unmatched` (k_pose_scan)
  // the keypoint tracker's gated vote (k_pose_circles and the GATE instantiations of the tile only; nullptr otherwise)
  float4* circ;              // [M + T] (xc, yc, r, 1 or 0 = no circle) of the M poses, then of the T tracks of the call
  const float* limit;        // [T] the limit of each track (sa_pose_gate.h), +inf: none
  // the OKS metric (sa_pose_oks.h; the OKS instantiations only; nullptr otherwise)
  const float* var2;         // [P] the per-point constants
  float* area;               // [M + T] the areas of the extents, beside circ; NaN: the item has no point
};
constexpr uint32_t POSE_NOBODY = 0xffffffffu;

// What the cell loop and the assignment see of a call: one scene.  It lies at column col0 of the call's factor and at pose pose0 of
// the call's rows, mask, bid words and results, and has gains and a tap of its own with leading dimension T; the single call's one scene
// lies at 0 of everything.  Columns are LOCAL everywhere: in the bid words, in the LDS tables, in out_col.
struct PoseView {
  uint32_t M, T;        // the scene's poses and tracks
  uint32_t col0, ldf;   // its first column in the factor, the factor's leading dimension (the tracks of the call)
  uint32_t pose0;       // its first pose
  int64_t* gain;        // [M][T]
  float* tap;           // [M][T] or nullptr
};
__device__ __forceinline__ PoseView pose_scene(const PoseArgs& a, const SaPoseSeg& g) {
  return PoseView{g.m, g.n, g.track0, a.T, g.pose0, a.gain + g.cell0, a.tap ? a.tap + g.cell0 : nullptr};
}
// scene s < S of the call: a batch reads its table, the single calls carry theirs in the kernel arguments (block-uniform either way)
__device__ __forceinline__ SaPoseSeg pose_seg(const PoseArgs& a, uint32_t s) { return a.segs ? a.segs[s] : a.one; }
// The last scene whose `key` (tile0, pose0: ascending, 0 in scene 0) is not beyond x: scenes that have none of the counted thing share
// their key with the next that has some, and the last of an equal run is that one.  At most 16 steps; with S == 1 the table is not read.
__device__ __forceinline__ uint32_t pose_seg_at(const PoseArgs& a, uint32_t SaPoseSeg::*key, uint32_t x) {
  uint32_t lo = 0, hi = a.S;   // segs[lo].key <= x; hi == S or segs[hi].key > x
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.segs[mid].*key <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// OKS: no factor is needed — the mean plane alone is read, (x, y) go where the tile expects the factor's, and fac1 holds 0 for "has a
// state", NaN otherwise.
template <bool TRACK, bool OKS>
__global__ __launch_bounds__(PF_THREADS) void k_pose_factor(const PoseArgs a) {
  const uint32_t t = blockIdx.x * PF_THREADS + threadIdx.x;
  if (t < a.M) a.best[t] = 0ull;
  if (TRACK && t < a.T) a.col_row[t] = POSE_NOBODY;   // (the grid covers T * P >= T threads)
  if (t >= a.T * a.P) return;   // (T * P < 2^31: the bank's own limit)
  const uint32_t j = t / a.P, p = t - j * a.P;
  const uint32_t slot = a.slots ? a.slots[j] : j;
  const size_t at = (size_t)slot * a.P + p;
  sa_pkf_fac f{0.f, 0.f, 0.f, 0.f, 0.f};
  bool ok = a.has[at] != 0;
  if (OKS) {
    if (ok) {
      const float4 m = a.plane[0][at];
      f.mx = m.x, f.my = m.y;
    }
  } else if (ok) {
    sa_pkf s;
    pt_load(a, at, s);
    ok = sa_pkf_factor(a.pw, s, f);
  }
  const size_t o = (size_t)p * a.T + j;
  a.fac4[o] = make_float4(f.mx, f.my, f.l00, f.l10);
  a.fac1[o] = ok ? f.l11 : NAN;   // (a factor's l11 is the root of a positive number: never NaN)
}

// (point p of pose i as the cell functions take it, x = NaN for an absent one: sa_point_at<SRC>(a.src, i, a.P, p), sa_point_rows.h)
__device__ __forceinline__ bool pose_factor_at(const PoseArgs& a, const PoseView& v, uint32_t p, uint32_t j, sa_pkf_fac& f) {
  const size_t o = (size_t)p * v.ldf + v.col0 + j;
  const float4 q = a.fac4[o];
  f.mx = q.x; f.my = q.y; f.l00 = q.z; f.l10 = q.w;
  f.l11 = a.fac1[o];
  return f.l11 == f.l11;
}

// The gate's circles (sa_pose_gate.h), ONE launch: one thread per item t < M + T, the M poses then the T listed tracks, each walking its
// P points.  A pose's points that count are the present ones (sa_pose_extent<SRC>, the tile's own rule); a track's are the stored means of
// its points that have a state — the vote matches stored states, not predicted ones.  Reads: as the tile and k_pose_factor (slot < cap,
// p < P); writes circ[t], t < M + T.
// OKS: the same walk also leaves the area of each item's rectangle in area[t], t < M + T (sa_pose_oks.h) — the one launch serves the gate
// and the metric.  The tile reads area[pose0 + i], i < the scene's M, and area[M + col0 + j], j < the scene's T; var2[p], p < P.
template <int SRC, bool OKS>
__global__ __launch_bounds__(PF_THREADS) void k_pose_circles(const PoseArgs a) {
  const uint32_t t = blockIdx.x * PF_THREADS + threadIdx.x;
  if (t >= a.M + a.T) return;
  sa_pose_rect q;
  sa_pose_rect_clear(q);
  if (t < a.M) sa_pose_extent<SRC>(a.src, t, a.P, q);
  else {
    const uint32_t j = t - a.M;
    const size_t at = (size_t)(a.slots ? a.slots[j] : j) * a.P;
    for (uint32_t p = 0; p < a.P; ++p)
      if (a.has[at + p] != 0) {
        const float4 m = a.plane[0][at + p];
        sa_pose_rect_add(q, m.x, m.y);
      }
  }
  sa_geo c;
  const bool ok = sa_pose_circle(q, c);
  a.circ[t] = make_float4(c.xc, c.yc, c.r, ok ? 1.f : 0.f);
  if (OKS) a.area[t] = sa_oks_area(q);
}

// the tile (i0, j0) of scene v: i0 < v.M, j0 < v.T
// GATE (the keypoint tracker with a finite limit in the call): a lane also holds its track's circle and limit, a row's circle is read as
// a broadcast (one address per wave), and a refused cell (sa_pose_refused) has w = NaN before the gain: it has no tap value, no gain and
// never bids.
// OKS (sa_pose_oks.h): a lane also holds its track's area, the areas of the wave's rows are read as broadcasts IN FRONT of the point loop
// — the scale s2 of a cell divides inside it, point by point —, var2[p] is a wave-uniform read, and a cell refused by its scale has
// w = NaN before the gain, like one refused by the gate.
template <int SRC, bool GATE, bool OKS>
__device__ __forceinline__ void pose_tile(const PoseArgs& a, const PoseView& v, uint32_t i0, uint32_t j0, float2 (*s_z)[TILE_CHUNK]) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t j = j0 + lane;
  const bool col = j < v.T;
  float sum[TILE_ROWS];
  uint32_t k[TILE_ROWS];
#pragma unroll
  for (uint32_t r = 0; r < TILE_ROWS; ++r) { sum[r] = 0.f; k[r] = 0u; }
  float4 tc = make_float4(0.f, 0.f, 0.f, 0.f);
  float lim = INFINITY;
  if (GATE && col) {
    tc = a.circ[a.M + v.col0 + j];
    lim = a.limit[v.col0 + j];
  }
  float s2[TILE_ROWS];
  if (OKS) {
    const float ta = col ? a.area[a.M + v.col0 + j] : NAN;
#pragma unroll
    for (uint32_t r = 0; r < TILE_ROWS; ++r) {
      const uint32_t i = i0 + wave * TILE_ROWS + r;
      s2[r] = sa_oks_scale(i < v.M ? a.area[v.pose0 + i] : NAN, ta);
    }
  }
  for (uint32_t p0 = 0; p0 < a.P; p0 += TILE_CHUNK) {
    const uint32_t cn = a.P - p0 < TILE_CHUNK ? a.P - p0 : TILE_CHUNK;
    if (p0) __syncthreads();   // the chunk before has been read
    for (uint32_t e = tid; e < TILE_M * cn; e += TILE_THREADS) {
      const uint32_t r = e / cn, pp = e - r * cn;
      s_z[r][pp] = i0 + r < v.M ? sa_point_at<SRC>(a.src, v.pose0 + i0 + r, a.P, p0 + pp) : make_float2(NAN, 0.f);
    }
    __syncthreads();
    for (uint32_t pp = 0; pp < cn; ++pp) {
      sa_pkf_fac f{0.f, 0.f, 0.f, 0.f, 0.f};
      const bool ok = col && pose_factor_at(a, v, p0 + pp, j, f);
      const float var2 = OKS ? a.var2[p0 + pp] : 0.f;
#pragma unroll
      for (uint32_t r = 0; r < TILE_ROWS; ++r) {
        const float2 z = s_z[wave * TILE_ROWS + r][pp];
        if (OKS) sa_oks_acc(sum[r], k[r], ok, f.mx, f.my, z.x == z.x, z.x, z.y, s2[r], var2);
        else sa_pose_acc(sum[r], k[r], ok, f, z.x == z.x, z.x, z.y);
      }
    }
  }
#pragma unroll
  for (uint32_t r = 0; r < TILE_ROWS; ++r) {
    const uint32_t i = i0 + wave * TILE_ROWS + r;
    if (i >= v.M) break;   // (wave-uniform)
    float w = sa_pose_weight(sum[r], k[r], a.min_common);
    if (OKS && sa_oks_refused(s2[r])) w = NAN;
    if (GATE && col) {
      const float4 pc = a.circ[v.pose0 + i];
      if (sa_pose_refused(pc.w != 0.f, sa_geo{pc.x, pc.y, pc.z, 0.f}, tc.w != 0.f, sa_geo{tc.x, tc.y, tc.z, 0.f}, lim)) w = NAN;
    }
    const int64_t g = col ? sa_pose_gain(w, a.threshold_q) : 0;
    if (col) {
      const size_t at = (size_t)i * v.T + j;
      v.gain[at] = g;
      if (v.tap) v.tap[at] = w;
    }
    unsigned long long word = g > 0 ? sa_pose_word(g, j) : 0ull;
#pragma unroll
    for (int o = 32; o; o >>= 1) {
      const unsigned long long other = __shfl_xor(word, o);
      word = other > word ? other : word;
    }
    if (lane == 0 && word) __hip_atomic_fetch_max(a.best + v.pose0 + i, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// A 1-D grid over the tiles of all scenes, scene after scene, a scene's tiles row-major.  The block finds its scene as the last one
// whose first tile is not beyond it (pose_seg_at: block-uniform, so the reads are scalar).  A grid dimension per scene would need
// max-over-scenes tiles in the other dimension and let every block of a smaller scene start only to leave: with one 2048 x 2048
// scene among 63 of 100 x 100 that is 64 x 4096 blocks for 4096 + 63 * 14 tiles of work.  The single call is the grid of its one scene.
template <int SRC, bool GATE, bool OKS>
__global__ __launch_bounds__(TILE_THREADS) void k_pose_tile(const PoseArgs a) {
  __shared__ float2 s_z[TILE_M][TILE_CHUNK];
  const SaPoseSeg g = pose_seg(a, pose_seg_at(a, &SaPoseSeg::tile0, blockIdx.x));
  if (g.tiles_x == 0u) return;   // (the plan gives no tile to such a scene: the grid has none that lands here)
  const uint32_t t = blockIdx.x - g.tile0, ty = t / g.tiles_x, tx = t - ty * g.tiles_x;
  const uint32_t i0 = ty * TILE_M, j0 = tx * TILE_T;
  if (i0 >= g.m || j0 >= g.n) return;
  pose_tile<SRC, GATE, OKS>(a, pose_scene(a, g), i0, j0, s_z);
}

// Wave 0 compacts the items i < n that `keep` in ascending order: put(i, at) for the at-th of them; every lane returns their number.
template <class Keep, class Put>
__device__ __forceinline__ uint32_t pose_compact(uint32_t n, uint32_t lane, Keep keep, Put put) {
  uint32_t kept = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += 64) {
    const uint32_t i = i0 + lane;
    const bool k = i < n && keep(i);
    const unsigned long long m = __ballot(k);
    if (k) put(i, kept + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)));
    kept += (uint32_t)__popcll(m);
  }
  return kept;
}

// the assignment of scene v by one workgroup -> its search roots (every thread returns them)
// TRACK (sa_points_track): it also leaves, for k_pose_step, the pose that took each track, each unmatched pose's rank among the scene's
// unmatched poses, and their number at unmatched[scene] — all from s_rmatch, the rows' side of the final matching.
// OKS: w of a matched cell is the OKS cell function's, with the cell's own scale; the match was a usable edge, so nothing refuses it.
template <int SRC, bool TRACK, bool OKS>
__device__ __forceinline__ uint32_t pose_assign(const PoseArgs& a, const PoseView& v, uint32_t scene) {
  __shared__ int64_t s_u[SA_POSE_MAX];
  __shared__ int32_t s_rmatch[SA_POSE_MAX], s_cmatch[SA_POSE_MAX], s_pred[SA_POSE_MAX];
  __shared__ uint32_t s_roots[SA_POSE_MAX];
  __shared__ unsigned long long s_part[2 * AS_NT / 64];
  __shared__ uint32_t s_n;
  const uint32_t q = threadIdx.x, lane = q & 63u;
  const uint32_t M = v.M, T = v.T;
  for (uint32_t j = q; j < T; j += AS_NT) s_cmatch[j] = -1;   // (as u32: above every row)
  __syncthreads();
  // greedy start: every row bids for the column of its heaviest gain, a column goes to the lowest row that bids for it
  for (uint32_t i = q; i < M; i += AS_NT) {
    const unsigned long long word = a.best[v.pose0 + i];
    s_u[i] = -sa_pose_word_gain(word);
    const int32_t bc = word ? (int32_t)sa_pose_word_col(word) : -1;
    s_rmatch[i] = bc;
    if (bc >= 0) atomicMin((uint32_t*)&s_cmatch[bc], i);
  }
  __syncthreads();
  if (q < 64) {  // the rows that lost their bid are the search roots, ascending
    const auto lost = [&](uint32_t i) {
      const int32_t bc = s_rmatch[i];
      const bool pend = bc >= 0 && s_cmatch[bc] != (int32_t)i;
      if (pend) s_rmatch[i] = -1;
      return pend;
    };
    const uint32_t n = pose_compact(M, lane, lost, [&](uint32_t i, uint32_t at) { s_roots[at] = i; });
    if (lane == 0) s_n = n;
  }
  __syncthreads();
  const uint32_t n_roots = s_n;
  sa_dense_ws w;
  w.gain = v.gain; w.ld = T; w.T = T;
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
      const float s2 = OKS ? sa_oks_scale(a.area[v.pose0 + i], a.area[a.M + v.col0 + (uint32_t)c]) : 0.f;
      for (uint32_t p = 0; p < a.P; ++p) {
        sa_pkf_fac f;
        const bool ok = pose_factor_at(a, v, p, (uint32_t)c, f);
        const float2 z = sa_point_at<SRC>(a.src, v.pose0 + i, a.P, p);
        if (OKS) sa_oks_acc(sum, k, ok, f.mx, f.my, z.x == z.x, z.x, z.y, s2, a.var2[p]);
        else sa_pose_acc(sum, k, ok, f, z.x == z.x, z.x, z.y);
      }
      wv = sa_pose_weight(sum, k, a.min_common);
    }
    a.out_col[v.pose0 + i] = c;
    a.out_w[v.pose0 + i] = wv;
    if (TRACK && c >= 0) a.col_row[v.col0 + (uint32_t)c] = v.pose0 + i;   // (a column has one row: nobody else writes this word)
  }
  if (TRACK && q < 64) {  // the unmatched poses, ascending, as the roots were compacted
    const uint32_t n = pose_compact(M, lane, [&](uint32_t i) { return s_rmatch[i] < 0; }, [&](uint32_t i, uint32_t at) { a.rank[v.pose0 + i] = at; });
    if (lane == 0) a.unmatched[scene] = n;
  }
  return n_roots;
}

// One workgroup per scene.  A scene without poses or without tracks has no bid word anybody wrote and no gains: it leaves
// with -1 / NaN for its poses and 0 roots before the tables are touched (block-uniform: no barrier is skipped by a part of the block).
// TRACK: all its poses are unmatched, pose i the i-th of them.
template <int SRC, bool TRACK, bool OKS>
__global__ __launch_bounds__(AS_NT) void k_pose_assign(const PoseArgs a) {
  const SaPoseSeg g = pose_seg(a, blockIdx.x);
  uint32_t n_roots = 0;
  if (g.m == 0u || g.n == 0u) {
    for (uint32_t i = threadIdx.x; i < g.m; i += AS_NT) {
      a.out_col[g.pose0 + i] = -1;
      a.out_w[g.pose0 + i] = NAN;
      if (TRACK) a.rank[g.pose0 + i] = i;
    }
    if (TRACK && threadIdx.x == 0) a.unmatched[blockIdx.x] = g.m;
  } else n_roots = pose_assign<SRC, TRACK, OKS>(a, pose_scene(a, g), blockIdx.x);
  if (threadIdx.x == 0) a.out_roots[blockIdx.x] = n_roots;
}

// sa_points_track_batch: scene_base = the exclusive prefix of the S <= 65535 per-scene counts, by ONE workgroup.  A thread sums a run of
// `per` consecutive scenes, the 256 run sums are scanned in LDS (Hillis-Steele, 8 steps), the thread walks its run again.
constexpr uint32_t SCAN_THREADS = 256;
__global__ __launch_bounds__(SCAN_THREADS) void k_pose_scan(const PoseArgs a) {
  __shared__ uint32_t s_sum[SCAN_THREADS];
  const uint32_t q = threadIdx.x, per = (a.S + SCAN_THREADS - 1u) / SCAN_THREADS;
  const uint32_t lo = q * per < a.S ? q * per : a.S, hi = lo + per < a.S ? lo + per : a.S;
  uint32_t sum = 0;
  for (uint32_t s = lo; s < hi; ++s) sum += a.unmatched[s];
  s_sum[q] = sum;
  __syncthreads();
  for (uint32_t o = 1; o < SCAN_THREADS; o <<= 1) {
    const uint32_t add = q >= o ? s_sum[q - o] : 0u;
    __syncthreads();
    s_sum[q] += add;
    __syncthreads();
  }
  uint32_t base = s_sum[q] - sum;   // exclusive
  for (uint32_t s = lo; s < hi; ++s) {
    a.scene_base[s] = base;
    base += a.unmatched[s];
  }
}

// sa_points_track: the filter behind the vote, ONE launch.  One thread per (item, point), t = item * P + p < (M + T) * P < 2^31 (checked
// by the call); the items are the M poses, then the T listed tracks.
//   A pose steps the state of its track (sa_pkf_step, what k_points runs for sa_points_step): the slot of its matched column, or —
//   unmatched — slot T_old + scene_base + rank, taken as fresh: has is read as 0 and always written, so the grown planes need no
//   clearing.  The point is sa_point_at<SRC>'s: the tile's presence rule and widening.  Without a vote (out_col == nullptr) every pose
//   is unmatched and pose i is the i-th of them.
//   A track is predicted iff the call coasts, nobody took it (col_row; nullptr: no vote, nobody took any) and the point has a state.
// No two threads touch one state: a matched track is written by its pose's threads and skipped by its own, a coasted one by its own
// only, and new slots are distinct because (scene_base + rank) counts the unmatched poses in front.  Bounds: a listed slot < T_old <=
// cap, a new slot < T_old + M <= cap (reserved by the call); rank, col, col_row and the mask as in the vote.  No atomics, no LDS.
struct PoseStepArgs {
  PoseArgs a;
  float vw;
  uint32_t coast, T_old;
  float4* plane[5];
  uint8_t* has;
  float* out_xy;   // [M][P][2] or nullptr
};
template <int SRC>
__global__ __launch_bounds__(PF_THREADS) void k_pose_step(const PoseStepArgs k) {
  const PoseArgs& a = k.a;
  const uint32_t t = blockIdx.x * PF_THREADS + threadIdx.x;
  if (t >= (a.M + a.T) * a.P) return;
  const uint32_t item = t / a.P, p = t - item * a.P;
  sa_pkf s;
  if (item >= a.M) {   // a listed track
    const uint32_t j = item - a.M;
    if (!k.coast || (a.col_row && a.col_row[j] != POSE_NOBODY)) return;
    const size_t at = (size_t)(a.slots ? a.slots[j] : j) * a.P + p;
    if (k.has[at] == 0) return;
    pt_load(k, at, s);
    sa_pkf_predict(a.pw, k.vw, s);
    pt_store(k, at, s);
    return;
  }
  const uint32_t i = item;
  const int32_t c = a.out_col ? a.out_col[i] : -1;
  const bool fresh = c < 0;
  uint32_t slot = k.T_old + i;   // without a vote
  if (a.out_col) {
    // The column and the rank are the scene's own; the pose's scene is the last one whose first pose is not beyond it.  scene_base:
    // k_pose_scan wrote it iff the call has a table; the single calls' one scene starts at 0.
    const uint32_t sc = pose_seg_at(a, &SaPoseSeg::pose0, i);
    if (fresh) slot = k.T_old + (a.segs ? a.scene_base[sc] : 0u) + a.rank[i];
    else {
      const uint32_t j = pose_seg(a, sc).track0 + (uint32_t)c;
      slot = a.slots ? a.slots[j] : j;
    }
  }
  const size_t at = (size_t)slot * a.P + p;
  const float2 z = sa_point_at<SRC>(a.src, i, a.P, p);
  const bool present = z.x == z.x;
  bool has = !fresh && k.has[at] != 0;
  if (has) pt_load(k, at, s);
  has = sa_pkf_step(a.pw, k.vw, has, s, present, z.x, z.y);
  if (has) pt_store(k, at, s);
  if (has || fresh) k.has[at] = has ? 1 : 0;
  if (k.out_xy) ((float2*)k.out_xy)[t] = has ? make_float2(s.mean[0], s.mean[1]) : make_float2(NAN, NAN);
}

// The three launches between four events (b->pev): tiles = the blocks of the tile launch (the plan's total), one assignment workgroup
// per scene.  A vote with extents (a.circ, b->gev: a gated vote, or any vote under OKS): k_pose_circles between two events of its own in
// front of them; the GATE tile iff there are limits (a.limit), the OKS forms iff the bank's metric is OKS (a.var2).  r counts each
// launch where it happens.
template <int SRC, bool TRACK, bool OKS>
hipError_t launch_metric(sa_points* b, const PoseArgs& a, uint32_t tiles, PoseRan& r) {
  const uint64_t cells = (uint64_t)a.T * a.P;
  const uint32_t fb = (uint32_t)(((cells > a.M ? cells : a.M) + PF_THREADS - 1) / PF_THREADS);
  hipStream_t st = b->st;
  hipEvent_t *ev = b->pev, *gev = b->gev;
  hipError_t h;
  if (a.circ) {
    if ((h = hipEventRecord(gev[0], st)) != hipSuccess) return h;
    hipLaunchKernelGGL((k_pose_circles<SRC, OKS>), dim3((a.M + a.T + PF_THREADS - 1) / PF_THREADS), dim3(PF_THREADS), 0, st, a);
    if ((h = hipGetLastError()) != hipSuccess) return h;
    ++r.extents_launches;
    if ((h = hipEventRecord(gev[1], st)) != hipSuccess) return h;
  }
  if ((h = hipEventRecord(ev[0], st)) != hipSuccess) return h;
  hipLaunchKernelGGL((k_pose_factor<TRACK, OKS>), dim3(fb), dim3(PF_THREADS), 0, st, a);
  if ((h = hipGetLastError()) != hipSuccess) return h;
  ++r.vote_launches;
  if ((h = hipEventRecord(ev[1], st)) != hipSuccess) return h;
  if (a.limit) hipLaunchKernelGGL((k_pose_tile<SRC, true, OKS>), dim3(tiles), dim3(TILE_THREADS), 0, st, a);
  else hipLaunchKernelGGL((k_pose_tile<SRC, false, OKS>), dim3(tiles), dim3(TILE_THREADS), 0, st, a);
  if ((h = hipGetLastError()) != hipSuccess) return h;
  ++r.vote_launches;
  if ((h = hipEventRecord(ev[2], st)) != hipSuccess) return h;
  hipLaunchKernelGGL((k_pose_assign<SRC, TRACK, OKS>), dim3(a.S), dim3(AS_NT), 0, st, a);
  if ((h = hipGetLastError()) != hipSuccess) return h;
  ++r.vote_launches;
  return hipEventRecord(ev[3], st);
}
template <int SRC, bool TRACK>
hipError_t launch_as(sa_points* b, const PoseArgs& a, uint32_t tiles, PoseRan& r) {
  return a.var2 ? launch_metric<SRC, TRACK, true>(b, a, tiles, r) : launch_metric<SRC, TRACK, false>(b, a, tiles, r);
}
// A call that does not track is its vote.  A tracking call: the vote (if there is one: pev[0] .. pev[3]), the scene scan of a call with
// a table that voted, the step: pev[3], tev[0], tev[1].
template <int SRC>
hipError_t launch_call_as(sa_points* b, const PoseStepArgs& k, bool track, bool vote, uint32_t tiles, PoseRan& r) {
  if (!track) return launch_as<SRC, false>(b, k.a, tiles, r);
  hipStream_t st = b->st;
  hipError_t h;
  if (vote) h = launch_as<SRC, true>(b, k.a, tiles, r);
  else h = hipEventRecord(b->pev[3], st);
  if (h != hipSuccess) return h;
  if (vote && k.a.segs) {
    hipLaunchKernelGGL(k_pose_scan, dim3(1), dim3(SCAN_THREADS), 0, st, k.a);
    if ((h = hipGetLastError()) != hipSuccess) return h;
    ++r.scan_launches;
  }
  if ((h = hipEventRecord(b->tev[0], st)) != hipSuccess) return h;
  const uint64_t threads = ((uint64_t)k.a.M + k.a.T) * k.a.P;
  hipLaunchKernelGGL(k_pose_step<SRC>, dim3((uint32_t)((threads + PF_THREADS - 1) / PF_THREADS)), dim3(PF_THREADS), 0, st, k);
  if ((h = hipGetLastError()) != hipSuccess) return h;
  ++r.step_launches;
  return hipEventRecord(b->tev[1], st);
}
hipError_t launch(sa_points* b, const PoseStepArgs& k, int32_t elem, bool track, bool vote, uint32_t tiles, PoseRan& r) {
  return sa_point_elem(elem, [&](auto src) { return launch_call_as<decltype(src)::value>(b, k, track, vote, tiles, r); });
}

// What a call is.  The single calls are a plan of one scene (plan_one) without a table: their scene travels in the kernel arguments.
struct PoseCall {
  const char* what = nullptr;
  SaPosePlan plan;                        // where the scenes lie in the call's arrays (sa_pose_plan.h); poses, tracks: the sums
  bool table = false;                     // a batch, also one of one scene: the call uploads the plan's segment table and, when it tracks, runs k_pose_scan
  std::vector<uint32_t> slots;            // [tracks] the slot of each, or empty: 0, 1, 2, ...
  const sa_point_rows* rows = nullptr;    // the poses; not read when there is none
  sa_pose_options opt{};                  // the vote's min_common and threshold
  const float* limits = nullptr;          // the keypoint tracker, at least one finite limit: [tracks], the vote is gated
  float* tap = nullptr;                   // every scene's matrix, or nullptr
  bool want_circ = false;                 // a gated vote also copies its circles back
  // a tracking call (track_call): behind the vote, or without one, the scene scan and the step run before the one copy back and the one wait
  bool track = false;
  uint32_t coast = 0, T_old = 0, n_new = 0;   // T_old: the bank's tracks in front of the call
  const uint32_t *track_counts = nullptr, *pose_counts = nullptr;   // [scenes], what the plan was made of
  const uint64_t* new_ids = nullptr;      // [n_new]; the keypoint tracker: none, the new ids are first_id, + 1, ... (its counter: never an id of the bank)
  bool tracker = false;
  uint64_t first_id = 0;
  uint64_t* out_track = nullptr;          // nullptr: the tracker, which reads out_plan
  float *out_weight = nullptr, *out_xy = nullptr;
  uint32_t *out_roots = nullptr, *out_created = nullptr;
  SaPoseTrackPlan* out_plan = nullptr;
};

// Everything behind the refusals: the uploads, the launches, the copies out, the ONE wait.  s.res: [m] columns, [m] weights, then the
// roots, one word per scene.  A call votes iff it has a pair; one that does not vote is a tracking call (the others return before).
int run(sa_points* b, const PoseCall& c, PoseRan& s) {
  sa_engine* e = b->e;
  hipStream_t st = b->st;
  const SaPosePlan& plan = c.plan;
  const uint32_t m = plan.poses, n = plan.tracks;
  const size_t n_scenes = plan.segs.size();
  const bool vote = plan.cells != 0;
  const uint64_t np = (uint64_t)n * b->P, cells = plan.cells;
  SA_TRY(make_events(b, b->pev));
  if (c.track) SA_TRY(make_events(b, b->tev));
  PoseArgs a{};
  a.M = m, a.T = n, a.P = b->P, a.S = (uint32_t)n_scenes, a.pw = b->pw;
  a.min_common = c.opt.min_common, a.threshold_q = sa_pose_threshold_q(c.opt.threshold);
  int32_t elem = SA_ELEM_F32;
  if (c.table) {   // the segment table: ONE upload
    const size_t bytes = n_scenes * sizeof(SaPoseSeg);
    SA_TRY(sa_engine_ensure(e, b->d_segs, bytes));
    SA_HIPCHK(e, hipMemcpyAsync(b->d_segs.p, plan.segs.data(), bytes, hipMemcpyHostToDevice, st));
    s.bytes_h2d += bytes;
    a.segs = (const SaPoseSeg*)b->d_segs.p;
  } else a.one = plan.segs[0];
  if (!c.slots.empty()) {
    SA_TRY(sa_engine_ensure(e, b->d_slots, (size_t)n * 4));
    SA_HIPCHK(e, hipMemcpyAsync(b->d_slots.p, c.slots.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    s.bytes_h2d += (uint64_t)n * 4;
    a.slots = (const uint32_t*)b->d_slots.p;
  }
  if (m) SA_TRY(sa_point_rows_stage(e, st, b->P, m, c.rows, b->d_pts, b->d_index, b->d_mask, a.src, elem, s.bytes_h2d, s.src_bytes));
  const bool gated = c.limits && vote, oks = b->metric == SA_POSE_METRIC_OKS && vote;
  if (gated || oks) {   // the extents launch: room for the circles; for the gate the limits beside the slot table, for the metric the areas
    SA_TRY(make_events(b, b->gev));
    SA_TRY(sa_engine_ensure(e, b->d_circ, ((size_t)m + n) * 16));
    a.circ = (float4*)b->d_circ.p;
    if (gated) {
      SA_TRY(sa_engine_ensure(e, b->d_limit, (size_t)n * 4));
      SA_HIPCHK(e, hipMemcpyAsync(b->d_limit.p, c.limits, (size_t)n * 4, hipMemcpyHostToDevice, st));
      s.bytes_h2d += (uint64_t)n * 4;
      a.limit = (const float*)b->d_limit.p;
    }
    if (oks) {
      SA_TRY(sa_engine_ensure(e, b->d_area, ((size_t)m + n) * 4));
      a.area = (float*)b->d_area.p, a.var2 = (const float*)b->d_var2.p;
    }
  }
  if (vote) {
    SA_TRY(sa_engine_ensure(e, b->d_fac4, (size_t)np * 16));
    SA_TRY(sa_engine_ensure(e, b->d_fac1, (size_t)np * 4));
    SA_TRY(sa_engine_ensure(e, b->d_gain, (size_t)cells * 8));
    SA_TRY(sa_engine_ensure(e, b->d_best, (size_t)m * 8));
    SA_TRY(sa_engine_ensure(e, b->d_res, (size_t)m * 8 + n_scenes * 4));
  }
  if (c.tap) {
    SA_TRY(sa_engine_ensure(e, b->d_tap, (size_t)cells * 4));
    a.tap = (float*)b->d_tap.p;
  }
  for (int k = 0; k < 5; ++k) a.plane[k] = (const float4*)b->plane[k].p;
  a.has = (const uint8_t*)b->has.p;
  a.fac4 = (float4*)b->d_fac4.p, a.fac1 = (float*)b->d_fac1.p, a.gain = (int64_t*)b->d_gain.p, a.best = (unsigned long long*)b->d_best.p;
  if (vote) a.out_col = (int32_t*)b->d_res.p, a.out_w = (float*)b->d_res.p + m, a.out_roots = (uint32_t*)b->d_res.p + 2 * (size_t)m;
  const uint64_t xy_bytes = c.track && c.out_xy ? (uint64_t)m * b->P * 8 : 0;
  PoseStepArgs k{};   // (a call that does not track reads k.a alone)
  if (c.track && vote) {   // col_row [n], rank [m], unmatched [scenes], scene_base [scenes]
    SA_TRY(sa_engine_ensure(e, b->d_trk, ((size_t)n + m + 2 * n_scenes) * 4));
    a.col_row = (uint32_t*)b->d_trk.p, a.rank = a.col_row + n, a.unmatched = a.rank + m, a.scene_base = a.unmatched + n_scenes;
  }
  if (xy_bytes) {
    SA_TRY(sa_engine_ensure(e, b->d_out, (size_t)xy_bytes));
    k.out_xy = (float*)b->d_out.p;
  }
  k.a = a, k.vw = b->vw, k.coast = c.coast, k.T_old = c.T_old;
  for (int r = 0; r < 5; ++r) k.plane[r] = (float4*)b->plane[r].p;
  k.has = (uint8_t*)b->has.p;
  SA_HIPCHK(e, launch(b, k, elem, c.track, vote, plan.tiles, s));
  if (vote) {
    s.res.resize((size_t)m * 2 + n_scenes);
    SA_HIPCHK(e, hipMemcpyAsync(s.res.data(), b->d_res.p, s.res.size() * 4, hipMemcpyDeviceToHost, st));
    s.bytes_d2h += s.res.size() * 4;
  }
  if (c.tap) {
    SA_HIPCHK(e, hipMemcpyAsync(c.tap, b->d_tap.p, (size_t)cells * 4, hipMemcpyDeviceToHost, st));
    s.bytes_d2h += cells * 4;
  }
  if (gated && c.want_circ) {
    s.circ.resize(((size_t)m + n) * 4);
    SA_HIPCHK(e, hipMemcpyAsync(s.circ.data(), b->d_circ.p, s.circ.size() * 4, hipMemcpyDeviceToHost, st));
    s.bytes_d2h += s.circ.size() * 4;
  }
  if (xy_bytes) {
    SA_HIPCHK(e, hipMemcpyAsync(c.out_xy, b->d_out.p, (size_t)xy_bytes, hipMemcpyDeviceToHost, st));
    s.bytes_d2h += xy_bytes;
  }
  SA_HIPCHK(e, hipStreamSynchronize(st));
  for (size_t k = 0; vote && k < n_scenes; ++k) s.roots += s.res[(size_t)m * 2 + k];
  float ms = 0.f;
  hipEvent_t first = b->pev[vote ? 0 : 3];
  if (a.var2) first = b->gev[0];   // under OKS the extents are a launch of the vote itself
  SA_HIPCHK(e, hipEventElapsedTime(&ms, first, c.track ? b->tev[1] : b->pev[3]));
  s.device_ms = ms;
  for (int k = 0; vote && k < 3; ++k) {
    SA_HIPCHK(e, hipEventElapsedTime(&ms, b->pev[k], b->pev[k + 1]));
    s.kernel_ms[k] = ms;
  }
  if (a.circ) {
    SA_HIPCHK(e, hipEventElapsedTime(&ms, b->gev[0], b->gev[1]));
    s.gate_ms = ms;
  }
  if (c.track) {
    SA_HIPCHK(e, hipEventElapsedTime(&ms, b->pev[3], b->tev[0]));
    s.kernel_ms[3] = ms;
    SA_HIPCHK(e, hipEventElapsedTime(&ms, b->tev[0], b->tev[1]));
    s.kernel_ms[4] = ms;
  }
  return SA_OK;
}
// poses [m0, m0 + m) of the results against the scene's n tracks `ids` -> the poses that got a track
uint32_t give_out(const PoseRan& s, size_t m_all, uint32_t m0, uint32_t m, uint32_t n, const uint64_t* ids, uint64_t* out_track, float* out_weight) {
  uint32_t matched = 0;
  for (uint32_t i = m0; i < m0 + m; ++i) {
    const int32_t c = (int32_t)s.res[i];
    const bool hit = c >= 0 && (uint32_t)c < n;
    out_track[i] = hit ? ids[c] : 0;
    std::memcpy(out_weight + i, &s.res[m_all + i], 4);
    matched += hit;
  }
  return matched;
}

static_assert(sizeof(SaPoseSeg) == 32, "the device reads this layout");
static_assert(SA_POSE_PLAN_SIDE == SA_POSE_MAX && SA_POSE_PLAN_SCENES == SA_POSE_BATCH_SCENES && SA_POSE_PLAN_CELLS == SA_POSE_BATCH_CELLS,
              "sa_pose_plan.h states the limits of the public headers");
static_assert(SA_POSE_PLAN_TILE_M == TILE_M && SA_POSE_PLAN_TILE_T == TILE_T, "the plan counts the tiles of k_pose_tile");

// the plan of a batch, or the refusal that names the scene
int plan_scenes(sa_engine* e, const char* what, uint32_t n_scenes, const uint32_t* track_counts, const uint32_t* pose_counts, SaPosePlan& plan) {
  uint32_t bad = 0;
  switch (sa_pose_plan(n_scenes, track_counts, pose_counts, SA_POSE_MAX, &plan, &bad)) {
    case SA_POSE_FITS: break;
    case SA_POSE_TOO_MANY_SCENES: return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: %u scenes; one call takes at most %u", what, n_scenes, SA_POSE_BATCH_SCENES);
    case SA_POSE_SCENE_TOO_LARGE:
      return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: scene %u has %u poses x %u tracks; a scene takes at most %u of either", what, bad, pose_counts[bad],
                            track_counts[bad], SA_POSE_MAX);
    case SA_POSE_TOO_MANY_POSES: return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: with scene %u the poses of the call no longer fit 32 bits", what, bad);
    case SA_POSE_TOO_MANY_TRACKS: return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: with scene %u the tracks of the call no longer fit 32 bits", what, bad);
    case SA_POSE_TOO_MANY_CELLS:
      return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: with scene %u (%u poses x %u tracks) the call has more than %u pairs", what, bad, pose_counts[bad],
                            track_counts[bad], SA_POSE_BATCH_CELLS);
  }
  return SA_OK;
}

// the single calls' own size refusal, then their one scene of m poses x n tracks as a plan: within the side it always fits
int plan_one(sa_engine* e, const char* what, uint32_t n, uint32_t m, SaPosePlan& plan) {
  if (m > SA_POSE_MAX || n > SA_POSE_MAX)
    return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: %u poses x %u tracks; one call takes at most %u of either", what, m, n, SA_POSE_MAX);
  uint32_t bad = 0;
  sa_pose_plan(1u, &n, &m, SA_POSE_MAX, &plan, &bad);
  return SA_OK;
}

// what sa_points_track(_batch) refuse about their m poses and n listed tracks (null = every track), and the tracks' slots: ONE check_ids
int track_inputs(sa_points* b, const char* what, uint32_t n, const uint64_t* track_ids, uint32_t m, const sa_point_rows* poses, PoseCall& c) {
  if (m && (!c.out_track || !c.out_weight)) return sa_engine_fail(b->e, SA_ERR_BAD_ARG, "%s: null argument", what);
  if (m) SA_TRY(check_rows(b, what, m, poses));
  if (track_ids) SA_TRY(check_ids(b, what, n, track_ids, true, c.slots));
  return SA_OK;
}

// what the three tracking calls describe alike
PoseCall track_desc(sa_points* b, const char* what, const sa_point_rows* poses, const sa_pose_track_options* o, float* out_weight, float* out_xy) {
  PoseCall c;
  c.what = what, c.rows = poses, c.opt = sa_pose_options{(uint32_t)sizeof(sa_pose_options), o->min_common, o->threshold, 0u};
  c.track = true, c.coast = o->coast, c.T_old = b->T, c.out_weight = out_weight, c.out_xy = out_xy;
  return c;
}

// A tracking call behind the refusals about its poses, its listed tracks and its plan: the refusals of the new ids, the room for T + m
// tracks, run() with its one wait, then the created ids into the table in the order the device gave them slots (sa_pose_track_plan.h).
int track_call(sa_points* b, const PoseCall& c, PoseRan& r) {
  sa_engine* e = b->e;
  const char* what = c.what;
  const uint32_t m = c.plan.poses, n = c.plan.tracks, n_scenes = (uint32_t)c.plan.segs.size();
  if (!c.tracker) {
    if (c.n_new < m) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: %u new ids for %u poses; one id is offered per pose", what, c.n_new, m);
    if (c.n_new && !c.new_ids) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null new ids", what);
    std::unordered_set<uint64_t> seen;
    seen.reserve((size_t)c.n_new * 2u);
    for (uint32_t i = 0; i < c.n_new; ++i) {
      if (c.new_ids[i] == 0) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: new id 0 at %u", what, i);
      if (!seen.insert(c.new_ids[i]).second) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: new id %llu twice in one call", what, (unsigned long long)c.new_ids[i]);
      if (b->slot_of.count(c.new_ids[i]))   // (the listed tracks are tracks of the bank: this covers track_ids)
        return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: new id %llu is a track of the bank", what, (unsigned long long)c.new_ids[i]);
    }
  }
  if (((uint64_t)c.T_old + m) * b->P >= 0x80000000ull)
    return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: %llu tracks x %u points reach 2^31", what, (unsigned long long)c.T_old + m, b->P);
  if (m) SA_TRY(reserve(b, (uint64_t)c.T_old + m));
  sa_pose_track_stats s{};
  s.scenes = n_scenes, s.poses = m, s.tracks = n;
  *c.out_created = 0;
  if (c.out_roots) std::fill(c.out_roots, c.out_roots + n_scenes, 0u);
  if (m == 0 && (!c.coast || n == 0)) {   // neither a pose nor a track to coast
    b->last_track = s;
    return SA_OK;
  }
  const int rc = run(b, c, r);
  if (rc != SA_OK) {
    b->broken = true;
    return rc;
  }
  const bool vote = c.plan.cells != 0;
  std::vector<int32_t> cols((size_t)m, -1);
  if (vote) std::memcpy(cols.data(), r.res.data(), (size_t)m * 4);
  SaPoseTrackPlan tp;
  sa_pose_track_plan(n_scenes, c.track_counts, c.pose_counts, cols.data(), c.slots.empty() ? nullptr : c.slots.data(), c.T_old, &tp);
  const auto new_id = [&](uint32_t k) { return c.tracker ? c.first_id + k : c.new_ids[k]; };
  for (uint32_t i = 0; i < m; ++i) {   // (a matched pose's slot is its track's: the listed tracks are resolved once)
    const bool hit = tp.rank[i] == SA_POSE_TRACK_NONE;
    if (c.out_track) c.out_track[i] = hit ? b->ids[tp.slot[i]] : new_id(tp.rank[i]);
    c.out_weight[i] = NAN;
    if (hit) std::memcpy(c.out_weight + i, &r.res[(size_t)m + i], 4);
  }
  for (uint32_t k = 0; k < tp.created; ++k) {
    b->ids.push_back(new_id(k));
    b->slot_of.emplace(new_id(k), b->T++);
  }
  for (uint32_t k = 0; c.out_roots && vote && k < n_scenes; ++k) c.out_roots[k] = r.res[(size_t)m * 2 + k];
  *c.out_created = tp.created;
  ran_into(s, r);
  s.vote_launches = r.vote_launches + (c.tracker ? 0u : r.extents_launches);   // (the tracker reports the extents as its gate launch)
  s.step_launches = r.scan_launches + r.step_launches;
  s.matched = tp.matched, s.created = tp.created, s.coasted = c.coast ? (uint32_t)tp.coasted.size() : 0u;
  b->last_track = s;
  if (c.out_plan) *c.out_plan = std::move(tp);
  return SA_OK;
}

}  // namespace

namespace sa_pt {

// the refusals the calls share
int check_options(sa_engine* e, const char* what, const sa_pose_options* o) {
  if (!o) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null options", what);
  if (o->struct_size != sizeof(sa_pose_options)) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: options.struct_size %u (%zu)", what, o->struct_size, sizeof(sa_pose_options));
  if (o->min_common == 0) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: min_common must be >= 1", what);
  if (!sa_point_finite(o->threshold) || o->threshold < 0.0f) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: threshold %g must be finite and >= 0", what, (double)o->threshold);
  return SA_OK;
}

int check_track_options(sa_engine* e, const char* what, const sa_pose_track_options* o) {
  if (!o) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null options", what);
  if (o->struct_size != sizeof(sa_pose_track_options))
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: options.struct_size %u (%zu)", what, o->struct_size, sizeof(sa_pose_track_options));
  const sa_pose_options po{(uint32_t)sizeof(sa_pose_options), o->min_common, o->threshold, 0u};
  SA_TRY(check_options(e, what, &po));
  if (o->coast > 1u) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: coast %u must be 0 or 1", what, o->coast);
  return SA_OK;
}

int sort_check(sa_points* b, const char* what, uint32_t n_scenes, const uint32_t* track_counts, const uint32_t* pose_counts,
               const sa_point_rows* poses, uint64_t T_after) {
  SaPosePlan plan;
  SA_TRY(plan_scenes(b->e, what, n_scenes, track_counts, pose_counts, plan));
  if (plan.poses) SA_TRY(check_rows(b, what, plan.poses, poses));
  if ((T_after + plan.poses) * b->P >= 0x80000000ull)
    return sa_engine_fail(b->e, SA_ERR_UNSUPPORTED, "%s: %llu tracks x %u points reach 2^31", what, (unsigned long long)(T_after + plan.poses), b->P);
  return SA_OK;
}

// (sort_check has refused what track_inputs would about the poses; the tracks come as slots)
int sort_track(sa_points* b, const char* what, uint32_t n_scenes, const uint32_t* track_counts, const uint32_t* pose_counts,
               const sa_point_rows* poses, const uint32_t* slots, const float* limits, uint64_t first_id, const sa_pose_track_options* o,
               float* out_weight, float* out_xy, SaPoseTrackPlan* out_plan, PoseRan& r) {
  PoseCall c = track_desc(b, what, poses, o, out_weight, out_xy);
  SA_TRY(plan_scenes(b->e, what, n_scenes, track_counts, pose_counts, c.plan));
  uint32_t created = 0;
  c.table = true, c.track_counts = track_counts, c.pose_counts = pose_counts, c.out_created = &created, c.out_plan = out_plan;
  c.slots.assign(slots, slots + c.plan.tracks);
  c.limits = limits, c.tracker = true, c.first_id = first_id;
  *out_plan = SaPoseTrackPlan();
  out_plan->unmatched.assign(n_scenes, 0u);
  for (uint32_t k = 0; o->coast && k < c.plan.tracks; ++k) out_plan->coasted.push_back(k);   // (what holds if nothing runs: no pose, nothing coasts)
  return track_call(b, c, r);
}

int sort_peek(sa_points* b, const char* what, uint32_t n_scenes, const uint32_t* track_counts, const uint32_t* pose_counts,
              const sa_point_rows* poses, const uint32_t* slots, const float* limits, const sa_pose_track_options* o, int32_t* out_cols,
              float* out_weight, float* out_tap, PoseRan& r) {
  PoseCall c;
  SA_TRY(plan_scenes(b->e, what, n_scenes, track_counts, pose_counts, c.plan));
  const uint32_t m = c.plan.poses, n = c.plan.tracks;
  for (uint32_t i = 0; i < m; ++i) { out_cols[i] = -1; out_weight[i] = NAN; }
  if (c.plan.cells == 0) return SA_OK;
  c.what = what, c.table = true, c.rows = poses, c.opt = sa_pose_options{(uint32_t)sizeof(sa_pose_options), o->min_common, o->threshold, 0u};
  c.slots.assign(slots, slots + n);
  c.limits = limits, c.tap = out_tap, c.want_circ = out_tap != nullptr;
  SA_TRY(run(b, c, r));
  for (uint32_t k = 0; !r.circ.empty() && k < n_scenes; ++k) {   // the refused pairs, by the rule the tile applied
    const SaPoseSeg& g = c.plan.segs[k];
    for (uint32_t i = g.pose0; i < g.pose0 + g.m; ++i)
      for (uint32_t j = g.track0; j < g.track0 + g.n; ++j) {
        const float* pc = r.circ.data() + (size_t)i * 4;
        const float* tc = r.circ.data() + ((size_t)m + j) * 4;
        r.refused_pairs += sa_pose_refused(pc[3] != 0.f, sa_geo{pc[0], pc[1], pc[2], 0.f}, tc[3] != 0.f, sa_geo{tc[0], tc[1], tc[2], 0.f}, limits[j]);
      }
  }
  for (const SaPoseSeg& g : c.plan.segs)
    for (uint32_t i = g.pose0; i < g.pose0 + g.m; ++i) {
      const int32_t col = (int32_t)r.res[i];
      if (col >= 0 && (uint32_t)col < g.n) {
        out_cols[i] = col;
        std::memcpy(out_weight + i, &r.res[(size_t)m + i], 4);
      }
    }
  return SA_OK;
}

}  // namespace sa_pt

extern "C" {

void sa_pose_track_options_default(sa_pose_track_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->struct_size = sizeof *o;
  o->min_common = 1;
  o->threshold = 1.0f;
  o->coast = 1;
}

int sa_points_track(sa_points* b, uint32_t n_tracks, const uint64_t* track_ids, uint32_t m, const sa_point_rows* poses, uint32_t n_new,
                    const uint64_t* new_ids, const sa_pose_track_options* o, uint64_t* out_track, float* out_weight, float* out_xy,
                    uint32_t* out_created) {
  const char* what = "sa_points_track";
  if (!b) return SA_ERR_BAD_ARG;
  SA_TRY(enter(b, what));
  b->last_track = sa_pose_track_stats{};
  sa_engine* e = b->e;
  SA_TRY(check_track_options(e, what, o));
  if (!out_created) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null out_created", what);
  const uint32_t n = track_ids ? n_tracks : b->T;
  PoseCall c = track_desc(b, what, poses, o, out_weight, out_xy);
  c.out_track = out_track, c.out_created = out_created, c.track_counts = &n, c.pose_counts = &m, c.n_new = n_new, c.new_ids = new_ids;
  SA_TRY(track_inputs(b, what, n, track_ids, m, poses, c));
  SA_TRY(plan_one(e, what, n, m, c.plan));
  PoseRan r;
  return track_call(b, c, r);
}

int sa_points_track_batch(sa_points* b, uint32_t n_scenes, const uint32_t* track_counts, const uint64_t* track_ids,
                          const uint32_t* pose_counts, const sa_point_rows* poses, uint32_t n_new, const uint64_t* new_ids,
                          const sa_pose_track_options* o, uint64_t* out_track, float* out_weight, float* out_xy, uint32_t* out_roots,
                          uint32_t* out_created) {
  const char* what = "sa_points_track_batch";
  if (!b) return SA_ERR_BAD_ARG;
  SA_TRY(enter(b, what));
  b->last_track = sa_pose_track_stats{};
  sa_engine* e = b->e;
  SA_TRY(check_track_options(e, what, o));
  if (!out_created) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null out_created", what);
  if (n_scenes == 0) {
    *out_created = 0;
    return SA_OK;
  }
  if (!track_counts || !pose_counts || !track_ids) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null counts or track ids", what);
  PoseCall c = track_desc(b, what, poses, o, out_weight, out_xy);
  SA_TRY(plan_scenes(e, what, n_scenes, track_counts, pose_counts, c.plan));
  c.table = true, c.out_track = out_track, c.out_roots = out_roots, c.out_created = out_created;
  c.track_counts = track_counts, c.pose_counts = pose_counts, c.n_new = n_new, c.new_ids = new_ids;
  SA_TRY(track_inputs(b, what, c.plan.tracks, track_ids, c.plan.poses, poses, c));
  PoseRan r;
  return track_call(b, c, r);
}

int sa_points_track_last(sa_points* b, sa_pose_track_stats* out) {
  if (!b || !out) return SA_ERR_BAD_ARG;
  *out = b->last_track;
  out->struct_size = sizeof *out;
  return SA_OK;
}

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
  SA_TRY(check_options(e, what, o));
  if (m == 0) return SA_OK;
  if (!out_track || !out_weight) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
  SA_TRY(check_rows(b, what, m, poses));
  const uint32_t n = track_ids ? n_tracks : b->T;
  PoseCall c;
  if (track_ids) SA_TRY(check_ids(b, what, n, track_ids, true, c.slots));
  SA_TRY(plan_one(e, what, n, m, c.plan));
  if (n == 0) {
    for (uint32_t i = 0; i < m; ++i) { out_track[i] = 0; out_weight[i] = NAN; }
    b->last_pose.poses = m;
    return SA_OK;
  }
  c.what = what, c.rows = poses, c.opt = *o, c.tap = out_matrix;
  PoseRan r;
  SA_TRY(run(b, c, r));
  sa_pose_stats s{};
  ran_into(s, r);
  s.poses = m, s.tracks = n, s.launches = r.extents_launches + r.vote_launches;
  s.matched = give_out(r, m, 0, m, n, track_ids ? track_ids : b->ids.data(), out_track, out_weight);
  b->last_pose = s;
  return SA_OK;
}

int sa_points_associate_batch(sa_points* b, uint32_t n_scenes, const uint32_t* track_counts, const uint64_t* track_ids,
                              const uint32_t* pose_counts, const sa_point_rows* poses, const sa_pose_options* o, uint64_t* out_track,
                              float* out_weight, uint32_t* out_roots, float* out_matrix) {
  const char* what = "sa_points_associate_batch";
  if (!b) return SA_ERR_BAD_ARG;
  SA_TRY(enter(b, what));
  b->last_pose_batch = sa_pose_batch_stats{};
  sa_engine* e = b->e;
  SA_TRY(check_options(e, what, o));
  if (n_scenes == 0) return SA_OK;
  if (!track_counts || !pose_counts || !track_ids) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null counts or track ids", what);
  PoseCall c;
  const SaPosePlan& plan = c.plan;
  SA_TRY(plan_scenes(e, what, n_scenes, track_counts, pose_counts, c.plan));
  const uint32_t m = plan.poses, n = plan.tracks;
  if (m && (!out_track || !out_weight)) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
  if (m) SA_TRY(check_rows(b, what, m, poses));
  if (m) SA_TRY(check_ids(b, what, n, track_ids, true, c.slots));
  sa_pose_batch_stats s{};
  s.scenes = n_scenes, s.poses = m, s.tracks = n;
  if (plan.cells == 0) {   // no pose, or no pose that has a track to be matched to: nothing is launched
    for (uint32_t i = 0; i < m; ++i) { out_track[i] = 0; out_weight[i] = NAN; }
    if (out_roots) std::fill(out_roots, out_roots + n_scenes, 0u);
    b->last_pose_batch = s;
    return SA_OK;
  }
  c.what = what, c.table = true, c.rows = poses, c.opt = *o, c.tap = out_matrix;
  PoseRan r;
  SA_TRY(run(b, c, r));
  ran_into(s, r);
  for (uint32_t k = 0; k < n_scenes; ++k) {
    const SaPoseSeg& g = plan.segs[k];
    s.matched += give_out(r, m, g.pose0, g.m, g.n, track_ids + g.track0, out_track, out_weight);
    if (out_roots) out_roots[k] = r.res[(size_t)m * 2 + k];
  }
  s.tiles = plan.tiles, s.launches = r.extents_launches + r.vote_launches;
  b->last_pose_batch = s;
  return SA_OK;
}

int sa_points_associate_batch_last(sa_points* b, sa_pose_batch_stats* out) {
  if (!b || !out) return SA_ERR_BAD_ARG;
  *out = b->last_pose_batch;
  out->struct_size = sizeof *out;
  return SA_OK;
}

void sa_pose_metric_default(sa_pose_metric* m) {
  if (!m) return;
  std::memset(m, 0, sizeof *m);
  m->struct_size = sizeof *m;
  m->kind = SA_POSE_METRIC_MAHALANOBIS;
}

int sa_points_set_metric(sa_points* b, const sa_pose_metric* m) {
  const char* what = "sa_points_set_metric";
  if (!b) return SA_ERR_BAD_ARG;
  SA_TRY(enter(b, what));
  sa_engine* e = b->e;
  if (!m) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null metric", what);
  if (m->struct_size != sizeof(sa_pose_metric)) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: struct_size %u (%zu)", what, m->struct_size, sizeof(sa_pose_metric));
  if (m->reserved != 0) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: reserved must be 0", what);
  if (m->kind == SA_POSE_METRIC_MAHALANOBIS) {
    if (m->n_sigmas != 0) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: %u sigmas; the Mahalanobis metric takes none", what, m->n_sigmas);
    b->metric = SA_POSE_METRIC_MAHALANOBIS;
    b->sigmas.clear();
    return SA_OK;
  }
  if (m->kind != SA_POSE_METRIC_OKS) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: unknown kind %u", what, m->kind);
  if (m->n_sigmas != b->P) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: %u sigmas for a bank of %u points", what, m->n_sigmas, b->P);
  if (!m->sigmas) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null sigmas", what);
  std::vector<float> var2(b->P);
  for (uint32_t p = 0; p < b->P; ++p) {
    if (!sa_point_finite(m->sigmas[p]) || !(m->sigmas[p] > 0.0f))
      return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: sigma %u = %g must be finite and > 0", what, p, (double)m->sigmas[p]);
    var2[p] = sa_oks_var2(m->sigmas[p]);
  }
  // nothing is refused from here on; the previous metric stays if the device does not take the upload
  SA_TRY(sa_engine_ensure(e, b->d_var2, (size_t)b->P * 4));
  SA_HIPCHK(e, hipMemcpyAsync(b->d_var2.p, var2.data(), (size_t)b->P * 4, hipMemcpyHostToDevice, b->st));
  SA_HIPCHK(e, hipStreamSynchronize(b->st));
  b->sigmas.assign(m->sigmas, m->sigmas + b->P);
  b->metric = SA_POSE_METRIC_OKS;
  return SA_OK;
}

int sa_points_get_metric(sa_points* b, uint32_t* out_kind, float* out_sigmas) {
  if (!b || !out_kind) return SA_ERR_BAD_ARG;
  *out_kind = b->metric;
  if (out_sigmas && b->metric == SA_POSE_METRIC_OKS) std::copy(b->sigmas.begin(), b->sigmas.end(), out_sigmas);
  return SA_OK;
}

int sa_points_associate_last(sa_points* b, sa_pose_stats* out) {
  if (!b || !out) return SA_ERR_BAD_ARG;
  *out = b->last_pose;
  out->struct_size = sizeof *out;
  return SA_OK;
}

}  // extern "C"
