// sa_pose_nms.hip — non-maximum suppression of poses by OKS (include/similari_pose_nms.h): the poses of one scene or of a batch of scenes,
// filtered and ranked on the host from their scores, their pairs weighed and the greedy pass run on the device, in three launches
// whatever the number of scenes.
//
// The arithmetic is sa_pose_nms.h over sa_pose_oks.h, shared with the host build of tests/emu_pose_nms; the layout of the scenes and of
// their masks is sa_frames_plan.h, shared with the box path (sa_engine.hip: frames_nms), and the greedy pass is the box path's
// k_nms_sweep<S> (sa_upkeep.hip: sa_launch_nms_sweep), which does not care what metric set the bits.  What is here: the calls and
// their refusals, one host path (nms_call; a single call and the tap are the plan of one scene) and two kernels.  The check of the
// poses' descriptor and the read of one point under the presence rule are sa_point_rows.h, shared with the bank and the vote; the
// staging is this file's own, because it gathers the survivors in rank order into the call's one upload.
//
//   k_pose_nms_lay<SRC>  one thread per surviving pose t of the call, in rank order: row rank[t] of the source (f32, f16 or bf16,
//                        widened exactly; SA_ROW_NONE: no point) under the presence rule (sa_point_of<SRC>) -> its points
//                        POINT-MAJOR, pts[p * total + t] (x, y as one 8-byte piece, x = NaN for an absent point), and the area of
//                        its extent, area[t].  The shape
//                        k_pose_factor gives the vote's tile: consecutive lanes of the pair kernel, which are consecutive poses, read
//                        consecutive memory for each point, and a pose's row — strided, 2 or 3 components, 2 or 4 bytes each — is
//                        walked once per call instead of once per block that meets the pose.
//   k_pose_nms_mask<TAP> 256 threads, one block per (16 rows x 64 columns) word band of a scene's pair matrix: lane = column pose j,
//                        wave w owns rows 4 w .. 4 w + 3 (the shape of pose_tile, sa_pose.hip).  The 16 row poses' points are staged in
//                        LDS, at most 64 points at a time (8 KiB whatever P is), and every read of them is a broadcast: all lanes of a
//                        wave read the address of (point, row).  Each thread walks p ascending with (sum, k) of its four pairs in
//                        registers; a row's 64 bits are one ballot, written by lane 0 — no atomics.  The mask is exactly k_nms_mask's:
//                        bit (i, j) for i < j in rank order, row i of a scene at mask_off + i * W, one 64-bit word per 64 columns.  A word
//                        wholly on or below the diagonal is written 0 without reading a point; a block beyond its scene's extent leaves
//                        at once.  TAP (sa_pose_nms_matrix, one scene): every cell also leaves w, NaN on and below the diagonal.
//
// Bounds.  A scene's poses are [first, first + count) of the call's `total` (sa_frames_plan: back to back), so i, j < count of the
// scene are below total in pts (P * total pieces), area and keep (total each).  The source is a SaPointSrc of `total` items
// (sa_point_rows.h, where the bounds of a point's read are stated): its index is the rank table — total entries, each SA_ROW_NONE or a
// row sa_point_rows_check found below n_rows of a span inside one registered block, or below total of the staged rows — and its mask
// the present flags, staged in rank order.  var2 has P entries.  Mask words: row i < count, word blockIdx.x < W
// because 64 * blockIdx.x < count, inside the scene's count * W words at mask_off, inside mask_words (the plan's sum).  The grid's z is
// the scene, below n_scenes <= 65535; the table has n_scenes entries.  The tap is [count][count] of the one scene.
//
// Reference: src/utils/nms.rs:32-72.
#include "sa_store.h"
#include "sa_frames_plan.h"
#include "sa_pose_nms.h"
#include "sa_point_rows.h"
#include "../../include/similari_pose_nms.h"

#include <cmath>
#include <cstring>
#include <string>

static_assert(SA_POSE_NMS_MAX == SA_FRAMES_NMS_MAX && SA_POSE_NMS_MAX_SCENES == SA_FRAMES_MAX_SCENES, "the header states the plan's limits");
static_assert(sizeof(SaFrameSeg) == 24, "the device reads this layout");

struct SaPoseNms {
  DevBuf d_up, d_pts, d_area, d_mask, d_keep, d_tap;   // the call's one upload; [P][total] sa_xy; [total] f32; the masks; [total] u8; [m'][m'] f32
  hipEvent_t ev[2] = {nullptr, nullptr};               // in front of the first launch, behind the last
  sa_pose_nms_stats last{};
};
void sa_pose_nms_release(SaPoseNms* s) {
  if (!s) return;
  for (DevBuf* b : {&s->d_up, &s->d_pts, &s->d_area, &s->d_mask, &s->d_keep, &s->d_tap}) sa_engine_free(*b);
  for (hipEvent_t ev : s->ev)
    if (ev) hipEventDestroy(ev);
  delete s;
}

namespace {

constexpr uint32_t LAY_THREADS = 256;
constexpr uint32_t NM_ROWS = 16, NM_COLS = 64, NM_THREADS = 256, NM_CHUNK = 64, NM_WAVE_ROWS = NM_ROWS / (NM_THREADS / 64);

struct LayArgs {
  uint32_t total, P;
  SaPointSrc src;          // the points of the `total` surviving poses (sa_point_rows.h): index = the rank table, the mask in rank order
  sa_xy* pts;              // [P][total]
  float* area;             // [total]
};
template <int SRC>
__global__ __launch_bounds__(LAY_THREADS) void k_pose_nms_lay(const LayArgs a) {
  const uint32_t t = blockIdx.x * LAY_THREADS + threadIdx.x;
  if (t >= a.total) return;
  sa_pose_rect q;
  sa_pose_rect_clear(q);
  const uint32_t r = sa_point_row(a.src, t);
  for (uint32_t p = 0; p < a.P; ++p) {   // sa_pose_extent's walk, which also lays each point out: the row is read once
    const float2 z = sa_point_of<SRC>(a.src, r, t, a.P, p);
    a.pts[(size_t)p * a.total + t] = sa_xy{z.x, z.y};
    if (z.x == z.x) sa_pose_rect_add(q, z.x, z.y);   // (sa_pose_nms_area's walk, without reading the points back)
  }
  a.area[t] = sa_oks_area(q);
}

struct MaskArgs {
  const SaFrameSeg* segs;
  const sa_xy* pts;
  const float* area;
  const float* var2;
  uint64_t* mask;
  float* tap;              // TAP: [count][count] of the call's one scene
  uint32_t total, P, min_common;
  float thr;
};
template <bool TAP>
__global__ __launch_bounds__(NM_THREADS) void k_pose_nms_mask(const MaskArgs a) {
  __shared__ sa_xy s_z[NM_CHUNK][NM_ROWS];
  const SaFrameSeg seg = a.segs[blockIdx.z];   // blockIdx.z = scene (a block-uniform address: scalar loads)
  const uint32_t n = seg.count, W = seg.W;
  const uint32_t i0 = blockIdx.y * NM_ROWS, j0 = blockIdx.x * NM_COLS;
  if (i0 >= n || j0 >= n) return;
  uint64_t* __restrict__ mask = a.mask + seg.mask_off;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (j0 + (NM_COLS - 1u) <= i0) {   // the whole word lies on or below the diagonal: no pair with i < j
    if (tid < NM_ROWS && i0 + tid < n) mask[(size_t)(i0 + tid) * W + blockIdx.x] = 0ull;
    if (TAP)
      for (uint32_t e = tid; e < NM_ROWS * NM_COLS; e += NM_THREADS) {
        const uint32_t i = i0 + e / NM_COLS, j = j0 + e % NM_COLS;
        if (i < n && j < n) a.tap[(size_t)i * n + j] = NAN;
      }
    return;
  }
  const size_t first = seg.first;
  const uint32_t j = j0 + lane;
  const bool col = j < n;
  const float area_j = col ? a.area[first + j] : NAN;
  float s2[NM_WAVE_ROWS], sum[NM_WAVE_ROWS];
  uint32_t k[NM_WAVE_ROWS];
#pragma unroll
  for (uint32_t r = 0; r < NM_WAVE_ROWS; ++r) {
    const uint32_t i = i0 + wave * NM_WAVE_ROWS + r;
    s2[r] = sa_oks_scale(i < n ? a.area[first + i] : NAN, area_j);   // (a broadcast read: one address per wave)
    sum[r] = 0.f;
    k[r] = 0u;
  }
  for (uint32_t p0 = 0; p0 < a.P; p0 += NM_CHUNK) {
    const uint32_t cn = a.P - p0 < NM_CHUNK ? a.P - p0 : NM_CHUNK;
    if (p0) __syncthreads();   // the chunk before has been read
    for (uint32_t e = tid; e < NM_ROWS * cn; e += NM_THREADS) {   // 16 consecutive poses of one point: 128 consecutive bytes
      const uint32_t pp = e / NM_ROWS, r = e % NM_ROWS;
      s_z[pp][r] = i0 + r < n ? a.pts[(size_t)(p0 + pp) * a.total + first + i0 + r] : sa_xy{NAN, 0.f};
    }
    __syncthreads();
    for (uint32_t pp = 0; pp < cn; ++pp) {
      const sa_xy zj = col ? a.pts[(size_t)(p0 + pp) * a.total + first + j] : sa_xy{NAN, 0.f};   // 64 consecutive pieces per wave
      const float var2 = a.var2[p0 + pp];
#pragma unroll
      for (uint32_t r = 0; r < NM_WAVE_ROWS; ++r) sa_pose_nms_acc(sum[r], k[r], s_z[pp][wave * NM_WAVE_ROWS + r], zj, s2[r], var2);
    }
  }
#pragma unroll
  for (uint32_t r = 0; r < NM_WAVE_ROWS; ++r) {
    const uint32_t i = i0 + wave * NM_WAVE_ROWS + r;
    if (i >= n) break;   // (wave-uniform)
    const float w = sa_pose_nms_weight(sum[r], k[r], a.min_common, s2[r]);
    const bool pair = col && i < j;
    const unsigned long long bits = __ballot(pair && sa_pose_nms_suppresses(w, a.thr));
    if (lane == 0) mask[(size_t)i * W + blockIdx.x] = bits;
    if (TAP && col) a.tap[(size_t)i * n + j] = pair ? w : NAN;
  }
}

template <int SRC>
hipError_t launch_lay(const LayArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_pose_nms_lay<SRC>, dim3((a.total + LAY_THREADS - 1) / LAY_THREADS), dim3(LAY_THREADS), 0, st, a);
  return hipGetLastError();
}

// ---- the host ----------------------------------------------------------------------------------------------------------------------
struct NmsCall {
  const char* who;   // the entry point, as its refusals name it
  bool batch;        // refusals name the scene
  // the tap (one scene): the order and the matrix instead of the keeps
  uint32_t* out_order = nullptr;
  float* out_w = nullptr;
  uint32_t* out_m = nullptr;
};
std::string where(const NmsCall& c, uint32_t scene) { return c.batch ? std::string(c.who) + ": scene " + std::to_string(scene) : std::string(c.who); }

int check_options(sa_engine* e, const char* who, const sa_pose_nms_options* o) {
  if (!o) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null options", who);
  if (o->struct_size != sizeof(sa_pose_nms_options))
    return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: options.struct_size %u (%zu)", who, o->struct_size, sizeof(sa_pose_nms_options));
  if (o->points == 0) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: options.points must be at least 1", who);
  if (o->min_common == 0) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: options.min_common must be at least 1", who);
  if (o->n_sigmas != o->points) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: options.n_sigmas %u, but points is %u", who, o->n_sigmas, o->points);
  if (!o->sigmas) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null options.sigmas", who);
  for (uint32_t p = 0; p < o->points; ++p)
    if (!std::isfinite(o->sigmas[p]) || !(o->sigmas[p] > 0.f))
      return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: options.sigmas[%u] = %g is not finite and > 0", who, p, (double)o->sigmas[p]);
  return SA_OK;
}
// Every call: the refusals, the host half (sa_pose_nms_rank per scene), the plan, ONE upload, the launches, the copy back, ONE wait.
// A refused call leaves the outputs alone and the stats zeroed.
int nms_call(sa_engine* e, const NmsCall& c, const sa_pose_nms_options* o, uint32_t n_scenes, const uint32_t* counts, const sa_point_rows* poses,
             const float* scores, uint32_t* const* out_keep, uint32_t* out_n) {
  SaPoseNms*& slot = sa_engine_pose_nms(e);
  if (!slot) slot = new SaPoseNms();
  SaPoseNms* S = slot;
  S->last = sa_pose_nms_stats{};
  const bool tap = c.out_w != nullptr;
  SA_TRY(check_options(e, c.who, o));
  if (n_scenes > SA_FRAMES_MAX_SCENES)
    return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: at most %u scenes per call (got %u)", c.who, SA_FRAMES_MAX_SCENES, n_scenes);
  uint64_t m_all = 0;
  for (uint32_t s = 0; s < n_scenes; ++s) {
    if (counts[s] && !tap && !out_keep[s]) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null out_keep", where(c, s).c_str());
    m_all += counts[s];
  }
  if (m_all > 0xfffffffeull) return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: more than 2^32 - 2 poses in one call", c.who);
  if (m_all) {
    SA_TRY(sa_point_rows_check(e, c.who, o->points, m_all, poses, sa_engine_device(e), SaPointRowsWords{"poses", "poses", "this engine runs on"}));
    if (!scores) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null scores", c.who);
  }
  // the host half: per scene the poses that pass, in rank order, as indices into the scene
  std::vector<std::vector<uint32_t>> src(n_scenes);
  std::vector<uint32_t> kept(n_scenes), row0(n_scenes);
  uint32_t at = 0;
  for (uint32_t s = 0; s < n_scenes; ++s) {
    row0[s] = at;
    if (counts[s]) sa_pose_nms_rank(counts[s], scores + at, o->score_threshold, src[s]);
    kept[s] = (uint32_t)src[s].size();
    at += counts[s];
  }
  SaFramesPlan plan;
  uint32_t bad = 0;
  switch (sa_frames_plan(n_scenes, kept.data(), true, &plan, &bad)) {
    case SA_FRAMES_FITS: break;
    case SA_FRAMES_TOO_MANY_SCENES: return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: at most %u scenes per call (got %u)", c.who, SA_FRAMES_MAX_SCENES, n_scenes);
    case SA_FRAMES_SCENE_TOO_LARGE:
      return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: at most %u poses pass to the pair stage (got %u)", where(c, bad).c_str(), SA_POSE_NMS_MAX, kept[bad]);
    default: return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: more than 2^32 - 1 poses in one call", where(c, bad).c_str());
  }
  if (tap && plan.total > SA_POSE_NMS_TAP_MAX)
    return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: the tap takes at most %u poses that pass the filter (got %u)", c.who, SA_POSE_NMS_TAP_MAX, plan.total);
  sa_pose_nms_stats fs{};
  fs.scenes = n_scenes;
  fs.poses = plan.total;
  const uint32_t total = plan.total, P = o->points;
  if (!total) {
    if (tap) *c.out_m = 0;
    else
      for (uint32_t s = 0; s < n_scenes; ++s) out_n[s] = 0;
    S->last = fs;
    return SA_OK;
  }
  int device = 0;
  hipStream_t st = nullptr;
  SA_TRY(sa_engine_drain(e, &device, &st));
  for (auto& ev : S->ev)
    if (!ev) SA_HIPCHK(e, hipEventCreate(&ev));
  // ONE block: the segment table, the rank table, var2, the staged poses (a host source only), the present flags (a mask only)
  const sa_dev_rows* d = poses->dev;
  const uint32_t comps = poses->comps;
  const size_t seg_bytes = (size_t)n_scenes * sizeof(SaFrameSeg), rank_bytes = (size_t)total * 4, var_bytes = (size_t)P * 4;
  const size_t row_bytes = (size_t)P * comps * 4, pose_bytes = d ? 0 : (size_t)total * row_bytes;
  const size_t flag_bytes = poses->present ? (size_t)total * P : 0;
  const size_t o_rank = seg_bytes, o_var = o_rank + rank_bytes, o_pose = o_var + var_bytes, o_flag = o_pose + pose_bytes, up_bytes = o_flag + flag_bytes;
  std::vector<uint8_t> up(up_bytes);
  std::memcpy(up.data(), plan.segs.data(), seg_bytes);
  uint32_t* rank = (uint32_t*)(up.data() + o_rank);
  float* var2 = (float*)(up.data() + o_var);
  for (uint32_t p = 0; p < P; ++p) var2[p] = sa_oks_var2(o->sigmas[p]);
  uint64_t rows_read = 0;
  for (uint32_t s = 0; s < n_scenes; ++s)
    for (uint32_t i = 0; i < kept[s]; ++i) {
      const uint32_t t = plan.segs[s].first + i, r = row0[s] + src[s][i];   // r: the pose's place among the call's poses
      if (d) {
        rank[t] = d->index ? d->index[r] : r;   // (the caller's index composed; SA_ROW_NONE stays SA_ROW_NONE)
        rows_read += rank[t] != SA_ROW_NONE;
      } else {
        rank[t] = t;
        std::memcpy(up.data() + o_pose + (size_t)t * row_bytes, poses->host + (size_t)r * P * comps, row_bytes);
      }
      if (flag_bytes) std::memcpy(up.data() + o_flag + (size_t)t * P, poses->present + (size_t)r * P, P);
    }
  SA_TRY(sa_engine_ensure(e, S->d_up, up_bytes));
  SA_TRY(sa_engine_ensure(e, S->d_pts, (size_t)total * P * sizeof(sa_xy)));
  SA_TRY(sa_engine_ensure(e, S->d_area, (size_t)total * 4));
  SA_TRY(sa_engine_ensure(e, S->d_mask, (size_t)plan.mask_words * 8));
  if (tap) SA_TRY(sa_engine_ensure(e, S->d_tap, (size_t)total * total * 4));
  else SA_TRY(sa_engine_ensure(e, S->d_keep, total));
  const char* dup = (const char*)S->d_up.p;
  SA_HIPCHK(e, hipMemcpyAsync(S->d_up.p, up.data(), up_bytes, hipMemcpyHostToDevice, st));
  LayArgs la{};
  la.total = total, la.P = P;   // (the view by hand, out of the one block: sa_point_rows_stage uploads a caller's rows as they come)
  la.src = SaPointSrc{d ? (const char*)d->base : dup + o_pose, d ? d->row_stride : (uint64_t)P * comps, (const uint32_t*)(dup + o_rank),
                      flag_bytes ? (const uint8_t*)(dup + o_flag) : nullptr, comps, poses->min_score};
  la.pts = (sa_xy*)S->d_pts.p, la.area = (float*)S->d_area.p;
  MaskArgs ma{};
  ma.segs = (const SaFrameSeg*)dup, ma.pts = la.pts, ma.area = la.area, ma.var2 = (const float*)(dup + o_var);
  ma.mask = (uint64_t*)S->d_mask.p, ma.tap = tap ? (float*)S->d_tap.p : nullptr;
  ma.total = total, ma.P = P, ma.min_common = o->min_common, ma.thr = o->nms_threshold;
  const int32_t elem = d ? d->elem : SA_ELEM_F32;
  SA_HIPCHK(e, hipEventRecord(S->ev[0], st));
  SA_HIPCHK(e, sa_point_elem(elem, [&](auto src) { return launch_lay<decltype(src)::value>(la, st); }));
  const dim3 grid((plan.max_count + NM_COLS - 1) / NM_COLS, (plan.max_count + NM_ROWS - 1) / NM_ROWS, n_scenes);
  if (tap) hipLaunchKernelGGL(k_pose_nms_mask<true>, grid, dim3(NM_THREADS), 0, st, ma);
  else hipLaunchKernelGGL(k_pose_nms_mask<false>, grid, dim3(NM_THREADS), 0, st, ma);
  SA_HIPCHK(e, hipGetLastError());
  fs.launches = 2;
  std::vector<uint8_t> keep;
  if (tap) {
    SA_HIPCHK(e, hipEventRecord(S->ev[1], st));
    SA_HIPCHK(e, hipMemcpyAsync(c.out_w, S->d_tap.p, (size_t)total * total * 4, hipMemcpyDeviceToHost, st));
    fs.bytes_d2h = (uint64_t)total * total * 4;
  } else {
    SA_HIPCHK(e, sa_launch_nms_sweep(ma.mask, ma.segs, n_scenes, plan.sweep_S, (uint8_t*)S->d_keep.p, st, nullptr));
    fs.launches = 3;
    SA_HIPCHK(e, hipEventRecord(S->ev[1], st));
    keep.resize(total);
    SA_HIPCHK(e, hipMemcpyAsync(keep.data(), S->d_keep.p, total, hipMemcpyDeviceToHost, st));
    fs.bytes_d2h = total;
  }
  SA_HIPCHK(e, hipStreamSynchronize(st));
  fs.host_waits = 1;
  fs.bytes_h2d = up_bytes;
  fs.src_bytes = d ? rows_read * P * comps * sa_point_elem_size(elem) : 0;
  float ms = 0.f;
  SA_HIPCHK(e, hipEventElapsedTime(&ms, S->ev[0], S->ev[1]));
  fs.device_ms = ms;
  if (tap) {
    std::memcpy(c.out_order, src[0].data(), (size_t)total * 4);
    *c.out_m = total;
  } else
    for (uint32_t s = 0; s < n_scenes; ++s) {
      uint32_t k = 0;
      for (uint32_t i = 0; i < kept[s]; ++i)
        if (keep[plan.segs[s].first + i]) out_keep[s][k++] = src[s][i];
      out_n[s] = k;
    }
  S->last = fs;
  return SA_OK;
}

// a null argument of the entry point itself: refused like every other, the stats zeroed
int refuse_null(sa_engine* e, const char* who) {
  if (e)
    if (SaPoseNms* s = sa_engine_pose_nms(e)) s->last = sa_pose_nms_stats{};
  return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null argument", who);
}

}  // namespace

void sa_pose_nms_options_default(sa_pose_nms_options* o) {
  if (!o) return;
  *o = sa_pose_nms_options{};
  o->struct_size = (uint32_t)sizeof(sa_pose_nms_options);
  o->points = 17;
  o->min_common = 1;
  o->nms_threshold = 0.9f;
  o->score_threshold = NAN;
}

int sa_pose_nms(sa_engine* e, const sa_pose_nms_options* o, uint32_t m, const sa_point_rows* poses, const float* scores, uint32_t* out_keep,
                uint32_t* out_n) {
  if (!e || !out_n || (m && !out_keep)) return refuse_null(e, "sa_pose_nms");
  return nms_call(e, NmsCall{"sa_pose_nms", false}, o, 1, &m, poses, scores, &out_keep, out_n);
}

int sa_pose_nms_batch(sa_engine* e, const sa_pose_nms_options* o, uint32_t n_scenes, const uint32_t* counts, const sa_point_rows* poses,
                      const float* scores, uint32_t* const* out_keep, uint32_t* out_n) {
  if (!e || (n_scenes && (!counts || !out_keep || !out_n))) return refuse_null(e, "sa_pose_nms_batch");
  return nms_call(e, NmsCall{"sa_pose_nms_batch", true}, o, n_scenes, counts, poses, scores, out_keep, out_n);
}

int sa_pose_nms_matrix(sa_engine* e, const sa_pose_nms_options* o, uint32_t m, const sa_point_rows* poses, const float* scores,
                       uint32_t* out_order, float* out_w, uint32_t* out_m) {
  if (!e || !out_m || (m && (!out_order || !out_w))) return refuse_null(e, "sa_pose_nms_matrix");
  if (!m) {   // (no matrix to tell the tap by)
    float none = 0.f;
    uint32_t no_order = 0;
    NmsCall c{"sa_pose_nms_matrix", false, &no_order, &none, out_m};
    return nms_call(e, c, o, 1, &m, poses, scores, nullptr, nullptr);
  }
  NmsCall c{"sa_pose_nms_matrix", false, out_order, out_w, out_m};
  return nms_call(e, c, o, 1, &m, poses, scores, nullptr, nullptr);
}

int sa_pose_nms_last(sa_engine* e, sa_pose_nms_stats* out) {
  if (!e || !out) return sa_engine_fail(e, SA_ERR_BAD_ARG, "sa_pose_nms_last: null argument");
  const SaPoseNms* s = sa_engine_pose_nms(e);
  *out = s ? s->last : sa_pose_nms_stats{};
  out->struct_size = (uint32_t)sizeof(sa_pose_nms_stats);
  return SA_OK;
}
