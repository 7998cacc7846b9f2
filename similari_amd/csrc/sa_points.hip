// sa_points.hip — point banks (include/similari_points.h): the Kalman states of T tracks x P keypoints on the engine's device, stepped
// in one launch per call.
//
// The arithmetic is sa_kalman_point.h, shared with the host build of tests/emu_points.  What is here: the bank (a slot table like a
// store's: ids, slot_of; capacity doubles), the refusals, and two kernels.  k_points<SRC> runs every state-changing call and the
// distance, one thread per (track of the call, point): the thread reads its point — out of the staged host rows or out of the caller's
// device block through sa_point_at<SRC> (sa_point_rows.h: the one read of a point, shared with the vote and pose NMS) —, its state out
// of the planes, applies the call's operation and writes the state and the output back.  k_points_move is the compaction of a removal.
// The bank's struct and the checks every call runs first — enter, check_ids, check_rows — are in sa_points_impl.h, which the pose
// association (sa_pose.hip) shares; the check of the rows themselves (the struct, then sa_dev_rows_layout and sa_dev_rows_span of
// similari_devrows.h) and their staging (sa_point_rows_stage) are sa_point_rows.h.
//
// Layout.  Five planes of float4 over cap * P — the mean and the four covariance rows of point (slot, p) at [slot * P + p] — and one
// byte plane `has`: consecutive lanes work on consecutive points, so every plane access of a wave is 64 consecutive 16-byte pieces.
// No LDS.  Bit 31 of a slot-table entry marks a track the call created: its `has` bytes are taken as 0 and written, whatever the
// plane held, so growing the planes needs no clearing launch.
//
// Reference: src/utils/kalman/kalman_2d_point.rs, kalman_2d_point_vec.rs, src/trackers/kalman_prediction.rs:13-32.
#include "sa_points_impl.h"
#include "sa_kalman_point.h"

#include <cstring>

namespace {

using namespace sa_pt;   // enter, check_ids, check_rows, reserve, pt_load, pt_store: sa_points_impl.h, shared with sa_pose.hip

constexpr uint32_t PT_THREADS = 256;
constexpr uint32_t PT_FRESH = 0x80000000u;
enum PtOp : uint32_t { PT_INITIATE, PT_PREDICT, PT_UPDATE, PT_DISTANCE, PT_STEP };

struct PtArgs {
  uint32_t op, n, P, mode;
  float pw, vw;
  const uint32_t* slots;    // [n] the slot of each track of the call, PT_FRESH set on one the call created; nullptr: 0, 1, 2, ...
  SaPointSrc src;           // the points of the n tracks (sa_point_rows.h); base nullptr: the call has none (predict)
  float4* plane[5];
  uint8_t* has;
  float* out;               // [n][P][2] the mean's x, y, or [n][P] the distance; nullptr: none
  uint8_t* seen;            // [n][P] 1 where the point was present; nullptr: none
};

// One thread per (track i of the call, point p), t = i * P + p < n * P < 2^31.  Reads: slots[i], point p of item i (SaPointSrc: its
// bounds are stated there), has and — where there is a state — the five plane pieces at slot * P + p.  Writes: the planes and has
// where the state changed, out and seen at t.  Every address is bounded by what the host checked: slot < cap, t < n * P.
template <int SRC>
__global__ __launch_bounds__(PT_THREADS) void k_points(const PtArgs a) {
  const uint32_t t = blockIdx.x * PT_THREADS + threadIdx.x;
  if (t >= a.n * a.P) return;
  const uint32_t i = t / a.P, p = t - i * a.P;
  const uint32_t sw = a.slots ? a.slots[i] : i;
  const bool fresh = (sw & PT_FRESH) != 0;
  const size_t at = (size_t)(sw & ~PT_FRESH) * a.P + p;
  float2 z = make_float2(NAN, 0.f);
  if (a.src.base) z = sa_point_at<SRC>(a.src, i, a.P, p);
  const bool present = z.x == z.x;   // (the filter reads z under `present` only: sa_kalman_point.h)
  const float zx = z.x, zy = z.y;
  bool has = !fresh && a.has[at] != 0;
  sa_pkf s;
  if (has) pt_load(a, at, s);
  bool changed = false;
  float d = NAN;
  switch (a.op) {
    case PT_INITIATE:
      if (present) {
        sa_pkf_initiate(a.pw, a.vw, zx, zy, s);
        has = changed = true;
      }
      break;
    case PT_PREDICT:
      if (has) {
        sa_pkf_predict(a.pw, a.vw, s);
        changed = true;
      }
      break;
    case PT_UPDATE:
      if (has && present) {
        sa_pkf_update(a.pw, s, zx, zy);
        changed = true;
      }
      break;
    case PT_DISTANCE:
      if (has && present) {
        d = sa_pkf_distance(a.pw, s, zx, zy);
        if (a.mode != SA_POINT_D2) d = sa_pkf_cost(d, a.mode == SA_POINT_COST_INVERTED);
      }
      break;
    default:
      has = sa_pkf_step(a.pw, a.vw, has, s, present, zx, zy);
      changed = has;
      break;
  }
  if (changed) pt_store(a, at, s);
  if (changed || fresh) a.has[at] = has ? 1 : 0;
  if (a.seen) a.seen[t] = present ? 1 : 0;
  if (a.out) {
    if (a.op == PT_DISTANCE) a.out[t] = d;
    else ((float2*)a.out)[t] = has ? make_float2(s.mean[0], s.mean[1]) : make_float2(NAN, NAN);
  }
}

// The compaction of a removal: move m takes the state of track moves[m].x into slot moves[m].y; sources lie at or behind the new end
// of the table, destinations in front of it, so no move reads what another writes.  One thread per (move, point).
struct PtMoveArgs {
  const uint2* moves;
  uint32_t n, P;
  float4* plane[5];
  uint8_t* has;
};
__global__ __launch_bounds__(PT_THREADS) void k_points_move(const PtMoveArgs a) {
  const uint32_t t = blockIdx.x * PT_THREADS + threadIdx.x;
  if (t >= a.n * a.P) return;
  const uint32_t m = t / a.P, p = t - m * a.P;
  const uint2 mv = a.moves[m];
  const size_t from = (size_t)mv.x * a.P + p, to = (size_t)mv.y * a.P + p;
  for (int k = 0; k < 5; ++k) a.plane[k][to] = a.plane[k][from];
  a.has[to] = a.has[from];
}

// The final states of the tracks that leave, ahead of the compaction: thread (k, p) copies point p of slot slots[k] into the staging
// block — mean [n][P] and cov [n][P][4] as float4, has [n][P] as bytes: per track the layout sa_points_get_state returns.  slots[k] <
// the bank's tracks <= cap (the host's table), t < n * P.
struct PtGatherArgs {
  const uint32_t* slots;
  uint32_t n, P;
  const float4* plane[5];
  const uint8_t* has;
  float4 *mean, *cov;
  uint8_t* out_has;
};
__global__ __launch_bounds__(PT_THREADS) void k_points_gather(const PtGatherArgs a) {
  const uint32_t t = blockIdx.x * PT_THREADS + threadIdx.x;
  if (t >= a.n * a.P) return;
  const uint32_t k = t / a.P, p = t - k * a.P;
  const size_t at = (size_t)a.slots[k] * a.P + p;
  a.mean[t] = a.plane[0][at];
  for (int r = 0; r < 4; ++r) a.cov[(size_t)t * 4 + r] = a.plane[1 + r][at];
  a.out_has[t] = a.has[at] ? 1 : 0;
}

void release(sa_points* b) {
  for (DevBuf& d : b->plane) sa_engine_free(d);
  for (DevBuf* d : {&b->has, &b->d_slots, &b->d_index, &b->d_pts, &b->d_mask, &b->d_out, &b->d_seen, &b->d_moves, &b->d_fac4, &b->d_fac1, &b->d_gain,
                    &b->d_tap, &b->d_best, &b->d_res, &b->d_segs, &b->d_trk, &b->d_circ, &b->d_limit, &b->d_leave, &b->d_stage, &b->d_var2, &b->d_area})
    sa_engine_free(*d);
  for (auto& ev : b->ev)
    if (ev) { hipEventDestroy(ev); ev = nullptr; }
  for (auto& ev : b->pev)
    if (ev) { hipEventDestroy(ev); ev = nullptr; }
  for (auto& ev : b->tev)
    if (ev) { hipEventDestroy(ev); ev = nullptr; }
  for (auto& ev : b->gev)
    if (ev) { hipEventDestroy(ev); ev = nullptr; }
}

hipError_t launch(const PtArgs& a, int32_t elem, hipStream_t st) {
  const dim3 grid((uint32_t)(((uint64_t)a.n * a.P + PT_THREADS - 1) / PT_THREADS)), block(PT_THREADS);
  sa_point_elem(elem, [&](auto src) { hipLaunchKernelGGL(k_points<decltype(src)::value>, grid, block, 0, st, a); });
  return hipGetLastError();
}

// Everything behind a call's refusals: the uploads, the ONE launch, the copies out, the wait, the stats.  slots: [n] as the kernel
// takes them, or empty (0, 1, 2, ...).
int run(sa_points* b, uint32_t op, uint32_t n, const std::vector<uint32_t>& slots, const sa_point_rows* rows, uint32_t mode, float* out) {
  sa_engine* e = b->e;
  hipStream_t st = b->st;
  const uint64_t np = (uint64_t)n * b->P;
  const uint32_t out_floats = op == PT_DISTANCE ? 1u : 2u;
  sa_points_stats s{};
  PtArgs a{};
  a.op = op, a.n = n, a.P = b->P, a.mode = mode, a.pw = b->pw, a.vw = b->vw;
  int32_t elem = SA_ELEM_F32;
  if (!slots.empty()) {
    SA_TRY(sa_engine_ensure(e, b->d_slots, (size_t)n * 4));
    SA_HIPCHK(e, hipMemcpyAsync(b->d_slots.p, slots.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    s.bytes_h2d += (uint64_t)n * 4;
    a.slots = (const uint32_t*)b->d_slots.p;
  }
  if (rows) SA_TRY(sa_point_rows_stage(e, st, b->P, n, rows, b->d_pts, b->d_index, b->d_mask, a.src, elem, s.bytes_h2d, s.src_bytes));
  if (out) {
    SA_TRY(sa_engine_ensure(e, b->d_out, (size_t)np * out_floats * 4));
    a.out = (float*)b->d_out.p;
  }
  if (rows) {
    SA_TRY(sa_engine_ensure(e, b->d_seen, (size_t)np));
    a.seen = (uint8_t*)b->d_seen.p;
  }
  for (int k = 0; k < 5; ++k) a.plane[k] = (float4*)b->plane[k].p;
  a.has = (uint8_t*)b->has.p;
  SA_HIPCHK(e, hipEventRecord(b->ev[0], st));
  SA_HIPCHK(e, launch(a, elem, st));
  SA_HIPCHK(e, hipEventRecord(b->ev[1], st));
  std::vector<uint8_t> seen;
  if (out) {
    SA_HIPCHK(e, hipMemcpyAsync(out, b->d_out.p, (size_t)np * out_floats * 4, hipMemcpyDeviceToHost, st));
    s.bytes_d2h += np * out_floats * 4;
  }
  if (rows) {
    seen.resize((size_t)np);
    SA_HIPCHK(e, hipMemcpyAsync(seen.data(), b->d_seen.p, (size_t)np, hipMemcpyDeviceToHost, st));
    s.bytes_d2h += np;
  }
  SA_HIPCHK(e, hipStreamSynchronize(st));
  float ms = 0.f;
  SA_HIPCHK(e, hipEventElapsedTime(&ms, b->ev[0], b->ev[1]));
  s.tracks = n, s.launches = 1, s.capacity = b->cap, s.points = np, s.device_ms = ms;
  for (uint8_t v : seen) s.present += v;
  b->last = s;
  return SA_OK;
}

// A call on known or new tracks with points: initiate and step create unknown ids, update and distance refuse them.
int call(sa_points* b, const char* what, uint32_t op, uint32_t n, const uint64_t* ids, const sa_point_rows* rows, uint32_t mode, float* out) {
  if (!b) return SA_ERR_BAD_ARG;
  SA_TRY(enter(b, what));
  b->last = sa_points_stats{};
  const bool creates = op == PT_INITIATE || op == PT_STEP;
  if (op == PT_DISTANCE && mode > SA_POINT_COST_INVERTED) return sa_engine_fail(b->e, SA_ERR_BAD_ARG, "%s: unknown mode %u", what, mode);
  if (n == 0) return SA_OK;
  if (!ids || (op == PT_DISTANCE && !out)) return sa_engine_fail(b->e, SA_ERR_BAD_ARG, "%s: null argument", what);
  if (op != PT_PREDICT) SA_TRY(check_rows(b, what, n, rows));
  std::vector<uint32_t> slots;
  SA_TRY(check_ids(b, what, n, ids, !creates, slots));
  const uint64_t fresh = (uint64_t)std::count(slots.begin(), slots.end(), SA_SEARCH_NONE), T1 = b->T + fresh;
  if (T1 * b->P >= 0x80000000ull) return sa_engine_fail(b->e, SA_ERR_UNSUPPORTED, "%s: %llu tracks x %u points reach 2^31", what, (unsigned long long)T1, b->P);
  SA_TRY(reserve(b, T1));
  for (uint32_t i = 0; i < n; ++i)
    if (slots[i] == SA_SEARCH_NONE) {
      slots[i] = b->T++ | PT_FRESH;
      b->ids.push_back(ids[i]);
      b->slot_of.emplace(ids[i], slots[i] & ~PT_FRESH);
    }
  const int rc = run(b, op, n, slots, rows, mode, out);
  if (rc != SA_OK) b->broken = true;
  return rc;
}

}  // namespace

namespace sa_pt {

int sort_remove(sa_points* b, const std::vector<uint32_t>& leaving, const std::vector<uint32_t>& what_is, uint8_t* stage, PoseRan& r) {
  sa_engine* e = b->e;
  hipStream_t st = b->st;
  const uint32_t n = (uint32_t)leaving.size(), T1 = (uint32_t)what_is.size(), P = b->P;
  if (n == 0) return SA_OK;
  SA_TRY(make_events(b, b->gev));
  const size_t np = (size_t)n * P;
  std::vector<uint2> moves;
  for (uint32_t s = 0; s < T1; ++s)
    if (what_is[s] != s) moves.push_back(make_uint2(what_is[s], s));
  SA_TRY(sa_engine_ensure(e, b->d_leave, (size_t)n * 4));
  SA_TRY(sa_engine_ensure(e, b->d_stage, np * 81));
  if (!moves.empty()) SA_TRY(sa_engine_ensure(e, b->d_moves, moves.size() * sizeof(uint2)));
  // the table: the leaving ids go, every moved track is found at its new slot
  for (uint32_t s : leaving) b->slot_of.erase(b->ids[s]);
  std::vector<uint64_t> ids(T1);
  for (uint32_t s = 0; s < T1; ++s) {
    ids[s] = b->ids[what_is[s]];
    if (what_is[s] != s) b->slot_of[ids[s]] = s;
  }
  b->ids.swap(ids);
  b->T = T1;
  b->broken = true;   // until everything is queued: the table has changed
  SA_HIPCHK(e, hipMemcpyAsync(b->d_leave.p, leaving.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  r.bytes_h2d += (uint64_t)n * 4;
  PtGatherArgs g{};
  g.slots = (const uint32_t*)b->d_leave.p, g.n = n, g.P = P, g.has = (const uint8_t*)b->has.p;
  for (int k = 0; k < 5; ++k) g.plane[k] = (const float4*)b->plane[k].p;
  g.mean = (float4*)b->d_stage.p, g.cov = g.mean + np, g.out_has = (uint8_t*)(g.cov + np * 4);
  SA_HIPCHK(e, hipEventRecord(b->gev[2], st));
  hipLaunchKernelGGL(k_points_gather, dim3((uint32_t)((np + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0, st, g);
  SA_HIPCHK(e, hipGetLastError());
  SA_HIPCHK(e, hipEventRecord(b->gev[3], st));
  if (!moves.empty()) {
    SA_HIPCHK(e, hipMemcpyAsync(b->d_moves.p, moves.data(), moves.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
    r.bytes_h2d += moves.size() * sizeof(uint2);
    PtMoveArgs a{};
    a.moves = (const uint2*)b->d_moves.p, a.n = (uint32_t)moves.size(), a.P = P, a.has = (uint8_t*)b->has.p;
    for (int k = 0; k < 5; ++k) a.plane[k] = (float4*)b->plane[k].p;
    hipLaunchKernelGGL(k_points_move, dim3((uint32_t)(((uint64_t)a.n * P + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0, st, a);
    SA_HIPCHK(e, hipGetLastError());
  }
  SA_HIPCHK(e, hipMemcpyAsync(stage, b->d_stage.p, np * 81, hipMemcpyDeviceToHost, st));
  r.bytes_d2h += np * 81;
  b->broken = false;
  return SA_OK;
}

int sort_remove_ms(sa_points* b, double* ms) {
  float f = 0.f;
  SA_HIPCHK(b->e, hipEventElapsedTime(&f, b->gev[2], b->gev[3]));
  *ms = f;
  return SA_OK;
}

}  // namespace sa_pt

// sa_engine_destroy: the engine goes first — free what the bank holds on its device, refuse every later call
void sa_points_orphan(sa_points* b) {
  release(b);
  b->e = nullptr;
}

extern "C" {

void sa_points_options_default(sa_points_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof *o);
  o->struct_size = sizeof *o;
  o->points = 17;
  o->position_weight = 1.0f / 20.0f;
  o->velocity_weight = 1.0f / 160.0f;
}

int sa_points_create(sa_engine* e, const sa_points_options* o, sa_points** out) {
  const char* what = "sa_points_create";
  if (out) *out = nullptr;
  if (!e) {
    // no engine: without a gfx950 device there cannot be one — say so, as sa_store_create does
    int count = 0;
    const hipError_t h = hipGetDeviceCount(&count);
    if (h != hipSuccess || count <= 0) {
      (void)hipGetLastError();
      return sa_engine_fail(nullptr, SA_ERR_NO_DEVICE, "no HIP device visible; the point bank has no CPU fallback");
    }
    bool gfx950 = false;
    for (int d = 0; d < count && !gfx950; ++d) {
      hipDeviceProp_t prop;
      gfx950 = hipGetDeviceProperties(&prop, d) == hipSuccess && std::strstr(prop.gcnArchName, "gfx950");
    }
    if (!gfx950) return sa_engine_fail(nullptr, SA_ERR_NO_DEVICE, "no gfx950 device; the point bank has no CPU fallback");
    return sa_engine_fail(nullptr, SA_ERR_BAD_ARG, "%s: null engine", what);
  }
  if (!o || !out) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
  if (o->struct_size != sizeof(sa_points_options)) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: struct_size %u (%zu)", what, o->struct_size, sizeof(sa_points_options));
  if (o->points == 0) return sa_engine_fail(e, SA_ERR_BAD_ARG, "%s: points must be >= 1", what);
  if (o->points >= 0x80000000u) return sa_engine_fail(e, SA_ERR_UNSUPPORTED, "%s: %u points reach 2^31", what, o->points);
  sa_points* b = new sa_points();
  b->e = e;
  const int rc = sa_engine_drain(e, &b->device, &b->st);
  if (rc != SA_OK) { delete b; return rc; }
  b->P = o->points;
  b->pw = o->position_weight;
  b->vw = o->velocity_weight;
  for (auto& ev : b->ev)
    if (hipEventCreate(&ev) != hipSuccess) {
      (void)hipGetLastError();
      release(b);
      delete b;
      return sa_engine_fail(e, SA_ERR_HIP, "%s: hipEventCreate failed", what);
    }
  sa_engine_attach_points(e, b);
  *out = b;
  return SA_OK;
}

void sa_points_destroy(sa_points* b) {
  if (!b) return;
  if (b->e) {
    hipSetDevice(b->device);
    if (b->st) hipStreamSynchronize(b->st);
    release(b);
    sa_engine_detach_points(b->e, b);
  }
  delete b;
}

int sa_points_initiate(sa_points* b, uint32_t n, const uint64_t* ids, const sa_point_rows* rows) {
  return call(b, "sa_points_initiate", PT_INITIATE, n, ids, rows, 0, nullptr);
}

int sa_points_predict(sa_points* b, uint32_t n, const uint64_t* ids, float* out_xy) {
  if (ids) return call(b, "sa_points_predict", PT_PREDICT, n, ids, nullptr, 0, out_xy);
  if (!b) return SA_ERR_BAD_ARG;
  SA_TRY(enter(b, "sa_points_predict"));
  b->last = sa_points_stats{};
  if (!b->T) return SA_OK;
  const int rc = run(b, PT_PREDICT, b->T, {}, nullptr, 0, out_xy);
  if (rc != SA_OK) b->broken = true;
  return rc;
}

int sa_points_update(sa_points* b, uint32_t n, const uint64_t* ids, const sa_point_rows* rows, float* out_xy) {
  return call(b, "sa_points_update", PT_UPDATE, n, ids, rows, 0, out_xy);
}

int sa_points_distance(sa_points* b, uint32_t n, const uint64_t* ids, const sa_point_rows* rows, uint32_t mode, float* out) {
  return call(b, "sa_points_distance", PT_DISTANCE, n, ids, rows, mode, out);
}

int sa_points_step(sa_points* b, uint32_t n, const uint64_t* ids, const sa_point_rows* rows, float* out_xy) {
  return call(b, "sa_points_step", PT_STEP, n, ids, rows, 0, out_xy);
}

int sa_points_remove(sa_points* b, uint32_t n, const uint64_t* ids) {
  const char* what = "sa_points_remove";
  if (!b) return SA_ERR_BAD_ARG;
  SA_TRY(enter(b, what));
  b->last = sa_points_stats{};
  if (n == 0) return SA_OK;
  if (!ids) return sa_engine_fail(b->e, SA_ERR_BAD_ARG, "%s: null ids", what);
  std::vector<uint32_t> slots;
  SA_TRY(check_ids(b, what, n, ids, false, slots));
  // The last track moves into each hole in turn, in call order; what_is[s]: the slot, as the planes hold it now, whose state ends in s.
  std::vector<uint32_t> what_is(b->T);
  for (uint32_t s = 0; s < b->T; ++s) what_is[s] = s;
  const uint32_t T0 = b->T;
  for (uint32_t i = 0; i < n; ++i) {
    const auto it = b->slot_of.find(ids[i]);
    if (it == b->slot_of.end()) continue;
    const uint32_t hole = it->second, last = b->T - 1;
    b->slot_of.erase(it);
    if (hole != last) {
      b->ids[hole] = b->ids[last];
      b->slot_of[b->ids[hole]] = hole;
      what_is[hole] = what_is[last];
    }
    b->ids.pop_back();
    --b->T;
  }
  std::vector<uint2> moves;
  for (uint32_t s = 0; s < b->T; ++s)
    if (what_is[s] != s) moves.push_back(make_uint2(what_is[s], s));
  if (b->T == T0) return SA_OK;
  sa_points_stats s{};
  s.tracks = T0 - b->T, s.capacity = b->cap;
  if (!moves.empty()) {
    const int rc = [&]() -> int {
      sa_engine* e = b->e;
      SA_TRY(sa_engine_ensure(e, b->d_moves, moves.size() * sizeof(uint2)));
      SA_HIPCHK(e, hipMemcpyAsync(b->d_moves.p, moves.data(), moves.size() * sizeof(uint2), hipMemcpyHostToDevice, b->st));
      PtMoveArgs a{};
      a.moves = (const uint2*)b->d_moves.p, a.n = (uint32_t)moves.size(), a.P = b->P, a.has = (uint8_t*)b->has.p;
      for (int k = 0; k < 5; ++k) a.plane[k] = (float4*)b->plane[k].p;
      SA_HIPCHK(e, hipEventRecord(b->ev[0], b->st));
      hipLaunchKernelGGL(k_points_move, dim3((uint32_t)(((uint64_t)a.n * a.P + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0, b->st, a);
      SA_HIPCHK(e, hipGetLastError());
      SA_HIPCHK(e, hipEventRecord(b->ev[1], b->st));
      SA_HIPCHK(e, hipStreamSynchronize(b->st));
      float ms = 0.f;
      SA_HIPCHK(e, hipEventElapsedTime(&ms, b->ev[0], b->ev[1]));
      s.device_ms = ms;
      return SA_OK;
    }();
    if (rc != SA_OK) {
      b->broken = true;
      return rc;
    }
    s.launches = 1;
    s.bytes_h2d = moves.size() * sizeof(uint2);
    s.points = (uint64_t)moves.size() * b->P;
  }
  b->last = s;
  return SA_OK;
}

int sa_points_count(sa_points* b, uint32_t* out_n) {
  if (!b || !out_n) return SA_ERR_BAD_ARG;
  if (!b->e || b->broken) return enter(b, "sa_points_count");
  *out_n = b->T;
  return SA_OK;
}

int sa_points_order(sa_points* b, uint64_t* out_ids, uint32_t cap, uint32_t* out_n) {
  if (!b || !out_n) return SA_ERR_BAD_ARG;
  if (!b->e || b->broken) return enter(b, "sa_points_order");
  *out_n = b->T;
  if (out_ids) std::memcpy(out_ids, b->ids.data(), (size_t)(cap < b->T ? cap : b->T) * 8);
  return SA_OK;
}

int sa_points_get_state(sa_points* b, uint64_t id, uint8_t* has, float* mean, float* cov) {
  const char* what = "sa_points_get_state";
  if (!b) return SA_ERR_BAD_ARG;
  SA_TRY(enter(b, what));
  if (!has || !mean || !cov) return sa_engine_fail(b->e, SA_ERR_BAD_ARG, "%s: null argument", what);
  if (id == 0) return sa_engine_fail(b->e, SA_ERR_BAD_ARG, "%s: id 0", what);
  const auto it = b->slot_of.find(id);
  if (it == b->slot_of.end()) return sa_engine_fail(b->e, SA_ERR_NOT_FOUND, "%s: unknown track id %llu", what, (unsigned long long)id);
  const size_t at = (size_t)it->second * b->P;
  SA_HIPCHK(b->e, hipMemcpyAsync(has, (const uint8_t*)b->has.p + at, b->P, hipMemcpyDeviceToHost, b->st));
  SA_HIPCHK(b->e, hipMemcpyAsync(mean, (const float4*)b->plane[0].p + at, (size_t)b->P * 16, hipMemcpyDeviceToHost, b->st));
  std::vector<float> rows((size_t)b->P * 16);
  for (int r = 0; r < 4; ++r)
    SA_HIPCHK(b->e, hipMemcpyAsync(rows.data() + (size_t)r * b->P * 4, (const float4*)b->plane[1 + r].p + at, (size_t)b->P * 16, hipMemcpyDeviceToHost, b->st));
  SA_HIPCHK(b->e, hipStreamSynchronize(b->st));
  for (uint32_t p = 0; p < b->P; ++p) {
    has[p] = has[p] ? 1 : 0;
    for (int r = 0; r < 4; ++r) std::memcpy(cov + (size_t)p * 16 + r * 4, rows.data() + ((size_t)r * b->P + p) * 4, 16);
    if (!has[p]) {
      for (int k = 0; k < 4; ++k) mean[(size_t)p * 4 + k] = NAN;
      for (int k = 0; k < 16; ++k) cov[(size_t)p * 16 + k] = NAN;
    }
  }
  return SA_OK;
}

int sa_points_set_state(sa_points* b, uint64_t id, const uint8_t* has, const float* mean, const float* cov) {
  const char* what = "sa_points_set_state";
  if (!b) return SA_ERR_BAD_ARG;
  SA_TRY(enter(b, what));
  if (!has || !mean || !cov) return sa_engine_fail(b->e, SA_ERR_BAD_ARG, "%s: null argument", what);
  if (id == 0) return sa_engine_fail(b->e, SA_ERR_BAD_ARG, "%s: id 0", what);
  const auto it = b->slot_of.find(id);
  if (it == b->slot_of.end()) return sa_engine_fail(b->e, SA_ERR_NOT_FOUND, "%s: unknown track id %llu", what, (unsigned long long)id);
  const size_t at = (size_t)it->second * b->P;
  std::vector<uint8_t> h(b->P);
  std::vector<float> m((size_t)b->P * 4, 0.f), rows((size_t)b->P * 16, 0.f);
  for (uint32_t p = 0; p < b->P; ++p) {
    h[p] = has[p] ? 1 : 0;
    if (!h[p]) continue;
    std::memcpy(m.data() + (size_t)p * 4, mean + (size_t)p * 4, 16);
    for (int r = 0; r < 4; ++r) std::memcpy(rows.data() + ((size_t)r * b->P + p) * 4, cov + (size_t)p * 16 + r * 4, 16);
  }
  const int rc = [&]() -> int {
    SA_HIPCHK(b->e, hipMemcpyAsync((uint8_t*)b->has.p + at, h.data(), b->P, hipMemcpyHostToDevice, b->st));
    SA_HIPCHK(b->e, hipMemcpyAsync((float4*)b->plane[0].p + at, m.data(), (size_t)b->P * 16, hipMemcpyHostToDevice, b->st));
    for (int r = 0; r < 4; ++r)
      SA_HIPCHK(b->e, hipMemcpyAsync((float4*)b->plane[1 + r].p + at, rows.data() + (size_t)r * b->P * 4, (size_t)b->P * 16, hipMemcpyHostToDevice, b->st));
    SA_HIPCHK(b->e, hipStreamSynchronize(b->st));
    return SA_OK;
  }();
  if (rc != SA_OK) b->broken = true;
  return rc;
}

int sa_points_last(sa_points* b, sa_points_stats* out) {
  if (!b || !out) return SA_ERR_BAD_ARG;
  *out = b->last;
  out->struct_size = sizeof *out;
  return SA_OK;
}

}  // extern "C"
