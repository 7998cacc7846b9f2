// sa_engine.hip — host side of the C ABI (include/similari_assoc.h): device-resident track tables per
// scene, per-batch staging, the kernel pipeline, parity taps and hipEvent timing.  No CPU compute path:
// without a gfx950 device sa_engine_create fails with SA_ERR_NO_DEVICE.
#include "sa_engine.h"
#include "sa_framerows.h"
#include "sa_frames_plan.h"
#include "sa_kalman.h"
#include "sa_slot_out.h"
#include "../../include/similari_frames.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <mutex>
#include <vector>

namespace {

thread_local std::string g_create_error;

enum KernelId {
  KID_FRAME = 0, KID_FRAME_VISUAL, KID_VISUAL, KID_BESTFIT_TILE, KID_BESTFIT_RESOLVE, KID_ASSIGN_SMALL,
  KID_ASSIGN_LABEL, KID_ASSIGN_SOLVE, KID_D2H, KID_WIDEN, KID_COUNT
};
const char* kKernelNames[KID_COUNT] = {
    "k_frame", "k_frame_visual", "k_visual_cost", "k_bestfit_tile", "k_bestfit_resolve", "k_assign_small",
    "k_assign_label", "k_assign_solve", "d2h_results", "k_widen_rows"};

struct HostBuf {  // pinned
  void* p = nullptr;
  size_t cap = 0;
};

struct alignas(128) SceneTable {   // (aligned: the tracker facade works on different scenes from different threads, sa_tracks_apply_collect_slot)
  uint64_t scene_id = 0;
  uint32_t T = 0, cap = 0;
  std::vector<uint64_t> ids;                       // slot -> id
  // id -> slot.  A caller that hands out increasing ids (gen_track_id: every tracker of the reference) keeps `ids` ascending, and the
  // lookup is a binary search; the hash map exists only for tables whose ids arrived out of order (built on first use, kept in step
  // afterwards) — so appending a row or compacting the table does not touch a hash map at all.
  bool ascending = true;
  bool map_built = false;
  std::unordered_map<uint64_t, uint32_t> slot_of;
  DevBuf spare[SA_TABLE_ARRAYS];                   // sa_tracks_remove compacts the table into these and swaps (no allocation per call)
  HostBuf h_index;                                 // ... the kept rows' old indices (mapped pinned memory the gather kernel reads in place)
  void* d_index = nullptr;
  uint64_t in_set[4] = {0, 0, 0, 0};               // per bank: stamp of the request set of THAT bank the scene was last added to (bank_add) — a scene
                                                   // staged into another bank in between must not hide a duplicate in this one
  bool staged = false;                             // sa_tracks_remove_stage has filled h_index; sa_tracks_remove_commit queues the gather
  uint32_t staged_rows = 0;                        // ... rows that stay
  uint64_t index_drain = ~0ull;                    // sa_engine::drain_count when the last gather that reads h_index was queued (~0: none): the
                                                   // buffer may be rewritten once the engine has been drained since
  DevBuf geo, ext, verts, epoch, maha, feat, fnorm, fpresent, fcount, tids;
  DevBuf ffrag;                    // the feature bank once more, in FRAGMENT order (sa_frag_index): every kernel that writes rows of `feat`
                                   // writes this twin too; the k-split contraction's wave-loads read it
  DevBuf kf, fquality;             // device-side upkeep: Kalman mean(10) + cov(100) per track, feature quality per bank slot
  std::vector<uint8_t> full;       // slot -> the device holds a full Kalman state for it (sa_tracks_apply / sa_tracks_set_state)
  uint32_t eu_valu_left = 0;       // euclidean engines: frames of THIS scene still to run on the vector-pipe kernel after one of its frames
                                   // reported itself ill-conditioned for the matrix-core expansion (sa_config.euclid_backoff_frames)
  uint32_t pos_left = 0;           // VisualSORT: rows without a visual group in THIS scene's newest collected frame (out_stats[2]) — the hint
                                   // that picks the next frame's positional mode (sa_lazy_positional); 0 until a frame has reported
};

struct alignas(128) Slot {  // one scene of a request set (aligned: see SceneTable)
  SceneTable* scene = nullptr;
  uint64_t epoch = 0;
  uint32_t N = 0, T = 0;
  int has_feats = 0, has_quality = 0, has_own = 0, has_fpresent = 0;
  // raw inputs: offsets of this scene's block inside the bank's staging arena (raw | quality | own | fpresent | features) and, once
  // the arena is on the device, the device addresses
  size_t o_raw = 0, o_q = 0, o_own = 0, o_fp = 0, o_feat = 0;
  const float* feats_inplace = nullptr;  // the caller's features lie in a pinned block (sa_host_alloc): DMA'd from there into feat_raw
  const float* feats_inplace_dev = nullptr;  // the same rows through the block's device mapping (the ingest kernel reads them)
  const float* feats_device = nullptr;   // the caller's features lie in DEVICE memory (sa_device_block_register): read where they are
                                         // when 16-byte aligned, else copied device-to-device into feat_raw
  void *p_raw = nullptr, *p_quality = nullptr, *p_own = nullptr, *p_fpresent = nullptr, *p_feat_raw = nullptr;
  DevBuf feat_raw;                        // destination of an in-place feature upload
  // include/similari_framerows.h: the scene was added by a *_dev call (rows_dev); rows_widen: its features are gathered and widened out of
  // the caller's device memory into feat_raw by the upload's widen launch (every source but the one today's pointer route reads in place)
  bool rows_dev = false, rows_widen = false;
  sa_dev_rows rows{};                     // ... the descriptor (its index has been consumed: the row table lies in the arena at o_rows)
  size_t o_rows = 0;                      // u32[N] source row per detection, SA_ROW_NONE = no feature
  uint32_t rows_present = 0;              // detections with a feature
  // derived candidates
  DevBuf geo, verts, z, conf, usable, feat, fnorm;
  // matrices + vote + assignment state
  DevBuf pos, vis, quant;
  DevBuf vis_max_key, row_part_w, row_part_t, col_part_w, col_part_q, row_has, vis_winner, col_excluded, vote_best;
  DevBuf parent, label, next_row, e_cnt, e_use, e_edge, u, u_use, v, rmatch, cmatch, dist, pred, cstamp, cscan, cnext, rdist, rnext;
  DevBuf win_col;                              // device-side upkeep: the winners as table columns
  DevBuf lab, crow, cwin, big_rows, big_bcol, dq, dense;  // general tail: component labels, the dense solver's queue and lists; both tails: its matrix
  DevBuf stats;                                // [4] words raised by the first phase, moved to h_out and re-armed by the tail
  DevBuf tap;                                  // SA_FLAG_TAP: row words [n] | column words [t] | edge counts [n], written by the assignment tail
  HostBuf h_apply, h_pred, h_fix;
  void *d_pred = nullptr, *d_apply = nullptr, *d_fix = nullptr;  // device views of the three
  HostBuf h_out;    // ids[N] then votes[N]: mapped pinned memory the finalisation writes directly (no D2H copy)
  void* d_out = nullptr;  // device view of h_out
  size_t done_off = 0;    // where the slot's completion word lies in h_out (slot_reserve)
  bool table_collected = false;   // sa_tracks_apply_collect_table has done the host side of the scene's table for the queued upkeep step
  int table_bad = 0;              // ... and what it found (SA_OK or the error the collect reports)
  uint32_t N_res = 0, T_res = 0;  // extents the slot's buffers are reserved for (slot_reserve)
  uint32_t vb_n = 0, vb_t = 0;  // rows / columns the vote-word block (vote_best) is laid out for: row words | column words | row class words | column class words
  bool ran = false;
  bool reports_left = false;   // the slot's last frame ran the tail that writes its leftover rows into out_stats[2] (k_assign_small, vote words, TC = 1)
  bool poly_pending = false;   // sa_tracks_apply_collect_slot has run: the polygons of refreshed ORIENTED rows are still to be queued (sa_tracks_apply_collect_end)
  bool fused_pending = false;  // sa_batch_run_apply has queued the upkeep of this slot behind its association; sa_tracks_apply_collect finishes the host side
  uint64_t fused_id_base = 0;  // ... ids of the tracks that start: fused_id_base + 1 + (per candidate ? candidate index : rank among the new ones)
  int fused_per_candidate = 0;
  uint32_t fused_T0 = 0;       // rows of the scene's table when the upkeep was queued
  bool apply_pending = false;  // sa_tracks_apply_begin has queued the upkeep of this slot; sa_tracks_apply_end (or the next entry point that needs the table) finishes it
  bool fill_pending = false;   // sa_batch_add_deferred laid the slot out; sa_batch_fill (any thread) has yet to copy the caller's arrays in
  sa_detections pend_d{};      // ... the caller's arrays
  const float* const* pend_rows = nullptr;
  bool prepped = true;     // the frame-preparation blocks ran with the frame (false: a lean frame left them out; ensure_prepped runs them on demand)
  bool needs_init = true;  // e_cnt / u / parent were (re)allocated, or a run may have died half-way: k_slot_init before the next frame
};

// What a captured frame was recorded for: its plan, the geometry the plan does not hold, the descriptors it reads (compared bytewise)
struct GraphKey { SaFramePlan plan; uint32_t ns, maxN, maxT, tile_bm, tile_bn, feats_mask; const void* ds; };

// One request set (the scenes of one sa_associate_batch / one pipelined ticket) and everything that has to exist once per set in
// flight.  The engine owns SA_BANKS of them: the synchronous entry points work on the current one; the pipelined entry points
// (sa_pipe_*) rotate through them, so that the H2D copies of set n+1 (copy stream) overlap the kernels of set n (compute stream) and
// the copy of set n+2 is already queued behind it when the host comes back from waiting for set n.
// Staging arena: ONE pinned host block and its device twin per bank — every scene's raw | quality | own | fpresent | features,
// then the SceneDev descriptor array — so that a whole request set crosses PCIe in one DMA (plus one per scene whose features the
// caller keeps in a pinned block of its own).
struct Bank {
  std::vector<Slot*> slots;  // pool; the first n_slots are live
  uint32_t n_slots = 0;
  uint64_t set_stamp = ~0ull; // unique per request set (bank_clear draws a new one)
  HostBuf h_arena;
  void* h_arena_dev = nullptr;  // the pinned arena as the device sees it
  DevBuf d_arena;
  size_t used = 0;           // bytes of scene inputs appended to the host arena so far
  size_t desc_off = 0;       // where the descriptor array went (set by bank_upload)
  bool uploaded = false;     // the scene inputs are on the device (a replayed frame uploads nothing)
  std::vector<uint8_t> desc_last;
  uint32_t tile_bm = 64, tile_bn = 64;  // tile of the visual cost kernel for this set (sa_visual_tile)
  SaFramePlan plan{};                   // this set's launches (bank_prepare; the positional mode: bank_launch)
  uint32_t launches = 0;                // kernels this set's frame consists of: counted where they are enqueued (enqueue_frame), so a replayed graph keeps its own
  bool assoc_event = false;             // sa_batch_run_apply: ev_done marks the end of the ASSOCIATION (the frame's last dispatch carries it); the
                                        // upkeep kernels run behind it — sa_batch_fetch waits for the event only, so that the caller's own
                                        // bookkeeping overlaps them
  uint64_t done_seq = 0;                // != 0: the set's last launch reports by completion WORDS (k_assign_small stores this number behind every scene's
                                        // results; the host polls: wait_done), ev_done is NOT recorded for it
  std::atomic<bool> assoc_waited{false};// ... and has been waited for (sa_batch_results from several threads: one trip into the runtime, not one per slot)
  bool want_apply = false;              // sa_batch_run_apply: bank_upload appends the set's ApplyScene array to the arena (behind the descriptors: the same DMA)
  size_t apply_off = 0;                 // ... where it went
  // SA_FLAG_GRAPH: the per-frame launches captured once into a hipGraph (re-captured when the launch geometry changes)
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  GraphKey graph_key{};      // launch geometry + kernel selection of the captured frame (run_pipeline)
  // pipelined tickets
  hipEvent_t ev_staged = nullptr, ev_done = nullptr;
  hipEvent_t ev_apply = nullptr;   // sa_batch_run_apply: carried by the last upkeep dispatch of the set (sa_tracks_apply_collect waits for it)
  bool apply_event = false;
  hipEvent_t ev_kf = nullptr;      // VisualSORT: the set's last KALMAN dispatch (the predicted boxes are out; the feature-bank dispatches run on)
  bool kf_event = false;
  uint64_t apply_seq = 0;          // sa_engine::busy_seq right after that dispatch: unchanged at the wait = the engine is drained
  bool staged_inline = false;  // the request set was uploaded on the compute stream itself (no hand-over event to wait for)
  uint64_t ticket = 0;       // 0 = none
  int state = 0;             // 0 idle, 1 staged (H2D queued), 2 launched (pipeline queued), 3 done and waited
};
#define SA_BANKS 3

}  // namespace

struct sa_engine {
  sa_config cfg{};
  std::vector<uint64_t> cons_delta;
  std::vector<float> cons_dist;
  SaParams P{};
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipStream_t copy_stream = nullptr;  // sa_pipe_*: H2D of the next request set beside the kernels of the current one
  Bank banks[SA_BANKS];
  Bank* B = &banks[0];               // the bank the synchronous entry points, the taps and sa_tracks_apply refer to
  uint64_t B_ticket = 0;             // != 0: B was bound by sa_pipe_wait(ticket); slot numbers mean THAT ticket's scenes for as long as its bank
                                     // has not been recycled by a later sa_pipe_stage (bound_bank_ok)
  uint64_t next_ticket = 1;
  uint32_t K = 1, D = 0, Dp = 0;
  bool bf_words_euclid = false;         // euclidean, bank depth 1: k_visual_euclid can reduce the vote into the vote words (frames up to 1024 x 1024)
  bool bf_tile_forced = false;          // SA_FLAG_BESTFIT_TILE: the weight matrix + k_bestfit_tile also where the contraction could vote itself
  bool bf_partials = false;             // the contraction emits the BestFit partials itself (cosine, bank depth 1): no weight matrix,
                                        // no k_bestfit_tile; the parity taps re-run it in matrix mode
  bool visual = false;
  bool eu_mfma_ok = false;              // euclidean engines: the expansion is usable at this feature length (eu_rho < 1/3)
  float eu_rho = 0.f;
  std::string err;
  std::atomic<uint32_t> n_staged{0}; // scenes between sa_tracks_remove_stage and sa_tracks_remove_commit
  std::mutex err_mu;                 // (sa_batch_fill / sa_tracks_apply_collect_slot run on several threads: fail() serialises its writes)
  std::unordered_map<uint64_t, SceneTable*> scenes;
  bool synced = true;
  uint64_t drain_count = 0;          // how often the engine has been found drained (engine_idle): "has X retired?" = "was there a drain since X was queued?"
  uint64_t busy_seq = 0;             // counts the enqueues since the engine was created (SA_BUSY): "nothing was queued since event X" is a comparison
  // The LAST thing queued carried a completion event of its own (the upkeep's last dispatch, the gather of sa_tracks_remove): draining the
  // engine is then one event wait — a stream synchronisation costs a marker packet's trip through the command processor (~10 us) even
  // when the queue has long been idle.  Valid while busy_seq == tail_seq.
  uint64_t done_counter = 0;   // sequence numbers of the launches that report by completion words (Bank::done_seq)
  hipEvent_t tail_ev = nullptr;
  uint64_t tail_seq = 0;
  hipEvent_t ev_misc = nullptr;      // (the event sa_tracks_remove's gather carries)
  uint64_t gather_seq = 0;           // busy_seq right after sa_tracks_remove's gather, when the engine was drained before it (0: n/a): while it
                                     // equals busy_seq the ONLY thing in flight is that gather, which touches the scene's table and its own
                                     // index buffer — staging the next request set need not wait for it (only_gather_in_flight)
  bool copy_dirty = false;           // something was queued on the copy stream since the last full synchronisation: the tail event says nothing about it
  // device buffers that were replaced while work that may still read them was queued: freed at the next full sync, or — pipelined
  // loops never reach one — by sa_pipe_wait once every ticket issued before the replacement has been waited for (tag = the ticket
  // number that was next when the buffer was replaced)
  struct Garbage { void* p; uint64_t tag; };
  std::vector<Garbage> garbage;
  std::vector<Slot*> applying;  // slots between sa_tracks_apply_begin and _end
  // upload scratch for upserts
  DevBuf nms_mask;
  DevBuf up_raw, up_slots, up_epochs, up_ids, up_mean, up_cov, up_feats, up_present, up_index;
  HostBuf up_host;
  // profiling
  bool profile = false;
  uint32_t n_cu = 0;                    // compute units of the device (sa_one_launch)
  const Bank* last_bank = nullptr;      // the bank whose frame was launched last (sa_debug_frame_launches)
  uint32_t pos_flags = 0;               // sa_config.flags + the SA_POSITIONAL=eager|lazy override read at creation: the positional mode's switches
  struct ProfRec { int kid; hipEvent_t a, b; };
  std::vector<ProfRec> prof_open;
  std::vector<hipEvent_t> ev_pool;
  double prof_ms[KID_COUNT] = {0};
  uint64_t prof_n[KID_COUNT] = {0};
  hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;
  std::vector<sa_store*> stores;   // feature stores on this engine (sa_search.hip): sa_engine_destroy orphans them
  std::vector<sa_points*> point_banks;   // point banks on this engine (sa_points.hip): likewise
  sa_framerows_stats fr_last{};    // the last request-set upload that had a *_dev slot (sa_framerows_last)
  sa_frames_stats frames_last{};   // the last sa_own_areas_batch / sa_nms_batch (sa_frames_last)
  SaPoseNms* pose_nms = nullptr;   // pose NMS on this engine (sa_pose_nms.hip): its buffers, events and last stats
};

#define SA_BUSY(e) do { (e)->synced = false; ++(e)->busy_seq; } while (0)
// (sa_tracks_apply_begin without its _end yet: whatever needs the finished table calls this first; defined next to sa_tracks_apply)
static int finish_applies(sa_engine* e);

namespace {

int fail(sa_engine* e, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (e) { std::lock_guard<std::mutex> lk(e->err_mu); e->err = buf; }
  else g_create_error = buf;
  return code;
}

#define HIPCHK(e, call)                                                                              \
  do {                                                                                               \
    hipError_t _s = (call);                                                                          \
    if (_s != hipSuccess) return fail((e), SA_ERR_HIP, "%s failed: %s (%d)", #call, hipGetErrorString(_s), (int)_s); \
  } while (0)

int dev_ensure(sa_engine* e, DevBuf& b, size_t bytes, bool keep = false) {
  if (bytes <= b.cap && b.p) return SA_OK;
  size_t ncap = bytes < 256 ? 256 : bytes;
  if (keep && b.cap) ncap = ncap < b.cap * 2 ? b.cap * 2 : ncap;
  // a buffer that grows once usually grows again (a track table gains a few rows every frame): a quarter of slack on regrowth,
  // or every frame would pay a dozen hipMalloc / hipFree pairs (~0.3 ms at 1000 tracks)
  else if (b.cap) ncap += ncap / 4;
  void* np = nullptr;
  hipError_t s = hipMalloc(&np, ncap);
  if (s != hipSuccess) return fail(e, SA_ERR_OOM, "hipMalloc(%zu) failed: %s", ncap, hipGetErrorString(s));
  if (b.p) {
    if (keep && b.cap) HIPCHK(e, hipMemcpyAsync(np, b.p, b.cap, hipMemcpyDeviceToDevice, e->stream));
    e->garbage.push_back({b.p, e->next_ticket});  // freed once nothing queued can still read it
  }
  b.p = np;
  b.cap = ncap;
  return SA_OK;
}
// Entry points that a thread of the caller's pool may run (the facade's scene jobs, its result driver) or that only wait / copy: the
// thread's current device is whatever its creator left (device 0 on a fresh thread), the engine's resources live on e->device.
static inline void bind_device(sa_engine* e) {
  if (hipSetDevice(e->device) != hipSuccess) (void)hipGetLastError();
}
int host_ensure(sa_engine* e, HostBuf& b, size_t bytes) {
  if (bytes <= b.cap && b.p) return SA_OK;
  // (a (re)allocation may come from a thread of the caller's pool — sa_tracks_apply_collect_slot, sa_tracks_remove_stage —, whose current
  // device is not necessarily the engine's: the mapping belongs to the engine's device)
  if (e && hipSetDevice(e->device) != hipSuccess) (void)hipGetLastError();
  if (b.p) hipHostFree(b.p);
  b.p = nullptr;
  b.cap = 0;
  size_t ncap = bytes < 4096 ? 4096 : bytes + bytes / 2;
  hipError_t s = hipHostMalloc(&b.p, ncap, hipHostMallocMapped | hipHostMallocCoherent);
  if (s != hipSuccess) return fail(e, SA_ERR_OOM, "hipHostMalloc(%zu) failed: %s", ncap, hipGetErrorString(s));
  b.cap = ncap;
  return SA_OK;
}
#define TRY(x)                   \
  do {                           \
    int _r = (x);                \
    if (_r != SA_OK) return _r;  \
  } while (0)
// host_ensure for a mapped buffer the device reads or writes in place: its device view `dev` is derived again when the block moved
int mapped_ensure(sa_engine* e, HostBuf& b, void*& dev, size_t bytes) {
  void* before = b.p;
  TRY(host_ensure(e, b, bytes));
  if (b.p != before || !dev) HIPCHK(e, hipHostGetDevicePointer(&dev, b.p, 0));
  return SA_OK;
}

// nothing but sa_tracks_remove's gather is in flight: entry points that only stage HOST buffers (the arena of the next request set) skip
// the "busy monitor" wait — the launches they queue are ordered behind the gather on the compute stream anyway
static inline bool only_gather_in_flight(const sa_engine* e) { return !e->synced && e->gather_seq != 0 && e->gather_seq == e->busy_seq && !e->copy_dirty; }
// what a drained engine owes: replaced buffers freed, open profile records resolved
int engine_idle(sa_engine* e);
int engine_sync(sa_engine* e) {
  if (e->tail_ev && e->tail_seq == e->busy_seq && !e->synced && !e->copy_dirty) {  // the last enqueue signals an event of its own: wait for that
    hipError_t we = hipEventSynchronize(e->tail_ev);
    if (we == hipSuccess) return engine_idle(e);
    (void)hipGetLastError();
  }
  if (e->copy_stream) HIPCHK(e, hipStreamSynchronize(e->copy_stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->copy_dirty = false;
  return engine_idle(e);
}
int engine_idle(sa_engine* e) {
  ++e->drain_count;
  for (auto& g : e->garbage) hipFree(g.p);
  e->garbage.clear();
  e->synced = true;
  // resolve open profile records
  for (auto& r : e->prof_open) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      e->prof_ms[r.kid] += ms;
      e->prof_n[r.kid] += 1;
    }
    e->ev_pool.push_back(r.a);
    e->ev_pool.push_back(r.b);
  }
  e->prof_open.clear();
  return SA_OK;
}

// The compute stream alone (sa_tracks_apply: its kernels and the mapped results are all on it): the copy stream may be busy with the
// ingest of the NEXT request set — that is the overlap the pipelined entry points exist for — and is left alone.
int compute_sync(sa_engine* e) {
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return SA_OK;
}

// Slot numbers of sa_tracks_apply / sa_batch_fetch / the taps mean the scenes of the bank e->B points at.  After sa_pipe_wait(ticket)
// that is the ticket's bank — until a later sa_pipe_stage recycles it for another request set: from then on the slots would silently
// mean the NEW set's scenes with the caller's OLD winners and new_ids.  Refuse instead.
int bound_bank_ok(sa_engine* e, const char* who) {
  if (e->B_ticket && (e->B->ticket != e->B_ticket || e->B->state != 3))
    return fail(e, SA_ERR_STATE, "%s: the request set of ticket %llu is gone (its bank was recycled by a later sa_pipe_stage); "
                "call it right after sa_pipe_wait, before staging %d more sets", who, (unsigned long long)e->B_ticket, SA_BANKS - 1);
  return SA_OK;
}

hipEvent_t prof_event(sa_engine* e) {
  if (!e->ev_pool.empty()) {
    hipEvent_t ev = e->ev_pool.back();
    e->ev_pool.pop_back();
    return ev;
  }
  hipEvent_t ev = nullptr;
  // device-scope release: a dispatch that carries a default event ends with a SYSTEM-scope release the same kernel inside the plain
  // pipeline does not pay (~1.5 us on the fused first phase) — the instrumented duration should be the pipeline's, the one rocprofv3 reads
  if (hipEventCreateWithFlags(&ev, hipEventReleaseToDevice) != hipSuccess) { (void)hipGetLastError(); hipEventCreate(&ev); }
  return ev;
}
struct ProfScope {
  sa_engine* e;
  int kid;
  hipEvent_t a = nullptr, b = nullptr;
  ProfScope(sa_engine* e_, int k) : e(e_), kid(k) {
    if (e->profile) {
      a = prof_event(e);
      b = prof_event(e);
      sa_prof_start = a;  // the next SA_LAUNCH stamps a / b with the dispatch's begin / end
      sa_prof_stop = b;
    }
  }
  ~ProfScope() {
    if (e->profile) {
      sa_prof_start = sa_prof_stop = nullptr;
      if (a) e->prof_open.push_back({kid, a, b});
    }
  }
};

int check_box(sa_engine* e, const sa_box& b, const char* what, uint32_t i) {
  if (!(b.aspect > 0.0f) || !(b.height > 0.0f))
    return fail(e, SA_ERR_BAD_ARG, "%s[%u]: aspect and height must be > 0 (bbox.rs:453-456)", what, i);
  if (!(b.confidence >= 0.0f && b.confidence <= 1.0f))
    return fail(e, SA_ERR_BAD_ARG, "%s[%u]: confidence must lie in [0, 1] (bbox.rs:123-126)", what, i);
  return SA_OK;
}

// cos / sin of (angle as f64) from the host's libm, through ONE sincos() call: Polygon::from (bbox.rs:287-330) takes angle.cos() and
// angle.sin() of the same value, which LLVM (rustc, x86_64-unknown-linux-gnu) lowers to a single sincos libcall (SelectionDAG merges an
// FSIN / FCOS pair on one operand where the C library has sincos) — and glibc's sincos is NOT bit-identical to its separate cos and
// sin (they differ in the last bit for about one angle in a thousand on this host: different fused-multiply-add variants).  gcc does
// the same merge in the oracle; clang does not for plain libm calls (math-errno), so it is spelled out on both sides.  The
// bit-exact IoU gate needs identical vertices.  Boxes without an angle use c = 1, s = 0.
void fill_raw(BoxRaw* dst, const sa_box* src, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    dst[i].box = src[i];
    double a = (double)(src[i].has_angle ? src[i].angle : 0.0f);
    if (a == 0.0) { dst[i].c = 1.0; dst[i].s = 0.0; }
    else ::sincos(a, &dst[i].s, &dst[i].c);
  }
}

SceneTable* get_scene(sa_engine* e, uint64_t id, bool create) {
  auto it = e->scenes.find(id);
  if (it != e->scenes.end()) return it->second;
  if (!create) return nullptr;
  SceneTable* s = new SceneTable();
  s->scene_id = id;
  e->scenes[id] = s;
  return s;
}

int scene_reserve(sa_engine* e, SceneTable* s, uint32_t need) {
  if (need <= s->cap) return SA_OK;
  uint32_t ncap = s->cap ? s->cap : 64;
  while (ncap < need) ncap *= 2;
  const size_t KDp = (size_t)e->K * e->Dp;
  TRY(dev_ensure(e, s->geo, (size_t)ncap * sizeof(sa_geo), true));
  TRY(dev_ensure(e, s->ext, (size_t)ncap * sizeof(sa_ext), true));
  TRY(dev_ensure(e, s->verts, (size_t)ncap * 8 * sizeof(double), true));
  TRY(dev_ensure(e, s->epoch, (size_t)ncap * 8, true));
  TRY(dev_ensure(e, s->maha, (size_t)ncap * 20 * sizeof(float), true));
  TRY(dev_ensure(e, s->tids, (size_t)ncap * 8, true));
  TRY(dev_ensure(e, s->kf, (size_t)ncap * 110 * sizeof(float), true));
  if (e->visual) {
    TRY(dev_ensure(e, s->feat, (size_t)ncap * KDp * sizeof(float), true));
    TRY(dev_ensure(e, s->ffrag, sa_frag_bytes((size_t)ncap * e->K, e->Dp), true));   // (blocks of 32 rows, rows ascending: growth appends)
    TRY(dev_ensure(e, s->fnorm, (size_t)ncap * e->K * sizeof(float), true));
    TRY(dev_ensure(e, s->fpresent, (size_t)ncap * e->K, true));
    TRY(dev_ensure(e, s->fcount, (size_t)ncap * 4, true));
    TRY(dev_ensure(e, s->fquality, (size_t)ncap * e->K * sizeof(float), true));
  }
  s->cap = ncap;
  return SA_OK;
}

// id -> row of the scene's table (false: no such track)
bool find_slot(SceneTable* sc, uint64_t id, uint32_t* out) {
  if (sc->ascending) {
    auto it = std::lower_bound(sc->ids.begin(), sc->ids.end(), id);
    if (it == sc->ids.end() || *it != id) return false;
    if (out) *out = (uint32_t)(it - sc->ids.begin());
    return true;
  }
  if (!sc->map_built) {
    sc->slot_of.clear();
    for (uint32_t s = 0; s < (uint32_t)sc->ids.size(); ++s) sc->slot_of[sc->ids[s]] = s;
    sc->map_built = true;
  }
  auto it = sc->slot_of.find(id);
  if (it == sc->slot_of.end()) return false;
  if (out) *out = it->second;
  return true;
}
// a new row at the end of the table (the caller has checked that the id is new)
void append_id(SceneTable* sc, uint64_t id) {
  if (sc->ascending && !sc->ids.empty() && id < sc->ids.back()) sc->ascending = false;  // (find_slot builds the map when it is next needed)
  if (!sc->ascending && sc->map_built) sc->slot_of[id] = (uint32_t)sc->ids.size();
  sc->ids.push_back(id);
}

Slot* get_slot(Bank* b, uint32_t i) {
  while (b->slots.size() <= i) b->slots.push_back(new Slot());
  return b->slots[i];
}

// The pinned half of a bank's staging arena, content-preserving on regrowth (scenes are appended one sa_batch_add at a time).
int arena_reserve(sa_engine* e, Bank* b, size_t bytes) {
  if (bytes <= b->h_arena.cap && b->h_arena.p) return SA_OK;
  size_t ncap = bytes < 65536 ? 65536 : bytes + bytes / 2;
  void* np = nullptr;
  hipError_t s = hipHostMalloc(&np, ncap, hipHostMallocPortable);
  if (s != hipSuccess) return fail(e, SA_ERR_OOM, "hipHostMalloc(%zu) failed: %s", ncap, hipGetErrorString(s));
  if (b->h_arena.p) {
    if (!e->synced) TRY(engine_sync(e));  // a DMA may still be reading the old block
    if (b->used) std::memcpy(np, b->h_arena.p, b->used);
    hipHostFree(b->h_arena.p);
  }
  b->h_arena.p = np;
  b->h_arena.cap = ncap;
  if (hipHostGetDevicePointer(&b->h_arena_dev, np, 0) != hipSuccess) { (void)hipGetLastError(); b->h_arena_dev = nullptr; }
  return SA_OK;
}
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }

// a slot's result block (sa_slot_out.h) through its host pointer / its device view
static inline sa_slot_out::View out_view(const Slot* s) { return sa_slot_out::View(s->h_out.p, s->N); }
static inline sa_slot_out::View out_view_dev(const Slot* s) { return sa_slot_out::View(s->d_out, s->N); }
int slot_reserve(sa_engine* e, Slot* s, uint32_t N, uint32_t T) {
  // Reserved extents: a tracker's table breathes (tracks start, idle ones are evicted) and most of a slot's buffers are sized N x T —
  // sizing them by the frame would reallocate a few of them (hipMalloc, slot init, later hipFree) every time T sets a new record.  The
  // first frame and every record reserve half as much again, in steps of 256.
  if (N > s->N_res) s->N_res = (N + N / 2 + 255u) & ~255u;
  if (T > s->T_res) s->T_res = (T + T / 2 + 255u) & ~255u;
  const size_t n = s->N_res ? s->N_res : 1, t = s->T_res ? s->T_res : 1, K = e->K, Dp = e->Dp ? e->Dp : 32;
  const size_t CT = (t + 63) / 64, RT = (n + 63) / 64;
  TRY(dev_ensure(e, s->geo, n * sizeof(sa_geo)));
  TRY(dev_ensure(e, s->verts, n * 8 * sizeof(double)));
  TRY(dev_ensure(e, s->z, n * 5 * 4));
  TRY(dev_ensure(e, s->conf, n * 4));
  TRY(dev_ensure(e, s->usable, n));
  if (e->visual) {
    if (s->feats_inplace || s->rows_widen || (s->feats_device && ((uintptr_t)s->feats_device & 15u))) TRY(dev_ensure(e, s->feat_raw, n * (e->D ? e->D : 1) * 4));
    TRY(dev_ensure(e, s->feat, n * Dp * 4));
    TRY(dev_ensure(e, s->fnorm, n * 4));
    TRY(dev_ensure(e, s->vis, n * t * K * 4));
  }
  TRY(dev_ensure(e, s->vis_max_key, ((n + 31) / 32) * ((t * K + 63) / 64) * 4));  // covers 64x64 (cosine) and 32x128 (euclidean) tiles: the most slots any plan needs
  if (e->visual) {
    TRY(dev_ensure(e, s->row_part_w, n * CT * 8));
    TRY(dev_ensure(e, s->row_part_t, n * CT * 4));
    TRY(dev_ensure(e, s->col_part_w, RT * t * 8));
    TRY(dev_ensure(e, s->col_part_q, RT * t * 4));
  }
  if (e->visual && (n > s->vb_n || t > s->vb_t || !s->vote_best.p)) {
    // vote words: one per candidate and per track (and per count class for banks of 2 .. SA_CLS_MAXK observations) — sized by the frame,
    // with room to grow (a tracker's table gains a few rows per frame); all ones between frames (bank_launch establishes that once)
    const size_t cn = std::max<size_t>(n + n / 4, SA_SMALL_N), ct = std::max<size_t>(t + t / 4, SA_SMALL_N);
    const size_t kc = (K >= 2 && K <= SA_CLS_MAXK) ? K : 0;
    TRY(dev_ensure(e, s->vote_best, (cn + ct) * (1 + kc) * 8, false));
    s->vb_n = (uint32_t)cn; s->vb_t = (uint32_t)ct;
    s->needs_init = true;
  }
  TRY(dev_ensure(e, s->row_has, n));
  TRY(dev_ensure(e, s->vis_winner, n * 4));
  TRY(dev_ensure(e, s->col_excluded, t));
  void *p_par = s->parent.p, *p_ec = s->e_cnt.p, *p_u = s->u.p;
  TRY(dev_ensure(e, s->parent, (n + t) * 4));
  TRY(dev_ensure(e, s->label, n * 4));
  TRY(dev_ensure(e, s->next_row, n * 4));
  TRY(dev_ensure(e, s->e_cnt, n * 4));
  TRY(dev_ensure(e, s->e_use, n * 4));
  TRY(dev_ensure(e, s->e_edge, n * t * sizeof(SaEdge)));
  TRY(dev_ensure(e, s->u, n * 8));
  TRY(dev_ensure(e, s->u_use, n * 8));
  if (s->parent.p != p_par || s->e_cnt.p != p_ec || s->u.p != p_u) s->needs_init = true;
  TRY(dev_ensure(e, s->v, t * 8));
  TRY(dev_ensure(e, s->rmatch, n * 4));
  TRY(dev_ensure(e, s->cmatch, t * 4));
  TRY(dev_ensure(e, s->dist, t * 8));
  TRY(dev_ensure(e, s->pred, t * 4));
  TRY(dev_ensure(e, s->cstamp, t * 4));
  TRY(dev_ensure(e, s->cscan, t * 4));
  TRY(dev_ensure(e, s->cnext, t * 4));
  TRY(dev_ensure(e, s->rdist, n * 8));
  TRY(dev_ensure(e, s->rnext, n * 4));
  TRY(dev_ensure(e, s->win_col, n * 4));
  {  // the general tail's component labels and the lists of its cooperative solver (a batch takes that tail when ANY scene needs it)
    TRY(dev_ensure(e, s->lab, n * 4));
    TRY(dev_ensure(e, s->crow, n * SA_CROW * 8));
    TRY(dev_ensure(e, s->cwin, t * 4));
    TRY(dev_ensure(e, s->big_rows, n * 4));
    TRY(dev_ensure(e, s->big_bcol, n * 4));
    TRY(dev_ensure(e, s->dq, 2 * n * 4));
  }
  {  // the dense solver's matrix: zero between frames (the solver wipes what it wrote), established after (re)allocation
    void* before = s->dense.p;
    // (a tracker's table grows by a few rows per frame: doubling instead of the usual quarter of slack — every regrowth of this
    // one is a hipMalloc of megabytes plus a memset)
    if (n * t * 8 > s->dense.cap && s->dense.cap) TRY(dev_ensure(e, s->dense, std::max(n * t * 8, 2 * s->dense.cap)));
    TRY(dev_ensure(e, s->dense, n * t * 8));
    if (s->dense.p != before) s->needs_init = true;
  }
  {
    void* before = s->stats.p;
    TRY(dev_ensure(e, s->stats, SA_STATS_BYTES));   // (the stats words, the general tail's queue words, a one-launch frame's ticket block)
    if (s->stats.p != before) s->needs_init = true;
  }
  if (e->cfg.flags & SA_FLAG_TAP) TRY(dev_ensure(e, s->tap, (n * 8 + t * 8) * (e->K > 1 && e->K <= SA_CLS_MAXK ? e->K : 1) + n * 4));
  {
    void* before = s->h_out.p;   // (the result block: sa_slot_out.h)
    TRY(mapped_ensure(e, s->h_out, s->d_out, sa_slot_out::bytes(s->N_res)));
    if (s->h_out.p != before || s->done_off != sa_slot_out::done_off(s->N_res)) {
      s->done_off = sa_slot_out::done_off(s->N_res);
      __atomic_store_n(sa_slot_out::done_word(s->h_out.p, s->done_off), 0ull, __ATOMIC_RELEASE);
    }
  }
  return SA_OK;
}

// (host code is also parsed in the device pass, where the members are global-address-space pointers: cast to the member type)
void fill_scene_dev(sa_engine* e, const Bank* bk, Slot* s, SceneDev* d) {
  SceneTable* sc = s->scene;
  std::memset(d, 0, sizeof *d);
  d->N = s->N; d->T = s->T; d->K = e->K; d->Dp = e->Dp;
  d->TK = s->T * e->K; d->estride = s->T ? s->T : 1;
  d->D = e->D;
  d->flags = (s->has_feats ? SCN_HAS_FEATS : 0u) | (s->has_quality ? SCN_HAS_QUALITY : 0u) | (s->has_own ? SCN_HAS_OWN : 0u) |
             (s->has_fpresent ? SCN_HAS_FPRESENT : 0u) | (bk->plan.vote == SaVote::tile_words ? SCN_WORDS10 : 0u) | (bk->plan.vote == SaVote::class_words ? SCN_WORDSK : 0u);
  d->CT = (s->T + 63) / 64; d->RT = (s->N + 63) / 64;
  if (bk->plan.partials) { d->CT = (s->T + bk->tile_bn - 1) / bk->tile_bn; d->RT = (s->N + bk->tile_bm - 1) / bk->tile_bm; }  // the contraction's own tile grid
  d->nkeys = e->visual ? ((s->N + bk->tile_bm - 1) / bk->tile_bm) * ((s->T * e->K + bk->tile_bn - 1) / bk->tile_bn) : 0;
  if (bk->plan.vote == SaVote::class_words) d->nkeys = ((s->N + 63) / 64) * ((s->T + 64 / e->K - 1) / (64 / e->K));  // whole-track tiles: floor(64 / K) tracks each
  d->epoch = s->epoch;
  d->t_geo = (decltype(d->t_geo))(sc->geo.p); d->t_ext = (decltype(d->t_ext))(sc->ext.p); d->t_verts = (decltype(d->t_verts))(sc->verts.p); d->t_epoch = (decltype(d->t_epoch))(sc->epoch.p);
  d->t_maha = (decltype(d->t_maha))(sc->maha.p); d->t_feat = (decltype(d->t_feat))(sc->feat.p); d->t_ffrag = (decltype(d->t_ffrag))(sc->ffrag.p); d->t_fnorm = (decltype(d->t_fnorm))(sc->fnorm.p);
  d->t_fpresent = (decltype(d->t_fpresent))(sc->fpresent.p); d->t_fcount = (decltype(d->t_fcount))(sc->fcount.p); d->t_ids = (decltype(d->t_ids))(sc->tids.p);
  d->c_raw = (decltype(d->c_raw))(s->p_raw); d->c_quality = (decltype(d->c_quality))(s->p_quality); d->c_own = (decltype(d->c_own))(s->p_own);
  d->c_fpresent_in = (decltype(d->c_fpresent_in))(s->p_fpresent); d->c_feat_raw = (decltype(d->c_feat_raw))(s->p_feat_raw);
  d->c_geo = (decltype(d->c_geo))(s->geo.p); d->c_verts = (decltype(d->c_verts))(s->verts.p); d->c_z = (decltype(d->c_z))(s->z.p);
  d->c_conf = (decltype(d->c_conf))(s->conf.p); d->c_feat = (decltype(d->c_feat))((e->D == e->Dp && s->has_feats) ? s->p_feat_raw : s->feat.p); /* D == Dp: no padding, one copy */ d->c_fnorm = (decltype(d->c_fnorm))(s->fnorm.p);
  d->c_usable = (decltype(d->c_usable))(s->usable.p);
  d->pos = (decltype(d->pos))(s->pos.p); d->vis = (decltype(d->vis))(s->vis.p);
  d->vis_max_key = (decltype(d->vis_max_key))(s->vis_max_key.p);
  d->row_part_w = (decltype(d->row_part_w))(s->row_part_w.p); d->row_part_t = (decltype(d->row_part_t))(s->row_part_t.p);
  d->col_part_w = (decltype(d->col_part_w))(s->col_part_w.p); d->col_part_q = (decltype(d->col_part_q))(s->col_part_q.p);
  d->row_best = (decltype(d->row_best))(s->vote_best.p); d->col_best = (decltype(d->col_best))((unsigned long long*)s->vote_best.p + s->vb_n);
  d->row_cls = (decltype(d->row_cls))((unsigned long long*)s->vote_best.p + (size_t)s->vb_n + s->vb_t);
  d->col_cls = (decltype(d->col_cls))((unsigned long long*)s->vote_best.p + (size_t)s->vb_n + s->vb_t + (size_t)s->vb_n * e->K);
  d->row_has = (decltype(d->row_has))(s->row_has.p); d->vis_winner = (decltype(d->vis_winner))(s->vis_winner.p); d->col_excluded = (decltype(d->col_excluded))(s->col_excluded.p);
  d->parent = (decltype(d->parent))(s->parent.p); d->label = (decltype(d->label))(s->label.p); d->next_row = (decltype(d->next_row))(s->next_row.p);
  d->e_cnt = (decltype(d->e_cnt))(s->e_cnt.p); d->e_use = (decltype(d->e_use))(s->e_use.p); d->e_edge = (decltype(d->e_edge))(s->e_edge.p);
  d->u = (decltype(d->u))(s->u.p); d->u_use = (decltype(d->u_use))(s->u_use.p); d->v = (decltype(d->v))(s->v.p); d->rmatch = (decltype(d->rmatch))(s->rmatch.p); d->cmatch = (decltype(d->cmatch))(s->cmatch.p);
  d->dist = (decltype(d->dist))(s->dist.p); d->pred = (decltype(d->pred))(s->pred.p); d->cstamp = (decltype(d->cstamp))(s->cstamp.p); d->cscan = (decltype(d->cscan))(s->cscan.p);
  d->cnext = (decltype(d->cnext))(s->cnext.p); d->rdist = (decltype(d->rdist))(s->rdist.p); d->rnext = (decltype(d->rnext))(s->rnext.p);
  const sa_slot_out::View out = out_view_dev(s);
  d->out_track_id = (decltype(d->out_track_id))(out.ids()); d->out_vote = (decltype(d->out_vote))(out.votes());
  d->quant = (decltype(d->quant))(s->quant.p);
  d->win_col = (decltype(d->win_col))(s->win_col.p);
  d->lab = (decltype(d->lab))(s->lab.p); d->crow = (decltype(d->crow))(s->crow.p); d->cwin = (decltype(d->cwin))(s->cwin.p); d->big_rows = (decltype(d->big_rows))(s->big_rows.p);
  d->big_bcol = (decltype(d->big_bcol))(s->big_bcol.p); d->dq = (decltype(d->dq))(s->dq.p); d->dense = (decltype(d->dense))(s->dense.p);
  d->stats = (decltype(d->stats))(s->stats.p);
  d->out_stats = (decltype(d->out_stats))(out.stats());
  d->out_win = (decltype(d->out_win))(out.cols());
  d->out_done = (decltype(d->out_done))(sa_slot_out::done_word(s->d_out, s->done_off));
  if (s->tap.p) {  // SA_FLAG_TAP: [N] row words | [T] column words | [N] edge counts (sizes as slot_reserve laid them out)
    const size_t n = s->N ? s->N : 1, t = s->T ? s->T : 1;
    const size_t wk = bk->plan.vote == SaVote::class_words ? e->K : 1;  // class words: K per candidate / track
    d->tap_row_best = (decltype(d->tap_row_best))(s->tap.p);
    d->tap_col_best = (decltype(d->tap_col_best))((unsigned long long*)s->tap.p + n * wk);
    d->tap_ecnt = (decltype(d->tap_ecnt))((unsigned long long*)s->tap.p + (n + t) * wk);
  }
}

// The arguments of a slot's upkeep step (sa_upkeep.hip): Kalman half `a`, feature-bank half `b` (visual engines).  new_row / new_ids:
// device-visible arrays — table row and id of every candidate that starts a track — or both nullptr: drawn on the device from
// s->fused_* (sa_batch_run_apply).  part: 0 = both halves in one launch, 1 / 2 = the halves as launches of their own, Kalman first — the
// rows a registered device block is read in place for then leave the caller's memory with the Kalman dispatch (ApplyArgs::copy_src,
// into s->feat_raw, which the caller has reserved) and the bank half reads the slot's copy.
void fill_apply_args(sa_engine* e, Slot* s, const uint32_t* new_row, const uint64_t* new_ids, int part, ApplyArgs& a, BankArgs& b, bool frame_known = true) {
  SceneTable* sc = s->scene;
  const uint32_t n = s->N;
  a = ApplyArgs{};
  b = BankArgs{};
  a.c_raw = (const BoxRaw*)s->p_raw; a.win_col = (const int32_t*)s->win_col.p; a.new_row = new_row;
  a.new_ids = new_ids; a.n = n; a.epoch = s->epoch;
  a.T0 = s->fused_T0; a.id_base = s->fused_id_base; a.id_per_candidate = s->fused_per_candidate;
  a.kf = (float*)sc->kf.p; a.geo = (sa_geo*)sc->geo.p; a.ext = (sa_ext*)sc->ext.p; a.verts = (double*)sc->verts.p; a.t_epoch = (uint64_t*)sc->epoch.p;
  a.t_ids = (uint64_t*)sc->tids.p; a.maha = (float*)sc->maha.p; a.out_pred = (sa_box*)s->d_pred;
  const bool in_place = e->visual && s->has_feats && e->D == e->Dp && s->feats_device && s->p_feat_raw == (void*)s->feats_device;
  if (part != 0 && in_place && n) { a.copy_src = (const float*)s->feats_device; a.copy_dst = (float*)s->feat_raw.p; a.copy_row_floats = e->D; }
  if (!e->visual) return;
  b.c_raw = a.c_raw; b.win_col = a.win_col; b.new_row = a.new_row; b.T0 = a.T0; b.n = n; b.K = e->K; b.Dp = e->Dp;
  b.c_feat = s->has_feats ? (const float*)(e->D == e->Dp ? ((part != 0 && in_place) ? s->feat_raw.p : s->p_feat_raw) : s->feat.p) : nullptr;
  // (rows that need no padding: the frame may have run lean — the step then forms the norms of the rows it stores itself, bit for bit what
  // the preparation block would have written; padded rows: the preparation blocks rode in the frame, sa_batch_run_apply / ensure_prepped.
  // frame_known = false: the arguments are built BEFORE the frame's launches are chosen — s->prepped still describes the slot's previous frame)
  b.c_fnorm = (e->D != e->Dp || (frame_known && s->prepped)) ? (const float*)s->fnorm.p : nullptr;
  b.c_fpresent_in = s->has_fpresent ? (const uint8_t*)s->p_fpresent : nullptr;
  b.c_quality = s->has_quality ? (const float*)s->p_quality : nullptr;
  b.c_own = s->has_own ? (const float*)s->p_own : nullptr;
  b.t_feat = (float*)sc->feat.p; b.t_ffrag = (float*)sc->ffrag.p; b.t_fnorm = (float*)sc->fnorm.p; b.t_fpresent = (uint8_t*)sc->fpresent.p;
  b.t_fquality = (float*)sc->fquality.p; b.t_fcount = (uint32_t*)sc->fcount.p;
  b.minimal_area = e->cfg.visual_minimal_area; b.q_collect = e->cfg.visual_minimal_quality_collect;
  b.own_collect = e->cfg.visual_minimal_own_area_percentage_collect;
}

// Brings a bank's request set onto the device through stream `st`: the scene inputs appended to the staging arena (once per
// set: a replayed frame uploads nothing), the features a caller keeps in pinned blocks of its own (DMA'd in place), and the
// descriptor array, which is appended to the arena so that it travels in the same DMA; a run that finds inputs and descriptors
// unchanged (a benchmark loop) copies nothing.  `may_be_busy`: an earlier copy out of the host arena may still be queued (the
// synchronous entry points; a pipelined bank is idle by construction).
int bank_upload(sa_engine* e, Bank* b, hipStream_t st, bool may_be_busy, hipEvent_t done = nullptr, bool* done_recorded = nullptr) {
  const uint32_t ns = b->n_slots;
  const size_t dbytes = (size_t)ns * sizeof(SceneDev);
  const size_t desc_off = align_up(b->used, 256);
  // (sa_batch_run_apply: the set's ApplyScene array behind the descriptors — one upload for everything the set's launches read)
  const size_t abytes = b->want_apply ? (size_t)ns * sizeof(ApplyScene) : 0;
  const size_t apply_off = abytes ? desc_off + align_up(dbytes, 256) : desc_off + dbytes;
  // (include/similari_framerows.h: the widen launch's per-scene arguments behind those — still the same upload)
  uint32_t nw = 0;
  for (uint32_t i = 0; i < ns; ++i) nw += (b->slots[i]->rows_widen && b->slots[i]->rows_present) ? 1u : 0u;
  const size_t wbytes = (size_t)nw * sizeof(SaWidenSlot);
  const size_t widen_off = wbytes ? align_up(apply_off + abytes, 256) : apply_off + abytes;
  const size_t total = widen_off + wbytes;
  const size_t tail_bytes = total - desc_off;   // descriptors (+ padding + upkeep arguments + widen arguments)
  void* before = b->d_arena.p;
  TRY(dev_ensure(e, b->d_arena, total));
  if (b->d_arena.p != before) { b->uploaded = false; b->desc_last.clear(); }
  TRY(arena_reserve(e, b, total));
  uint8_t* dbase = (uint8_t*)b->d_arena.p;
  for (uint32_t i = 0; i < ns; ++i) {
    Slot* s = b->slots[i];
    s->p_raw = dbase + s->o_raw; s->p_quality = dbase + s->o_q; s->p_own = dbase + s->o_own; s->p_fpresent = dbase + s->o_fp;
    if (s->rows_widen) s->p_feat_raw = s->feat_raw.p;
    else if (s->feats_device) s->p_feat_raw = ((uintptr_t)s->feats_device & 15u) ? s->feat_raw.p : (void*)s->feats_device;
    else s->p_feat_raw = s->feats_inplace ? s->feat_raw.p : (void*)(dbase + s->o_feat);
  }
  std::vector<uint8_t> build(tail_bytes, 0);
  SceneDev* bd = (SceneDev*)build.data();
  for (uint32_t i = 0; i < ns; ++i) fill_scene_dev(e, b, b->slots[i], &bd[i]);
  if (abytes) {
    ApplyScene* as = (ApplyScene*)(build.data() + (apply_off - desc_off));
    for (uint32_t i = 0; i < ns; ++i) fill_apply_args(e, b->slots[i], nullptr, nullptr, e->visual ? 1 : 0, as[i].a, as[i].b, false);
  }
  b->apply_off = apply_off;
  uint32_t w_maxn = 0;
  int w_elem = -2;   // the widened scenes' common element type, -1: they differ
  if (nw) {
    SaWidenSlot* ws = (SaWidenSlot*)(build.data() + (widen_off - desc_off));
    for (uint32_t i = 0, k = 0; i < ns; ++i) {
      const Slot* s = b->slots[i];
      if (!s->rows_widen || !s->rows_present) continue;
      ws[k].base = (const char*)s->rows.base; ws[k].row_stride = s->rows.row_stride; ws[k].table = (const uint32_t*)(dbase + s->o_rows);
      ws[k].dst = (float*)s->feat_raw.p; ws[k].n = s->N; ws[k].elem = s->rows.elem;
      ++k;
      w_maxn = std::max(w_maxn, s->N);
      w_elem = w_elem == -2 ? s->rows.elem : (w_elem == s->rows.elem ? w_elem : -1);
    }
  }
  const bool same_descs = b->desc_off == desc_off && b->desc_last.size() == tail_bytes && tail_bytes && std::memcmp(b->desc_last.data(), build.data(), tail_bytes) == 0;
  if (b->uploaded && same_descs) return SA_OK;
  if (may_be_busy && !e->synced && !only_gather_in_flight(e)) TRY(engine_sync(e));
  uint8_t* h = (uint8_t*)b->h_arena.p;
  std::memcpy(h + desc_off, build.data(), tail_bytes);
  b->desc_off = desc_off;
  b->desc_last.swap(build);
  if (!b->uploaded) {
    // the ingest kernel (the shader engines pull the pinned blocks through their device mapping: 2 MB in 40 us, against 57 for one
    // hipMemcpyAsync on one SDMA engine) wherever source and destination allow 16-byte accesses, hipMemcpyAsync otherwise
    SaCopySegs segs;
    segs.n = 0;
    auto flush = [&](bool last = false) -> int {
      // the last launch of the upload carries the hand-over event as its own completion signal
      const bool attach = last && done && segs.n;
      if (segs.n) HIPCHK(e, sa_launch_ingest(segs, 24u, st, attach ? done : nullptr));
      if (attach && done_recorded) *done_recorded = true;
      segs.n = 0;
      return SA_OK;
    };
    auto move = [&](const void* src_host, const void* src_dev, void* dst, size_t bytes) -> int {
      if (!bytes) return SA_OK;
      if (!src_dev || (((uintptr_t)src_dev | (uintptr_t)dst) & 15u)) {
        HIPCHK(e, hipMemcpyAsync(dst, src_host, bytes, hipMemcpyHostToDevice, st));
        return SA_OK;
      }
      if (segs.n == SA_COPY_SEGS) TRY(flush());
      segs.s[segs.n].src = src_dev; segs.s[segs.n].dst = dst; segs.s[segs.n].bytes = bytes;
      ++segs.n;
      return SA_OK;
    };
    TRY(move(h, b->h_arena_dev, dbase, total));
    for (uint32_t i = 0; i < ns; ++i) {
      Slot* s = b->slots[i];
      if (s->feats_inplace && s->N) TRY(move(s->feats_inplace, s->feats_inplace_dev, s->feat_raw.p, (size_t)s->N * e->D * 4));
      if (s->feats_device && s->N && ((uintptr_t)s->feats_device & 15u))  // the kernels read rows with 16-byte loads
        HIPCHK(e, hipMemcpyAsync(s->feat_raw.p, s->feats_device, (size_t)s->N * e->D * 4, hipMemcpyDeviceToDevice, st));
    }
    // include/similari_framerows.h: rows gathered and widened out of the callers' device memory — ONE launch for every such scene of the
    // set, behind the ingest that brings the arena (the row tables and the launch's arguments live there).  With a hand-over event it is
    // the upload's last launch and carries it: a pipelined ticket's kernels must not start before the rows are widened.
    bool any_dev = false;
    sa_framerows_stats fs{};
    for (uint32_t i = 0; i < ns; ++i) {
      Slot* s = b->slots[i];
      any_dev = any_dev || s->rows_dev;
      if (!s->rows_widen) continue;
      if (!s->rows_present) {   // nobody brought a feature: the rows the frame reads are zeros, nothing of the caller's is read
        HIPCHK(e, hipMemsetAsync(s->feat_raw.p, 0, (size_t)s->N * e->D * 4, st));
        continue;
      }
      const uint32_t* tb = (const uint32_t*)(h + s->o_rows);
      const uint32_t eb = sa_widen_elem_bytes(s->rows.elem);
      for (uint32_t r = 0; r < s->N; ++r)
        if (tb[r] != SA_ROW_NONE) {
          ++fs.rows;
          fs.wide_rows += sa_widen_row_is_wide((uint64_t)(uintptr_t)s->rows.base + (uint64_t)tb[r] * s->rows.row_stride * eb, e->D) ? 1u : 0u;   // the kernel's own test
          fs.src_bytes += (uint64_t)e->D * eb;
        }
    }
    TRY(flush(nw == 0));
    if (nw) {
      // (profiled: the dispatch stamps the profile's two events instead, and the caller records the hand-over itself)
      hipEvent_t pa = e->profile ? prof_event(e) : nullptr, pb = e->profile ? prof_event(e) : nullptr;
      HIPCHK(e, sa_launch_widen_rows((const SaWidenSlot*)(dbase + widen_off), nw, w_maxn, e->D, w_elem, st, pa, pa ? pb : done));
      if (pa) e->prof_open.push_back({KID_WIDEN, pa, pb});
      else if (done && done_recorded) *done_recorded = true;
      fs.launches = 1;
    }
    if (any_dev) e->fr_last = fs;
    b->uploaded = true;
  } else {
    HIPCHK(e, hipMemcpyAsync(dbase + desc_off, h + desc_off, tail_bytes, hipMemcpyHostToDevice, st));
  }
  SA_BUSY(e);
  return SA_OK;
}

// What a lean frame left out (enqueue_frame), on demand: the preparation blocks of the bank's scenes as a launch of their own.
int ensure_prepped(sa_engine* e, Bank* b) {
  bool need = false;
  uint32_t maxN = 0, maxT = 0;
  for (uint32_t i = 0; i < b->n_slots; ++i) {
    Slot* s = b->slots[i];
    need = need || (s->ran && !s->prepped);
    maxN = s->N > maxN ? s->N : maxN;
    maxT = s->T > maxT ? s->T : maxT;
  }
  if (!need) return SA_OK;
  const SceneDev* ds = (const SceneDev*)((const uint8_t*)b->d_arena.p + b->desc_off);
  HIPCHK(e, sa_launch_frame(ds, b->n_slots, maxN, maxT, e->visual, e->P, e->stream, SaPrep::only));
  for (uint32_t i = 0; i < b->n_slots; ++i) b->slots[i]->prepped = true;
  SA_BUSY(e);
  return SA_OK;
}

// The engine's constants as the launches of a frame with plan `pl` take them.
static SaParams frame_params(const sa_engine* e, const SaFramePlan& pl) {
  SaParams P = e->P;
  P.lazy_pos = pl.lazy ? 1u : 0u;
  P.force_general = pl.tail == SaTail::general ? 1u : 0u;  // (the launches below decide by this, not by the frame's size: the tail's reach depends on the vote's form too)
  P.vote_words = pl.vote == SaVote::cell_words ? 1u : 0u;  // the cost kernels reduce into the words only when they vote themselves (one observation per track)
  P.eu_mfma = pl.eu_mfma ? 1u : 0u;
  P.eu_rho = e->eu_rho;
  return P;
}
// The per-frame launches for the staged scenes, in order, on the engine's stream (and, when `fork`, the positional kernel on
// the side stream between two events).  Also the body of the captured graph.
int enqueue_frame(sa_engine* e, Bank* b, const SceneDev* ds, uint32_t ns, uint32_t maxN, uint32_t maxT, hipEvent_t done = nullptr, bool* done_attached = nullptr) {
  hipStream_t st = e->stream;
  const SaFramePlan& pl = b->plan;
  const bool words = pl.vote != SaVote::resolve;
  const SaParams P = frame_params(e, pl);
  SaParams Pt = P;                         // k_bestfit_tile: the words of deeper banks
  Pt.vote_words = pl.vote == SaVote::tile_words ? 1u : 0u;
  // the frame's LAST launch carries the caller's completion event as its own completion signal (sa_pipe_launch), unless the frame is
  // being profiled (the launch then stamps the profile's events) or captured into a graph (the caller does not ask then)
  const bool attach = done && maxN && !e->profile;
  // the caller wants to know when the results are in: every scene's workgroup of the one-workgroup tail says so itself, in a word behind
  // its results that the host polls (wait_done) — the dispatch carries no completion signal and the next dispatch of the queue (the upkeep
  // step, the next frame of a pipelined loop) starts ~4.6 us earlier; SA_FLAG_SIGNAL_COMPLETION: the signal
#ifdef SA_FORCE_SIGNAL_COMPLETION   /* (A/B builds: scripts/gpu_ab.sh) */
  const bool by_words = false;
#else
  const bool by_words = attach && pl.tail != SaTail::general && !(e->cfg.flags & SA_FLAG_SIGNAL_COMPLETION);
#endif
  hipError_t le;
  b->done_seq = 0;
  b->launches = 0;
  if (pl.one_launch) {
    // the whole frame in the first phase's launch (SaFramePlan::one_launch): it is the last launch too
    if (maxN) {
      if (by_words) b->done_seq = ++e->done_counter;
      else if (attach) sa_done_event = done;
      le = sa_launch_frame_visual(ds, ns, maxN, maxT, e->K, P, st, pl, b->done_seq);
      ++b->launches;
    } else le = hipSuccess;   // (no detection anywhere: no tail, and no vote to prepare for one)
    if (le != hipSuccess) b->done_seq = 0;
    if (done_attached) *done_attached = (attach && sa_done_event == nullptr) || b->done_seq != 0;
    sa_done_event = nullptr;
    HIPCHK(e, le);
    return SA_OK;
  }
  if (pl.fused) { ProfScope ps(e, KID_FRAME_VISUAL); HIPCHK(e, sa_launch_frame_visual(ds, ns, maxN, maxT, e->K, P, st, pl)); ++b->launches; }
  else { ProfScope ps(e, KID_FRAME); HIPCHK(e, sa_launch_frame(ds, ns, maxN, maxT, e->visual, P, st, pl.prep)); ++b->launches; }
  if (e->visual) {
    if (!pl.fused) { ProfScope ps(e, KID_VISUAL); HIPCHK(e, sa_launch_visual(ds, ns, maxN, maxT * e->K, P, st, pl.partials)); ++b->launches; }
    if (!pl.partials && (pl.vote == SaVote::resolve || pl.vote == SaVote::tile_words)) { ProfScope ps(e, KID_BESTFIT_TILE); HIPCHK(e, sa_launch_bestfit_tile(ds, ns, maxN, maxT, Pt, st)); ++b->launches; }
  }
  if (e->visual && !words) { ProfScope ps(e, KID_BESTFIT_RESOLVE); HIPCHK(e, sa_launch_bestfit_resolve(ds, ns, maxN, maxT, st, pl.partials)); ++b->launches; }
  if (pl.tail != SaTail::general) {
    ProfScope ps(e, KID_ASSIGN_SMALL);
    if (by_words) b->done_seq = ++e->done_counter;
    else if (attach) sa_done_event = done;
    le = sa_launch_assign_small(ds, ns, maxN, P, st, pl.tail, words, b->done_seq);
    if (maxN) ++b->launches;
    if (le != hipSuccess) b->done_seq = 0;
  } else {
    // (with vote words the label kernel also turns them into the verdicts the solver honours, and the solver re-arms them).
    // Measured and dropped (round 4): the label step as the FIRST PHASE of the solver's launch, its row workgroups meeting at a counter
    // barrier behind one agent-scope release / acquire each — one launch less, but the barrier and its cache maintenance cost what the
    // launch did: C4 k_assign_solve 5.5 -> 8.75 us, frame 21.8 -> 22.0; 1000 x 1500 VisualSORT 36.2 -> 36.6; C5 solve 6.0 -> 12.8.
    { ProfScope ps(e, KID_ASSIGN_LABEL); HIPCHK(e, sa_launch_assign_label(ds, ns, maxN, maxT, st, words)); }
    ProfScope ps(e, KID_ASSIGN_SOLVE);
    if (attach) sa_done_event = done;
    le = sa_launch_assign_solve(ds, ns, maxN, maxT, P, st, words);
    if (maxN) b->launches += 2;
  }
  if (done_attached) *done_attached = (attach && sa_done_event == nullptr) || b->done_seq != 0;  // taken by the launch (or replaced by the completion words)
  sa_done_event = nullptr;  // never left behind for another launch of this thread, whatever happened
  HIPCHK(e, le);
  return SA_OK;
}

// The whole per-frame device pipeline for a bank's request set: upload (through `up`: the compute stream itself, or the copy
// stream with the hand-over event of the pipelined entry points) and 2-6 launches (enqueue_frame) on the compute stream, no
// host decisions in between.
int bank_prepare(sa_engine* e, Bank* b, uint32_t* maxN_out, uint32_t* maxT_out, bool count_frame = true) {
  const uint32_t ns = b->n_slots;
  uint32_t maxN = 0, maxT = 0;
  for (uint32_t i = 0; i < ns; ++i) {
    Slot* s = b->slots[i];
    if (s->fill_pending) return fail(e, SA_ERR_STATE, "slot %u was added with sa_batch_add_deferred and never filled (sa_batch_fill)", i);
    s->T = s->scene->T;  // tracks may have been upserted since sa_batch_add
    maxN = s->N > maxN ? s->N : maxN;
    maxT = s->T > maxT ? s->T : maxT;
  }
  if (maxN >= (1u << 24)) return fail(e, SA_ERR_UNSUPPORTED, "a scene brings %u detections: fewer than 2^24 per scene (the assignment's queue entries)", maxN);
  if (maxT > 32768u) return fail(e, SA_ERR_UNSUPPORTED, "a scene holds %u tracks: at most 32768 per scene (the assignment's column keys)", maxT);
  for (uint32_t i = 0; i < ns; ++i) TRY(slot_reserve(e, b->slots[i], b->slots[i]->N, b->slots[i]->T));
  // Euclidean engines: the matrix-core path unless a recent frame reported itself ill-conditioned for the expansion (most of its
  // cells needed the direct recompute: features far from the origin compared with their spread) — then the vector-pipe kernel for
  // that SCENE's next sa_config.euclid_backoff_frames frames (256 by default), and another try.  A request set runs ONE kernel
  // family: the vector-pipe one while any of its scenes is backing off.
  bool backing_off = false, all_feats = true;
  for (uint32_t i = 0; i < ns; ++i) {
    SceneTable* sc = b->slots[i]->scene;
    all_feats = all_feats && b->slots[i]->has_feats;
    if (e->cfg.visual_kind != SA_VIS_EUCLIDEAN) continue;
    backing_off = backing_off || sc->eu_valu_left != 0;
    if (sc->eu_valu_left && count_frame) --sc->eu_valu_left;
  }
  struct Ask { const sa_engine* e; uint32_t ns, maxN, maxT; } const ask{e, ns, maxN, maxT};
  const auto visual_ok = [](const void* c, bool eu_mfma, bool vote_words, bool class_words) {
    const Ask& a = *(const Ask*)c;
    SaParams P = a.e->P;
    P.eu_mfma = eu_mfma ? 1u : 0u; P.vote_words = vote_words ? 1u : 0u;
    return sa_frame_visual_ok(a.ns, a.maxN, a.maxT, a.e->K, a.e->D, P, class_words);
  };
  b->plan = sa_frame_plan({e->cfg.positional_kind, e->cfg.visual_kind, e->cfg.flags, e->K, maxN, maxT, e->bf_partials, e->bf_words_euclid,
                           e->bf_tile_forced, e->eu_mfma_ok, all_feats, backing_off, visual_ok, &ask});
  if (e->visual) sa_visual_tile(e->cfg.visual_kind, b->plan.eu_mfma, maxN, maxT * e->K, ns, e->Dp, e->P.gemm_plan, &b->tile_bm, &b->tile_bn);
  *maxN_out = maxN;
  *maxT_out = maxT;
  return SA_OK;
}

int bank_launch(sa_engine* e, Bank* b, uint32_t maxN, uint32_t maxT, hipEvent_t done = nullptr, bool* done_attached = nullptr) {
  const uint32_t ns = b->n_slots;
  b->done_seq = 0;
  SA_BUSY(e);
  const SceneDev* ds = (const SceneDev*)((const uint8_t*)b->d_arena.p + b->desc_off);
  hipStream_t st = e->stream;
  // assignment state that the tail kernels keep clean from frame to frame: establish it after (re)allocation
  for (uint32_t i = 0; i < ns; ++i) {
    Slot* s = b->slots[i];
    if (!s->needs_init) continue;
    HIPCHK(e, sa_launch_slot_init((uint32_t*)s->e_cnt.p, (int64_t*)s->u.p, (uint32_t)(s->e_cnt.cap / 4 < s->u.cap / 8 ? s->e_cnt.cap / 4 : s->u.cap / 8),
                                  (uint32_t*)s->parent.p, (uint32_t)(s->parent.cap / 4), st));
    if (s->vote_best.p) HIPCHK(e, hipMemsetAsync(s->vote_best.p, 0xFF, s->vote_best.cap, st));  // vote words: all ones = no group
    HIPCHK(e, hipMemsetAsync(s->stats.p, 0, SA_STATS_BYTES, st));
    HIPCHK(e, hipMemsetAsync(s->dense.p, 0, s->dense.cap, st));  // (a frame that died half-way may have left gains behind)
    s->needs_init = false;
  }
  // The positional stage's mode (sa_plan.h): by the scenes' hints from their newest collected frames — no wait for the frame in flight.
  uint32_t max_left = 0;
  for (uint32_t i = 0; i < ns; ++i) {
    Slot* s = b->slots[i];
    // a set launched again as it stands (sa_batch_run / sa_batch_time without new staging): the hint from the slot's own last report, as far
    // as it has arrived — read, not awaited (a frame still in flight leaves the older value: it only picks a mode)
    if (s->ran && s->reports_left && s->h_out.p) {
      s->scene->pos_left = __atomic_load_n(out_view(s).stats() + sa_slot_out::STAT_LEFTOVER, __ATOMIC_RELAXED);
    }
    max_left = s->scene->pos_left > max_left ? s->scene->pos_left : max_left;
  }
  b->plan.lazy = sa_lazy_positional(b->plan.lazy_possible, e->pos_flags, max_left);
  // ... and with it, whether the tail rides in the first phase's launch (SaFramePlan::one_launch)
  b->plan.one_launch = false;
  e->last_bank = b;
  // (asked for, and not ruled out by the config, first: the launch's shape is host work that a frame on the two-launch form does not need)
  if (b->plan.lazy && b->plan.fused && (e->cfg.flags & SA_FLAG_ONE_LAUNCH) && !(e->cfg.flags & SA_FLAG_SEPARATE_TAIL) && !e->profile) {
    SaPlanInputs in{};
    in.flags = e->cfg.flags; in.n_cu = e->n_cu; in.profile = e->profile;
    uint32_t blocks = 0;
    const bool helped = sa_frame_visual_helped(ns, maxN, maxT, e->K, frame_params(e, b->plan), b->plan, &blocks);
    b->plan.one_launch = sa_one_launch(b->plan, in, helped, blocks);
  }
  if ((e->cfg.flags & SA_FLAG_GRAPH) && !e->profile) {
    // The captured launches read every per-frame value (epoch, pointers, sizes of each scene) from the descriptor array in device
    // memory at replay; what is baked into the graph is the launch geometry and the kernel selection.  Recapture only when one
    // of those changes: a tracker that bumps the epoch every frame replays the same graph.
    uint32_t feats_mask = 0;
    for (uint32_t i = 0; i < ns; ++i) feats_mask = feats_mask * 31u + (b->slots[i]->has_feats ? 1u : 0u) + 7u;
    GraphKey key;
    std::memset(&key, 0, sizeof key);  // (padding included)
    key.plan = b->plan; key.ns = ns; key.maxN = maxN; key.maxT = maxT; key.tile_bm = b->tile_bm; key.tile_bn = b->tile_bn;
    key.feats_mask = feats_mask; key.ds = ds;
    if (!b->graph_exec || std::memcmp(&key, &b->graph_key, sizeof key) != 0) {
      if (b->graph_exec) { hipGraphExecDestroy(b->graph_exec); b->graph_exec = nullptr; }
      if (b->graph) { hipGraphDestroy(b->graph); b->graph = nullptr; }
      std::memset(&b->graph_key, 0, sizeof b->graph_key);
      HIPCHK(e, hipStreamSynchronize(st));  // the uploads must not be part of the capture
      HIPCHK(e, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
      int rc = enqueue_frame(e, b, ds, ns, maxN, maxT);
      hipError_t ce = hipStreamEndCapture(st, &b->graph);
      if (rc != SA_OK || ce != hipSuccess) {
        if (b->graph) { hipGraphDestroy(b->graph); b->graph = nullptr; }
        for (uint32_t i = 0; i < ns; ++i) b->slots[i]->needs_init = true;  // nothing ran, but keep the rule of the eager path
        if (rc != SA_OK) return rc;
        return fail(e, SA_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(ce));
      }
      HIPCHK(e, hipGraphInstantiate(&b->graph_exec, b->graph, nullptr, nullptr, 0));
      std::memcpy(&b->graph_key, &key, sizeof key);
    }
    hipError_t ge = hipGraphLaunch(b->graph_exec, st);
    if (ge != hipSuccess) {
      for (uint32_t i = 0; i < ns; ++i) b->slots[i]->needs_init = true;
      return fail(e, SA_ERR_HIP, "hipGraphLaunch failed: %s", hipGetErrorString(ge));
    }
  } else {
    int rc = enqueue_frame(e, b, ds, ns, maxN, maxT, done, done_attached);
    if (rc != SA_OK) {  // a frame that died half-way may leave the self-cleaning state dirty
      for (uint32_t i = 0; i < ns; ++i) b->slots[i]->needs_init = true;
      return rc;
    }
  }
  // per launch, replays of a captured graph included: what the frame's launches did (not) prepare, and whether its tail reports leftover rows
  for (uint32_t i = 0; i < ns; ++i) {
    b->slots[i]->ran = true; b->slots[i]->prepped = b->plan.prep == SaPrep::all; b->slots[i]->reports_left = b->plan.reports_left;
  }
  return SA_OK;
}

// The end of a request set's association, as its last launch reports it: completion words (Bank::done_seq — every scene's workgroup of
// the one-workgroup tail stores the launch's sequence number behind its results; polled here) or the completion signal of the dispatch
// (ev_done).  The poll looks at the stream now and then: a queue that has run dry without the words (a fault inside the launch) must not
// hang the caller.
int wait_done(sa_engine* e, Bank* b) {
  if (!b->done_seq) {
    hipError_t we = hipEventSynchronize(b->ev_done);
    if (we != hipSuccess) return fail(e, SA_ERR_HIP, "hipEventSynchronize failed: %s", hipGetErrorString(we));
    return SA_OK;
  }
  const uint64_t want = b->done_seq;
  uint32_t next = 0;   // slots [0, next) have reported
  auto all_in = [&]() {
    for (; next < b->n_slots; ++next) {
      const Slot* s = b->slots[next];
      if (__atomic_load_n(sa_slot_out::done_word(s->h_out.p, s->done_off), __ATOMIC_ACQUIRE) != want) return false;
    }
    return true;
  };
  // Poll for a bounded time (a frame's words arrive within tens of microseconds: the runtime is not touched on the way), then BLOCK on the
  // stream like the hipEventSynchronize this replaces — a request set queued behind another tenant's kernel, or under a debugger, costs no
  // host core while it waits and is never declared failed while its launches can still run (sa_config.poll_spin_us).
  const int64_t budget_us = e->cfg.poll_spin_us < 0 ? 0 : e->cfg.poll_spin_us == 0 ? 2000 : e->cfg.poll_spin_us;
  if (budget_us > 0) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 1;; ++spin) {
      if (all_in()) return SA_OK;
#if defined(__x86_64__)
      __builtin_ia32_pause();
#endif
      if ((spin & 255u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(budget_us)) break;
    }
  }
  const hipError_t q = hipStreamSynchronize(e->stream);   // (waits for the upkeep queued behind the tail as well: the slow path's price)
  if (q != hipSuccess) { (void)hipGetLastError(); return fail(e, SA_ERR_HIP, "the request set's launches failed: %s", hipGetErrorString(q)); }
  if (all_in()) return SA_OK;
  return fail(e, SA_ERR_HIP, "the assignment tail retired without reporting the results of slot %u", next);
}

int run_pipeline(sa_engine* e) {
  Bank* b = e->B;
  if (!b->n_slots) return SA_OK;
  uint32_t maxN = 0, maxT = 0;
  TRY(bank_prepare(e, b, &maxN, &maxT));
  TRY(bank_upload(e, b, e->stream, true));
  return bank_launch(e, b, maxN, maxT);
}

}  // namespace

// =====================================================================================================
// C ABI
// =====================================================================================================
extern "C" {

uint32_t sa_api_version(void) { return SA_API_VERSION; }
// Not part of the API (no header declares it): host-side bookkeeping for the tests of the launch plan — how many kernels the frame of the
// request set launched last consists of (kept per bank where the kernels are enqueued: a replayed graph reports its own capture's).
uint32_t sa_debug_frame_launches(const sa_engine* e) { return e && e->last_bank ? e->last_bank->launches : 0u; }
// ... and the compute units the plan counts blocks against (SaPlanInputs::n_cu), so that those tests hold on any part
uint32_t sa_debug_compute_units(const sa_engine* e) { return e ? e->n_cu : 0u; }

void sa_config_default(sa_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof *c);
  c->struct_size = sizeof(sa_config);
  c->device = -1;
  c->positional_kind = SA_POS_IOU;
  c->positional_threshold = 0.3f;        // DEFAULT_SORT_IOU_THRESHOLD  sort.rs:31
  c->positional_min_confidence = 0.05f;  // DEFAULT_MINIMAL_SORT_CONFIDENCE  sort/metric.rs:11
  c->visual_kind = SA_VIS_NONE;
  c->max_observations = 1;
  c->visual_min_votes = 1;
  c->visual_minimal_track_length = 1;
  c->max_idle_epochs = 5;
  c->kf_position_weight = 1.0f / 20.0f;
  c->kf_velocity_weight = 1.0f / 160.0f;
}

const char* sa_last_error(const sa_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

int sa_engine_create(const sa_config* cfg, sa_engine** out) {
  if (!cfg || !out) return fail(nullptr, SA_ERR_BAD_ARG, "sa_engine_create: null argument");
  *out = nullptr;
  if (cfg->max_observations > SA_MAX_BANK && cfg->visual_kind != SA_VIS_NONE)
    return fail(nullptr, SA_ERR_UNSUPPORTED, "at most %d observations per track", SA_MAX_BANK);
  if (cfg->struct_size != sizeof(sa_config))
    return fail(nullptr, SA_ERR_BAD_ARG, "sa_config.struct_size %u != %zu", cfg->struct_size, sizeof(sa_config));
  if (cfg->n_constraints > SA_MAX_CONSTRAINTS)
    return fail(nullptr, SA_ERR_UNSUPPORTED, "at most %d spatio-temporal constraints", SA_MAX_CONSTRAINTS);
  if (cfg->n_constraints && (!cfg->constraint_epoch_delta || !cfg->constraint_max_dist))
    return fail(nullptr, SA_ERR_BAD_ARG, "constraint arrays are null");
  if (cfg->positional_kind != SA_POS_IOU && cfg->positional_kind != SA_POS_MAHALANOBIS)
    return fail(nullptr, SA_ERR_BAD_ARG, "bad positional_kind");
  if (cfg->visual_kind < SA_VIS_NONE || cfg->visual_kind > SA_VIS_EUCLIDEAN)
    return fail(nullptr, SA_ERR_BAD_ARG, "bad visual_kind");
  if (cfg->visual_kind != SA_VIS_NONE && (cfg->feature_len == 0 || cfg->max_observations == 0))
    return fail(nullptr, SA_ERR_BAD_ARG, "visual engines need feature_len > 0 and max_observations > 0");
  if (cfg->visual_kind == SA_VIS_COSINE && !(cfg->visual_threshold >= -1.0f && cfg->visual_threshold <= 1.0f))
    return fail(nullptr, SA_ERR_BAD_ARG, "cosine threshold must lie within [-1, 1] (visual_sort/metric.rs:39-44)");
  if (cfg->visual_kind == SA_VIS_EUCLIDEAN && !(cfg->visual_threshold > 0.0f))
    return fail(nullptr, SA_ERR_BAD_ARG, "euclidean threshold must be positive (visual_sort/metric.rs:33-36)");
  for (uint32_t i = 0; i < cfg->n_constraints; ++i)
    if (!(cfg->constraint_max_dist[i] > 0.0f))
      return fail(nullptr, SA_ERR_BAD_ARG, "constraint distance must be positive (spatio_temporal_constraints.rs:38-41)");

  int count = 0;
  hipError_t s = hipGetDeviceCount(&count);
  if (s != hipSuccess || count <= 0)
    return fail(nullptr, SA_ERR_NO_DEVICE, "no HIP device visible (%s); this engine has no CPU fallback",
                s == hipSuccess ? "count = 0" : hipGetErrorString(s));
  int dev = cfg->device;
  if (dev < 0) {
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  }
  if (dev >= count) return fail(nullptr, SA_ERR_BAD_ARG, "device %d out of range (%d visible)", dev, count);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return fail(nullptr, SA_ERR_HIP, "hipGetDeviceProperties failed");
  if (!std::strstr(prop.gcnArchName, "gfx950"))
    return fail(nullptr, SA_ERR_NO_DEVICE, "device %d is %s; kernels are built for gfx950 (MI355X) only", dev, prop.gcnArchName);
  if (hipSetDevice(dev) != hipSuccess) return fail(nullptr, SA_ERR_HIP, "hipSetDevice(%d) failed", dev);

  sa_engine* e = new sa_engine();
  e->cfg = *cfg;
  e->device = dev;
  e->cons_delta.assign(cfg->constraint_epoch_delta, cfg->constraint_epoch_delta + cfg->n_constraints);
  e->cons_dist.assign(cfg->constraint_max_dist, cfg->constraint_max_dist + cfg->n_constraints);
  e->cfg.constraint_epoch_delta = e->cons_delta.data();
  e->cfg.constraint_max_dist = e->cons_dist.data();
  e->visual = cfg->visual_kind != SA_VIS_NONE;
  e->K = e->visual ? cfg->max_observations : 1;
  {
    // SA_FLAG_BESTFIT_TILE keeps the two-kernel BestFit (weight matrix + k_bestfit_tile) for A/B runs and for the tests of that path
    const bool bf = (cfg->flags & SA_FLAG_BESTFIT_TILE) != 0;
    e->bf_partials = cfg->visual_kind == SA_VIS_COSINE && e->K == 1 && cfg->visual_min_votes <= 1 && !bf;
    e->bf_words_euclid = cfg->visual_kind == SA_VIS_EUCLIDEAN && e->K == 1 && cfg->visual_min_votes <= 1 && !bf;
    e->bf_tile_forced = bf;
  }
  e->D = e->visual ? cfg->feature_len : 0;
  e->Dp = e->visual ? (e->D + 31u) / 32u * 32u : 0;
  // matrix-core euclidean: a cell is trusted to 1e-5 relative when d^2 >= rho (|a|^2 + |b|^2); rho = twice the largest error of the
  // f32 expansion observed (3.8e-8 sqrt(D) of |a|^2 + |b|^2, scripts/euclid_error_model.py) over the 2e-5 the gate leaves for d^2
  e->eu_rho = 5e-3f * std::sqrt((float)(e->Dp ? e->Dp : 32u));
  e->eu_mfma_ok = cfg->visual_kind == SA_VIS_EUCLIDEAN && e->eu_rho < 0.3334f;
  e->profile = (cfg->flags & SA_FLAG_PROFILE) != 0;
  e->n_cu = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 0u;
  e->pos_flags = cfg->flags;
  // (runs a whole suite in one forced mode without touching its configs; a mode the config itself asks for — or a tapped engine's eager
  // edges — stays as the config says)
  const char* pm = std::getenv("SA_POSITIONAL");
  if (pm && !(e->pos_flags & (SA_FLAG_EAGER_POSITIONAL | SA_FLAG_LAZY_POSITIONAL))) {
    if (!std::strcmp(pm, "eager")) e->pos_flags |= SA_FLAG_EAGER_POSITIONAL;
    else if (!std::strcmp(pm, "lazy") && !(e->pos_flags & SA_FLAG_TAP)) e->pos_flags |= SA_FLAG_LAZY_POSITIONAL;
  }
  if (cfg->stream) e->stream = (hipStream_t)cfg->stream;
  else {
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) {
      delete e;
      return fail(nullptr, SA_ERR_HIP, "hipStreamCreate failed");
    }
    e->own_stream = true;
  }
  SaParams& P = e->P;
  std::memset(&P, 0, sizeof P);
  P.positional_kind = cfg->positional_kind;
  P.visual_kind = cfg->visual_kind;
  P.positional_threshold = cfg->positional_threshold;
  P.visual_threshold = cfg->visual_threshold;
  // new-track threshold: IoU(t) -> t ; Mahalanobis -> MAHALANOBIS_NEW_TRACK_THRESHOLD = 1.0 (sort.rs:379)
  float thr = cfg->positional_kind == SA_POS_MAHALANOBIS ? 1.0f : cfg->positional_threshold;
  P.threshold_q = sa_quantise(thr);
  P.min_votes = cfg->visual_min_votes;
  P.min_track_len = cfg->visual_minimal_track_length;
  P.min_confidence = cfg->positional_min_confidence;
  P.visual_minimal_area = cfg->visual_minimal_area;
  P.visual_minimal_quality_use = cfg->visual_minimal_quality_use;
  P.visual_minimal_own_area_use = cfg->visual_minimal_own_area_percentage_use;
  P.kf_position_weight = cfg->kf_position_weight;
  P.kf_velocity_weight = cfg->kf_velocity_weight;
  P.max_idle = cfg->max_idle_epochs;
  P.vote_words = 0;  // set per frame by enqueue_frame
  P.force_general = (cfg->flags & SA_FLAG_GENERAL_TAIL) ? 1u : 0u;
  P.gemm_plan = cfg->gemm_plan > 0 ? cfg->gemm_plan - 1 : -1;
  P.staged_loop = (cfg->flags & SA_FLAG_STAGED_LOOP) ? 1u : 0u;
  P.no_yield = (cfg->flags & SA_FLAG_NO_YIELD) ? 1u : 0u;
  P.row_major_tiles = (cfg->flags & SA_FLAG_XCD_TILES) ? 0u : ((cfg->flags & SA_FLAG_ROW_TILES) ? 2u : 1u);
  P.Dp = e->Dp;
  P.cons.n = cfg->n_constraints;
  for (uint32_t i = 0; i < cfg->n_constraints; ++i) {
    P.cons.delta[i] = cfg->constraint_epoch_delta[i];
    P.cons.max_dist[i] = cfg->constraint_max_dist[i];
  }
  hipEventCreate(&e->ev_t0);
  hipEventCreate(&e->ev_t1);
  if (hipEventCreate(&e->ev_misc) != hipSuccess) { (void)hipGetLastError(); e->ev_misc = nullptr; }
  {
    // the copy stream at the highest priority the device offers: its few ingest workgroups should be dispatched ahead of the
    // compute stream's thousands, or the DMA of the next request set queues behind the current set's tiles
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = hi = 0;
    if (hipStreamCreateWithPriority(&e->copy_stream, hipStreamNonBlocking, hi) != hipSuccess) e->copy_stream = nullptr;
  }
  for (Bank& bk : e->banks) {
    hipEventCreate(&bk.ev_staged);  // also handed to hipExtLaunchKernelGGL as the ingest dispatch's completion event
    hipEventCreate(&bk.ev_done);    // handed to hipExtLaunchKernelGGL as the completion event of a frame's last dispatch (enqueue_frame)
    hipEventCreate(&bk.ev_apply);
    hipEventCreate(&bk.ev_kf);
  }
  *out = e;
  return SA_OK;
}

static void free_dev(DevBuf& b) {
  if (b.p) hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}
static void free_host(HostBuf& b) {
  if (b.p) hipHostFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}

void sa_engine_destroy(sa_engine* e) {
  if (!e) return;
  hipSetDevice(e->device);
  for (sa_store* st : e->stores) sa_store_orphan(st);   // their device memory goes now; each later call on them is refused
  e->stores.clear();
  for (sa_points* pb : e->point_banks) sa_points_orphan(pb);
  e->point_banks.clear();
  if (e->copy_stream) hipStreamSynchronize(e->copy_stream);
  hipStreamSynchronize(e->stream);
  sa_pose_nms_release(e->pose_nms);
  e->pose_nms = nullptr;
  for (auto& g : e->garbage) hipFree(g.p);
  for (auto& kv : e->scenes) {
    SceneTable* s = kv.second;
    for (DevBuf* b : {&s->geo, &s->ext, &s->verts, &s->epoch, &s->maha, &s->feat, &s->ffrag, &s->fnorm, &s->fpresent, &s->fcount, &s->tids, &s->kf, &s->fquality}) free_dev(*b);
    for (DevBuf& b : s->spare) free_dev(b);
    free_host(s->h_index);
    delete s;
  }
  for (Bank& bk : e->banks) {
    for (Slot* s : bk.slots) {
      for (DevBuf* b : {&s->feat_raw, &s->geo, &s->verts, &s->z, &s->conf,
                        &s->usable, &s->feat, &s->fnorm, &s->pos, &s->vis, &s->quant, &s->vis_max_key, &s->row_part_w,
                        &s->row_part_t, &s->col_part_w, &s->col_part_q, &s->row_has, &s->vis_winner, &s->col_excluded, &s->vote_best,
                        &s->parent, &s->label, &s->next_row, &s->e_cnt, &s->e_use, &s->e_edge, &s->u, &s->u_use, &s->v, &s->rmatch,
                        &s->cmatch, &s->dist, &s->pred, &s->cstamp, &s->cscan, &s->cnext, &s->rdist, &s->rnext, &s->win_col,
                        &s->stats, &s->tap, &s->lab, &s->crow, &s->cwin, &s->big_rows, &s->big_bcol, &s->dq, &s->dense})
        free_dev(*b);
      free_host(s->h_apply);
      free_host(s->h_fix);
      free_host(s->h_pred);
      free_host(s->h_out);
      delete s;
    }
    free_dev(bk.d_arena);
    free_host(bk.h_arena);
    if (bk.graph_exec) hipGraphExecDestroy(bk.graph_exec);
    if (bk.graph) hipGraphDestroy(bk.graph);
    if (bk.ev_staged) hipEventDestroy(bk.ev_staged);
    if (bk.ev_done) hipEventDestroy(bk.ev_done);
    if (bk.ev_apply) hipEventDestroy(bk.ev_apply);
    if (bk.ev_kf) hipEventDestroy(bk.ev_kf);
  }
  for (DevBuf* b : {&e->nms_mask, &e->up_raw, &e->up_slots, &e->up_epochs, &e->up_ids, &e->up_mean, &e->up_cov, &e->up_feats,
                    &e->up_present, &e->up_index})
    free_dev(*b);
  free_host(e->up_host);
  for (auto& r : e->prof_open) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
  for (hipEvent_t ev : e->ev_pool) hipEventDestroy(ev);
  if (e->ev_misc) hipEventDestroy(e->ev_misc);
  if (e->ev_t0) hipEventDestroy(e->ev_t0);
  if (e->ev_t1) hipEventDestroy(e->ev_t1);
  if (e->copy_stream) hipStreamDestroy(e->copy_stream);
  if (e->own_stream) hipStreamDestroy(e->stream);
  delete e;
}

// ---- track state -------------------------------------------------------------------------------------
int sa_tracks_upsert(sa_engine* e, uint64_t scene_id, const sa_tracks* t) {
  if (!e || !t) return fail(e, SA_ERR_BAD_ARG, "sa_tracks_upsert: null argument");
  TRY(finish_applies(e));
  const uint32_t n = t->n;
  if (!n) { get_scene(e, scene_id, true); return SA_OK; }
  if (!t->ids || !t->boxes || !t->epochs) return fail(e, SA_ERR_BAD_ARG, "sa_tracks_upsert: ids/boxes/epochs are required");
  if (e->cfg.positional_kind == SA_POS_MAHALANOBIS && (!t->kf_mean || !t->kf_cov))
    return fail(e, SA_ERR_BAD_ARG, "Mahalanobis engines need kf_mean and kf_cov");
  for (uint32_t i = 0; i < n; ++i) {
    if (t->ids[i] == 0) return fail(e, SA_ERR_BAD_ARG, "track id must be > 0 (sort/voting.rs:57)");
    TRY(check_box(e, t->boxes[i], "tracks.boxes", i));
  }
  {  // one row per id and call: two entries for the same id would be written to the same table row by different threads
    std::vector<uint64_t> sorted_ids(t->ids, t->ids + n);
    std::sort(sorted_ids.begin(), sorted_ids.end());
    for (uint32_t i = 1; i < n; ++i)
      if (sorted_ids[i] == sorted_ids[i - 1])
        return fail(e, SA_ERR_BAD_ARG, "sa_tracks_upsert: track id %llu given twice in one call", (unsigned long long)sorted_ids[i]);
  }
  HIPCHK(e, hipSetDevice(e->device));
  SceneTable* sc = get_scene(e, scene_id, true);
  std::vector<uint32_t> slots(n);
  uint32_t T = sc->T;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t at;
    if (find_slot(sc, t->ids[i], &at)) slots[i] = at;
    else {
      slots[i] = T;
      append_id(sc, t->ids[i]);
      ++T;
    }
  }
  TRY(scene_reserve(e, sc, T));
  sc->T = T;
  sc->full.resize(T, 0);
  for (uint32_t i = 0; i < n; ++i) sc->full[slots[i]] = 0;  // an upsert carries the 5 x 5 projection only
  const uint32_t K = e->K, D = e->D;
  const bool feats = e->visual;
  // pinned staging: raw | slots | epochs | ids | mean | cov | present | feats
  size_t o_raw = 0, o_slots = o_raw + (size_t)n * sizeof(BoxRaw), o_ep = o_slots + (size_t)n * 4;
  o_ep = (o_ep + 7) & ~(size_t)7;
  size_t o_ids = o_ep + (size_t)n * 8, o_mean = o_ids + (size_t)n * 8, o_cov = o_mean + (size_t)n * 5 * 4;
  size_t o_pres = o_cov + (size_t)n * 25 * 4, o_feat = (o_pres + (size_t)n * K + 15) & ~(size_t)15;
  size_t total = o_feat + (feats ? (size_t)n * K * D * 4 : 0);
  TRY(engine_sync(e));  // the staging buffer may still be in flight from the previous call
  TRY(host_ensure(e, e->up_host, total));
  uint8_t* h = (uint8_t*)e->up_host.p;
  fill_raw((BoxRaw*)(h + o_raw), t->boxes, n);
  std::memcpy(h + o_slots, slots.data(), (size_t)n * 4);
  std::memcpy(h + o_ep, t->epochs, (size_t)n * 8);
  std::memcpy(h + o_ids, t->ids, (size_t)n * 8);
  const bool kf = t->kf_mean && t->kf_cov;
  if (kf) {
    std::memcpy(h + o_mean, t->kf_mean, (size_t)n * 5 * 4);
    std::memcpy(h + o_cov, t->kf_cov, (size_t)n * 25 * 4);
  }
  bool have_feats = feats && t->feats;
  if (feats) {
    if (have_feats) {
      if (t->feat_present) std::memcpy(h + o_pres, t->feat_present, (size_t)n * K);
      else std::memset(h + o_pres, 1, (size_t)n * K);
      std::memcpy(h + o_feat, t->feats, (size_t)n * K * D * 4);
    } else std::memset(h + o_pres, 0, (size_t)n * K);
  }
  hipStream_t st = e->stream;
  TRY(dev_ensure(e, e->up_raw, (size_t)n * sizeof(BoxRaw)));
  TRY(dev_ensure(e, e->up_slots, (size_t)n * 4));
  TRY(dev_ensure(e, e->up_epochs, (size_t)n * 8));
  TRY(dev_ensure(e, e->up_ids, (size_t)n * 8));
  HIPCHK(e, hipMemcpyAsync(e->up_raw.p, h + o_raw, (size_t)n * sizeof(BoxRaw), hipMemcpyHostToDevice, st));
  HIPCHK(e, hipMemcpyAsync(e->up_slots.p, h + o_slots, (size_t)n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(e, hipMemcpyAsync(e->up_epochs.p, h + o_ep, (size_t)n * 8, hipMemcpyHostToDevice, st));
  HIPCHK(e, hipMemcpyAsync(e->up_ids.p, h + o_ids, (size_t)n * 8, hipMemcpyHostToDevice, st));
  if (kf) {
    TRY(dev_ensure(e, e->up_mean, (size_t)n * 5 * 4));
    TRY(dev_ensure(e, e->up_cov, (size_t)n * 25 * 4));
    HIPCHK(e, hipMemcpyAsync(e->up_mean.p, h + o_mean, (size_t)n * 5 * 4, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(e->up_cov.p, h + o_cov, (size_t)n * 25 * 4, hipMemcpyHostToDevice, st));
  }
  PrepTrackArgs a{};
  a.raw = (const BoxRaw*)e->up_raw.p; a.slots = (const uint32_t*)e->up_slots.p; a.epochs = (const uint64_t*)e->up_epochs.p;
  a.ids = (const uint64_t*)e->up_ids.p;
  a.kf_mean = kf ? (const float*)e->up_mean.p : nullptr; a.kf_cov = kf ? (const float*)e->up_cov.p : nullptr;
  a.n = n;
  a.geo = (sa_geo*)sc->geo.p; a.ext = (sa_ext*)sc->ext.p; a.verts = (double*)sc->verts.p; a.t_epoch = (uint64_t*)sc->epoch.p; a.t_ids = (uint64_t*)sc->tids.p;
  a.maha = (float*)sc->maha.p;
  HIPCHK(e, sa_launch_prep_tracks(a, e->P, st));
  if (feats) {
    TRY(dev_ensure(e, e->up_present, (size_t)n * K));
    HIPCHK(e, hipMemcpyAsync(e->up_present.p, h + o_pres, (size_t)n * K, hipMemcpyHostToDevice, st));
    if (have_feats) {
      TRY(dev_ensure(e, e->up_feats, (size_t)n * K * D * 4));
      HIPCHK(e, hipMemcpyAsync(e->up_feats.p, h + o_feat, (size_t)n * K * D * 4, hipMemcpyHostToDevice, st));
    }
    HIPCHK(e, sa_launch_pad_features(have_feats ? (const float*)e->up_feats.p : nullptr, n * K, D, e->Dp, K,
                                     (const uint32_t*)e->up_slots.p, (const uint8_t*)e->up_present.p, (float*)sc->feat.p,
                                     (float*)sc->fnorm.p, (uint8_t*)sc->fpresent.p, (uint32_t*)sc->fcount.p, st, (float*)sc->ffrag.p));
  }
  SA_BUSY(e);
  return engine_sync(e);
}

// Rows leave, the others close ranks IN ORDER (the column order is part of the solvers' tie-breaks).  Cheap enough to be called every
// few frames by a tracker that evicts the tracks its frames can no longer match (sa_tracker.cpp): every array of the table is compacted
// into a spare of the same capacity by ONE gather launch on the compute stream and swapped in — no allocation, no host copy of table
// data, no synchronisation (whatever reads the table next is ordered behind the launch); the kept rows' old indices travel through a
// mapped pinned buffer the kernel reads in place; ascending ids need no hash map (find_slot).
// sa_tracks_remove in three steps.
// (1) stage: which rows stay — their old indices into the scene's mapped index buffer.  Touches the scene only: different scenes may be
// staged by different threads at once (may_sync = false: where the engine would have to be drained first — the index buffer may still be
// read by an earlier gather of the same scene, or has to grow — the call answers SA_ERR_STATE and nothing has changed).
static int remove_stage(sa_engine* e, SceneTable* sc, uint32_t n, const uint64_t* ids, bool may_sync) {
  // No drain: the gather is ordered on the compute stream behind whatever still reads or writes the table, and the arrays it fills are the
  // ones the previous gather of this scene read — also behind it.  The one thing the HOST writes is this scene's index buffer: it must not
  // be rewritten while an earlier gather of the SAME scene may still be reading it (two removals on one scene with no drain between them;
  // removals on different scenes — a batch tracker evicting from several of its scenes in one predict() — chain freely).
  if (sc->index_drain == e->drain_count && !e->synced) {
    if (!may_sync) return SA_ERR_STATE;
    TRY(engine_sync(e));
  }
  const size_t need = (size_t)std::max<uint32_t>(sc->cap, sc->T ? sc->T : 1) * 4;   // (for the table's capacity: grows with the table, not per call)
  if (need > sc->h_index.cap || !sc->h_index.p || !sc->d_index) {
    if (!e->synced) {
      if (!may_sync) return SA_ERR_STATE;
      TRY(engine_sync(e));   // (the block is about to be replaced)
    }
    TRY(mapped_ensure(e, sc->h_index, sc->d_index, need));
  }
  uint32_t* keep = (uint32_t*)sc->h_index.p;
  uint32_t nT = 0;
  bool walked = false;
  if (sc->ascending) {   // ascending table, ascending list (every tracker of the reference): one walk over both
    bool asc = true;
    for (uint32_t i = 1; i < n && asc; ++i) asc = ids[i] > ids[i - 1];
    if (asc) {
      uint32_t j = 0;
      for (uint32_t r = 0; r < sc->T; ++r) {
        if (j < n && sc->ids[r] == ids[j]) { ++j; continue; }
        keep[nT++] = r;
      }
      if (j != n) return fail(e, SA_ERR_NOT_FOUND, "unknown track id %llu", (unsigned long long)ids[j]);
      walked = true;
    }
  }
  if (!walked) {
    std::vector<uint8_t> drop(sc->T, 0);
    for (uint32_t i = 0; i < n; ++i) {
      uint32_t at;
      if (!find_slot(sc, ids[i], &at)) return fail(e, SA_ERR_NOT_FOUND, "unknown track id %llu", (unsigned long long)ids[i]);
      drop[at] = 1;
    }
    for (uint32_t r = 0; r < sc->T; ++r)
      if (!drop[r]) keep[nT++] = r;
  }
  sc->staged = true;
  sc->staged_rows = nT;
  e->n_staged.fetch_add(1, std::memory_order_relaxed);
  return SA_OK;
}
// (2) the gather's arguments (the spare arrays exist from here on)
static int remove_build(sa_engine* e, SceneTable* sc, SaGatherTable* g) {
  *g = SaGatherTable{};
  const uint32_t nT = sc->staged_rows;
  if (!nT) return SA_OK;
  const uint32_t K = e->K;
  DevBuf* arrs[SA_TABLE_ARRAYS] = {&sc->geo, &sc->ext, &sc->verts, &sc->epoch, &sc->maha, &sc->tids, &sc->kf, &sc->feat, &sc->fnorm, &sc->fpresent, &sc->fcount, &sc->fquality};
  const uint32_t rowb[SA_TABLE_ARRAYS] = {(uint32_t)sizeof(sa_geo), (uint32_t)sizeof(sa_ext), 64u, 8u, 80u, 8u, 440u, K * e->Dp * 4u, K * 4u, K, 4u, K * 4u};
  const uint32_t na = e->visual ? SA_TABLE_ARRAYS : 7u;
  g->n_arrays = na; g->rows = nT; g->index = (const uint32_t*)sc->d_index;
  for (uint32_t k = 0; k < na; ++k) {
    if (sc->spare[k].cap < arrs[k]->cap || !sc->spare[k].p) {
      if (sc->spare[k].p) e->garbage.push_back({sc->spare[k].p, e->next_ticket});
      sc->spare[k] = DevBuf{};
      TRY(dev_ensure(e, sc->spare[k], arrs[k]->cap));
    }
    g->src[k] = arrs[k]->p; g->dst[k] = sc->spare[k].p; g->row_bytes[k] = rowb[k];
  }
  if (e->visual) { g->frag = (float*)sc->ffrag.p; g->frag_array = 7u; g->frag_K = K; g->frag_Dp = e->Dp; }  // (array 7 = the bank)
  return SA_OK;
}
// (3) the gather has been queued: the compacted arrays become the table, the host's id list follows
static void remove_commit(sa_engine* e, SceneTable* sc) {
  const uint32_t nT = sc->staged_rows;
  sc->staged = false;
  if (nT) {
    DevBuf* arrs[SA_TABLE_ARRAYS] = {&sc->geo, &sc->ext, &sc->verts, &sc->epoch, &sc->maha, &sc->tids, &sc->kf, &sc->feat, &sc->fnorm, &sc->fpresent, &sc->fcount, &sc->fquality};
    const uint32_t na = e->visual ? SA_TABLE_ARRAYS : 7u;
    for (uint32_t k = 0; k < na; ++k) std::swap(*arrs[k], sc->spare[k]);   // (the old arrays are next call's spares: nothing queued reads them after the gather)
    sc->index_drain = e->drain_count;
  }
  const uint32_t* keep = (const uint32_t*)sc->h_index.p;
  sc->full.resize(sc->T, 0);
  for (uint32_t r = 0; r < nT; ++r) { sc->ids[r] = sc->ids[keep[r]]; sc->full[r] = sc->full[keep[r]]; }
  sc->T = nT;
  sc->ids.resize(nT);
  sc->full.resize(nT);
  sc->map_built = false;   // (tables whose ids are not ascending rebuild their map on the next lookup)
}
static bool upkeep_pending(const sa_engine* e) {
  if (!e->applying.empty()) return true;
  for (const Bank& bk : e->banks)
    for (uint32_t i = 0; i < bk.n_slots; ++i)
      if (bk.slots[i]->fused_pending || bk.slots[i]->poly_pending) return true;
  return false;
}
int sa_tracks_remove_stage(sa_engine* e, uint64_t scene_id, uint32_t n, const uint64_t* ids) {
  if (!e || (n && !ids)) return fail(e, SA_ERR_BAD_ARG, "sa_tracks_remove_stage: null argument");
  bind_device(e);
  if (upkeep_pending(e)) return SA_ERR_STATE;   // (an upkeep step has yet to be collected: the serial sa_tracks_remove_many finishes it first)
  SceneTable* sc = get_scene(e, scene_id, false);
  if (!sc) return fail(e, SA_ERR_NOT_FOUND, "unknown scene %llu", (unsigned long long)scene_id);
  if (sc->staged) return fail(e, SA_ERR_STATE, "scene %llu has a removal staged already", (unsigned long long)scene_id);
  if (!n) return SA_OK;
  return remove_stage(e, sc, n, ids, false);
}
// Nothing of what was staged is queued: every scene's table stays as it is (a caller whose OTHER scenes failed to stage, or that gives the
// request set up, calls this — a scene left staged would make the next sa_tracks_remove_many commit a stale row list).
int sa_tracks_remove_abort(sa_engine* e) {
  if (!e) return SA_ERR_BAD_ARG;
  e->n_staged.store(0, std::memory_order_relaxed);
  for (auto& kv : e->scenes) { kv.second->staged = false; kv.second->staged_rows = 0; }
  return SA_OK;
}
int sa_tracks_remove_commit(sa_engine* e) {
  if (!e) return SA_ERR_BAD_ARG;
  if (!e->n_staged.load(std::memory_order_relaxed)) return SA_OK;
  e->n_staged.store(0, std::memory_order_relaxed);
  std::vector<SceneTable*> scs;
  for (auto& kv : e->scenes)
    if (kv.second->staged) scs.push_back(kv.second);
  if (scs.empty()) return SA_OK;
  HIPCHK(e, hipSetDevice(e->device));
  std::vector<SaGatherTable> gs(scs.size());
  for (size_t k = 0; k < scs.size(); ++k) {
    int rc = remove_build(e, scs[k], &gs[k]);
    if (rc != SA_OK) { for (SceneTable* sc : scs) sc->staged = false; return rc; }   // (nothing has been queued: every table is as it was)
  }
  const bool was_idle = e->synced || only_gather_in_flight(e);
  bool launched = false;
  SaGatherTables set{};
  for (size_t k = 0; k < scs.size(); ++k) {   // the gathers, SA_GATHER_SET scenes per launch (their arguments travel by value)
    if (gs[k].rows) set.t[set.n++] = gs[k];
    const bool last = k + 1 == scs.size();
    if (set.n == SA_GATHER_SET || (last && set.n)) {
      if (sa_launch_gather_tables(set, e->stream, last ? e->ev_misc : nullptr) != hipSuccess) {
        for (SceneTable* sc : scs) sc->staged = false;
        return fail(e, SA_ERR_HIP, "sa_tracks_remove: gather launch failed: %s", hipGetErrorString(hipGetLastError()));
      }
      SA_BUSY(e);
      launched = true;
      if (last && e->ev_misc) { e->tail_ev = e->ev_misc; e->tail_seq = e->busy_seq; }
      set.n = 0;
    }
  }
  // (nothing but gathers in flight since the last drain: staging the next request set need not wait, only_gather_in_flight)
  if (launched) e->gather_seq = was_idle ? e->busy_seq : 0;
  for (SceneTable* sc : scs) remove_commit(e, sc);
  return SA_OK;
}
int sa_tracks_remove_many(sa_engine* e, uint32_t n_scenes, const uint64_t* scene_ids, const uint32_t* counts, const uint64_t* const* ids) {
  if (!e || (n_scenes && (!scene_ids || !counts || !ids))) return fail(e, SA_ERR_BAD_ARG, "sa_tracks_remove_many: null argument");
  TRY(finish_applies(e));
  std::vector<SceneTable*> scs;
  for (uint32_t i = 0; i < n_scenes; ++i) {
    if (!counts[i]) continue;
    if (!ids[i]) return fail(e, SA_ERR_BAD_ARG, "sa_tracks_remove_many: null id list");
    SceneTable* sc = get_scene(e, scene_ids[i], false);
    if (!sc) return fail(e, SA_ERR_NOT_FOUND, "unknown scene %llu", (unsigned long long)scene_ids[i]);
    for (SceneTable* other : scs)
      if (other == sc) return fail(e, SA_ERR_BAD_ARG, "scene %llu appears twice in one call", (unsigned long long)scene_ids[i]);
    scs.push_back(sc);
  }
  HIPCHK(e, hipSetDevice(e->device));
  size_t k = 0;
  for (uint32_t i = 0; i < n_scenes; ++i) {   // every scene's host side first: a failure here leaves every table as it was
    if (!counts[i]) continue;
    // (a scene staged earlier is staged AGAIN from the ids given here: what an aborted call left behind must not be committed)
    scs[k]->staged = false;
    int rc = remove_stage(e, scs[k], counts[i], ids[i], true);
    if (rc != SA_OK) { sa_tracks_remove_abort(e); return rc; }
    ++k;
  }
  return sa_tracks_remove_commit(e);
}
int sa_tracks_remove(sa_engine* e, uint64_t scene_id, uint32_t n, const uint64_t* ids) {
  if (!e || (n && !ids)) return fail(e, SA_ERR_BAD_ARG, "sa_tracks_remove: null argument");
  if (!get_scene(e, scene_id, false)) return fail(e, SA_ERR_NOT_FOUND, "unknown scene %llu", (unsigned long long)scene_id);
  if (!n) return finish_applies(e);
  return sa_tracks_remove_many(e, 1, &scene_id, &n, &ids);
}

int sa_tracks_count(sa_engine* e, uint64_t scene_id, uint32_t* out_n) {
  if (!e || !out_n) return fail(e, SA_ERR_BAD_ARG, "sa_tracks_count: null argument");
  SceneTable* sc = get_scene(e, scene_id, false);
  *out_n = sc ? sc->T : 0;
  return SA_OK;
}

int sa_tracks_order(sa_engine* e, uint64_t scene_id, uint64_t* out_ids, uint32_t cap, uint32_t* out_n) {
  if (!e || !out_n) return fail(e, SA_ERR_BAD_ARG, "sa_tracks_order: null argument");
  SceneTable* sc = get_scene(e, scene_id, false);
  uint32_t T = sc ? sc->T : 0;
  *out_n = T;
  if (out_ids)
    for (uint32_t i = 0; i < T && i < cap; ++i) out_ids[i] = sc->ids[i];
  return SA_OK;
}

// ---- batches ------------------------------------------------------------------------------------------
static std::atomic<uint64_t> g_set_stamp{0};
static void bank_clear(Bank* b) {
  b->set_stamp = g_set_stamp.fetch_add(1, std::memory_order_relaxed) + 1;
  b->assoc_event = false;
  b->done_seq = 0;
  b->assoc_waited.store(false, std::memory_order_relaxed);
  b->apply_event = false;
  b->kf_event = false;
  b->n_slots = 0;
  b->used = 0;
  b->uploaded = false;
  b->state = 0;
  b->ticket = 0;
}

int sa_batch_begin(sa_engine* e) {
  if (!e) return SA_ERR_BAD_ARG;
  TRY(finish_applies(e));
  HIPCHK(e, hipSetDevice(e->device));
  for (Bank& bk : e->banks)
    if (bk.state == 1 || bk.state == 2)
      return fail(e, SA_ERR_STATE, "ticket %llu is still outstanding: sa_pipe_wait it before a synchronous batch", (unsigned long long)bk.ticket);
  // "busy monitor": the previous batch must have drained (sort/batch_api.rs:233-241).  (Known drained already — the last thing queued was
  // waited for through its own completion event, fused_collect —: no stream synchronisation, which would cost a marker packet's round
  // trip through the command processor, ~10 us, even on an idle queue.)
  if (!e->synced && !only_gather_in_flight(e)) TRY(engine_sync(e));
  e->B_ticket = 0;      // the synchronous entry points own e->B from here on
  bank_clear(e->B);
  return SA_OK;
}

// Slot numbers mean the scenes of the bank e->B points at (bound_bank_ok): the one look-up of every entry point that takes one.
static int live_slot(sa_engine* e, uint32_t slot, Slot** s) {
  if (slot >= e->B->n_slots) return fail(e, SA_ERR_BAD_ARG, "slot %u out of range (%u staged)", slot, e->B->n_slots);
  *s = e->B->slots[slot];
  return SA_OK;
}

// ---- pinned host blocks handed out to callers (sa_host_alloc): process-wide registry, looked up per staged frame ----
static std::mutex g_pin_mu;
struct PinBlock { const char* host; size_t bytes; const char* dev; };
static std::vector<PinBlock> g_pins;
extern "C" void* sa_host_alloc(uint64_t bytes) {
  void* p = nullptr;
  if (!bytes || hipHostMalloc(&p, (size_t)bytes, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) { (void)hipGetLastError(); d = nullptr; }
  std::lock_guard<std::mutex> lk(g_pin_mu);
  g_pins.push_back({(const char*)p, (size_t)bytes, (const char*)d});
  return p;
}
extern "C" void sa_host_free(void* block) {
  if (!block) return;
  {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (size_t i = 0; i < g_pins.size(); ++i)
      if (g_pins[i].host == (const char*)block) { g_pins.erase(g_pins.begin() + i); break; }
  }
  (void)hipHostFree(block);
}
// is [p, p + bytes) inside a block from sa_host_alloc?  *dev = the same range as the device sees it (nullptr: not mapped)
static bool in_pinned_block(const void* p, size_t bytes, const void** dev = nullptr) {
  std::lock_guard<std::mutex> lk(g_pin_mu);
  const char* q = (const char*)p;
  for (const auto& b : g_pins)
    if (q >= b.host && q + bytes <= b.host + b.bytes) {
      if (dev) *dev = b.dev ? b.dev + (q - b.host) : nullptr;
      return true;
    }
  return false;
}

__attribute__((visibility("hidden"))) bool sa_in_pinned_host_block(const void* p, size_t bytes) { return p && in_pinned_block(p, bytes); }   // (the tracker facade, sa_tracker.cpp)

// ---- device blocks the caller's own producers write detection features into (sa_device_block_register) ----
struct DevBlock { const char* base; size_t bytes; int device; };
static std::vector<DevBlock> g_dev_blocks;
extern "C" int sa_device_block_register(const void* dev_ptr, uint64_t bytes, int device) {
  if (!dev_ptr || !bytes) return SA_ERR_BAD_ARG;
  if (device < 0 && hipGetDevice(&device) != hipSuccess) { (void)hipGetLastError(); return SA_ERR_NO_DEVICE; }  // < 0: the calling thread's current device
  std::lock_guard<std::mutex> lk(g_pin_mu);
  for (auto& b : g_dev_blocks)
    if (b.base == (const char*)dev_ptr) { b.bytes = (size_t)bytes; b.device = device; return SA_OK; }
  g_dev_blocks.push_back({(const char*)dev_ptr, (size_t)bytes, device});
  return SA_OK;
}
extern "C" void sa_device_block_unregister(const void* dev_ptr) {
  std::lock_guard<std::mutex> lk(g_pin_mu);
  for (size_t i = 0; i < g_dev_blocks.size(); ++i)
    if (g_dev_blocks[i].base == (const char*)dev_ptr) { g_dev_blocks.erase(g_dev_blocks.begin() + i); return; }
}
// is [p, p + bytes) inside a registered device block?  *device = the block's device
static bool in_device_block(const void* p, size_t bytes, int* device) {
  std::lock_guard<std::mutex> lk(g_pin_mu);
  const char* q = (const char*)p;
  for (const auto& b : g_dev_blocks)
    if (q >= b.base && q + bytes <= b.base + b.bytes) { *device = b.device; return true; }
  return false;
}
extern "C" __attribute__((visibility("hidden"))) bool sa_in_device_block(const void* p, size_t bytes, int* device) { return p && in_device_block(p, bytes, device); }   // (rows from device memory, sa_devrows.hip)

// Appends one scene of a request set to bank `b`: host work only — the boxes (with libm's cos / sin of their angles), the optional
// per-detection arrays and the features are laid out in the bank's pinned staging arena; bank_upload moves the arena in one DMA.
// The copy half of bank_add: the caller's arrays into the slot's block of the pinned arena.  Touches nothing but that block (and, on a bad
// box, the engine's error string under its mutex): slots of one set may be filled by different threads at once.
static int slot_fill(sa_engine* e, Bank* b, Slot* s, bool check) {
  const sa_detections* d = &s->pend_d;
  const float* const* feat_rows = s->pend_rows;
  const uint32_t N = s->N, D = e->D;
  s->fill_pending = false;
  if (!N) return SA_OK;
  if (check)
    for (uint32_t i = 0; i < N; ++i) TRY(check_box(e, d->boxes[i], "detections.boxes", i));
  uint8_t* h = (uint8_t*)b->h_arena.p;
  fill_raw((BoxRaw*)(h + s->o_raw), d->boxes, N);
  if (s->has_quality) std::memcpy(h + s->o_q, d->feat_quality, (size_t)N * 4);
  if (s->has_own) std::memcpy(h + s->o_own, d->own_area, (size_t)N * 4);
  if (s->has_fpresent && !s->rows_widen) std::memcpy(h + s->o_fp, d->feat_present, N);   // (rows_widen: bank_add wrote presence and row table)
  if (s->has_feats && !s->feats_inplace && !s->feats_device && !s->rows_widen) {
    float* dst0 = (float*)(h + s->o_feat);
    if (feat_rows) {
      for (uint32_t i = 0; i < N; ++i) {
        float* dst = dst0 + (size_t)i * D;
        if (feat_rows[i]) std::memcpy(dst, feat_rows[i], (size_t)D * 4);
        else std::memset(dst, 0, (size_t)D * 4);
      }
    } else std::memcpy(dst0, d->feats, (size_t)N * D * 4);
  }
  return SA_OK;
}
// rows (include/similari_framerows.h): the features come out of the caller's device memory as the descriptor says — checked here, on the
// host, before anything of the slot is touched; its index is consumed here too (the row table goes into the arena).
static int bank_add(sa_engine* e, Bank* b, uint64_t scene_id, uint64_t epoch, const sa_detections* d, const float* const* feat_rows,
                    uint32_t* out_slot, bool defer, const sa_dev_rows* rows, const char* what) {
  const uint32_t N = d->n;
  SaFrameRows fr;
  if (rows) TRY(sa_framerows_check(e, what, e->device, e->D, e->visual, d, rows, &fr));
  // a source today's pointer route reads in place is handed to it: f32, contiguous, no index, everybody present, 16-byte aligned
  const float* const feats = rows ? (fr.in_place ? (const float*)rows->base : nullptr) : d->feats;
  SceneTable* sc = get_scene(e, scene_id, true);
  // (a scene once per request set: the set's stamp on the scene instead of a walk over the slots — Batch* trackers stage dozens per call)
  const size_t bi = (size_t)(b - &e->banks[0]) & 3u;
  if (sc->in_set[bi] == b->set_stamp) return fail(e, SA_ERR_STATE, "scene %llu is already part of this batch", (unsigned long long)scene_id);
  Slot* s = get_slot(b, b->n_slots);
  if (s->ran && s->h_out.p && s->scene) {
    // what the slot's previous frame reported (the bank is idle: that frame has retired), for the scene that frame belonged to
    const uint32_t* st = out_view(s).stats();
    if (e->cfg.visual_kind == SA_VIS_EUCLIDEAN && st[sa_slot_out::STAT_EUCLID_ILL]) s->scene->eu_valu_left = e->cfg.euclid_backoff_frames ? e->cfg.euclid_backoff_frames : 256u;
    if (s->reports_left) s->scene->pos_left = st[sa_slot_out::STAT_LEFTOVER];
  }
  s->scene = sc;
  s->epoch = epoch;
  s->N = N;
  s->T = sc->T;
  s->ran = false;
  s->has_feats = e->visual && (feats != nullptr || feat_rows != nullptr || rows != nullptr);
  s->rows_dev = rows != nullptr;
  s->rows_widen = rows && !fr.in_place && N;
  s->rows_present = rows ? fr.present : 0;
  if (rows) s->rows = *rows;
  s->has_quality = d->feat_quality != nullptr;
  s->has_own = d->own_area != nullptr;
  s->has_fpresent = d->feat_present != nullptr || (s->rows_widen && fr.index_absent);   // (SA_ROW_NONE: absent like feat_present[i] == 0)
  const uint32_t D = e->D;
  const size_t fbytes = (size_t)N * D * 4;
  // the caller's block is pinned (sa_host_alloc): the DMA reads it in place, no staging copy
  const void* feats_dev = nullptr;
  int feats_on = -1;
  s->feats_device = (s->has_feats && !feat_rows && N && in_device_block(feats, fbytes, &feats_on)) ? feats : nullptr;
  if (s->feats_device && feats_on != e->device) {
    s->feats_device = nullptr;
    return fail(e, SA_ERR_BAD_ARG, "detections.feats lies in a block registered for device %d, this engine runs on device %d", feats_on, e->device);
  }
  s->feats_inplace = (s->has_feats && !feat_rows && N && !s->feats_device && in_pinned_block(feats, fbytes, &feats_dev)) ? feats : nullptr;
  s->feats_inplace_dev = s->feats_inplace ? (const float*)feats_dev : nullptr;
  // every sub-array on a 256-byte boundary of the arena (16-byte loads of features and boxes, whole cache lines per scene)
  s->o_raw = align_up(b->used, 256);
  s->o_q = align_up(s->o_raw + (size_t)N * sizeof(BoxRaw), 256);
  s->o_own = align_up(s->o_q + (size_t)N * 4, 256);
  s->o_fp = align_up(s->o_own + (size_t)N * 4, 256);
  // features on a 4 KB boundary of their own: the contraction streams them as 16-byte loads of Dp-float rows
  s->o_rows = align_up(s->o_fp + N, 256);
  s->o_feat = align_up(s->o_rows + (s->rows_widen ? (size_t)N * 4 : 0), 4096);
  const size_t end = s->o_feat + ((s->has_feats && !s->feats_inplace && !s->feats_device && !s->rows_widen) ? fbytes : 0);
  TRY(arena_reserve(e, b, end + 256));
  if (s->rows_widen) {
    uint8_t* h = (uint8_t*)b->h_arena.p;
    sa_framerows_table(d, rows, (uint32_t*)(h + s->o_rows), s->has_fpresent ? h + s->o_fp : nullptr);
  }
  s->pend_d = *d;
  s->pend_d.feats = feats;
  s->pend_rows = feat_rows;
  s->fill_pending = true;
  b->used = end;
  b->uploaded = false;
  if (out_slot) *out_slot = b->n_slots;
  b->n_slots++;
  sc->in_set[bi] = b->set_stamp;   // (only now: an add that failed above has added nothing, and may be retried in the same set)
  return defer ? SA_OK : slot_fill(e, b, s, false);
}

// The one way into the current request set, behind the five sa_batch_add* calls.  what: the name the call answers by.  dev: a *_dev call —
// `rows` must be given, and a null engine gets no text (the others leave one in the thread's creation-error slot).  defer: see sa_batch_fill.
static int stage_scene(sa_engine* e, const char* what, bool dev, uint64_t scene_id, uint64_t epoch, const sa_detections* d,
                       const float* const* feat_rows, const sa_dev_rows* rows, bool defer, uint32_t* out_slot) {
  if (dev && !e) return SA_ERR_BAD_ARG;
  if (!e || !d) return fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
  if (dev && !rows) return fail(e, SA_ERR_BAD_ARG, "%s: null rows", what);
  if (d->n && !d->boxes) return fail(e, SA_ERR_BAD_ARG, "detections.boxes is null");
  if (!defer)
    for (uint32_t i = 0; i < d->n; ++i) TRY(check_box(e, d->boxes[i], "detections.boxes", i));
  bind_device(e);
  return bank_add(e, e->B, scene_id, epoch, d, feat_rows, out_slot, defer, rows, what);
}
int sa_batch_add(sa_engine* e, uint64_t scene_id, uint64_t epoch, const sa_detections* d, uint32_t* out_slot) {
  return stage_scene(e, "sa_batch_add", false, scene_id, epoch, d, nullptr, nullptr, false, out_slot);
}
// sa_batch_add with the feature rows given one pointer per detection (nullptr = no feature) instead of one N x D block: the
// tracker facade receives its observations that way (VisualSortObservation.feature) and would otherwise assemble the block only
// for it to be copied again into the pinned staging buffer — 2 MB twice per frame at C2.  (It answers as sa_batch_add.)
int sa_batch_add_rows(sa_engine* e, uint64_t scene_id, uint64_t epoch, const sa_detections* d, const float* const* feat_rows,
                      uint32_t* out_slot) {
  return stage_scene(e, "sa_batch_add", false, scene_id, epoch, d, feat_rows, nullptr, false, out_slot);
}
// Batch*::predict stages dozens of scenes per call: the layout of a request set is serial bookkeeping (offsets in one arena), the copies
// are not — sa_batch_add_deferred lays a scene out and remembers the caller's arrays, sa_batch_fill(slot) validates the boxes and copies
// (libm's sincos of oriented boxes included); fills of DIFFERENT slots may run on different threads at once, but not beside an add.
int sa_batch_add_deferred(sa_engine* e, uint64_t scene_id, uint64_t epoch, const sa_detections* d, const float* const* feat_rows, uint32_t* out_slot) {
  return stage_scene(e, "sa_batch_add_deferred", false, scene_id, epoch, d, feat_rows, nullptr, true, out_slot);
}
int sa_batch_add_dev(sa_engine* e, uint64_t scene_id, uint64_t epoch, const sa_detections* d, const sa_dev_rows* rows, uint32_t* out_slot) {
  return stage_scene(e, "sa_batch_add_dev", true, scene_id, epoch, d, nullptr, rows, false, out_slot);
}
int sa_batch_add_deferred_dev(sa_engine* e, uint64_t scene_id, uint64_t epoch, const sa_detections* d, const sa_dev_rows* rows, uint32_t* out_slot) {
  return stage_scene(e, "sa_batch_add_deferred_dev", true, scene_id, epoch, d, nullptr, rows, true, out_slot);
}
int sa_batch_fill(sa_engine* e, uint32_t slot) {
  if (!e) return SA_ERR_BAD_ARG;
  bind_device(e);
  Slot* s;
  TRY(live_slot(e, slot, &s));
  if (!s->fill_pending) return SA_OK;
  return slot_fill(e, e->B, s, true);
}

int sa_batch_run(sa_engine* e) {
  if (!e) return SA_ERR_BAD_ARG;
  HIPCHK(e, hipSetDevice(e->device));
  TRY(finish_applies(e));  // (the launches read the track tables: see sa_pipe_launch)
  return run_pipeline(e);
}

int sa_batch_sync(sa_engine* e) {
  if (!e) return SA_ERR_BAD_ARG;
  return engine_sync(e);
}

// (a wait of the assignment tail ran out: whatever the frame left half-way — queues, the dense solver's matrix — is re-established
// before the bank's slots run again)
static void bank_mark_dirty(Bank* b) {
  for (uint32_t i = 0; i < b->n_slots; ++i) b->slots[i]->needs_init = true;
}
// The end of bank b's association, waited for once per set (sa_batch_results from several threads: one trip into the runtime, not one per slot)
static int assoc_wait_once(sa_engine* e, Bank* b) {
  if (b->assoc_waited.load(std::memory_order_acquire)) return SA_OK;
  TRY(wait_done(e, b));
  b->assoc_waited.store(true, std::memory_order_release);
  return SA_OK;
}
// "The results are in", behind the call's wait: k_assign_solve's waits for the scene's row workgroups are bounded, and one that ran out (not all
// workgroups resident, e.g. a partitioned or heavily shared device) leaves a mark in slot s instead of a hung queue.  ticket: for the pipelined text.
static int results_in(sa_engine* e, Bank* b, const Slot* s, uint64_t ticket = 0) {
  if (!out_view(s).gave_up()) return SA_OK;
  bank_mark_dirty(b);
  if (ticket) return fail(e, SA_ERR_HIP, "the assignment tail gave up waiting for its row workgroups: the results of ticket %llu are not valid", (unsigned long long)ticket);
  return fail(e, SA_ERR_HIP, "the assignment tail gave up waiting for its row workgroups: the frame's results are not valid");
}
int sa_batch_fetch(sa_engine* e, uint32_t slot, uint64_t* out_track_id, uint8_t* out_voting_type) {
  if (!e) return SA_ERR_BAD_ARG;
  TRY(bound_bank_ok(e, "sa_batch_fetch"));
  bind_device(e);
  Slot* s;
  TRY(live_slot(e, slot, &s));
  if (!s->ran) return fail(e, SA_ERR_STATE, "sa_batch_fetch before sa_batch_run");
  if (e->B->assoc_event) {  // (the upkeep queued behind the association is still running: the winners are in)
    TRY(wait_done(e, e->B));
  } else if (!e->synced) TRY(engine_sync(e));
  TRY(results_in(e, e->B, s));
  const sa_slot_out::View out = out_view(s);
  if (out_track_id) std::memcpy(out_track_id, out.ids(), (size_t)s->N * 8);
  if (out_voting_type) std::memcpy(out_voting_type, out.votes(), s->N);
  return SA_OK;
}

// The winners of a slot as COLUMNS of the scene's track table (sa_tracks_order), -1 = none: out of the same mapped block as the ids.
// (It waits, but does not look at the tail's mark, and leaves a waited ticket's engine undrained: DESIGN.md §5.)
int sa_batch_fetch_cols(sa_engine* e, uint32_t slot, int32_t* out_cols) {
  if (!e) return SA_ERR_BAD_ARG;
  TRY(bound_bank_ok(e, "sa_batch_fetch_cols"));
  bind_device(e);
  Slot* s;
  TRY(live_slot(e, slot, &s));
  if (!out_cols && s->N) return fail(e, SA_ERR_BAD_ARG, "sa_batch_fetch_cols: null argument");
  if (!s->N) return SA_OK;
  if (!s->ran) return fail(e, SA_ERR_STATE, "sa_batch_fetch_cols before sa_batch_run");
  if (e->B->assoc_event) {
    TRY(wait_done(e, e->B));
  } else if (!e->synced && !e->B_ticket) TRY(engine_sync(e));
  std::memcpy(out_cols, out_view(s).cols(), (size_t)s->N * 4);
  return SA_OK;
}

// sa_batch_fetch + sa_batch_fetch_cols without the copies: the slot's results where the assignment tail wrote them (mapped pinned
// memory), valid until the next sa_batch_begin / sa_pipe_stage that recycles the bank.  Waits for the association like sa_batch_fetch;
// after sa_batch_run_apply that wait is one event, and the call may be made for different slots from different threads.
int sa_batch_results(sa_engine* e, uint32_t slot, const uint64_t** out_track_id, const uint8_t** out_voting_type, const int32_t** out_cols) {
  if (!e) return SA_ERR_BAD_ARG;
  TRY(bound_bank_ok(e, "sa_batch_results"));
  bind_device(e);
  Slot* s;
  TRY(live_slot(e, slot, &s));
  if (!s->ran && !s->fused_pending) return fail(e, SA_ERR_STATE, "sa_batch_results before sa_batch_run");
  if (e->B->assoc_event) {
    TRY(assoc_wait_once(e, e->B));
  } else if (!e->synced) TRY(engine_sync(e));
  TRY(results_in(e, e->B, s));
  const sa_slot_out::View out = out_view(s);
  if (out_track_id) *out_track_id = out.ids();
  if (out_voting_type) *out_voting_type = out.votes();
  if (out_cols) *out_cols = out.cols();
  return SA_OK;
}

// sa_associate_batch and _dev (rows: nullptr, or a descriptor pointer per scene, null: the scene as sa_batch_add takes it; dev: see stage_scene)
static int associate_batch(sa_engine* e, const char* what, bool dev, uint32_t n_scenes, const sa_scene_request* req, const sa_dev_rows* const* rows,
                           const sa_scene_result* res) {
  if (dev && !e) return SA_ERR_BAD_ARG;
  if (!e || (n_scenes && (!req || !res))) return fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
  TRY(sa_batch_begin(e));
  for (uint32_t i = 0; i < n_scenes; ++i) {
    if (rows && rows[i]) TRY(stage_scene(e, what, true, req[i].scene_id, req[i].epoch, &req[i].detections, nullptr, rows[i], false, nullptr));
    else TRY(sa_batch_add(e, req[i].scene_id, req[i].epoch, &req[i].detections, nullptr));
  }
  TRY(sa_batch_run(e));
  TRY(sa_batch_sync(e));
  for (uint32_t i = 0; i < n_scenes; ++i) TRY(sa_batch_fetch(e, i, res[i].out_track_id, res[i].out_voting_type));
  return SA_OK;
}
static int associate_one(sa_engine* e, const char* what, bool dev, uint64_t scene_id, uint64_t epoch, const sa_detections* d, const sa_dev_rows* rows,
                         uint64_t* out_track_id, uint8_t* out_voting_type) {
  if (dev && !e) return SA_ERR_BAD_ARG;
  if (!e || !d) return fail(e, SA_ERR_BAD_ARG, "%s: null argument", what);
  if (dev && !rows) return fail(e, SA_ERR_BAD_ARG, "%s: null rows", what);
  const sa_scene_request rq{scene_id, epoch, *d};
  const sa_scene_result rs{out_track_id, out_voting_type};
  return associate_batch(e, dev ? "sa_associate_batch_dev" : "sa_associate_batch", dev, 1, &rq, dev ? &rows : nullptr, &rs);
}
int sa_associate_batch(sa_engine* e, uint32_t n_scenes, const sa_scene_request* req, const sa_scene_result* res) {
  return associate_batch(e, "sa_associate_batch", false, n_scenes, req, nullptr, res);
}
int sa_associate_batch_dev(sa_engine* e, uint32_t n_scenes, const sa_scene_request* req, const sa_dev_rows* const* rows, const sa_scene_result* res) {
  return associate_batch(e, "sa_associate_batch_dev", true, n_scenes, req, rows, res);
}
int sa_associate(sa_engine* e, uint64_t scene_id, uint64_t epoch, const sa_detections* d, uint64_t* out_track_id,
                 uint8_t* out_voting_type) {
  return associate_one(e, "sa_associate", false, scene_id, epoch, d, nullptr, out_track_id, out_voting_type);
}
int sa_associate_dev(sa_engine* e, uint64_t scene_id, uint64_t epoch, const sa_detections* d, const sa_dev_rows* rows, uint64_t* out_track_id,
                     uint8_t* out_voting_type) {
  return associate_one(e, "sa_associate_dev", true, scene_id, epoch, d, rows, out_track_id, out_voting_type);
}

// ---- pipelined request sets ---------------------------------------------------------------------------------
// SA_BANKS banks, two streams: the H2D of ticket n+1 (copy stream) runs beside the kernels of ticket n (compute stream), and with a
// third ticket outstanding the copy stream never waits for the host; the results land in mapped host memory, so sa_pipe_wait is one
// event wait and a few-kilobyte memcpy.
static Bank* bank_of_ticket(sa_engine* e, uint64_t ticket) {
  if (!ticket) return nullptr;
  for (Bank& bk : e->banks)
    if (bk.ticket == ticket) return &bk;
  return nullptr;
}

// (rows: nullptr, or one descriptor pointer per scene — include/similari_framerows.h; a null entry: the scene as sa_pipe_stage takes it)
static int pipe_stage(sa_engine* e, uint32_t n_scenes, const sa_scene_request* req, const sa_dev_rows* const* rows, uint64_t* out_ticket) {
  if (!e || !out_ticket || (n_scenes && !req)) return fail(e, SA_ERR_BAD_ARG, "sa_pipe_stage: null argument");
  TRY(finish_applies(e));
  *out_ticket = 0;
  for (uint32_t i = 0; i < n_scenes; ++i) {
    const sa_detections* d = &req[i].detections;
    if (d->n && !d->boxes) return fail(e, SA_ERR_BAD_ARG, "detections.boxes is null");
    for (uint32_t k = 0; k < d->n; ++k) TRY(check_box(e, d->boxes[k], "detections.boxes", k));
  }
  // an idle bank, the one whose ticket is older — but not the bank sa_tracks_apply / the taps are still bound to (the ticket waited
  // for last) while another one is idle: `stage(n+1); wait(n); apply(n); launch(n+1)` must find ticket n's scenes in place
  Bank* b = nullptr;
  bool outstanding = false;
  for (Bank& bk : e->banks) {
    outstanding = outstanding || bk.state == 1 || bk.state == 2;
    if ((bk.state == 0 || bk.state == 3) && !(e->B_ticket && &bk == e->B) && (!b || bk.ticket < b->ticket)) b = &bk;
  }
  if (!b && e->B_ticket && (e->B->state == 0 || e->B->state == 3)) b = e->B;
  if (!b) return fail(e, SA_ERR_STATE, "%d tickets are outstanding: sa_pipe_wait one of them first", SA_BANKS);
  HIPCHK(e, hipSetDevice(e->device));
  // first ticket after synchronous work (sa_batch_run without a sync, an upsert): the idle bank may be the one whose launches are
  // still queued — drain once; with tickets in flight the banks' own states say what is busy
  if (!outstanding && !e->synced) TRY(engine_sync(e));
  bank_clear(b);
  for (uint32_t i = 0; i < n_scenes; ++i) {
    int rc = bank_add(e, b, req[i].scene_id, req[i].epoch, &req[i].detections, nullptr, nullptr, false, rows ? rows[i] : nullptr, "sa_pipe_stage_dev");
    if (rc != SA_OK) { bank_clear(b); return rc; }
  }
  uint32_t maxN = 0, maxT = 0;
  TRY(bank_prepare(e, b, &maxN, &maxT, false));  // sa_pipe_launch prepares again (the tables may change in between) and counts the frame
  // A request set without bulk (plain SORT, or features that are in device memory already: tens of KB) goes up on the COMPUTE stream, in
  // order in front of its kernels: the copy stream buys nothing there and its hand-over costs a barrier packet per frame
  size_t moved = b->used;  // the arena, plus the feature rows the upload reads in place from a pinned block
  for (uint32_t i = 0; i < b->n_slots; ++i)
    if (b->slots[i]->feats_inplace) moved += (size_t)b->slots[i]->N * e->D * 4;
  const bool small_inline = moved <= (128u << 10);
  b->staged_inline = !e->copy_stream || small_inline;
  hipStream_t cs = b->staged_inline ? e->stream : e->copy_stream;
  if (!b->staged_inline) e->copy_dirty = true;
  if (b->staged_inline) {
    TRY(bank_upload(e, b, cs, false));
  } else {
    bool recorded = false;
    TRY(bank_upload(e, b, cs, false, b->ev_staged, &recorded));
    if (!recorded) HIPCHK(e, hipEventRecord(b->ev_staged, cs));
  }
  b->state = 1;
  b->ticket = e->next_ticket++;
  *out_ticket = b->ticket;
  return SA_OK;
}

int sa_pipe_stage(sa_engine* e, uint32_t n_scenes, const sa_scene_request* req, uint64_t* out_ticket) {
  return pipe_stage(e, n_scenes, req, nullptr, out_ticket);
}

int sa_pipe_launch(sa_engine* e, uint64_t ticket) {
  if (!e) return SA_ERR_BAD_ARG;
  Bank* b = bank_of_ticket(e, ticket);
  if (!b || b->state != 1) return fail(e, SA_ERR_STATE, "ticket %llu is not staged (unknown, launched already, or waited)", (unsigned long long)ticket);
  HIPCHK(e, hipSetDevice(e->device));
  // the kernels queued here read the track tables: an upkeep step that is still between sa_tracks_apply_begin and _end has written the
  // AXIS-ALIGNED polygon for refreshed oriented rows and queues the right one only when it is finished (apply_finish) — finish it first
  TRY(finish_applies(e));
  uint32_t maxN = 0, maxT = 0;
  TRY(bank_prepare(e, b, &maxN, &maxT));  // the track tables as they are NOW (an upsert / sa_tracks_apply may have come in between)
  if (!b->staged_inline) HIPCHK(e, hipStreamWaitEvent(e->stream, b->ev_staged, 0));
  TRY(bank_upload(e, b, e->stream, false));  // nothing, unless the descriptors changed since staging (then: the descriptors only)
  bool done_rides = false;  // the frame's last dispatch signals ev_done itself
  if (b->n_slots) TRY(bank_launch(e, b, maxN, maxT, b->ev_done, &done_rides));
  if (!done_rides) HIPCHK(e, hipEventRecord(b->ev_done, e->stream));
  b->state = 2;
  return SA_OK;
}

static int pipe_submit(sa_engine* e, uint32_t n_scenes, const sa_scene_request* req, const sa_dev_rows* const* rows, uint64_t* out_ticket) {
  TRY(pipe_stage(e, n_scenes, req, rows, out_ticket));
  return sa_pipe_launch(e, *out_ticket);
}
int sa_pipe_submit(sa_engine* e, uint32_t n_scenes, const sa_scene_request* req, uint64_t* out_ticket) {
  return pipe_submit(e, n_scenes, req, nullptr, out_ticket);
}
int sa_pipe_stage_dev(sa_engine* e, uint32_t n_scenes, const sa_scene_request* req, const sa_dev_rows* const* rows, uint64_t* out_ticket) {
  if (!e) return SA_ERR_BAD_ARG;   // (the *_dev forms — include/similari_framerows.h — answer a null engine without a text)
  return pipe_stage(e, n_scenes, req, rows, out_ticket);
}
int sa_pipe_submit_dev(sa_engine* e, uint32_t n_scenes, const sa_scene_request* req, const sa_dev_rows* const* rows, uint64_t* out_ticket) {
  if (!e) return SA_ERR_BAD_ARG;
  return pipe_submit(e, n_scenes, req, rows, out_ticket);
}
int sa_framerows_last(sa_engine* e, sa_framerows_stats* out) {
  if (!e || !out) return SA_ERR_BAD_ARG;
  *out = e->fr_last;
  out->struct_size = sizeof *out;
  return SA_OK;
}

int sa_pipe_wait(sa_engine* e, uint64_t ticket, const sa_scene_result* res) {
  if (!e) return SA_ERR_BAD_ARG;
  bind_device(e);
  Bank* b = bank_of_ticket(e, ticket);
  if (!b || (b->state != 2 && b->state != 3))
    return fail(e, SA_ERR_STATE, "ticket %llu has not been launched (or is unknown)", (unsigned long long)ticket);
  if (b->n_slots && !res) return fail(e, SA_ERR_BAD_ARG, "sa_pipe_wait: null result array");
  TRY(finish_applies(e));  // (slot numbers are about to mean THIS ticket's scenes: a pending sa_tracks_apply_end could no longer name its slot)
  if (b->state == 2) TRY(wait_done(e, b));
  for (uint32_t i = 0; i < b->n_slots; ++i) {
    const Slot* s = b->slots[i];
    TRY(results_in(e, b, s, ticket));
    const sa_slot_out::View out = out_view(s);
    if (res[i].out_track_id) std::memcpy(res[i].out_track_id, out.ids(), (size_t)s->N * 8);
    if (res[i].out_voting_type) std::memcpy(res[i].out_voting_type, out.votes(), s->N);
  }
  b->state = 3;
  e->B = b;  // slots of taps / sa_tracks_apply / sa_batch_fetch now mean this ticket's scenes
  e->B_ticket = ticket;
  // A pipelined loop never reaches engine_sync: buffers replaced on the way (a track table that grew, a slot that met a larger frame)
  // are freed here, once every ticket that was launched before the replacement has been waited for.
  if (!e->garbage.empty()) {
    uint64_t oldest = ~0ull;  // oldest ticket still launched and not waited for
    for (const Bank& bk : e->banks)
      if (bk.state == 2 && bk.ticket < oldest) oldest = bk.ticket;
    size_t keep = 0;
    for (size_t i = 0; i < e->garbage.size(); ++i) {
      if (e->garbage[i].tag <= oldest) hipFree(e->garbage[i].p);
      else e->garbage[keep++] = e->garbage[i];
    }
    e->garbage.resize(keep);
  }
  return SA_OK;
}

// ---- device-side track upkeep ---------------------------------------------------------------------------
// sa_tracks_apply in two halves: _begin validates, stages and QUEUES the upkeep kernels; _end waits for them, hands out the predicted
// boxes and queues the polygon fix-up of oriented boxes.  Between the two the host is free (the tracker facade does its own
// bookkeeping there); whatever needs the finished table first — the next request set, an upsert, a tap — finishes a pending one.
static int apply_finish(sa_engine* e, Slot* s, sa_box* out_predicted);
static int fused_collect(sa_engine* e, Slot* s, uint64_t* out_ids, sa_box* out_predicted);
static int polygon_fixups(sa_engine* e, Slot* s);
static int finish_applies(sa_engine* e) {
  while (!e->applying.empty()) TRY(apply_finish(e, e->applying.back(), nullptr));
  for (Bank& bk : e->banks)
    for (uint32_t i = 0; i < bk.n_slots; ++i) {
      if (bk.slots[i]->fused_pending) TRY(fused_collect(e, bk.slots[i], nullptr, nullptr));
      else if (bk.slots[i]->poly_pending) { bk.slots[i]->poly_pending = false; TRY(polygon_fixups(e, bk.slots[i])); }
    }
  return SA_OK;
}
// Queues the upkeep kernels of slot `s` (Kalman step + table rows, feature-bank policy: one launch) on the compute stream.  new_row / new_ids:
// device-visible arrays — table row and id of every candidate that starts a track (SA_NONE / 0 elsewhere).
static int apply_launch(sa_engine* e, Slot* s, const uint32_t* new_row, const uint64_t* new_ids) {
  TRY(mapped_ensure(e, s->h_pred, s->d_pred, (size_t)s->N * sizeof(sa_box)));
  ApplyArgs a;
  BankArgs b;
  fill_apply_args(e, s, new_row, new_ids, 0, a, b);
  HIPCHK(e, sa_launch_apply(a, e->visual ? &b : nullptr, e->P, e->stream, nullptr, 0));
  SA_BUSY(e);
  return SA_OK;
}
static inline bool oriented(const sa_box& b) { return b.has_angle && b.angle != 0.0f; }   // (its polygon needs cos / sin of the angle)
// One candidate of an upkeep step against the scene's table as the slot ran against it (T0 rows): a winner names a column of the table
// that holds its id and a full Kalman state; a candidate without one (winner 0) starts a track under new_id, which must be new.
static int check_upkeep_winner(sa_engine* e, SceneTable* sc, uint32_t T0, uint64_t winner, int32_t col, uint64_t new_id) {
  if (winner == 0)
    return find_slot(sc, new_id, nullptr) ? fail(e, SA_ERR_BAD_ARG, "new id %llu already exists in the scene", (unsigned long long)new_id) : SA_OK;
  if (col < 0 || (uint32_t)col >= T0 || sc->ids[col] != winner) return fail(e, SA_ERR_STATE, "winner %llu is not in the table", (unsigned long long)winner);
  if (!sc->full[col])
    return fail(e, SA_ERR_STATE, "track %llu was upserted without a Kalman state: device-side upkeep needs tracks created by "
                "sa_tracks_apply or seeded with sa_tracks_set_state", (unsigned long long)winner);
  return SA_OK;
}
int sa_tracks_apply_begin(sa_engine* e, uint32_t slot, const uint64_t* new_ids) {
  if (!e) return SA_ERR_BAD_ARG;
  TRY(bound_bank_ok(e, "sa_tracks_apply"));
  Slot* s;
  TRY(live_slot(e, slot, &s));
  if (!s->ran) return fail(e, SA_ERR_STATE, "sa_tracks_apply before sa_batch_run");
  HIPCHK(e, hipSetDevice(e->device));
  // the slot's winners must be in: a waited ticket's are (sa_pipe_wait); after a synchronous run the compute stream has to drain.
  // Never the copy stream: it may be carrying the NEXT request set's ingest, which is exactly what this call is meant to overlap.
  if (!e->synced && !e->B_ticket) TRY(engine_sync(e));
  SceneTable* sc = s->scene;
  const uint32_t n = s->N;
  if (!n) return SA_OK;
  if (s->T != sc->T) return fail(e, SA_ERR_STATE, "the scene's track table changed since the slot ran");
  if (e->visual && e->D != e->Dp) TRY(ensure_prepped(e, e->B));  // the feature-bank step reads the candidates' PADDED rows (rows that need no padding: it reads them where they were uploaded)
  const uint64_t* winners = out_view(s).ids();
  // the same winners as rows of the table (written next to the ids by the assignment tail): no lookup by id per candidate
  const int32_t* wcol = out_view(s).cols();
  sc->full.resize(sc->T, 0);
  uint32_t n_new = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (winners[i] == 0) {
      if (!new_ids || new_ids[i] == 0) return fail(e, SA_ERR_BAD_ARG, "candidate %u starts a track and needs new_ids[%u] > 0", i, i);
      ++n_new;
    }
    TRY(check_upkeep_winner(e, sc, sc->T, winners[i], wcol[i], winners[i] == 0 ? new_ids[i] : 0));
  }
  if (n_new > 1) {  // one row per new id
    std::vector<uint64_t> fresh;
    fresh.reserve(n_new);
    for (uint32_t i = 0; i < n; ++i)
      if (winners[i] == 0) fresh.push_back(new_ids[i]);
    std::sort(fresh.begin(), fresh.end());
    for (size_t k = 1; k < fresh.size(); ++k)
      if (fresh[k] == fresh[k - 1]) return fail(e, SA_ERR_BAD_ARG, "new id %llu given twice", (unsigned long long)fresh[k]);
  }
  const uint32_t T0 = sc->T;
  TRY(scene_reserve(e, sc, T0 + n_new));
  // staging: table row + id of every candidate that starts a track — in mapped pinned memory the kernel reads in place (12 KB at
  // 1000 candidates: two runtime copy calls and their DMA launches would cost more than the reads over the link)
  const size_t ids_off = ((size_t)n * 4 + 7) & ~(size_t)7;
  TRY(mapped_ensure(e, s->h_apply, s->d_apply, ids_off + (size_t)n * 8));
  uint32_t* h_row = (uint32_t*)s->h_apply.p;
  uint64_t* h_ids = (uint64_t*)((uint8_t*)s->h_apply.p + ids_off);
  uint32_t next = T0;
  for (uint32_t i = 0; i < n; ++i) {
    h_row[i] = winners[i] == 0 ? next++ : SA_NONE;
    h_ids[i] = winners[i] == 0 ? new_ids[i] : 0;
  }
  TRY(apply_launch(e, s, (const uint32_t*)s->d_apply, (const uint64_t*)((const uint8_t*)s->d_apply + ids_off)));
  // host side of the table: the new rows
  for (uint32_t i = 0; i < n; ++i)
    if (winners[i] == 0) {
      append_id(sc, new_ids[i]);
    }
  sc->T = T0 + n_new;
  sc->full.resize(sc->T, 1);  // (the winners' rows held a full state already: checked above)
  s->ran = false;  // the table the slot ran against is gone
  s->apply_pending = true;
  e->applying.push_back(s);
  return SA_OK;
}
// Oriented boxes: the polygon of a refreshed row needs cos / sin of the predicted angle from THIS side's libm (fill_raw does the same for
// every box that is uploaded; the device's sincos is not bit-identical to it).  The predicted boxes are on the host (h_pred), the rows of
// the tracks that started in h_apply; (row, box, cos, sin) go back through mapped memory to a kernel queued behind the step — no wait:
// whatever reads the table next is ordered behind it on the stream.
static int polygon_fixups(sa_engine* e, Slot* s) {
  SceneTable* sc = s->scene;
  const uint32_t n = s->N;
  const uint64_t* winners = out_view(s).ids();
  const int32_t* wcol = out_view(s).cols();
  const uint32_t* h_row = (const uint32_t*)s->h_apply.p;
  const sa_box* pb = (const sa_box*)s->h_pred.p;
  uint32_t nfix = 0;
  for (uint32_t i = 0; i < n; ++i) nfix += oriented(pb[i]) ? 1u : 0u;
  if (!nfix) return SA_OK;
  TRY(mapped_ensure(e, s->h_fix, s->d_fix, (size_t)nfix * sizeof(SaPolyFix)));
  SaPolyFix* fx = (SaPolyFix*)s->h_fix.p;
  uint32_t k = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (!oriented(pb[i])) continue;
    const double ang = (double)pb[i].angle;
    fx[k].row = winners[i] == 0 ? h_row[i] : (uint32_t)wcol[i];
    fx[k].pad = 0;
    fx[k].xc = pb[i].xc; fx[k].yc = pb[i].yc; fx[k].aspect = pb[i].aspect; fx[k].height = pb[i].height;
    ::sincos(ang, &fx[k].s, &fx[k].c);  // as fill_raw
    ++k;
  }
  HIPCHK(e, sa_launch_apply_polygons((const SaPolyFix*)s->d_fix, nfix, (double*)sc->verts.p, e->stream));
  SA_BUSY(e);
  return SA_OK;
}
static int apply_finish(sa_engine* e, Slot* s, sa_box* out_predicted) {
  HIPCHK(e, hipSetDevice(e->device));
  for (size_t k = 0; k < e->applying.size(); ++k)
    if (e->applying[k] == s) { e->applying.erase(e->applying.begin() + (long)k); break; }
  s->apply_pending = false;
  if (e->B_ticket) TRY(compute_sync(e));  // pipelined: leave the copy stream (the next set's ingest) alone
  else TRY(engine_sync(e));
  if (out_predicted) std::memcpy(out_predicted, s->h_pred.p, (size_t)s->N * sizeof(sa_box));
  return polygon_fixups(e, s);
}

// ---- the upkeep QUEUED BEHIND the association (sa_batch_run_apply / sa_tracks_apply_collect) ----------------------------
// sa_tracks_apply needs the winners on the host before it can queue the upkeep: wait for the frame, fetch, validate, draw ids, launch —
// the GPU idles through a host round trip and the caller waits twice.  When the ids of the tracks that start are a function of the
// winners alone — the reference draws them from a counter in candidate order (sort/simple_api.rs:165-187; Batch*: one per candidate,
// batch_api.rs:102-106) — the device can draw them itself: k_apply_ids turns the winners into (row, id) of every new track and the
// Kalman / feature-bank kernels run right behind the assignment tail on the same stream.  The host learns everything in ONE wait and
// replays the (trivial) id arithmetic for its own copy of the table.
// (1) the wait: the set's Kalman dispatch has retired — the predicted boxes and the table's rows are out (VisualSORT: the feature banks may
// still be moving, the engine stays busy)
static int fused_wait(sa_engine* e, Bank* ob) {
  if (ob && ob->kf_event) {
    hipError_t we = hipEventSynchronize(ob->ev_kf);
    if (we != hipSuccess) return fail(e, SA_ERR_HIP, "hipEventSynchronize failed: %s", hipGetErrorString(we));
  } else if (ob && ob->apply_event) {
    hipError_t we = hipEventSynchronize(ob->ev_apply);
    if (we != hipSuccess) return fail(e, SA_ERR_HIP, "hipEventSynchronize failed: %s", hipGetErrorString(we));
    if (e->busy_seq == ob->apply_seq && !e->copy_dirty) TRY(engine_idle(e));  // (that dispatch was the last thing queued on either stream: drained, without a marker packet)
  } else TRY(engine_sync(e));
  return SA_OK;
}
// (2) the host side of one slot's table: replays the id arithmetic of the kernels, validates the winners.  Touches the slot and its scene only
// (and the error string, under its mutex): different slots may be collected by different threads at once.
// (2a) the table: needs the association's winners only — may run while the Kalman dispatch is still on the device
static int fused_collect_table(sa_engine* e, Slot* s, uint64_t* out_ids) {
  if (s->table_collected) return s->table_bad;
  s->table_collected = true;
  s->table_bad = SA_OK;
  SceneTable* sc = s->scene;
  const uint32_t n = s->N, T0 = s->fused_T0;
  if (!n) return SA_OK;
  const uint64_t* winners = out_view(s).ids();
  const int32_t* wcol = out_view(s).cols();
  if (sc->T != T0) return s->table_bad = fail(e, SA_ERR_STATE, "the scene's track table changed while its upkeep was queued");
  if (int rc = host_ensure(e, s->h_apply, (size_t)n * 4); rc != SA_OK) return s->table_bad = rc;
  uint32_t* h_row = (uint32_t*)s->h_apply.p;
  sc->full.resize(T0, 0);
  uint32_t r = 0;
  int bad = SA_OK;
  for (uint32_t i = 0; i < n; ++i) {   // (a failure is recorded and the replay goes on: the last one's text stands)
    const uint64_t id = winners[i] ? 0 : s->fused_id_base + 1ull + (s->fused_per_candidate ? (uint64_t)i : (uint64_t)r);
    const bool above = !winners[i] && sc->ascending && (sc->ids.empty() || id > sc->ids.back());   // (no search: every tracker of the reference)
    if (int rc = above ? SA_OK : check_upkeep_winner(e, sc, T0, winners[i], wcol[i], id); rc != SA_OK) bad = rc;
    h_row[i] = winners[i] ? SA_NONE : T0 + r++;
    if (!winners[i]) append_id(sc, id);
    if (out_ids) out_ids[i] = id;
  }
  sc->T = T0 + r;
  sc->full.resize(sc->T, 1);
  s->ran = false;  // the table the slot ran against is gone
  s->table_bad = bad;
  return bad;
}
// (2b) what the Kalman dispatch left: the predicted boxes, and whether refreshed rows need their oriented polygons
static int fused_collect_host(sa_engine* e, Slot* s, uint64_t* out_ids, sa_box* out_predicted) {
  s->fused_pending = false;
  const uint32_t n = s->N;
  if (!n) return SA_OK;
  const bool had = s->table_collected;
  int bad = fused_collect_table(e, s, out_ids);
  if (had) bad = s->table_bad;   // (collected earlier, by sa_tracks_apply_collect_table: its verdict stands; the new ids went out there)
  if (out_predicted) std::memcpy(out_predicted, s->h_pred.p, (size_t)n * sizeof(sa_box));
  // (3) polygon_fixups — a launch, left to the thread that owns the engine's stream — only where a refreshed row is oriented
  const sa_box* pb = (const sa_box*)s->h_pred.p;
  s->poly_pending = bad == SA_OK && std::any_of(pb, pb + n, oriented);
  return bad;
}
static Bank* bank_of_slot(sa_engine* e, const Slot* s) {
  for (Bank& bk : e->banks)
    for (uint32_t i = 0; i < bk.n_slots; ++i)
      if (bk.slots[i] == s) return &bk;
  return nullptr;
}
static int fused_collect(sa_engine* e, Slot* s, uint64_t* out_ids, sa_box* out_predicted) {
  HIPCHK(e, hipSetDevice(e->device));
  s->fused_pending = false;
  TRY(fused_wait(e, bank_of_slot(e, s)));
  TRY(fused_collect_host(e, s, out_ids, out_predicted));
  if (!s->poly_pending) return SA_OK;
  s->poly_pending = false;
  return polygon_fixups(e, s);
}

int sa_tracks_apply_end(sa_engine* e, uint32_t slot, sa_box* out_predicted) {
  if (!e) return SA_ERR_BAD_ARG;
  TRY(bound_bank_ok(e, "sa_tracks_apply_end"));
  Slot* s;
  TRY(live_slot(e, slot, &s));
  if (!s->apply_pending) {
    // (an empty frame queues nothing; anything else: finished already by an entry point that needed the table — the boxes are still there)
    if (!s->N) return SA_OK;
    if (s->ran || !s->h_pred.p) return fail(e, SA_ERR_STATE, "sa_tracks_apply_end without sa_tracks_apply_begin");
    if (out_predicted) std::memcpy(out_predicted, s->h_pred.p, (size_t)s->N * sizeof(sa_box));
    return SA_OK;
  }
  return apply_finish(e, s, out_predicted);
}
int sa_tracks_apply(sa_engine* e, uint32_t slot, const uint64_t* new_ids, sa_box* out_predicted) {
  TRY(sa_tracks_apply_begin(e, slot, new_ids));
  return sa_tracks_apply_end(e, slot, out_predicted);
}

int sa_batch_run_apply(sa_engine* e, const uint64_t* id_base, int id_per_candidate) {
  if (!e) return SA_ERR_BAD_ARG;
  HIPCHK(e, hipSetDevice(e->device));
  TRY(finish_applies(e));
  if (e->B_ticket) return fail(e, SA_ERR_STATE, "sa_batch_run_apply works on a synchronous batch (sa_batch_begin / sa_batch_add), not on a waited ticket");
  Bank* b = e->B;
  if (!b->n_slots) return SA_OK;   // (an empty request set: nothing to run, nothing to apply — id_base may be NULL)
  if (!id_base) return fail(e, SA_ERR_BAD_ARG, "sa_batch_run_apply: null argument");
  // every scene's table with room for as many new tracks as it has candidates, the mapped block its predicted boxes land in, the buffer its
  // in-place feature rows are copied to — BEFORE the descriptors and the upkeep arguments are built (a table that grows moves)
  uint32_t kf_blocks = 0, bank_blocks = 0;
  for (uint32_t i = 0; i < b->n_slots; ++i) {
    Slot* s = b->slots[i];
    SceneTable* sc = s->scene;
    sc->full.resize(sc->T, 0);
    TRY(scene_reserve(e, sc, sc->T + s->N));
    s->fused_T0 = sc->T;
    s->fused_id_base = id_base[i];
    s->fused_per_candidate = id_per_candidate ? 1 : 0;
    if (!s->N) continue;
    TRY(mapped_ensure(e, s->h_pred, s->d_pred, (size_t)s->N * sizeof(sa_box)));
    const bool in_place = e->visual && s->has_feats && e->D == e->Dp && s->feats_device && !((uintptr_t)s->feats_device & 15u);
    if (in_place) TRY(dev_ensure(e, s->feat_raw, (size_t)s->N * e->D * 4));
    kf_blocks = std::max(kf_blocks, sa_apply_set_blocks(s->N, in_place, 1));
    bank_blocks = std::max(bank_blocks, sa_apply_set_blocks(s->N, false, 2));
  }
  b->want_apply = true;           // (bank_upload appends the scenes' upkeep arguments to the set's one upload)
  // (run_pipeline, with the end of the ASSOCIATION marked on the stream: the frame's last dispatch carries ev_done as its completion
  // signal, so that sa_batch_fetch can hand out the winners while the upkeep kernels queued below are still running)
  uint32_t maxN = 0, maxT = 0;
  bool rides = false;
  int rc = bank_prepare(e, b, &maxN, &maxT);
  if (rc == SA_OK) rc = bank_upload(e, b, e->stream, true);
  if (rc == SA_OK) rc = bank_launch(e, b, maxN, maxT, b->ev_done, &rides);
  if (rc == SA_OK && !rides) { if (hipEventRecord(b->ev_done, e->stream) != hipSuccess) rc = fail(e, SA_ERR_HIP, "hipEventRecord failed"); }
  b->assoc_event = rc == SA_OK;
  b->assoc_waited.store(false, std::memory_order_relaxed);
  b->want_apply = false;
  if (rc != SA_OK) return rc;
  if (!kf_blocks) return SA_OK;   // (no scene brought a detection)
  // The upkeep of the WHOLE set: one launch for every scene's Kalman step (rows and ids of the tracks that start are drawn inside the
  // kernel, from the winners) and, VisualSORT, one for every scene's feature bank behind it — Batch*::predict over 64 scenes queues two
  // dispatches, not 128.  The predicted boxes (all a caller of sa_tracks_apply_collect needs from the device) are out when the Kalman
  // dispatch retires (ev_kf); the banks (10+ us of row moves at 1000 x 3 x 512 floats) run on behind it; whatever touches the engine
  // next is ordered behind them on the stream, or waits for ev_apply.
  const ApplyScene* as = (const ApplyScene*)((const uint8_t*)b->d_arena.p + b->apply_off);
  if (hipError_t le = sa_launch_apply_set(as, b->n_slots, kf_blocks, e->K, e->P, e->stream, e->visual ? b->ev_kf : b->ev_apply, 1); le != hipSuccess)
    return fail(e, SA_ERR_HIP, "upkeep launch failed: %s", hipGetErrorString(le));
  SA_BUSY(e);
  if (e->visual) {
    b->kf_event = true;
    if (hipError_t le = sa_launch_apply_set(as, b->n_slots, bank_blocks, e->K, e->P, e->stream, b->ev_apply, 2); le != hipSuccess)
      return fail(e, SA_ERR_HIP, "upkeep launch failed: %s", hipGetErrorString(le));
    SA_BUSY(e);
  }
  b->apply_event = true; b->apply_seq = e->busy_seq; e->tail_ev = b->ev_apply; e->tail_seq = e->busy_seq;
  for (uint32_t i = 0; i < b->n_slots; ++i) {
    b->slots[i]->table_collected = false;
    if (b->slots[i]->N) b->slots[i]->fused_pending = true;
  }
  return SA_OK;
}

int sa_tracks_apply_collect(sa_engine* e, uint32_t slot, uint64_t* out_new_ids, sa_box* out_predicted) {
  if (!e) return SA_ERR_BAD_ARG;
  TRY(bound_bank_ok(e, "sa_tracks_apply_collect"));
  Slot* s;
  TRY(live_slot(e, slot, &s));
  if (!s->fused_pending) return s->N ? fail(e, SA_ERR_STATE, "sa_tracks_apply_collect without sa_batch_run_apply (or collected already)") : SA_OK;
  return fused_collect(e, s, out_new_ids, out_predicted);
}

// sa_tracks_apply_collect for a whole request set, in three steps, so that the per-scene host work can be spread over threads
// (Batch*::predict, 64 scenes): _begin waits ONCE for the set's Kalman dispatch; _slot does one scene's host side (ids of the tracks that
// started, predicted boxes) and may run for DIFFERENT slots on different threads at once; _end (the calling thread again) queues the
// polygons of refreshed oriented rows.  Any entry point that needs the finished table completes what is left.
// The host side of ONE scene's table for the upkeep step that sa_batch_run_apply queued — the ids of the tracks that start, the rows
// they take, the checks of the winners — which needs nothing but the association's results: a caller that has them (sa_batch_results)
// may do this while the Kalman dispatch is still running, per slot, on any thread; sa_tracks_apply_collect_slot then only hands out the boxes.
int sa_tracks_apply_collect_table(sa_engine* e, uint32_t slot, uint64_t* out_new_ids) {
  if (!e) return SA_ERR_BAD_ARG;
  bind_device(e);
  Slot* s;
  TRY(live_slot(e, slot, &s));
  if (!s->fused_pending) return s->N ? fail(e, SA_ERR_STATE, "sa_tracks_apply_collect_table without sa_batch_run_apply (or collected already)") : SA_OK;
  if (e->B->assoc_event) TRY(assoc_wait_once(e, e->B));
  return fused_collect_table(e, s, out_new_ids);
}
int sa_tracks_apply_collect_begin(sa_engine* e) {
  if (!e) return SA_ERR_BAD_ARG;
  TRY(bound_bank_ok(e, "sa_tracks_apply_collect_begin"));
  HIPCHK(e, hipSetDevice(e->device));
  bool any = false;
  for (uint32_t i = 0; i < e->B->n_slots; ++i) any = any || e->B->slots[i]->fused_pending;
  if (!any) return SA_OK;
  return fused_wait(e, e->B);
}
int sa_tracks_apply_collect_slot(sa_engine* e, uint32_t slot, uint64_t* out_new_ids, sa_box* out_predicted) {
  if (!e) return SA_ERR_BAD_ARG;
  bind_device(e);
  Slot* s;
  TRY(live_slot(e, slot, &s));
  if (!s->fused_pending) return s->N ? fail(e, SA_ERR_STATE, "sa_tracks_apply_collect_slot without sa_batch_run_apply (or collected already)") : SA_OK;
  return fused_collect_host(e, s, out_new_ids, out_predicted);
}
int sa_tracks_apply_collect_end(sa_engine* e) {
  if (!e) return SA_ERR_BAD_ARG;
  HIPCHK(e, hipSetDevice(e->device));
  for (uint32_t i = 0; i < e->B->n_slots; ++i) {
    Slot* s = e->B->slots[i];
    if (!s->poly_pending) continue;
    s->poly_pending = false;
    TRY(polygon_fixups(e, s));
  }
  return SA_OK;
}

int sa_tracks_get_state(sa_engine* e, uint64_t scene_id, uint64_t id, float* mean10, float* cov100, float* quality, uint8_t* present,
                        float* feats) {
  if (!e) return SA_ERR_BAD_ARG;
  TRY(finish_applies(e));
  SceneTable* sc = get_scene(e, scene_id, false);
  if (!sc) return fail(e, SA_ERR_NOT_FOUND, "unknown scene %llu", (unsigned long long)scene_id);
  uint32_t found_row = 0;
  if (!find_slot(sc, id, &found_row)) return fail(e, SA_ERR_NOT_FOUND, "unknown track id %llu", (unsigned long long)id);
  HIPCHK(e, hipSetDevice(e->device));
  TRY(engine_sync(e));
  const uint32_t r = found_row, K = e->K;
  if (mean10) HIPCHK(e, hipMemcpy(mean10, (float*)sc->kf.p + (size_t)r * 110, 40, hipMemcpyDeviceToHost));
  if (cov100) HIPCHK(e, hipMemcpy(cov100, (float*)sc->kf.p + (size_t)r * 110 + 10, 400, hipMemcpyDeviceToHost));
  if (e->visual) {
    if (quality) HIPCHK(e, hipMemcpy(quality, (float*)sc->fquality.p + (size_t)r * K, (size_t)K * 4, hipMemcpyDeviceToHost));
    if (present) HIPCHK(e, hipMemcpy(present, (uint8_t*)sc->fpresent.p + (size_t)r * K, K, hipMemcpyDeviceToHost));
    if (feats)
      for (uint32_t k = 0; k < K; ++k)
        HIPCHK(e, hipMemcpy(feats + (size_t)k * e->D, (float*)sc->feat.p + ((size_t)r * K + k) * e->Dp, (size_t)e->D * 4, hipMemcpyDeviceToHost));
  }
  return SA_OK;
}

int sa_tracks_set_state(sa_engine* e, uint64_t scene_id, uint64_t id, const float* mean10, const float* cov100, const float* quality) {
  if (!e || !mean10 || !cov100) return fail(e, SA_ERR_BAD_ARG, "sa_tracks_set_state: null argument");
  TRY(finish_applies(e));
  SceneTable* sc = get_scene(e, scene_id, false);
  if (!sc) return fail(e, SA_ERR_NOT_FOUND, "unknown scene %llu", (unsigned long long)scene_id);
  uint32_t found_row = 0;
  if (!find_slot(sc, id, &found_row)) return fail(e, SA_ERR_NOT_FOUND, "unknown track id %llu", (unsigned long long)id);
  HIPCHK(e, hipSetDevice(e->device));
  TRY(engine_sync(e));
  const uint32_t r = found_row, K = e->K;
  HIPCHK(e, hipMemcpy((float*)sc->kf.p + (size_t)r * 110, mean10, 40, hipMemcpyHostToDevice));
  HIPCHK(e, hipMemcpy((float*)sc->kf.p + (size_t)r * 110 + 10, cov100, 400, hipMemcpyHostToDevice));
  if (e->visual && quality) HIPCHK(e, hipMemcpy((float*)sc->fquality.p + (size_t)r * K, quality, (size_t)K * 4, hipMemcpyHostToDevice));
  sc->full.resize(sc->T, 0);
  sc->full[r] = 1;
  return SA_OK;
}

// ---- non-maximum suppression ------------------------------------------------------------------------------
// The host half (nms.rs:36-56): the boxes whose score passes the threshold (no score:
// score.unwrap_or(f32::MAX)) and whose extent is positive, as indices into `boxes`, by rank descending — the score, or the height of a
// box without one — and stable in the caller's order.
static void nms_rank(uint32_t n, const sa_box* boxes, const float* scores, float score_threshold, std::vector<uint32_t>& src) {
  const float thr = score_threshold == score_threshold ? score_threshold : -3.4028234663852886e38f;
  struct Cand { uint32_t src; float rank; };
  std::vector<Cand> c;
  c.reserve(n);
  for (uint32_t i = 0; i < n; ++i) {
    const bool has = scores && scores[i] == scores[i];
    const float sc = has ? scores[i] : 3.4028234663852886e38f;  // score.unwrap_or(f32::MAX) > score_threshold
    if (!(sc > thr && boxes[i].height > 0.0f && boxes[i].aspect > 0.0f)) continue;
    c.push_back({i, has ? scores[i] : boxes[i].height});
  }
  std::stable_sort(c.begin(), c.end(), [](const Cand& a, const Cand& b) { return a.rank > b.rank; });
  src.resize(c.size());
  for (size_t i = 0; i < c.size(); ++i) src[i] = c[i].src;
}
// ---- NMS and own areas of a call's scenes (include/similari_frames.h) ---------------------------------------
// One staging block per call: the BoxRaw rows of every scene back to back, the segment table (sa_frames_plan.h) and — own areas —
// the zeroed status words, one upload; the results lie behind them in the same device block and come back in one copy.  The batch
// calls and the single calls are wrappers around frames_nms / frames_own_areas: a single call is the plan of one scene, with pointers
// to its own arguments.
struct FramesCall {
  const char* who;   // the entry point, as its refusals name it
  bool batch;        // refusals name the scene; the dispatches carry the stamps sa_frames_last's device_ms is read from
};
static std::string frames_where(const FramesCall& c, uint32_t scene) {
  return c.batch ? std::string(c.who) + ": scene " + std::to_string(scene) : std::string(c.who);
}
static_assert(SA_FRAMES_NMS_MAX == SA_NMS_MAX, "one limit for the pair stage");
static int frames_plan_checked(sa_engine* e, const FramesCall& c, uint32_t n_scenes, const uint32_t* counts, bool nms, SaFramesPlan* plan) {
  uint32_t bad = 0;
  switch (sa_frames_plan(n_scenes, counts, nms, plan, &bad)) {
    case SA_FRAMES_FITS: return SA_OK;
    case SA_FRAMES_TOO_MANY_SCENES: return fail(e, SA_ERR_UNSUPPORTED, "%s: at most %u scenes per call (got %u)", c.who, SA_FRAMES_MAX_SCENES, n_scenes);
    case SA_FRAMES_SCENE_TOO_LARGE:
      return fail(e, SA_ERR_UNSUPPORTED, "%s: at most %u boxes pass to the pair stage (got %u)", frames_where(c, bad).c_str(), SA_NMS_MAX, counts[bad]);
    default: return fail(e, SA_ERR_UNSUPPORTED, "%s: more than 2^32 - 1 boxes in one call", frames_where(c, bad).c_str());
  }
}
// What a batch call leaves for sa_frames_last.
static void frames_finish(sa_engine* e, sa_frames_stats& fs) {
  float ms = 0.f;
  if (fs.launches) {
    if (hipEventElapsedTime(&ms, e->ev_t0, e->ev_t1) == hipSuccess) fs.device_ms = ms;
    else (void)hipGetLastError();
  }
  e->frames_last = fs;
}

// exclusively_owned_areas + ..._normalized_shares (clipping/bbox_own_areas.rs:8-46) for the boxes of every scene; fs: what ran.
static int frames_own_areas(sa_engine* e, const FramesCall& c, uint32_t n_scenes, const uint32_t* counts, const sa_box* const* boxes,
                            float* const* out_share, sa_frames_stats& fs) {
  SaFramesPlan plan;
  TRY(frames_plan_checked(e, c, n_scenes, counts, false, &plan));
  for (uint32_t s = 0; s < n_scenes; ++s) {
    if (!counts[s]) continue;
    if (!boxes[s] || !out_share[s]) return fail(e, SA_ERR_BAD_ARG, "%s: null argument", frames_where(c, s).c_str());
    for (uint32_t i = 0; i < counts[s]; ++i) {
      const int rc = check_box(e, boxes[s][i], "boxes", i);
      if (rc == SA_OK) continue;
      if (!c.batch) return rc;   // a single call refuses in check_box's own words
      const std::string why = e->err;
      return fail(e, rc, "%s: %s", frames_where(c, s).c_str(), why.c_str());
    }
  }
  fs.scenes = n_scenes;
  fs.boxes = plan.total;
  if (!plan.total) return SA_OK;
  HIPCHK(e, hipSetDevice(e->device));
  TRY(engine_sync(e));
  const uint32_t total = plan.total;
  const size_t raw_bytes = (size_t)total * sizeof(BoxRaw), seg_bytes = (size_t)n_scenes * sizeof(SaFrameSeg);
  const size_t o_status = raw_bytes + seg_bytes, up_bytes = o_status + (size_t)n_scenes * 4, out_bytes = ((size_t)n_scenes + total) * 4;
  TRY(host_ensure(e, e->up_host, o_status + out_bytes));
  uint8_t* h = (uint8_t*)e->up_host.p;
  for (uint32_t s = 0; s < n_scenes; ++s) fill_raw((BoxRaw*)h + plan.segs[s].first, boxes[s], counts[s]);
  memcpy(h + raw_bytes, plan.segs.data(), seg_bytes);
  memset(h + o_status, 0, (size_t)n_scenes * 4);
  TRY(dev_ensure(e, e->up_raw, o_status + out_bytes));
  uint8_t* d = (uint8_t*)e->up_raw.p;
  const BoxRaw* draw = (const BoxRaw*)d;
  const SaFrameSeg* dsegs = (const SaFrameSeg*)(d + raw_bytes);
  uint32_t* dstatus = (uint32_t*)(d + o_status);
  float* dshare = (float*)(dstatus + n_scenes);
  hipStream_t st = e->stream;
  hipEvent_t ev0 = c.batch ? e->ev_t0 : nullptr, ev1 = c.batch ? e->ev_t1 : nullptr;
  HIPCHK(e, hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, st));
  HIPCHK(e, sa_launch_own_areas(draw, dsegs, n_scenes, plan.max_count, dshare, dstatus, st, ev0, ev1));
  HIPCHK(e, hipMemcpyAsync(h + o_status, dstatus, out_bytes, hipMemcpyDeviceToHost, st));
  SA_BUSY(e);
  TRY(engine_sync(e));
  fs.launches = 1;
  fs.host_waits = 1;
  fs.bytes_h2d = up_bytes;
  fs.bytes_d2h = out_bytes;
  const uint32_t* hstatus = (const uint32_t*)(h + o_status);
  const float* hshare = (const float*)(hstatus + n_scenes);
  // The boxes the LDS-resident kernel gave up on (NaN shares: more than 127 overlapping neighbours, or more than 24 disjoint covered
  // stretches on one edge) of every scene whose status word says so: the spill path, in lists of SA_FRAMES_SPILL_LIST that share one
  // block of HBM scratch, sized by the largest scene among them.  bbox_own_areas.rs has no limit.
  std::vector<uint2> todo;
  uint32_t max_n = 0;
  for (uint32_t s = 0; s < n_scenes; ++s) {
    if (!(hstatus[s] & 3u)) continue;
    const SaFrameSeg& g = plan.segs[s];
    for (uint32_t i = 0; i < g.count; ++i)
      if (hshare[g.first + i] != hshare[g.first + i]) todo.push_back(make_uint2(s, i));
    max_n = std::max(max_n, g.count);
  }
  if (!todo.empty()) {
    const uint32_t batch = SA_FRAMES_SPILL_LIST;
    DevBuf scratch, dlist;
    int rc = dev_ensure(e, scratch, sa_own_big_scratch_bytes(max_n, batch));
    if (rc == SA_OK) rc = dev_ensure(e, dlist, todo.size() * sizeof(uint2));
    if (rc == SA_OK && hipMemcpyAsync(dlist.p, todo.data(), todo.size() * sizeof(uint2), hipMemcpyHostToDevice, st) != hipSuccess)
      rc = fail(e, SA_ERR_HIP, "%s: list upload failed", c.who);
    for (size_t o = 0; rc == SA_OK && o < todo.size(); o += batch) {
      const uint32_t cnt = (uint32_t)std::min<size_t>(batch, todo.size() - o);
      const bool last = o + batch >= todo.size();
      if (sa_launch_own_areas_big(draw, dsegs, max_n, (const uint2*)dlist.p + o, cnt, dshare, dstatus, scratch.p, st, last ? ev1 : nullptr) != hipSuccess)
        rc = fail(e, SA_ERR_HIP, "%s: spill launch failed: %s", c.who, hipGetErrorString(hipGetLastError()));
      ++fs.launches;
    }
    if (rc == SA_OK && hipMemcpyAsync(h + o_status, dstatus, out_bytes, hipMemcpyDeviceToHost, st) != hipSuccess)
      rc = fail(e, SA_ERR_HIP, "%s: result copy failed", c.who);
    SA_BUSY(e);
    const int rs = engine_sync(e);
    if (scratch.p) hipFree(scratch.p);
    if (dlist.p) hipFree(dlist.p);
    if (rc != SA_OK) return rc;
    if (rs != SA_OK) return rs;
    fs.spilled = (uint32_t)todo.size();
    fs.host_waits = 2;
    fs.bytes_h2d += todo.size() * sizeof(uint2);
    fs.bytes_d2h += out_bytes;
    for (uint32_t s = 0; s < n_scenes; ++s)
      if (hstatus[s] & 4u)
        return fail(e, SA_ERR_UNSUPPORTED, "%s: more than 512 disjoint stretches of one box edge are covered by other boxes", frames_where(c, s).c_str());
  }
  for (uint32_t s = 0; s < n_scenes; ++s)
    if (counts[s]) memcpy(out_share[s], hshare + plan.segs[s].first, (size_t)counts[s] * 4);
  return SA_OK;
}

// Non-maximum suppression of every scene: the host half (nms_rank), then the pair masks and the sweeps on the device; fs: what ran.
static int frames_nms(sa_engine* e, const FramesCall& c, uint32_t n_scenes, const uint32_t* counts, const sa_box* const* boxes,
                      const float* const* scores, float nms_threshold, float score_threshold, uint32_t* const* out_keep, uint32_t* out_n,
                      sa_frames_stats& fs) {
  if (n_scenes > SA_FRAMES_MAX_SCENES)
    return fail(e, SA_ERR_UNSUPPORTED, "%s: at most %u scenes per call (got %u)", c.who, SA_FRAMES_MAX_SCENES, n_scenes);
  for (uint32_t s = 0; s < n_scenes; ++s)
    if (counts[s] && (!boxes[s] || !out_keep[s])) return fail(e, SA_ERR_BAD_ARG, "%s: null argument", frames_where(c, s).c_str());
  std::vector<std::vector<uint32_t>> src(n_scenes);
  std::vector<uint32_t> m(n_scenes);
  for (uint32_t s = 0; s < n_scenes; ++s) {
    if (counts[s]) nms_rank(counts[s], boxes[s], scores ? scores[s] : nullptr, score_threshold, src[s]);
    m[s] = (uint32_t)src[s].size();
  }
  SaFramesPlan plan;
  TRY(frames_plan_checked(e, c, n_scenes, m.data(), true, &plan));
  fs.scenes = n_scenes;
  fs.boxes = plan.total;
  if (!plan.total) {
    for (uint32_t s = 0; s < n_scenes; ++s) out_n[s] = 0;
    return SA_OK;
  }
  HIPCHK(e, hipSetDevice(e->device));
  TRY(engine_sync(e));
  const uint32_t total = plan.total;
  const size_t raw_bytes = (size_t)total * sizeof(BoxRaw), seg_bytes = (size_t)n_scenes * sizeof(SaFrameSeg), up_bytes = raw_bytes + seg_bytes;
  TRY(host_ensure(e, e->up_host, up_bytes + total));
  uint8_t* h = (uint8_t*)e->up_host.p;
  std::vector<sa_box> sorted(total);
  for (uint32_t s = 0; s < n_scenes; ++s)
    for (uint32_t i = 0; i < m[s]; ++i) sorted[plan.segs[s].first + i] = boxes[s][src[s][i]];
  fill_raw((BoxRaw*)h, sorted.data(), total);  // libm cos / sin of the angle, as for every other box
  memcpy(h + raw_bytes, plan.segs.data(), seg_bytes);
  TRY(dev_ensure(e, e->up_raw, up_bytes + total));
  TRY(dev_ensure(e, e->nms_mask, (size_t)plan.mask_words * 8));
  uint8_t* d = (uint8_t*)e->up_raw.p;
  uint8_t* dkeep = d + up_bytes;
  hipStream_t st = e->stream;
  HIPCHK(e, hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, st));
  HIPCHK(e, sa_launch_nms((const BoxRaw*)d, (const SaFrameSeg*)(d + raw_bytes), n_scenes, plan.max_count, plan.sweep_S, nms_threshold,
                          (uint64_t*)e->nms_mask.p, dkeep, st, c.batch ? e->ev_t0 : nullptr, c.batch ? e->ev_t1 : nullptr));
  const uint8_t* hkeep = h + up_bytes;
  HIPCHK(e, hipMemcpyAsync(h + up_bytes, dkeep, total, hipMemcpyDeviceToHost, st));
  SA_BUSY(e);
  TRY(engine_sync(e));
  for (uint32_t s = 0; s < n_scenes; ++s) {
    uint32_t k = 0;
    for (uint32_t i = 0; i < m[s]; ++i)
      if (hkeep[plan.segs[s].first + i]) out_keep[s][k++] = src[s][i];
    out_n[s] = k;
  }
  fs.launches = 2;
  fs.host_waits = 1;
  fs.bytes_h2d = up_bytes;
  fs.bytes_d2h = total;
  return SA_OK;
}

int sa_nms(sa_engine* e, uint32_t n, const sa_box* boxes, const float* scores, float nms_threshold, float score_threshold,
           uint32_t* out_keep, uint32_t* out_n) {
  if (!e || !out_n || (n && (!boxes || !out_keep))) return fail(e, SA_ERR_BAD_ARG, "sa_nms: null argument");
  *out_n = 0;
  if (!n) return SA_OK;
  sa_frames_stats fs{};
  return frames_nms(e, FramesCall{"sa_nms", false}, 1, &n, &boxes, &scores, nms_threshold, score_threshold, &out_keep, out_n, fs);
}
int sa_own_areas(sa_engine* e, uint32_t n, const sa_box* boxes, float* out_share) {
  if (!e || (n && (!boxes || !out_share))) return fail(e, SA_ERR_BAD_ARG, "sa_own_areas: null argument");
  if (!n) return SA_OK;
  sa_frames_stats fs{};
  return frames_own_areas(e, FramesCall{"sa_own_areas", false}, 1, &n, &boxes, &out_share, fs);
}

int sa_own_areas_batch(sa_engine* e, uint32_t n_scenes, const uint32_t* counts, const sa_box* const* boxes, float* const* out_share) {
  if (!e) return fail(e, SA_ERR_BAD_ARG, "sa_own_areas_batch: null engine");
  e->frames_last = sa_frames_stats{};
  if (!n_scenes) return SA_OK;
  if (!counts || !boxes || !out_share) return fail(e, SA_ERR_BAD_ARG, "sa_own_areas_batch: null argument");
  sa_frames_stats fs{};
  TRY(frames_own_areas(e, FramesCall{"sa_own_areas_batch", true}, n_scenes, counts, boxes, out_share, fs));
  frames_finish(e, fs);
  return SA_OK;
}
int sa_nms_batch(sa_engine* e, uint32_t n_scenes, const uint32_t* counts, const sa_box* const* boxes, const float* const* scores,
                 float nms_threshold, float score_threshold, uint32_t* const* out_keep, uint32_t* out_n) {
  if (!e) return fail(e, SA_ERR_BAD_ARG, "sa_nms_batch: null engine");
  e->frames_last = sa_frames_stats{};
  if (!n_scenes) return SA_OK;
  if (!counts || !boxes || !out_keep || !out_n) return fail(e, SA_ERR_BAD_ARG, "sa_nms_batch: null argument");
  sa_frames_stats fs{};
  TRY(frames_nms(e, FramesCall{"sa_nms_batch", true}, n_scenes, counts, boxes, scores, nms_threshold, score_threshold, out_keep, out_n, fs));
  frames_finish(e, fs);
  return SA_OK;
}

int sa_frames_last(sa_engine* e, sa_frames_stats* out) {
  if (!e || !out) return fail(e, SA_ERR_BAD_ARG, "sa_frames_last: null argument");
  *out = e->frames_last;
  out->struct_size = (uint32_t)sizeof(sa_frames_stats);
  return SA_OK;
}

// ---- parity taps ----------------------------------------------------------------------------------------
static int tap_slot(sa_engine* e, uint32_t slot, Slot** out) {
  if (!e) return SA_ERR_BAD_ARG;
  TRY(bound_bank_ok(e, "tap"));
  Slot* s;
  TRY(live_slot(e, slot, &s));
  if (!s->ran) return fail(e, SA_ERR_STATE, "tap before sa_batch_run");
  HIPCHK(e, hipSetDevice(e->device));
  if (!e->synced) TRY(engine_sync(e));
  *out = s;
  return SA_OK;
}
int sa_tap_dims(sa_engine* e, uint32_t slot, uint32_t* n, uint32_t* t, uint32_t* k) {
  Slot* s;
  TRY(tap_slot(e, slot, &s));
  if (n) *n = s->N;
  if (t) *t = s->T;
  if (k) *k = e->K;
  return SA_OK;
}
// The product path never writes the dense positional matrix (the positional tiles emit the edges of the vote directly); the taps
// recompute it on demand from the slot's resident inputs with the DENSE specialisation of the same kernel, which touches no
// assignment state.  Valid until the slot's scene is upserted or re-staged.
static int dense_positional(sa_engine* e, Slot* s) {
  const size_t cells = (size_t)s->N * s->T;
  if (!cells) return SA_OK;
  TRY(dev_ensure(e, s->pos, cells * 4));
  SceneDev h;
  fill_scene_dev(e, e->B, s, &h);
  DevBuf tmp;
  TRY(dev_ensure(e, tmp, sizeof h));
  HIPCHK(e, hipMemcpy(tmp.p, &h, sizeof h, hipMemcpyHostToDevice));
  HIPCHK(e, sa_launch_positional_dense((const SceneDev*)tmp.p, 1, s->N, s->T, e->P, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  hipFree(tmp.p);
  return SA_OK;
}
int sa_tap_positional(sa_engine* e, uint32_t slot, float* out) {
  Slot* s;
  TRY(tap_slot(e, slot, &s));
  if (!out) return fail(e, SA_ERR_BAD_ARG, "null output");
  TRY(dense_positional(e, s));
  size_t bytes = (size_t)s->N * s->T * 4;
  if (bytes) HIPCHK(e, hipMemcpy(out, s->pos.p, bytes, hipMemcpyDeviceToHost));
  return SA_OK;
}
int sa_tap_visual(sa_engine* e, uint32_t slot, float* out) {
  Slot* s;
  TRY(tap_slot(e, slot, &s));
  if (!e->visual) return fail(e, SA_ERR_UNSUPPORTED, "engine has no visual part");
  if (!out) return fail(e, SA_ERR_BAD_ARG, "null output");
  size_t bytes = (size_t)s->N * s->T * e->K * 4;
  if (!bytes) return SA_OK;
  TRY(ensure_prepped(e, e->B));
  if (e->B->plan.partials || e->bf_words_euclid || e->B->plan.vote == SaVote::class_words) {
    // the product path never wrote the weight matrix (class words of deeper banks: neither) (euclidean: not on frames that used the vote words — re-running is harmless otherwise): run the contraction once more, in matrix mode, on the slot's resident inputs
    SceneDev h;
    fill_scene_dev(e, e->B, s, &h);
    DevBuf tmp;
    TRY(dev_ensure(e, tmp, sizeof h));
    HIPCHK(e, hipMemcpy(tmp.p, &h, sizeof h, hipMemcpyHostToDevice));
    SaParams P = e->P;
    P.eu_mfma = e->B->plan.eu_mfma ? 1u : 0u;  // the kernel the slot's descriptor (tile grid) was laid out for
    P.eu_rho = e->eu_rho;
    HIPCHK(e, sa_launch_visual((const SceneDev*)tmp.p, 1, s->N, s->T * e->K, P, e->stream, false));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    hipFree(tmp.p);
  }
  HIPCHK(e, hipMemcpy(out, s->vis.p, bytes, hipMemcpyDeviceToHost));
  return SA_OK;
}
int sa_tap_quantised(sa_engine* e, uint32_t slot, int64_t* out) {
  Slot* s;
  TRY(tap_slot(e, slot, &s));
  if (!out) return fail(e, SA_ERR_BAD_ARG, "null output");
  size_t cells = (size_t)s->N * s->T;
  if (!cells) return SA_OK;
  TRY(dense_positional(e, s));
  TRY(dev_ensure(e, s->quant, cells * 8));
  // one-scene descriptor array with the tap buffer attached
  SceneDev h;
  fill_scene_dev(e, e->B, s, &h);
  DevBuf tmp;
  TRY(dev_ensure(e, tmp, sizeof h));
  HIPCHK(e, hipMemcpy(tmp.p, &h, sizeof h, hipMemcpyHostToDevice));
  HIPCHK(e, sa_launch_quant_tap((const SceneDev*)tmp.p, 1, s->N, s->T, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, hipMemcpy(out, s->quant.p, cells * 8, hipMemcpyDeviceToHost));
  hipFree(tmp.p);
  return SA_OK;
}

// The polygons of a scene's track table (f64 vertices, 8 per row in table order): what the IoU cells clip against.
int sa_tap_track_polygons(sa_engine* e, uint64_t scene_id, double* out, uint32_t cap_rows, uint32_t* out_rows) {
  if (!e || !out_rows) return fail(e, SA_ERR_BAD_ARG, "sa_tap_track_polygons: null argument");
  TRY(finish_applies(e));
  SceneTable* sc = get_scene(e, scene_id, false);
  *out_rows = sc ? sc->T : 0;
  if (!sc || !sc->T || !out || cap_rows < sc->T) return SA_OK;
  HIPCHK(e, hipSetDevice(e->device));
  TRY(engine_sync(e));
  HIPCHK(e, hipMemcpy(out, sc->verts.p, (size_t)sc->T * 64, hipMemcpyDeviceToHost));
  return SA_OK;
}

// What the frame's OWN launches produced (SA_FLAG_TAP): the BestFit vote as the first phase reduced it.
int sa_tap_votes(sa_engine* e, uint32_t slot, double* row_w, int32_t* row_idx, double* col_w, int32_t* col_idx, int32_t* kind) {
  Slot* s;
  TRY(tap_slot(e, slot, &s));
  if (!e->visual) return fail(e, SA_ERR_UNSUPPORTED, "engine has no visual part");
  if (!(e->cfg.flags & SA_FLAG_TAP) || !s->tap.p) return fail(e, SA_ERR_STATE, "sa_tap_votes needs an engine created with SA_FLAG_TAP");
  if (!row_w || !row_idx || !col_w || !col_idx || !kind) return fail(e, SA_ERR_BAD_ARG, "null output");
  const Bank* b = e->B;
  const uint32_t N = s->N, T = s->T;
  *kind = (b->plan.partials || b->plan.vote == SaVote::cell_words) ? 1 : 2;
  if (!N || !T) return SA_OK;
  if (b->plan.vote == SaVote::class_words) {
    // class words (the whole-track tiles of the contraction): [N K] then [T K], (key of the f32 sum of a group's weights << 32 | index) per count class;
    // the group weight the tail compares is W = c max_dist - sum with the frame's max_dist folded from the first phase's slots
    const uint32_t K = e->K;
    std::vector<unsigned long long> w(((size_t)N + T) * K);
    HIPCHK(e, hipMemcpy(w.data(), s->tap.p, w.size() * 8, hipMemcpyDeviceToHost));
    const uint32_t nkeys = ((N + 63) / 64) * ((T + 64 / K - 1) / (64 / K));
    std::vector<uint32_t> keys(nkeys);
    HIPCHK(e, hipMemcpy(keys.data(), s->vis_max_key.p, (size_t)nkeys * 4, hipMemcpyDeviceToHost));
    uint32_t mk = 0;
    for (uint32_t v : keys) mk = v > mk ? v : mk;
    const double max_dist = mk ? (double)sa_key_f32(mk) : -1.0;
    auto best = [&](const unsigned long long* cls, double* wt, int32_t* idx) {
      *wt = NAN; *idx = -1;
      for (uint32_t c = 0; c < K; ++c) {
        if (cls[c] == ~0ull) continue;
        const double W = (double)(c + 1) * max_dist - (double)sa_key_f32((uint32_t)(cls[c] >> 32));
        const int32_t i = (int32_t)(uint32_t)cls[c];
        if (*idx < 0 || W > *wt || (W == *wt && i < *idx)) { *wt = W; *idx = i; }
      }
    };
    for (uint32_t i = 0; i < N; ++i) best(w.data() + (size_t)i * K, &row_w[i], &row_idx[i]);
    for (uint32_t j = 0; j < T; ++j) best(w.data() + ((size_t)N + j) * K, &col_w[j], &col_idx[j]);
    return SA_OK;
  }
  if (b->plan.vote != SaVote::resolve) {
    std::vector<unsigned long long> w((size_t)N + T);
    HIPCHK(e, hipMemcpy(w.data(), s->tap.p, (size_t)N * 8, hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(w.data() + N, (unsigned long long*)s->tap.p + (N ? N : 1), (size_t)T * 8, hipMemcpyDeviceToHost));
    auto decode = [&](unsigned long long word, double* wt, int32_t* idx) {
      if (word == ~0ull) { *wt = NAN; *idx = -1; return; }
      if (b->plan.vote == SaVote::cell_words) {  // (order-preserving key of the f32 weight << 32) | index
        *wt = (double)sa_key_f32((uint32_t)(word >> 32));
        *idx = (int32_t)(uint32_t)word;
      } else {              // ((2^54 - 1 - key54) << 10) | index, key54 = (f64 bits >> 9) + 1   (sa_vote_word10, sa_kernels.hip)
        const unsigned long long key = ((1ull << 54) - 1ull) - (word >> 10);
        const unsigned long long bits = (key - 1ull) << 9;
        double v;
        std::memcpy(&v, &bits, 8);
        *wt = v;
        *idx = (int32_t)(word & 1023u);
      }
    };
    for (uint32_t i = 0; i < N; ++i) decode(w[i], &row_w[i], &row_idx[i]);
    for (uint32_t j = 0; j < T; ++j) decode(w[(size_t)N + j], &col_w[j], &col_idx[j]);
    return SA_OK;
  }
  // beyond the vote words: the per-tile partials, folded the way k_bestfit_resolve folds them (tiles ascend with the index; the first
  // tile that attains the best weight keeps it).  RAW (bank depth 1): lightest weight wins; else heaviest group weight.
  const bool raw = b->plan.partials;
  const uint32_t CT = raw ? (T + b->tile_bn - 1) / b->tile_bn : (T + 63) / 64, RT = raw ? (N + b->tile_bm - 1) / b->tile_bm : (N + 63) / 64;
  std::vector<double> rw((size_t)CT * N), cw((size_t)RT * T);
  std::vector<int32_t> rt_((size_t)CT * N);
  std::vector<uint32_t> cq((size_t)RT * T);
  HIPCHK(e, hipMemcpy(rw.data(), s->row_part_w.p, rw.size() * 8, hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(rt_.data(), s->row_part_t.p, rt_.size() * 4, hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(cw.data(), s->col_part_w.p, cw.size() * 8, hipMemcpyDeviceToHost));
  HIPCHK(e, hipMemcpy(cq.data(), s->col_part_q.p, cq.size() * 4, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < N; ++i) {
    double bw = 0.0;
    int32_t bi = -1;
    for (uint32_t ct = 0; ct < CT; ++ct) {
      const int32_t t = rt_[(size_t)ct * N + i];
      const double w = rw[(size_t)ct * N + i];
      if (t >= 0 && (bi < 0 || (raw ? w < bw : w > bw))) { bw = w; bi = t; }
    }
    row_w[i] = bi >= 0 ? bw : NAN;
    row_idx[i] = bi;
  }
  for (uint32_t j = 0; j < T; ++j) {
    double bw = 0.0;
    int32_t bi = -1;
    for (uint32_t rt = 0; rt < RT; ++rt) {
      const uint32_t q = cq[(size_t)rt * T + j];
      const double w = cw[(size_t)rt * T + j];
      if (q != SA_NONE && (bi < 0 || (raw ? w < bw : w > bw))) { bw = w; bi = (int32_t)q; }
    }
    col_w[j] = bi >= 0 ? bw : NAN;
    col_idx[j] = bi;
  }
  return SA_OK;
}

// ... and the edges the positional tiles emitted (the records stay in e_edge; the tail copied the counts out before it cleared them).
int sa_tap_edges(sa_engine* e, uint32_t slot, uint32_t* counts, uint32_t cap, uint32_t* cols, int64_t* gains, uint32_t* out_total) {
  Slot* s;
  TRY(tap_slot(e, slot, &s));
  if (!(e->cfg.flags & SA_FLAG_TAP) || !s->tap.p) return fail(e, SA_ERR_STATE, "sa_tap_edges needs an engine created with SA_FLAG_TAP");
  if (!counts || !out_total) return fail(e, SA_ERR_BAD_ARG, "null output");
  const uint32_t N = s->N, T = s->T;
  *out_total = 0;
  if (!N) return SA_OK;
  HIPCHK(e, hipMemcpy(counts, (unsigned long long*)s->tap.p + ((size_t)(N ? N : 1) + (T ? T : 1)) * (e->B->plan.vote == SaVote::class_words ? e->K : 1), (size_t)N * 4, hipMemcpyDeviceToHost));
  uint64_t total = 0;
  uint32_t maxc = 0;
  for (uint32_t i = 0; i < N; ++i) { total += counts[i]; maxc = counts[i] > maxc ? counts[i] : maxc; }
  if (total > 0xffffffffull || maxc > T) return fail(e, SA_ERR_STATE, "sa_tap_edges: implausible edge counts (the slot did not run with the tap?)");
  *out_total = (uint32_t)total;
  if (!total || cap < total) return SA_OK;
  if (!cols || !gains) return fail(e, SA_ERR_BAD_ARG, "null output");
  // the first maxc records of every row: slot-major lists (one-workgroup tail) are maxc contiguous runs of N records,
  // row-major lists (general tail) N runs of maxc records, `estride` records apart
  const bool slot_major = e->B->plan.tail != SaTail::general;
  const size_t estride = T ? T : 1;
  std::vector<SaEdge> h((size_t)maxc * N);
  if (slot_major) HIPCHK(e, hipMemcpy(h.data(), s->e_edge.p, h.size() * sizeof(SaEdge), hipMemcpyDeviceToHost));
  else HIPCHK(e, hipMemcpy2D(h.data(), (size_t)maxc * sizeof(SaEdge), s->e_edge.p, estride * sizeof(SaEdge), (size_t)maxc * sizeof(SaEdge), N, hipMemcpyDeviceToHost));
  size_t o = 0;
  for (uint32_t i = 0; i < N; ++i)
    for (uint32_t k = 0; k < counts[i]; ++k, ++o) {
      const SaEdge& ed = slot_major ? h[(size_t)k * N + i] : h[(size_t)i * maxc + k];
      cols[o] = ed.col;
      gains[o] = ed.gain;
    }
  return SA_OK;
}

// ---- measurement ----------------------------------------------------------------------------------------
int sa_profile_enable(sa_engine* e, int on) {
  if (!e) return SA_ERR_BAD_ARG;
  TRY(engine_sync(e));
  e->profile = on != 0;
  return SA_OK;
}
int sa_profile_reset(sa_engine* e) {
  if (!e) return SA_ERR_BAD_ARG;
  TRY(engine_sync(e));
  for (int i = 0; i < KID_COUNT; ++i) { e->prof_ms[i] = 0; e->prof_n[i] = 0; }
  return SA_OK;
}
int sa_profile_read(sa_engine* e, sa_kernel_stat* out, uint32_t cap, uint32_t* out_n) {
  if (!e || !out_n) return SA_ERR_BAD_ARG;
  TRY(engine_sync(e));
  uint32_t n = 0;
  for (int i = 0; i < KID_COUNT; ++i) {
    if (!e->prof_n[i]) continue;
    if (out && n < cap) {
      std::memset(&out[n], 0, sizeof out[n]);
      std::snprintf(out[n].name, sizeof out[n].name, "%s", kKernelNames[i]);
      out[n].launches = e->prof_n[i];
      out[n].total_ms = e->prof_ms[i];
    }
    ++n;
  }
  *out_n = n;
  return SA_OK;
}
int sa_batch_time(sa_engine* e, uint32_t iters, double* out_ms_total) {
  if (!e || !out_ms_total) return SA_ERR_BAD_ARG;
  TRY(finish_applies(e));
  HIPCHK(e, hipSetDevice(e->device));
  TRY(engine_sync(e));
  HIPCHK(e, hipEventRecord(e->ev_t0, e->stream));
  for (uint32_t i = 0; i < iters; ++i) TRY(run_pipeline(e));
  HIPCHK(e, hipEventRecord(e->ev_t1, e->stream));
  TRY(engine_sync(e));
  float ms = 0.f;
  HIPCHK(e, hipEventElapsedTime(&ms, e->ev_t0, e->ev_t1));
  *out_ms_total = ms;
  return SA_OK;
}

int sa_feature_distance_matrix(sa_engine* e, int32_t kind, uint32_t n, uint32_t t, uint32_t d, const float* a,
                               const float* b, float* out, uint32_t iters, double* out_ms_total) {
  if (!e || !a || !b || !n || !t || !d) return fail(e, SA_ERR_BAD_ARG, "sa_feature_distance_matrix: bad argument");
  if (kind != SA_VIS_COSINE && kind != SA_VIS_EUCLIDEAN) return fail(e, SA_ERR_BAD_ARG, "kind must be cosine or euclidean");
  HIPCHK(e, hipSetDevice(e->device));
  TRY(engine_sync(e));
  const uint32_t d8 = (d + 31u) / 32u * 32u;
  DevBuf ra, rb, pa, pb, na, nb, o;
  TRY(dev_ensure(e, ra, (size_t)n * d * 4));
  TRY(dev_ensure(e, rb, (size_t)t * d * 4));
  TRY(dev_ensure(e, pa, (size_t)n * d8 * 4));
  TRY(dev_ensure(e, pb, (size_t)t * d8 * 4));
  TRY(dev_ensure(e, na, (size_t)n * 4));
  TRY(dev_ensure(e, nb, (size_t)t * 4));
  TRY(dev_ensure(e, o, (size_t)n * t * 4));
  int rc = SA_OK;
  do {
    hipStream_t st = e->stream;
    if (hipMemcpyAsync(ra.p, a, (size_t)n * d * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(rb.p, b, (size_t)t * d * 4, hipMemcpyHostToDevice, st) != hipSuccess) { rc = fail(e, SA_ERR_HIP, "H2D copy failed"); break; }
    if (sa_launch_pad_features((const float*)ra.p, n, d, d8, 1, nullptr, nullptr, (float*)pa.p, (float*)na.p, nullptr, nullptr, st) != hipSuccess ||
        sa_launch_pad_features((const float*)rb.p, t, d, d8, 1, nullptr, nullptr, (float*)pb.p, (float*)nb.p, nullptr, nullptr, st) != hipSuccess) { rc = fail(e, SA_ERR_HIP, "pad launch failed"); break; }
    // operands the plan's tile form reads in fragment order (sa_tile_plan.h; sa_gemm.hip: sa_frag_index): padded := its reordered copy
    const SaTileForm form = sa_tile_form(SaTileUse::matrix, sa_tile_resolve(SaTileUse::matrix, n, t, 1, d8, e->P.gemm_plan, false));
    auto reorder = [&](DevBuf& padded, DevBuf& spare, uint32_t rows, uint32_t round) {
      if (dev_ensure(e, spare, (size_t)((rows + round - 1u) / round * round) * d8 * 4) != SA_OK) return (int)SA_ERR_HIP;
      if (sa_launch_frag_reorder((const float*)padded.p, rows, d8, (float*)spare.p, st) != hipSuccess) return fail(e, SA_ERR_HIP, "reorder launch failed");
      std::swap(padded, spare);
      return (int)SA_OK;
    };
    if (kind == SA_VIS_COSINE && form.b_frag && (rc = reorder(pb, rb, t, 32u)) != SA_OK) break;
    if (kind == SA_VIS_COSINE && form.a_frag && (rc = reorder(pa, ra, n, 64u)) != SA_OK) break;
    // one warm-up launch, then `iters` timed launches of the contraction kernel alone
    if (sa_launch_distance_matrix(kind, (const float*)pa.p, (const float*)na.p, (const float*)pb.p, (const float*)nb.p, n, t, d8, (float*)o.p, st, e->P.gemm_plan) != hipSuccess) { rc = fail(e, SA_ERR_HIP, "kernel launch failed"); break; }
    hipEventRecord(e->ev_t0, st);
    for (uint32_t i = 0; i < iters; ++i)
      sa_launch_distance_matrix(kind, (const float*)pa.p, (const float*)na.p, (const float*)pb.p, (const float*)nb.p, n, t, d8, (float*)o.p, st, e->P.gemm_plan);
    hipEventRecord(e->ev_t1, st);
    if (hipStreamSynchronize(st) != hipSuccess) { rc = fail(e, SA_ERR_HIP, "stream sync failed: %s", hipGetErrorString(hipGetLastError())); break; }
    float ms = 0.f;
    hipEventElapsedTime(&ms, e->ev_t0, e->ev_t1);
    if (out_ms_total) *out_ms_total = ms;
    if (out && hipMemcpy(out, o.p, (size_t)n * t * 4, hipMemcpyDeviceToHost) != hipSuccess) { rc = fail(e, SA_ERR_HIP, "D2H copy failed"); break; }
  } while (0);
  hipStreamSynchronize(e->stream);
  for (DevBuf* bf : {&ra, &rb, &pa, &pb, &na, &nb, &o}) if (bf->p) hipFree(bf->p);
  return rc;
}

}  // extern "C"

// ---- what a feature store (sa_search.hip) shares with its engine: the device, the stream, the error slot ----
int sa_engine_drain(sa_engine* e, int* device, hipStream_t* stream) {
  HIPCHK(e, hipSetDevice(e->device));
  TRY(engine_sync(e));
  *device = e->device;
  *stream = e->stream;
  return SA_OK;
}
int sa_engine_fail(sa_engine* e, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return fail(e, code, "%s", buf);
}
bool sa_engine_bank_shape(const sa_engine* e, uint32_t* K, uint32_t* D, uint32_t* Dp) {
  *K = e->K, *D = e->D, *Dp = e->Dp;
  return e->visual;
}
int sa_engine_waste_resolve(sa_engine* e, const char* what, uint32_t n_scenes, const uint64_t* scene_ids, const uint32_t* counts,
                            const uint64_t* const* ids, std::vector<SaWasteScene>* scenes, std::vector<uint32_t>* rows) {
  TRY(finish_applies(e));
  std::vector<SceneTable*> seen;
  uint32_t first = 0;
  for (uint32_t i = 0; i < n_scenes; ++i) {
    if (!counts[i]) continue;
    if (!ids[i]) return fail(e, SA_ERR_BAD_ARG, "%s: null id list", what);
    SceneTable* sc = get_scene(e, scene_ids[i], false);
    if (!sc) return fail(e, SA_ERR_NOT_FOUND, "%s: unknown scene %llu", what, (unsigned long long)scene_ids[i]);
    for (SceneTable* other : seen)
      if (other == sc) return fail(e, SA_ERR_BAD_ARG, "%s: scene %llu appears twice in one call", what, (unsigned long long)scene_ids[i]);
    seen.push_back(sc);
    for (uint32_t j = 0; j < counts[i]; ++j) {
      uint32_t at;
      if (!find_slot(sc, ids[i][j], &at)) return fail(e, SA_ERR_NOT_FOUND, "%s: unknown track id %llu", what, (unsigned long long)ids[i][j]);
      rows->push_back(at);
    }
    scenes->push_back(SaWasteScene{(const float*)sc->feat.p, (const uint8_t*)sc->fpresent.p, (const float*)sc->fquality.p, first, counts[i]});
    first += counts[i];
  }
  return SA_OK;
}
int sa_engine_ensure(sa_engine* e, DevBuf& b, size_t bytes, bool keep) { return dev_ensure(e, b, bytes, keep); }
void sa_engine_free(DevBuf& b) { free_dev(b); }
SaPoseNms*& sa_engine_pose_nms(sa_engine* e) { return e->pose_nms; }
int sa_engine_device(const sa_engine* e) { return e->device; }
void sa_engine_attach_store(sa_engine* e, sa_store* s) { e->stores.push_back(s); }
void sa_engine_detach_store(sa_engine* e, sa_store* s) { e->stores.erase(std::remove(e->stores.begin(), e->stores.end(), s), e->stores.end()); }
void sa_engine_attach_points(sa_engine* e, sa_points* b) { e->point_banks.push_back(b); }
void sa_engine_detach_points(sa_engine* e, sa_points* b) {
  e->point_banks.erase(std::remove(e->point_banks.begin(), e->point_banks.end(), b), e->point_banks.end());
}
