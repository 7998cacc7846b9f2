// stub_engine.cpp — the part of include/similari_assoc.h that the tracker facade (sa_tracker.cpp) and the cluster router
// (sa_cluster.cpp) call, with no device behind it.  TEST INFRASTRUCTURE ONLY: it lets the two host files be linked with g++ and run
// under a thread or address sanitizer.
//
//   state        per-scene track tables in host vectors, in the engine's row order (appended in upsert / apply order, removals close gaps)
//   association  the oracle's or_associate on that table (oracle/oracle.cpp is compiled into the programs)
//   upkeep       sa_kalman.h on the host + the id rule of sa_batch_run_apply (a counter over the tracks that start, or one id per candidate)
//   threading    safe exactly where the header says the engine is: different scenes may be staged at once, different slots may be filled,
//                read and collected at once.  Everything else is plain memory, so that a sanitizer sees what the facade's hand-overs carry.
//   monitor      cheap atomic counters check the facade's use of the engine; a violation prints what overlapped with what and exits 3:
//                  * no sa_batch_add* beside a sa_batch_fill
//                  * no two calls on one slot or one scene's staging at once
//                  * the calling-thread-only entry points (and every entry point the header leaves non-re-entrant) overlap with nothing
// Plain SORT only (IoU and Mahalanobis).  Entry points no program reaches answer through unsupported(): the process exits 4, so nothing
// is silently skipped.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/similari_attrs.h"
#include "../../include/similari_framerows.h"
#include "../../include/similari_frames.h"
#include "../../include/similari_waste.h"
#include "../../oracle/oracle.h"
#include "../../similari_amd/csrc/sa_kalman.h"
#include "stub_engine.h"

namespace {

thread_local std::string g_create_err;

struct Counters {
  std::atomic<uint64_t> engines_created{0}, engines_destroyed{0}, sets_begun{0}, scenes_associated{0}, stages{0}, stages_off_thread{0}, commits{0},
      waves{0}, rows_removed{0}, fills_off_thread{0}, results_off_thread{0}, tables_off_thread{0}, slots_off_thread{0};
} g_count;

struct Row {
  uint64_t id = 0, epoch = 0;
  sa_box box{};
  bool full = false;   // a complete filter state (created by the upkeep step): only such a row can be stepped
  sa_kf kf{};
  float mean5[5] = {0}, cov25[25] = {0};
  void project() {
    for (int a = 0; a < 5; ++a) {
      mean5[a] = kf.mean[a];
      for (int b = 0; b < 5; ++b) cov25[a * 5 + b] = kf.cov[a * 10 + b];
    }
  }
};

struct Scene {
  std::vector<Row> rows;
  std::atomic<int> busy{0};   // calls working on this scene's staging
  bool staged = false;
  std::vector<uint32_t> staged_keep;   // rows that stay, in order
};

struct Slot {
  Scene* sc = nullptr;
  uint64_t scene_id = 0, epoch = 0;
  uint32_t n = 0;
  const sa_box* src = nullptr;   // a deferred add: the caller's boxes until the fill
  bool filled = false, ran = false, stepped = false, table_pending = false;
  std::vector<sa_box> boxes, pred;
  std::vector<uint64_t> win, new_id;
  std::vector<uint8_t> vote;
  std::vector<int32_t> col;
  std::vector<sa_kf> kf;   // per candidate: the destination track's state after the step
  std::atomic<int> busy{0};
};

}  // namespace

struct sa_engine {
  sa_config cfg{};
  std::vector<uint64_t> cons_delta;
  std::vector<float> cons_dist;
  std::map<uint64_t, Scene> scenes;   // node-based: a Scene's address is stable; inserted into by the calling-thread entry points only
  std::vector<std::unique_ptr<Slot>> slots;
  std::thread::id set_thread;   // who called sa_batch_begin for the staged set
  std::mutex err_mu;
  std::string err;
  // the usage monitor
  std::atomic<int> active{0}, exclusive{0}, adds{0}, fills{0};
  std::atomic<const char*> last_call{"(nothing)"};
};

namespace {

[[noreturn]] void violation(const char* what, const char* a, const char* b) {
  fprintf(stderr, "STUB ENGINE: contract violation: %s: %s overlapped with %s\n", what, a, b);
  fflush(stderr);
  _Exit(3);
}
[[noreturn]] void unsupported(const char* name) {
  fprintf(stderr, "STUB ENGINE: %s was reached, which the stub does not implement (SA_ERR_UNSUPPORTED)\n", name);
  fflush(stderr);
  _Exit(4);
}

// Every entry point opens one.  serial: the header leaves the call non-re-entrant on one handle (it must overlap with nothing);
// otherwise it is one of the calls the header allows side by side (per slot / per scene), checked by the slot's or scene's own counter.
struct Call {
  sa_engine* e;
  bool serial;
  Call(sa_engine* e_, const char* name, bool serial_) : e(e_), serial(serial_) {
    const char* other = e->last_call.exchange(name, std::memory_order_relaxed);
    const int before = e->active.fetch_add(1, std::memory_order_acq_rel);
    if (e->exclusive.load(std::memory_order_acquire) > 0) violation("a calling-thread-only entry point was running", name, other);
    if (serial) {
      if (before > 0) violation("a calling-thread-only entry point began while another call was running", name, other);
      e->exclusive.fetch_add(1, std::memory_order_acq_rel);
    }
  }
  ~Call() {
    if (serial) e->exclusive.fetch_sub(1, std::memory_order_acq_rel);
    e->active.fetch_sub(1, std::memory_order_acq_rel);
  }
};
struct Busy {   // one call at a time on a slot or on a scene's staging
  std::atomic<int>& w;
  Busy(std::atomic<int>& w_, const char* what, const char* name) : w(w_) {
    if (w.fetch_add(1, std::memory_order_acq_rel) != 0) violation(what, name, "another call on the same one");
  }
  ~Busy() { w.fetch_sub(1, std::memory_order_acq_rel); }
};

int efail(sa_engine* e, int code, const std::string& msg) {
  if (e) { std::lock_guard<std::mutex> lk(e->err_mu); e->err = msg; }
  else g_create_err = msg;
  return code;
}

bool bad_box(const sa_box& b) { return !(b.aspect > 0.0f) || !(b.height > 0.0f) || !(b.confidence >= 0.0f && b.confidence <= 1.0f); }

int check_boxes(sa_engine* e, const char* what, uint64_t scene, uint32_t n, const sa_box* boxes) {
  for (uint32_t i = 0; i < n; ++i)
    if (bad_box(boxes[i])) return efail(e, SA_ERR_BAD_ARG, std::string(what) + ": detection " + std::to_string(i) + " of scene " + std::to_string(scene) + ": bad box");
  return SA_OK;
}

// One scene-frame against the scene's table: the oracle's vote, and the winners as columns of the table.
void associate(sa_engine* e, const Scene* sc, uint64_t epoch, uint32_t n, const sa_box* boxes, uint64_t* win, uint8_t* vote, int32_t* col) {
  const uint32_t T = sc ? (uint32_t)sc->rows.size() : 0;
  std::vector<uint64_t> ids(T), epochs(T);
  std::vector<sa_box> tb(T);
  std::vector<float> m5((size_t)T * 5), c25((size_t)T * 25);
  for (uint32_t j = 0; j < T; ++j) {
    const Row& r = sc->rows[j];
    ids[j] = r.id; epochs[j] = r.epoch; tb[j] = r.box;
    std::memcpy(&m5[(size_t)j * 5], r.mean5, sizeof r.mean5);
    std::memcpy(&c25[(size_t)j * 25], r.cov25, sizeof r.cov25);
  }
  sa_tracks tr;
  std::memset(&tr, 0, sizeof tr);
  tr.n = T; tr.ids = ids.data(); tr.boxes = tb.data(); tr.epochs = epochs.data(); tr.kf_mean = m5.data(); tr.kf_cov = c25.data();
  sa_detections det;
  std::memset(&det, 0, sizeof det);
  det.n = n; det.boxes = boxes;
  std::vector<uint64_t> w(n, 0);
  std::vector<uint8_t> v(n, 0);
  or_frame_out fo;
  std::memset(&fo, 0, sizeof fo);
  fo.track_id = w.data(); fo.voting_type = v.data();
  or_associate(&e->cfg, T, &tr, epoch, &det, &fo);
  for (uint32_t i = 0; i < n; ++i) {
    if (win) win[i] = w[i];
    if (vote) vote[i] = v[i];
    if (col) {
      col[i] = -1;
      if (w[i])
        for (uint32_t j = 0; j < T; ++j)
          if (ids[j] == w[i]) { col[i] = (int32_t)j; break; }
    }
  }
  g_count.scenes_associated.fetch_add(1, std::memory_order_relaxed);
}

Scene* find_scene(sa_engine* e, uint64_t id) {
  auto it = e->scenes.find(id);
  return it == e->scenes.end() ? nullptr : &it->second;
}

int run_slot(sa_engine* e, Slot& s) {
  if (!s.filled) return efail(e, SA_ERR_STATE, "sa_batch_run: slot of scene " + std::to_string(s.scene_id) + " was not filled");
  s.win.assign(s.n, 0); s.vote.assign(s.n, 0); s.col.assign(s.n, -1);
  associate(e, s.sc, s.epoch, s.n, s.boxes.data(), s.win.data(), s.vote.data(), s.col.data());
  s.ran = true;
  s.stepped = false;
  s.table_pending = false;
  return SA_OK;
}

// The Kalman step of every candidate's destination track, into the slot (the table is read, not written).
int step_slot(sa_engine* e, Slot& s, const uint64_t* new_ids) {
  const float pw = e->cfg.kf_position_weight, vw = e->cfg.kf_velocity_weight;
  s.pred.resize(s.n); s.kf.resize(s.n); s.new_id.assign(s.n, 0);
  for (uint32_t i = 0; i < s.n; ++i) {
    if (s.win[i]) {
      const Row& r = s.sc->rows[(size_t)s.col[i]];
      if (!r.full) return efail(e, SA_ERR_STATE, "sa_tracks_apply: track " + std::to_string(r.id) + " has the 5 x 5 projection only and cannot be stepped");
      s.kf[i] = r.kf;
      s.pred[i] = sa_kf_make_prediction(pw, vw, true, s.kf[i], s.boxes[i]);
    } else {
      if (!new_ids[i]) return efail(e, SA_ERR_BAD_ARG, "sa_tracks_apply: candidate " + std::to_string(i) + " starts a track and has no id");
      s.new_id[i] = new_ids[i];
      s.pred[i] = sa_kf_make_prediction(pw, vw, false, s.kf[i], s.boxes[i]);
    }
  }
  s.stepped = true;
  s.table_pending = true;
  return SA_OK;
}

// The host side of the scene's table for a stepped slot: merged rows refreshed, started rows appended in candidate order.
void table_slot(Slot& s) {
  if (!s.table_pending) return;
  s.table_pending = false;
  for (uint32_t i = 0; i < s.n; ++i) {   // (columns refer to the table the slot voted against: started rows go behind it)
    Row nr;
    Row& r = s.win[i] ? s.sc->rows[(size_t)s.col[i]] : nr;
    r.kf = s.kf[i];
    r.full = true;
    r.box = s.pred[i];
    r.epoch = s.epoch;
    r.project();
    if (!s.win[i]) { r.id = s.new_id[i]; s.sc->rows.push_back(r); }
  }
}
void finish_tables(sa_engine* e) {
  for (auto& s : e->slots) table_slot(*s);
}

int remove_rows(sa_engine* e, Scene* sc, uint64_t scene_id, uint32_t n, const uint64_t* ids, std::vector<uint32_t>* keep) {
  if (!sc) return efail(e, SA_ERR_NOT_FOUND, "sa_tracks_remove: unknown scene " + std::to_string(scene_id));
  std::vector<uint8_t> gone(sc->rows.size(), 0);
  for (uint32_t k = 0; k < n; ++k) {
    size_t j = 0;
    while (j < sc->rows.size() && sc->rows[j].id != ids[k]) ++j;
    if (j == sc->rows.size()) return efail(e, SA_ERR_NOT_FOUND, "sa_tracks_remove: track " + std::to_string(ids[k]) + " is not in the table of scene " + std::to_string(scene_id));
    gone[j] = 1;
  }
  keep->clear();
  for (size_t j = 0; j < gone.size(); ++j)
    if (!gone[j]) keep->push_back((uint32_t)j);
  return SA_OK;
}
void gather(Scene* sc, const std::vector<uint32_t>& keep) {
  g_count.rows_removed.fetch_add(sc->rows.size() - keep.size(), std::memory_order_relaxed);
  for (size_t w = 0; w < keep.size(); ++w)
    if (keep[w] != w) sc->rows[w] = sc->rows[keep[w]];
  sc->rows.resize(keep.size());
}
uint32_t commit_staged(sa_engine* e) {
  uint32_t scenes = 0;
  for (auto& kv : e->scenes)
    if (kv.second.staged) { gather(&kv.second, kv.second.staged_keep); kv.second.staged = false; ++scenes; }
  return scenes;
}
void count_commit(uint32_t scenes) {
  if (!scenes) return;
  g_count.commits.fetch_add(1, std::memory_order_relaxed);
  if (scenes > 1) g_count.waves.fetch_add(1, std::memory_order_relaxed);
}

int add_slot(sa_engine* e, const char* name, uint64_t scene_id, uint64_t epoch, const sa_detections* d, uint32_t* out_slot, bool deferred) {
  if (!e || !d || !out_slot || (d->n && !d->boxes)) return efail(e, SA_ERR_BAD_ARG, std::string(name) + ": null argument");
  Call call(e, name, false);
  e->adds.fetch_add(1, std::memory_order_acq_rel);
  if (e->fills.load(std::memory_order_acquire) > 0) violation("an add beside a fill", name, "sa_batch_fill");
  int rc = SA_OK;
  std::unique_ptr<Slot> s(new Slot());
  s->sc = &e->scenes[scene_id];
  s->scene_id = scene_id; s->epoch = epoch; s->n = d->n;
  if (deferred) s->src = d->boxes;
  else {
    rc = check_boxes(e, name, scene_id, d->n, d->boxes);
    s->boxes.assign(d->boxes, d->boxes + d->n);
    s->filled = true;
  }
  if (rc == SA_OK) { *out_slot = (uint32_t)e->slots.size(); e->slots.push_back(std::move(s)); }
  e->adds.fetch_sub(1, std::memory_order_acq_rel);
  return rc;
}

Slot* slot_of(sa_engine* e, uint32_t slot) { return e && slot < e->slots.size() ? e->slots[slot].get() : nullptr; }
bool off_thread(const sa_engine* e) { return std::this_thread::get_id() != e->set_thread; }

}  // namespace

extern "C" {

void stub_read_counters(stub_counters* out) {
  out->engines_created = g_count.engines_created.load(); out->engines_destroyed = g_count.engines_destroyed.load();
  out->sets_begun = g_count.sets_begun.load(); out->scenes_associated = g_count.scenes_associated.load();
  out->stages = g_count.stages.load(); out->stages_off_thread = g_count.stages_off_thread.load();
  out->commits = g_count.commits.load(); out->waves = g_count.waves.load(); out->rows_removed = g_count.rows_removed.load();
  out->fills_off_thread = g_count.fills_off_thread.load(); out->results_off_thread = g_count.results_off_thread.load();
  out->tables_off_thread = g_count.tables_off_thread.load(); out->slots_off_thread = g_count.slots_off_thread.load();
}

void sa_config_default(sa_config* cfg) {
  if (!cfg) return;
  std::memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = sizeof *cfg;
  cfg->device = -1;
  cfg->positional_kind = SA_POS_IOU;
  cfg->positional_threshold = 0.3f;
  cfg->positional_min_confidence = 0.05f;
  cfg->visual_kind = SA_VIS_NONE;
  cfg->max_observations = 1;
  cfg->max_idle_epochs = 5;
  cfg->kf_position_weight = 1.0f / 20.0f;
  cfg->kf_velocity_weight = 1.0f / 160.0f;
}

int sa_engine_create(const sa_config* cfg, sa_engine** out) {
  if (!cfg || !out) return efail(nullptr, SA_ERR_BAD_ARG, "sa_engine_create: null argument");
  *out = nullptr;
  if (cfg->visual_kind != SA_VIS_NONE) return efail(nullptr, SA_ERR_UNSUPPORTED, "sa_engine_create: the stub engine serves plain SORT only");
  sa_engine* e = new sa_engine();
  e->cfg = *cfg;
  e->cons_delta.assign(cfg->constraint_epoch_delta, cfg->constraint_epoch_delta + cfg->n_constraints);
  e->cons_dist.assign(cfg->constraint_max_dist, cfg->constraint_max_dist + cfg->n_constraints);
  e->cfg.constraint_epoch_delta = e->cons_delta.data();
  e->cfg.constraint_max_dist = e->cons_dist.data();
  g_count.engines_created.fetch_add(1, std::memory_order_relaxed);
  *out = e;
  return SA_OK;
}
void sa_engine_destroy(sa_engine* e) {
  if (!e) return;
  { Call call(e, "sa_engine_destroy", true); }
  g_count.engines_destroyed.fetch_add(1, std::memory_order_relaxed);
  delete e;
}
const char* sa_last_error(const sa_engine* e) {
  if (!e) return g_create_err.c_str();
  // (the text is read by the thread that saw the failing status, or behind the facade's own hand-over from it)
  return e->err.c_str();
}
bool sa_in_pinned_host_block(const void*, size_t) { return false; }

// ---- track tables ----
int sa_tracks_upsert(sa_engine* e, uint64_t scene_id, const sa_tracks* t) {
  if (!e || !t || (t->n && (!t->ids || !t->boxes || !t->epochs))) return efail(e, SA_ERR_BAD_ARG, "sa_tracks_upsert: null argument");
  Call call(e, "sa_tracks_upsert", true);
  finish_tables(e);
  for (uint32_t i = 0; i < t->n; ++i)
    if (!t->ids[i] || bad_box(t->boxes[i])) return efail(e, SA_ERR_BAD_ARG, "sa_tracks_upsert: row " + std::to_string(i) + ": id 0 or bad box");
  Scene& sc = e->scenes[scene_id];
  for (uint32_t i = 0; i < t->n; ++i) {
    Row* r = nullptr;
    for (Row& o : sc.rows)
      if (o.id == t->ids[i]) { r = &o; break; }
    if (!r) { sc.rows.emplace_back(); r = &sc.rows.back(); }
    r->id = t->ids[i]; r->epoch = t->epochs[i]; r->box = t->boxes[i];
    r->full = false;
    if (t->kf_mean) std::memcpy(r->mean5, t->kf_mean + (size_t)i * 5, sizeof r->mean5);
    if (t->kf_cov) std::memcpy(r->cov25, t->kf_cov + (size_t)i * 25, sizeof r->cov25);
  }
  return SA_OK;
}

int sa_tracks_remove(sa_engine* e, uint64_t scene_id, uint32_t n, const uint64_t* ids) {
  if (!e || (n && !ids)) return efail(e, SA_ERR_BAD_ARG, "sa_tracks_remove: null argument");
  Call call(e, "sa_tracks_remove", true);
  finish_tables(e);
  Scene* sc = find_scene(e, scene_id);
  std::vector<uint32_t> keep;
  int rc = remove_rows(e, sc, scene_id, n, ids, &keep);
  if (rc != SA_OK) return rc;
  gather(sc, keep);
  return SA_OK;
}

int sa_tracks_remove_many(sa_engine* e, uint32_t n_scenes, const uint64_t* scene_ids, const uint32_t* counts, const uint64_t* const* ids) {
  if (!e || (n_scenes && (!scene_ids || !counts || !ids))) return efail(e, SA_ERR_BAD_ARG, "sa_tracks_remove_many: null argument");
  Call call(e, "sa_tracks_remove_many", true);
  finish_tables(e);
  std::vector<std::vector<uint32_t>> keep(n_scenes);
  for (uint32_t s = 0; s < n_scenes; ++s) {   // (either every table changes or none)
    int rc = remove_rows(e, find_scene(e, scene_ids[s]), scene_ids[s], counts[s], ids[s], &keep[s]);
    if (rc != SA_OK) return rc;
  }
  uint32_t scenes = commit_staged(e);
  for (uint32_t s = 0; s < n_scenes; ++s) { gather(find_scene(e, scene_ids[s]), keep[s]); scenes += counts[s] ? 1u : 0u; }
  count_commit(scenes);
  return SA_OK;
}

int sa_tracks_remove_stage(sa_engine* e, uint64_t scene_id, uint32_t n, const uint64_t* ids) {
  if (!e || (n && !ids)) return efail(e, SA_ERR_BAD_ARG, "sa_tracks_remove_stage: null argument");
  Call call(e, "sa_tracks_remove_stage", false);
  Scene* sc = find_scene(e, scene_id);
  if (!sc) return efail(e, SA_ERR_NOT_FOUND, "sa_tracks_remove_stage: unknown scene " + std::to_string(scene_id));
  Busy busy(sc->busy, "two calls on one scene's staging", "sa_tracks_remove_stage");
  for (auto& s : e->slots)
    if (s->sc == sc && s->table_pending) return efail(e, SA_ERR_STATE, "sa_tracks_remove_stage: an upkeep step of the scene is still to be collected");
  int rc = remove_rows(e, sc, scene_id, n, ids, &sc->staged_keep);
  if (rc != SA_OK) return rc;
  sc->staged = true;
  g_count.stages.fetch_add(1, std::memory_order_relaxed);
  if (off_thread(e)) g_count.stages_off_thread.fetch_add(1, std::memory_order_relaxed);
  return SA_OK;
}
int sa_tracks_remove_commit(sa_engine* e) {
  if (!e) return SA_ERR_BAD_ARG;
  Call call(e, "sa_tracks_remove_commit", true);
  count_commit(commit_staged(e));
  return SA_OK;
}
int sa_tracks_remove_abort(sa_engine* e) {
  if (!e) return SA_ERR_BAD_ARG;
  Call call(e, "sa_tracks_remove_abort", true);
  for (auto& kv : e->scenes) kv.second.staged = false;
  return SA_OK;
}

int sa_tracks_get_state(sa_engine* e, uint64_t scene_id, uint64_t id, float* mean10, float* cov100, float*, uint8_t*, float*) {
  if (!e) return SA_ERR_BAD_ARG;
  Call call(e, "sa_tracks_get_state", true);
  finish_tables(e);
  Scene* sc = find_scene(e, scene_id);
  if (sc)
    for (const Row& r : sc->rows)
      if (r.id == id) {
        if (!r.full) return efail(e, SA_ERR_STATE, "sa_tracks_get_state: the track has the 5 x 5 projection only");
        if (mean10) std::memcpy(mean10, r.kf.mean, sizeof r.kf.mean);
        if (cov100) std::memcpy(cov100, r.kf.cov, sizeof r.kf.cov);
        return SA_OK;
      }
  return efail(e, SA_ERR_NOT_FOUND, "sa_tracks_get_state: unknown track " + std::to_string(id));
}
int sa_tracks_set_state(sa_engine*, uint64_t, uint64_t, const float*, const float*, const float*) { unsupported("sa_tracks_set_state"); }

// ---- a request set ----
int sa_batch_begin(sa_engine* e) {
  if (!e) return SA_ERR_BAD_ARG;
  Call call(e, "sa_batch_begin", true);
  finish_tables(e);
  e->slots.clear();
  e->set_thread = std::this_thread::get_id();
  g_count.sets_begun.fetch_add(1, std::memory_order_relaxed);
  return SA_OK;
}
int sa_batch_add_rows(sa_engine* e, uint64_t scene_id, uint64_t epoch, const sa_detections* d, const float* const*, uint32_t* out_slot) {
  return add_slot(e, "sa_batch_add_rows", scene_id, epoch, d, out_slot, false);
}
int sa_batch_add_deferred(sa_engine* e, uint64_t scene_id, uint64_t epoch, const sa_detections* d, const float* const*, uint32_t* out_slot) {
  return add_slot(e, "sa_batch_add_deferred", scene_id, epoch, d, out_slot, true);
}
int sa_batch_add(sa_engine*, uint64_t, uint64_t, const sa_detections*, uint32_t*) { unsupported("sa_batch_add"); }
int sa_batch_add_dev(sa_engine*, uint64_t, uint64_t, const sa_detections*, const sa_dev_rows*, uint32_t*) { unsupported("sa_batch_add_dev"); }
int sa_batch_add_deferred_dev(sa_engine*, uint64_t, uint64_t, const sa_detections*, const sa_dev_rows*, uint32_t*) { unsupported("sa_batch_add_deferred_dev"); }

int sa_batch_fill(sa_engine* e, uint32_t slot) {
  Slot* s = slot_of(e, slot);
  if (!s) return efail(e, SA_ERR_BAD_ARG, "sa_batch_fill: no such slot");
  Call call(e, "sa_batch_fill", false);
  e->fills.fetch_add(1, std::memory_order_acq_rel);
  if (e->adds.load(std::memory_order_acquire) > 0) violation("a fill beside an add", "sa_batch_fill", "sa_batch_add*");
  int rc = SA_OK;
  {
    Busy busy(s->busy, "two calls on one slot", "sa_batch_fill");
    if (off_thread(e)) g_count.fills_off_thread.fetch_add(1, std::memory_order_relaxed);
    if (!s->filled) {
      rc = check_boxes(e, "sa_batch_fill", s->scene_id, s->n, s->src);
      if (rc == SA_OK) { s->boxes.assign(s->src, s->src + s->n); s->filled = true; s->src = nullptr; }
    }
  }
  e->fills.fetch_sub(1, std::memory_order_acq_rel);
  return rc;
}

int sa_batch_run(sa_engine* e) {
  if (!e) return SA_ERR_BAD_ARG;
  Call call(e, "sa_batch_run", true);
  finish_tables(e);
  for (auto& s : e->slots) { int rc = run_slot(e, *s); if (rc != SA_OK) return rc; }
  return SA_OK;
}
int sa_batch_run_apply(sa_engine* e, const uint64_t* id_base, int id_per_candidate) {
  if (!e || (!e->slots.empty() && !id_base)) return efail(e, SA_ERR_BAD_ARG, "sa_batch_run_apply: null argument");
  Call call(e, "sa_batch_run_apply", true);
  finish_tables(e);
  for (size_t k = 0; k < e->slots.size(); ++k) {
    Slot& s = *e->slots[k];
    int rc = run_slot(e, s);
    if (rc != SA_OK) return rc;
    std::vector<uint64_t> ids(s.n, 0);
    uint64_t rank = 0;
    for (uint32_t i = 0; i < s.n; ++i)
      if (!s.win[i]) ids[i] = id_base[k] + 1 + (id_per_candidate ? (uint64_t)i : rank++);
    rc = step_slot(e, s, ids.data());
    if (rc != SA_OK) return rc;
  }
  return SA_OK;
}
int sa_batch_sync(sa_engine* e) {
  if (!e) return SA_ERR_BAD_ARG;
  Call call(e, "sa_batch_sync", true);
  return SA_OK;
}
int sa_batch_fetch(sa_engine* e, uint32_t slot, uint64_t* out_track_id, uint8_t* out_voting_type) {
  Slot* s = slot_of(e, slot);
  if (!s || !s->ran) return efail(e, SA_ERR_STATE, "sa_batch_fetch: no results for that slot");
  Call call(e, "sa_batch_fetch", true);
  if (out_track_id) std::memcpy(out_track_id, s->win.data(), (size_t)s->n * sizeof(uint64_t));
  if (out_voting_type) std::memcpy(out_voting_type, s->vote.data(), s->n);
  return SA_OK;
}
int sa_batch_fetch_cols(sa_engine* e, uint32_t slot, int32_t* out_cols) {
  Slot* s = slot_of(e, slot);
  if (!s || !s->ran || !out_cols) return efail(e, SA_ERR_STATE, "sa_batch_fetch_cols: no results for that slot");
  Call call(e, "sa_batch_fetch_cols", true);
  std::memcpy(out_cols, s->col.data(), (size_t)s->n * sizeof(int32_t));
  return SA_OK;
}
int sa_batch_results(sa_engine* e, uint32_t slot, const uint64_t** out_track_id, const uint8_t** out_voting_type, const int32_t** out_cols) {
  Slot* s = slot_of(e, slot);
  if (!s || !s->ran) return efail(e, SA_ERR_STATE, "sa_batch_results: no results for that slot");
  Call call(e, "sa_batch_results", false);
  Busy busy(s->busy, "two calls on one slot", "sa_batch_results");
  if (off_thread(e)) g_count.results_off_thread.fetch_add(1, std::memory_order_relaxed);
  if (out_track_id) *out_track_id = s->win.data();
  if (out_voting_type) *out_voting_type = s->vote.data();
  if (out_cols) *out_cols = s->col.data();
  return SA_OK;
}

// ---- upkeep ----
int sa_tracks_apply_begin(sa_engine* e, uint32_t slot, const uint64_t* new_ids) {
  Slot* s = slot_of(e, slot);
  if (!s || !s->ran || !new_ids) return efail(e, SA_ERR_STATE, "sa_tracks_apply_begin: no results for that slot");
  Call call(e, "sa_tracks_apply_begin", true);
  int rc = step_slot(e, *s, new_ids);
  if (rc == SA_OK) table_slot(*s);
  return rc;
}
int sa_tracks_apply_end(sa_engine* e, uint32_t slot, sa_box* out_predicted) {
  Slot* s = slot_of(e, slot);
  if (!s || !s->stepped) return efail(e, SA_ERR_STATE, "sa_tracks_apply_end: no step for that slot");
  Call call(e, "sa_tracks_apply_end", true);
  if (out_predicted) std::memcpy(out_predicted, s->pred.data(), (size_t)s->n * sizeof(sa_box));
  return SA_OK;
}
int sa_tracks_apply_collect_table(sa_engine* e, uint32_t slot, uint64_t* out_new_ids) {
  Slot* s = slot_of(e, slot);
  if (!s || !s->stepped) return efail(e, SA_ERR_STATE, "sa_tracks_apply_collect_table: no step for that slot");
  Call call(e, "sa_tracks_apply_collect_table", false);
  Busy busy(s->busy, "two calls on one slot", "sa_tracks_apply_collect_table");
  Busy scene(s->sc->busy, "two calls on one scene's table", "sa_tracks_apply_collect_table");
  if (off_thread(e)) g_count.tables_off_thread.fetch_add(1, std::memory_order_relaxed);
  table_slot(*s);
  if (out_new_ids) std::memcpy(out_new_ids, s->new_id.data(), (size_t)s->n * sizeof(uint64_t));
  return SA_OK;
}
int sa_tracks_apply_collect_begin(sa_engine* e) {
  if (!e) return SA_ERR_BAD_ARG;
  Call call(e, "sa_tracks_apply_collect_begin", true);
  return SA_OK;
}
int sa_tracks_apply_collect_slot(sa_engine* e, uint32_t slot, uint64_t* out_new_ids, sa_box* out_predicted) {
  Slot* s = slot_of(e, slot);
  if (!s || !s->stepped) return efail(e, SA_ERR_STATE, "sa_tracks_apply_collect_slot: no step for that slot");
  Call call(e, "sa_tracks_apply_collect_slot", false);
  Busy busy(s->busy, "two calls on one slot", "sa_tracks_apply_collect_slot");
  Busy scene(s->sc->busy, "two calls on one scene's table", "sa_tracks_apply_collect_slot");
  if (off_thread(e)) g_count.slots_off_thread.fetch_add(1, std::memory_order_relaxed);
  table_slot(*s);   // (when nobody has: sa_tracks_apply_collect_table is optional)
  if (out_new_ids) std::memcpy(out_new_ids, s->new_id.data(), (size_t)s->n * sizeof(uint64_t));
  if (out_predicted) std::memcpy(out_predicted, s->pred.data(), (size_t)s->n * sizeof(sa_box));
  return SA_OK;
}
int sa_tracks_apply_collect_end(sa_engine* e) {
  if (!e) return SA_ERR_BAD_ARG;
  Call call(e, "sa_tracks_apply_collect_end", true);
  finish_tables(e);
  return SA_OK;
}

// ---- the router's call: stage, associate and copy back, scene by scene ----
int sa_associate_batch(sa_engine* e, uint32_t n_scenes, const sa_scene_request* req, const sa_scene_result* res) {
  if (!e || (n_scenes && (!req || !res))) return efail(e, SA_ERR_BAD_ARG, "sa_associate_batch: null argument");
  Call call(e, "sa_associate_batch", true);
  finish_tables(e);
  for (uint32_t s = 0; s < n_scenes; ++s) {
    int rc = check_boxes(e, "sa_associate_batch", req[s].scene_id, req[s].detections.n, req[s].detections.boxes);
    if (rc != SA_OK) return rc;
  }
  for (uint32_t s = 0; s < n_scenes; ++s)
    associate(e, find_scene(e, req[s].scene_id), req[s].epoch, req[s].detections.n, req[s].detections.boxes, res[s].out_track_id, res[s].out_voting_type, nullptr);
  return SA_OK;
}

// ---- out of scope (own areas, stores) ----
int sa_own_areas_batch(sa_engine*, uint32_t, const uint32_t*, const sa_box* const*, float* const*) { unsupported("sa_own_areas_batch"); }
uint32_t sa_store_depth(const sa_store*) { unsupported("sa_store_depth"); }
int sa_store_set_attrs(sa_store*, uint32_t, const uint64_t*, const sa_track_attrs*) { unsupported("sa_store_set_attrs"); }
int sa_tracks_waste(sa_engine*, sa_store*, uint32_t, uint32_t, const uint64_t*, const uint32_t*, const uint64_t* const*, const uint32_t*, uint32_t*) {
  unsupported("sa_tracks_waste");
}

}  // extern "C"
