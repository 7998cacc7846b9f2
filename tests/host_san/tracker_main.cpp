// tracker_main.cpp — the tracker facade (similari_amd/csrc/sa_tracker.cpp) over stub engines, for a thread or address sanitizer build.
// Every configuration runs the facade and the oracle's tracker (oracle/oracle_tracker.cpp) on the same seeded frames and compares after
// every request set: ids, epochs, lengths and custom ids exactly, boxes to 1e-5 (the reference's PartialEq, bbox.rs:537-545), the
// epochs, the active / idle / wasted sets.  The facade's source is part of this translation unit, so that the program can read the
// facade's own state for its coverage counters (which scratch set a request used, whether deferred bookkeeping was pending, whether a
// result handle had finished) — only ever at points where the facade's contract makes that state the calling thread's.
#include "../../similari_amd/csrc/sa_tracker.cpp"

#include "stub_engine.h"

extern "C" {
struct or_tracker;
or_tracker* or_tracker_create(const sa_tracker_options* o);
void or_tracker_destroy(or_tracker* t);
int or_tracker_predict_batch(or_tracker* t, uint32_t n_scenes, const uint64_t* scene_ids, const uint32_t* counts, const sa_observation* const* obs, sa_sort_track* const* out);
int or_tracker_skip_epochs(or_tracker* t, uint64_t scene, uint64_t n);
uint64_t or_tracker_current_epoch(or_tracker* t, uint64_t scene);
uint64_t or_tracker_active_tracks(or_tracker* t);
uint32_t or_tracker_wasted(or_tracker* t, sa_sort_track* out, uint32_t cap);
uint32_t or_tracker_idle_tracks(or_tracker* t, uint64_t scene, sa_sort_track* out, uint32_t cap);
}

#define CHECK(cond, ...) do { if (!(cond)) { printf("BAD [%s] set %d: ", g_where.c_str(), g_set); printf(__VA_ARGS__); printf("\n"); fflush(stdout); return 1; } } while (0)

namespace {

std::string g_where;
int g_set = 0;   // the request set of the configuration being run

struct Coverage {
  uint64_t sets = 0, tracks_compared = 0, state_checks = 0, refusals = 0;
  uint64_t begins_driver_asleep = 0, begins_driver_spinning = 0;   // by the gap the program left: behind a pause / a tracker that never spins, or right behind the last set
  std::atomic<uint64_t> taken_before_finish{0}, taken_after_finish{0};   // (a second thread takes scenes too)
  uint64_t scratch_set[2] = {0, 0};
  uint64_t flush_behind_launches = 0;   // a fused request began while the previous set's deferred bookkeeping was pending
  uint64_t handles_freed_early = 0, second_thread_handles = 0, next_begun_before_last_taken = 0;
  uint64_t evicted_tracks_seen = 0;
} g_cov;

struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 7) {}
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
  float uni(float a, float b) { return a + (b - a) * (float)(next() & 0xffffff) / (float)0x1000000; }
  bool chance(float p) { return uni(0.f, 1.f) < p; }
};

// One scene's objects: they drift, are born, are missed for a frame, and leave.
struct Obj { float x, y, vx, vy, aspect, h, angle; int64_t serial; };
struct SceneSim {
  uint64_t id = 0;
  std::vector<Obj> objs;
  int64_t serial = 0;
  uint32_t lo = 12, hi = 36;
  Obj born(Rng& r) {
    Obj o;
    o.x = r.uni(0.f, 3000.f); o.y = r.uni(0.f, 3000.f); o.vx = r.uni(-2.f, 2.f); o.vy = r.uni(-2.f, 2.f);
    o.aspect = r.uni(0.4f, 1.1f); o.h = r.uni(40.f, 80.f);
    o.angle = r.chance(0.3f) ? r.uni(0.05f, 0.6f) : 0.0f;
    o.serial = ++serial;
    return o;
  }
  void start(Rng& r, uint64_t scene, uint32_t lo_, uint32_t hi_) {
    id = scene; lo = lo_; hi = hi_;
    const uint32_t n = lo + r.next() % (hi - lo + 1);
    for (uint32_t i = 0; i < n; ++i) objs.push_back(born(r));
  }
  // the frame's detections, 8 to 40 of them
  void frame(Rng& r, float churn, std::vector<sa_observation>* out) {
    for (Obj& o : objs) { o.x += o.vx; o.y += o.vy; }
    for (Obj& o : objs)
      if (r.chance(churn)) o = born(r);   // a departure and a birth
    if (objs.size() < hi && r.chance(0.2f)) objs.push_back(born(r));
    if (objs.size() > lo && r.chance(0.2f)) objs.erase(objs.begin() + (long)(r.next() % objs.size()));
    out->clear();
    size_t may_miss = objs.size() > 8 ? objs.size() - 8 : 0;
    const size_t first = r.next() % objs.size();
    for (size_t k = 0; k < objs.size(); ++k) {
      const Obj& o = objs[(first + k) % objs.size()];
      if (may_miss && r.chance(0.08f)) { --may_miss; continue; }
      if (out->size() == 40) break;
      sa_observation ob;
      std::memset(&ob, 0, sizeof ob);
      ob.bbox.xc = o.x + r.uni(-1.f, 1.f); ob.bbox.yc = o.y + r.uni(-1.f, 1.f);
      ob.bbox.aspect = o.aspect; ob.bbox.height = o.h * r.uni(0.97f, 1.03f);
      ob.bbox.confidence = r.uni(0.5f, 1.0f);
      ob.bbox.has_angle = o.angle != 0.0f; ob.bbox.angle = o.angle;
      ob.feature_quality = NAN; ob.own_area = NAN;
      ob.has_custom_object_id = o.serial % 3 == 0;
      ob.custom_object_id = ob.has_custom_object_id ? o.serial : 0;
      out->push_back(ob);
    }
  }
};

bool box_eq(const sa_box& a, const sa_box& b) {
  const float eps = 1e-5f;
  const float aa = a.has_angle ? a.angle : 0.0f, ba = b.has_angle ? b.angle : 0.0f;
  return std::fabs(a.xc - b.xc) < eps && std::fabs(a.yc - b.yc) < eps && std::fabs(aa - ba) < eps && std::fabs(a.aspect - b.aspect) < eps && std::fabs(a.height - b.height) < eps;
}
bool track_eq(const sa_sort_track& a, const sa_sort_track& b) {
  return a.id == b.id && a.epoch == b.epoch && a.length == b.length && a.scene_id == b.scene_id && a.voting_type == b.voting_type &&
         a.has_custom_object_id == b.has_custom_object_id && a.custom_object_id == b.custom_object_id && box_eq(a.observed_bbox, b.observed_bbox) &&
         box_eq(a.predicted_bbox, b.predicted_bbox) && a.predicted_bbox.confidence == b.predicted_bbox.confidence;
}
int tracks_eq(const char* what, uint64_t scene, const sa_sort_track* a, const sa_sort_track* b, size_t n) {
  for (size_t i = 0; i < n; ++i)
    CHECK(track_eq(a[i], b[i]), "%s: scene %llu, track %zu of %zu: facade id %llu epoch %llu length %llu box (%g %g %g %g), oracle id %llu epoch %llu length %llu box (%g %g %g %g)", what,
          (unsigned long long)scene, i, n, (unsigned long long)a[i].id, (unsigned long long)a[i].epoch, (unsigned long long)a[i].length, a[i].predicted_bbox.xc, a[i].predicted_bbox.yc,
          a[i].predicted_bbox.aspect, a[i].predicted_bbox.height, (unsigned long long)b[i].id, (unsigned long long)b[i].epoch, (unsigned long long)b[i].length, b[i].predicted_bbox.xc,
          b[i].predicted_bbox.yc, b[i].predicted_bbox.aspect, b[i].predicted_bbox.height);
  g_cov.tracks_compared += n;
  return 0;
}

enum Mode { SINGLE, SYNC, HANDLE };
enum Manner { TAKE_ALL, POLL_READY, OVERLAP_NEXT, SECOND_THREAD };
struct Config {
  Mode mode = SINGLE;
  Manner manner = TAKE_ALL;
  uint32_t scenes = 1;
  int workers = 1, batch_ids = 0, device_upkeep = 1, kind = SA_POS_IOU, spin_us = -1;
  uint32_t n_devices = 0;
  int frames = 40;
  float churn = 0.02f;
  uint32_t lo = 12, hi = 36, waste_every = 10;
  uint64_t max_idle = 2;
  bool skips = true, drains = true;
  uint64_t seed = 1;
};

// the facade's trackers that do the work: itself, or the shards of a device group
std::vector<sa_tracker*> workers_of(sa_tracker* t) { return t->shards.empty() ? std::vector<sa_tracker*>{t} : t->shards; }

bool handle_finished(sa_batch_result* h) {
  if (!h->st) return false;
  std::lock_guard<std::mutex> lk(h->st->mu);
  return h->st->finished;
}

struct Run {
  Config c;
  sa_tracker* t = nullptr;
  or_tracker* o = nullptr;
  std::vector<SceneSim> sims;
  std::vector<uint64_t> scene_ids;
  std::vector<std::vector<sa_observation>> obs;
  std::vector<uint32_t> counts;
  std::vector<const sa_observation*> obs_p;
  std::vector<std::vector<sa_sort_track>> want, got;
  std::vector<sa_sort_track*> want_p, got_p;
  Rng rng{1};

  void point() {
    const uint32_t S = c.scenes;
    counts.resize(S); obs_p.resize(S); want.resize(S); got.resize(S); want_p.resize(S); got_p.resize(S);
    for (uint32_t s = 0; s < S; ++s) {
      counts[s] = (uint32_t)obs[s].size();
      obs_p[s] = obs[s].data();
      want[s].assign(counts[s], sa_sort_track{});
      got[s].assign(counts[s], sa_sort_track{});
      want_p[s] = want[s].data();
      got_p[s] = got[s].data();
    }
  }
  int compare_outputs(const char* what) {
    for (uint32_t s = 0; s < c.scenes; ++s)
      if (tracks_eq(what, scene_ids[s], got[s].data(), want[s].data(), counts[s])) return 1;
    return 0;
  }
  // what the next request will find: read while nothing is in flight
  void note_before_request(bool fused) {
    for (sa_tracker* w : workers_of(t)) {
      wait_outstanding(w);
      if (fused && w->pending) ++g_cov.flush_behind_launches;
    }
  }
  void note_after_request() {
    for (sa_tracker* w : workers_of(t)) {
      wait_outstanding(w);
      ++g_cov.scratch_set[w->cur_set & 1];
      for (auto& kv : w->scenes) g_cov.evicted_tracks_seen += kv.second.evicted.size();
    }
  }
  // one scene out of a handle into got[]; by_get: through the copying call, with a short array first
  int take_one(sa_batch_result* h, bool by_get, std::vector<std::vector<sa_sort_track>>* into, const std::vector<uint64_t>& ids) {
    const bool fin_before = handle_finished(h);
    uint64_t scene = 0;
    uint32_t n = 0;
    std::vector<sa_sort_track> buf;
    const sa_sort_track* p = nullptr;
    if (by_get) {
      int rc = sa_batch_result_get(h, &scene, nullptr, 0, &n);
      CHECK(rc == (n ? SA_ERR_BAD_ARG : SA_OK), "sa_batch_result_get with no room: %d", rc);
      if (n) {
        buf.resize(n);
        CHECK(sa_batch_result_get(h, &scene, buf.data(), n, &n) == SA_OK, "sa_batch_result_get");
      }
      p = buf.data();
    } else CHECK(sa_batch_result_take(h, &scene, &p, &n) == SA_OK, "sa_batch_result_take: %s", sa_tracker_last_error(nullptr));
    const bool fin_after = handle_finished(h);
    if (h->st) {
      if (!fin_after) ++g_cov.taken_before_finish;
      if (fin_before) ++g_cov.taken_after_finish;
    }
    size_t s = 0;
    while (s < ids.size() && ids[s] != scene) ++s;
    CHECK(s < ids.size(), "the handle delivered scene %llu, which was not in the request", (unsigned long long)scene);
    CHECK(n == (*into)[s].size(), "scene %llu: %u tracks for %zu observations", (unsigned long long)scene, n, (*into)[s].size());
    std::copy(p, p + n, (*into)[s].begin());
    return 0;
  }
};

int make_run(Run& R, const Config& c) {
  R.c = c;
  R.rng = Rng(c.seed);
  sa_tracker_options o;
  sa_tracker_options_default(&o, 0);
  o.history_length = 3;
  o.max_idle_epochs = c.max_idle;
  o.auto_waste_periodicity = c.waste_every;
  o.positional_kind = c.kind;
  o.batch_ids = c.batch_ids;
  o.device_upkeep = c.device_upkeep;
  o.workers = c.workers;
  o.spin_us = c.spin_us;
  const int32_t devices[4] = {0, 0, 0, 0};
  o.n_devices = c.n_devices;
  o.devices = c.n_devices ? devices : nullptr;
  CHECK(sa_tracker_create(&o, &R.t) == SA_OK, "sa_tracker_create: %s", sa_tracker_last_error(nullptr));
  sa_tracker_options oo = o;   // the oracle is ONE tracker whatever the facade is made of
  oo.n_devices = 0; oo.devices = nullptr;
  R.o = or_tracker_create(&oo);
  R.sims.resize(c.scenes);
  R.obs.resize(c.scenes);
  for (uint32_t s = 0; s < c.scenes; ++s) {
    R.scene_ids.push_back(3 + 2 * (uint64_t)s + (s % 3 == 2 ? 1 : 0));   // (neither dense nor all of one parity: the shards of a group get uneven shares)
    R.sims[s].start(R.rng, R.scene_ids[s], c.lo, c.hi);
  }
  return 0;
}
void end_run(Run& R) {
  if (R.t) sa_tracker_destroy(R.t);
  if (R.o) or_tracker_destroy(R.o);
  R.t = nullptr; R.o = nullptr;
}

// epochs and active tracks; idle: the idle sets as well; drain: also the wasted tracks, taken out of both.
int compare_state(Run& R, bool idle, bool drain) {
  uint64_t fa = 0;
  CHECK(sa_tracker_active_tracks(R.t, &fa) == SA_OK, "active_tracks");
  CHECK(fa == or_tracker_active_tracks(R.o), "active tracks: facade %llu, oracle %llu", (unsigned long long)fa, (unsigned long long)or_tracker_active_tracks(R.o));
  for (uint64_t scene : R.scene_ids) {
    uint64_t fe = 0;
    CHECK(sa_tracker_current_epoch(R.t, scene, &fe) == SA_OK, "current_epoch");
    CHECK(fe == or_tracker_current_epoch(R.o, scene), "epoch of scene %llu: facade %llu, oracle %llu", (unsigned long long)scene, (unsigned long long)fe,
          (unsigned long long)or_tracker_current_epoch(R.o, scene));
  }
  ++g_cov.state_checks;
  if (!idle) return 0;
  auto by_id = [](const sa_sort_track& a, const sa_sort_track& b) { return a.id < b.id; };
  for (uint64_t scene : R.scene_ids) {
    uint32_t fn = 0;
    CHECK(sa_tracker_idle_tracks(R.t, scene, nullptr, 0, &fn) == SA_OK, "idle_tracks");
    std::vector<sa_sort_track> f(fn + 1), w(fn + 1);
    CHECK(sa_tracker_idle_tracks(R.t, scene, f.data(), fn, &fn) == SA_OK, "idle_tracks");
    const uint32_t on = or_tracker_idle_tracks(R.o, scene, w.data(), fn);
    CHECK(fn == on, "idle tracks of scene %llu: facade %u, oracle %u", (unsigned long long)scene, fn, on);
    std::sort(f.begin(), f.begin() + fn, by_id);
    std::sort(w.begin(), w.begin() + fn, by_id);
    if (tracks_eq("idle", scene, f.data(), w.data(), fn)) return 1;
  }
  if (!drain) return 0;   // (wasted() wastes at once what has expired: the long runs leave that to the tracker's own cadence, so that rows pile up for the eviction path)
  uint32_t fn = 0;
  CHECK(sa_tracker_wasted(R.t, nullptr, 0, &fn) == SA_OK, "wasted");
  const uint32_t on = or_tracker_wasted(R.o, nullptr, 0);
  CHECK(fn == on, "wasted tracks: facade %u, oracle %u", fn, on);
  if (fn % 2) {   // handed out ...
    std::vector<sa_sort_track> f(fn), w(fn);
    CHECK(sa_tracker_wasted(R.t, f.data(), fn, &fn) == SA_OK, "wasted");
    or_tracker_wasted(R.o, w.data(), fn);
    std::sort(w.begin(), w.end(), by_id);
    if (tracks_eq("wasted", 0, f.data(), w.data(), fn)) return 1;
  } else {        // ... or thrown away
    std::vector<sa_sort_track> w(fn + 1);
    CHECK(sa_tracker_clear_wasted(R.t) == SA_OK, "clear_wasted");
    or_tracker_wasted(R.o, w.data(), fn + 1);
  }
  CHECK(sa_tracker_wasted(R.t, nullptr, 0, &fn) == SA_OK && fn == 0 && or_tracker_wasted(R.o, nullptr, 0) == 0, "wasted tracks behind a drain: facade %u", fn);
  return 0;
}

// Requests the facade refuses — a bad box in one scene, a null per-scene pointer, a scene id twice — through every entry point, on a
// single tracker and on a device group alike: the code, the text, and nothing has moved (the epochs here; the id counter and the waste
// cadence by the sets that follow, which are held against the oracle like every other).
int refuse(Run& R) {
  const uint32_t k = R.rng.next() % R.c.scenes;
  std::vector<sa_observation> spoilt = R.obs[k];
  if (spoilt.empty()) return 0;
  spoilt[R.rng.next() % spoilt.size()].bbox.aspect = R.rng.chance(0.5f) ? 0.0f : NAN;
  std::vector<const sa_observation*> p = R.obs_p;
  p[k] = spoilt.data();
  std::vector<uint64_t> before;
  for (uint64_t scene : R.scene_ids) before.push_back(or_tracker_current_epoch(R.o, scene));
  int rc = sa_tracker_predict(R.t, R.scene_ids[k], R.counts[k], spoilt.data(), R.got[k].data());
  CHECK(rc == SA_ERR_BAD_ARG && std::strstr(sa_tracker_last_error(R.t), "bad box"), "predict with a bad box: %d '%s'", rc, sa_tracker_last_error(R.t));
  rc = sa_tracker_predict_batch(R.t, R.c.scenes, R.scene_ids.data(), R.counts.data(), p.data(), R.got_p.data());
  CHECK(rc == SA_ERR_BAD_ARG && std::strstr(sa_tracker_last_error(R.t), "bad box"), "predict_batch with a bad box: %d '%s'", rc, sa_tracker_last_error(R.t));
  sa_batch_result* h = nullptr;
  rc = sa_tracker_predict_batch_begin(R.t, R.c.scenes, R.scene_ids.data(), R.counts.data(), p.data(), &h);
  CHECK(rc == SA_ERR_BAD_ARG && !h && std::strstr(sa_tracker_last_error(R.t), "bad box"), "predict_batch_begin with a bad box: %d '%s'", rc, sa_tracker_last_error(R.t));
  // What the request check refuses before it looks at a box: a null per-scene pointer, a scene id twice.  The texts are the ones the
  // facade had before that check became one function — a device group words a null pointer differently from a single tracker, and looks
  // at every output pointer before the first observations pointer — and a request with two faults reports the one it reported then.
  {
    const bool group = !R.t->shards.empty();
    const uint32_t S = R.c.scenes, k2 = (k + 1) % S;
    const unsigned long long idk = (unsigned long long)R.scene_ids[k];
    std::vector<const sa_observation*> no_obs = R.obs_p, no_obs_bad_box = p;
    std::vector<sa_sort_track*> no_out = R.got_p;
    std::vector<uint64_t> twice = R.scene_ids;
    no_obs[k] = nullptr;
    no_out[k] = nullptr;
    twice[k2] = twice[k];
    no_obs_bad_box[k2] = nullptr;   // (with S == 1: the spoilt scene itself)
    char null_obs[96], null_out[96], dup[96], null_first[96];
    snprintf(null_obs, sizeof null_obs, group ? "scene %llu: null observations" : "scene %llu: null observations / output", idk);
    snprintf(null_out, sizeof null_out, group ? "scene %llu: null output" : "scene %llu: null observations / output", idk);
    snprintf(dup, sizeof dup, "scene %llu appears twice in one batch", idk);
    snprintf(null_first, sizeof null_first, group ? "scene %llu: null observations" : "scene %llu: null observations / output", (unsigned long long)R.scene_ids[k2]);
    struct Case { const char* what; const uint64_t* ids; const sa_observation* const* obs; sa_sort_track* const* out; const char* text; };
    const Case cases[] = {
      {"a null observations pointer", R.scene_ids.data(), no_obs.data(), R.got_p.data(), null_obs},
      {"a null output pointer", R.scene_ids.data(), R.obs_p.data(), no_out.data(), null_out},
      {"a scene id twice", twice.data(), R.obs_p.data(), R.got_p.data(), dup},
      {"a scene id twice and a bad box", twice.data(), p.data(), R.got_p.data(), dup},                       // (the ids come first)
      {"null observations and a bad box", R.scene_ids.data(), no_obs_bad_box.data(), R.got_p.data(), null_first},   // (the pointers come first)
      {"null observations and a null output", R.scene_ids.data(), no_obs.data(), no_out.data(), null_out},   // (a group: every output first)
    };
    for (const Case& q : cases) {
      const bool dups = q.ids == twice.data();
      if (dups && S < 2) continue;
      rc = sa_tracker_predict_batch(R.t, S, q.ids, R.counts.data(), q.obs, q.out);
      CHECK(rc == SA_ERR_BAD_ARG && !std::strcmp(sa_tracker_last_error(R.t), q.text), "predict_batch with %s: %d '%s', expected '%s'", q.what, rc, sa_tracker_last_error(R.t), q.text);
      if (q.out != R.got_p.data() && q.obs == R.obs_p.data()) continue;   // (a handle has no output pointers)
      const char* text = q.out != R.got_p.data() ? null_obs : q.text;
      h = nullptr;
      rc = sa_tracker_predict_batch_begin(R.t, S, q.ids, R.counts.data(), q.obs, &h);
      CHECK(rc == SA_ERR_BAD_ARG && !h && !std::strcmp(sa_tracker_last_error(R.t), text), "predict_batch_begin with %s: %d '%s', expected '%s'", q.what, rc, sa_tracker_last_error(R.t), text);
    }
  }
  for (size_t s = 0; s < R.scene_ids.size(); ++s) {
    uint64_t e = 0;
    sa_tracker_current_epoch(R.t, R.scene_ids[s], &e);
    CHECK(e == before[s], "a refused set moved the epoch of scene %llu from %llu to %llu", (unsigned long long)R.scene_ids[s], (unsigned long long)before[s], (unsigned long long)e);
  }
  ++g_cov.refusals;
  return 0;
}

int run_config(const Config& c) {
  Run R;
  if (make_run(R, c)) return 1;
  const bool fused = fused_path(R.t->o, c.scenes);   // (by the whole request; the shards of a group decide again, each for its share)
  sa_batch_result* held = nullptr;                       // OVERLAP_NEXT: the previous set's handle, its last scene not taken yet
  std::vector<std::vector<sa_sort_track>> held_want, held_got;
  std::thread consumer;                                  // SECOND_THREAD: takes the previous set's scenes
  std::atomic<int> consumer_bad{0};
  std::vector<std::vector<sa_sort_track>> consumer_want, consumer_got;
  auto join_consumer = [&]() -> int {
    if (!consumer.joinable()) return 0;
    consumer.join();
    CHECK(consumer_bad.load() == 0, "the second thread's handle");
    for (uint32_t s = 0; s < c.scenes; ++s)
      if (tracks_eq("second thread", R.scene_ids[s], consumer_got[s].data(), consumer_want[s].data(), consumer_want[s].size())) return 1;
    return 0;
  };
  for (int f = 0; f < c.frames; ++f) {
    g_set = f;
    for (uint32_t s = 0; s < c.scenes; ++s) R.sims[s].frame(R.rng, c.churn, &R.obs[s]);   // (while a second thread may still be taking the last set)
    R.point();
    if (f == c.frames / 2 || f == c.frames / 2 + 1) {
      if (join_consumer()) return 1;
      if (refuse(R)) return 1;
    }
    or_tracker_predict_batch(R.o, c.scenes, R.scene_ids.data(), R.counts.data(), R.obs_p.data(), R.want_p.data());
    R.note_before_request(fused);
    const bool pause = f % 5 == 4;
    if (pause) std::this_thread::sleep_for(std::chrono::milliseconds(3));
    if (c.mode == SINGLE) {
      CHECK(sa_tracker_predict(R.t, R.scene_ids[0], R.counts[0], R.obs_p[0], R.got_p[0]) == SA_OK, "predict: %s", sa_tracker_last_error(R.t));
      if (R.compare_outputs("predict")) return 1;
    } else if (c.mode == SYNC) {
      CHECK(sa_tracker_predict_batch(R.t, c.scenes, R.scene_ids.data(), R.counts.data(), R.obs_p.data(), R.got_p.data()) == SA_OK, "predict_batch: %s", sa_tracker_last_error(R.t));
      if (R.compare_outputs("predict_batch")) return 1;
    } else {
      sa_batch_result* h = nullptr;
      CHECK(sa_tracker_predict_batch_begin(R.t, c.scenes, R.scene_ids.data(), R.counts.data(), R.obs_p.data(), &h) == SA_OK && h, "predict_batch_begin: %s", sa_tracker_last_error(R.t));
      if (fused && !c.n_devices) { if (pause || c.spin_us == 0) ++g_cov.begins_driver_asleep; else if (f) ++g_cov.begins_driver_spinning; }
      CHECK(sa_batch_result_size(h) == c.scenes, "sa_batch_result_size");
      if (c.manner == OVERLAP_NEXT) {
        if (held) {   // the last scene of the previous set, behind this set's begin
          if (R.take_one(held, false, &held_got, R.scene_ids)) return 1;
          uint64_t sc = 0; const sa_sort_track* p = nullptr; uint32_t n = 0;
          CHECK(sa_batch_result_take(held, &sc, &p, &n) == SA_ERR_STATE, "a take beyond the last scene");
          sa_batch_result_free(held);
          held = nullptr;
          for (uint32_t s = 0; s < c.scenes; ++s)
            if (tracks_eq("overlapped handle", R.scene_ids[s], held_got[s].data(), held_want[s].data(), held_want[s].size())) return 1;
          ++g_cov.next_begun_before_last_taken;
        }
        for (uint32_t s = 0; s + 1 < c.scenes; ++s)
          if (R.take_one(h, s % 2 == 1, &R.got, R.scene_ids)) return 1;
        held = h; held_want = R.want; held_got = R.got;
      } else if (c.manner == SECOND_THREAD) {
        if (join_consumer()) return 1;   // (the previous set's consumer ran beside this set's begin)
        if (f % 6 == 5 && c.scenes > 1) {   // a handle freed with scenes still in it
          if (R.take_one(h, false, &R.got, R.scene_ids)) return 1;
          sa_batch_result_free(h);
          ++g_cov.handles_freed_early;
        } else {
          consumer_want = R.want; consumer_got = R.got;
          const std::vector<uint64_t> ids = R.scene_ids;
          const uint32_t S = c.scenes;
          consumer = std::thread([h, S, ids, &consumer_got, &consumer_bad, &R] {
            for (uint32_t s = 0; s < S; ++s)
              if (R.take_one(h, s % 3 == 2, &consumer_got, ids)) consumer_bad.fetch_add(1);
            sa_batch_result_free(h);
          });
          ++g_cov.second_thread_handles;
        }
      } else {
        for (uint32_t s = 0; s < c.scenes; ++s) {
          if (c.manner == POLL_READY)
            while (!sa_batch_result_ready(h)) std::this_thread::yield();
          if (R.take_one(h, c.manner == POLL_READY && s % 2 == 0, &R.got, R.scene_ids)) return 1;
        }
        CHECK(!sa_batch_result_ready(h), "a drained handle says ready");
        sa_batch_result_free(h);
        if (R.compare_outputs("handle")) return 1;
      }
    }
    ++g_cov.sets;
    if (c.manner == SECOND_THREAD && consumer.joinable() && f % 2) continue;   // (every other set: the consumer is left running into the next begin)
    if (join_consumer()) return 1;
    R.note_after_request();
    if (f % 3 == 2 && compare_state(R, f % 9 == 8, c.drains && f % 9 == 8)) return 1;   // (two sets in three leave the deferred bookkeeping for the next request)
    if (c.skips && f > c.frames / 3 && f < c.frames / 3 + 12 && f % 4 == 0) {
      const uint64_t scene = R.scene_ids[(uint32_t)f % c.scenes], n = 1 + (uint64_t)f % 3;
      CHECK(sa_tracker_skip_epochs(R.t, scene, n) == SA_OK, "skip_epochs: %s", sa_tracker_last_error(R.t));
      or_tracker_skip_epochs(R.o, scene, n);
      if (compare_state(R, false, false)) return 1;
    }
  }
  if (join_consumer()) return 1;
  if (held) { sa_batch_result_free(held); ++g_cov.handles_freed_early; }
  if (compare_state(R, true, true)) return 1;
  end_run(R);
  return 0;
}

std::string name_of(const Config& c) {
  char buf[256];
  snprintf(buf, sizeof buf, "%s%s scenes=%u workers=%d batch_ids=%d device_upkeep=%d %s spin_us=%d devices=%u seed=%llu", c.mode == SINGLE ? "predict" : c.mode == SYNC ? "predict_batch" : "handle",
           c.mode != HANDLE ? "" : c.manner == TAKE_ALL ? "/take" : c.manner == POLL_READY ? "/poll" : c.manner == OVERLAP_NEXT ? "/overlap" : "/thread", c.scenes, c.workers, c.batch_ids,
           c.device_upkeep, c.kind == SA_POS_IOU ? "iou" : "mahalanobis", c.spin_us, c.n_devices, (unsigned long long)c.seed);
  return buf;
}

// Trackers destroyed with a driver alive, with a flight just posted, and with a handle still held.
int create_destroy(int reps) {
  g_where = "create and destroy";
  Config c;
  c.mode = HANDLE; c.scenes = 3; c.workers = 2; c.batch_ids = 1; c.lo = 8; c.hi = 10;
  for (int rep = 0; rep < reps; ++rep) {
    Run R;
    c.seed = 1000 + (uint64_t)rep;
    c.spin_us = rep % 2 ? 0 : -1;
    if (make_run(R, c)) return 1;
    sa_batch_result* h = nullptr;
    const int sets = 1 + rep % 2;
    for (int f = 0; f < sets; ++f) {
      for (uint32_t s = 0; s < c.scenes; ++s) R.sims[s].frame(R.rng, 0.02f, &R.obs[s]);
      R.point();
      if (h) sa_batch_result_free(h);
      CHECK(sa_tracker_predict_batch_begin(R.t, c.scenes, R.scene_ids.data(), R.counts.data(), R.obs_p.data(), &h) == SA_OK, "begin: %s", sa_tracker_last_error(R.t));
    }
    const int how = rep % 3;
    if (how == 0) {          // the driver alive and idle: every scene taken, the handle freed
      for (uint32_t s = 0; s < c.scenes; ++s)
        if (R.take_one(h, false, &R.got, R.scene_ids)) return 1;
      sa_batch_result_free(h);
      end_run(R);
    } else if (how == 1) {   // a flight just posted: destroy waits for it; the handle outlives the tracker
      end_run(R);
      if (R.take_one(h, false, &R.got, R.scene_ids)) return 1;
      sa_batch_result_free(h);
    } else {                 // a handle still held, one scene taken
      if (R.take_one(h, true, &R.got, R.scene_ids)) return 1;
      end_run(R);
      sa_batch_result_free(h);
    }
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const int scale = argc > 1 ? std::max(1, atoi(argv[1])) : 1;   // (frames per configuration of the grids: x scale)
  std::vector<Config> all;
  uint64_t seed = 1;
  // single scene: host and device upkeep, IoU and Mahalanobis, 300 frames, churn enough for the eviction path (64 expired rows)
  for (int dev = 0; dev < 2; ++dev)
    for (int kind : {SA_POS_IOU, SA_POS_MAHALANOBIS}) {
      Config c;
      c.mode = SINGLE; c.device_upkeep = dev; c.kind = kind; c.frames = 300; c.churn = 0.04f; c.waste_every = 100; c.max_idle = 2; c.lo = 20; c.hi = 36; c.drains = false; c.seed = seed++;
      all.push_back(c);
    }
  // the long batches: scenes evict from their pool threads, and together
  for (int manner = 0; manner < 2; ++manner) {
    Config c;
    c.mode = manner ? HANDLE : SYNC; c.scenes = 4; c.workers = 4; c.batch_ids = 1; c.frames = 120; c.churn = 0.06f; c.waste_every = 100; c.lo = 20; c.hi = 30; c.skips = false; c.drains = false; c.seed = seed++;
    all.push_back(c);
  }
  // synchronous batches
  for (uint32_t scenes : {1u, 3u, 16u})
    for (int workers : {1, 4, -4, 16})
      for (int ids = 0; ids < 2; ++ids) {
        Config c;
        c.mode = SYNC; c.scenes = scenes; c.workers = workers; c.batch_ids = ids; c.device_upkeep = (scenes + (uint32_t)ids + (uint32_t)(workers > 0)) % 3 ? 1 : 0;
        c.kind = (workers == -4) ? SA_POS_MAHALANOBIS : SA_POS_IOU;
        c.frames = (scenes == 16 ? 10 : 20) * scale; c.lo = scenes == 16 ? 8 : 12; c.hi = scenes == 16 ? 12 : 30; c.seed = seed++;
        all.push_back(c);
      }
  // result handles, consumed in order and from a second thread
  for (uint32_t scenes : {1u, 3u, 16u})
    for (int workers : {1, 4, -4, 16})
      for (int ids = 0; ids < 2; ++ids)
        for (int spin : {-1, 0})
          for (Manner m : {TAKE_ALL, POLL_READY, OVERLAP_NEXT, SECOND_THREAD}) {
            Config c;
            c.mode = HANDLE; c.manner = m; c.scenes = scenes; c.workers = workers; c.batch_ids = ids; c.spin_us = spin;
            c.kind = (workers == 16) ? SA_POS_MAHALANOBIS : SA_POS_IOU;
            c.frames = (scenes == 16 ? 8 : 12) * scale; c.lo = scenes == 16 ? 8 : 12; c.hi = scenes == 16 ? 12 : 24; c.seed = seed++;
            all.push_back(c);
          }
  // device groups: one id counter, one waste cadence
  for (uint32_t nd : {2u, 3u})
    for (int ids = 0; ids < 2; ++ids)
      for (Mode mode : {SYNC, HANDLE}) {
        Config c;
        c.mode = mode; c.manner = ids ? TAKE_ALL : POLL_READY; c.scenes = 7; c.workers = 2; c.batch_ids = ids; c.n_devices = nd; c.frames = 30 * scale; c.lo = 8; c.hi = 14; c.waste_every = 7;
        c.seed = seed++;
        all.push_back(c);
      }
  for (const Config& c : all) {
    g_where = name_of(c);
    if (run_config(c)) return 1;
  }
  if (create_destroy(100)) return 1;
  g_where = "coverage";
  stub_counters k;
  stub_read_counters(&k);
  CHECK(k.engines_created == k.engines_destroyed, "engines: %llu created, %llu destroyed", (unsigned long long)k.engines_created, (unsigned long long)k.engines_destroyed);
  CHECK(k.stages_off_thread > 0, "no eviction was staged from a pool thread (%llu stages, %llu commits, %llu rows removed, %llu evicted tracks seen)", (unsigned long long)k.stages, (unsigned long long)k.commits, (unsigned long long)k.rows_removed, (unsigned long long)g_cov.evicted_tracks_seen);
  CHECK(k.waves > 0, "no eviction wave: never two scenes in one commit (%llu commits)", (unsigned long long)k.commits);
  CHECK(g_cov.begins_driver_asleep > 0 && g_cov.begins_driver_spinning > 0, "driver: asleep %llu spinning %llu", (unsigned long long)g_cov.begins_driver_asleep, (unsigned long long)g_cov.begins_driver_spinning);
  CHECK(g_cov.taken_before_finish > 0 && g_cov.taken_after_finish > 0, "scenes taken before their set finished %llu, after %llu", (unsigned long long)g_cov.taken_before_finish.load(), (unsigned long long)g_cov.taken_after_finish.load());
  CHECK(g_cov.scratch_set[0] > 0 && g_cov.scratch_set[1] > 0, "scratch sets used: %llu / %llu", (unsigned long long)g_cov.scratch_set[0], (unsigned long long)g_cov.scratch_set[1]);
  CHECK(g_cov.flush_behind_launches > 0, "flush_pending never ran behind a later set's launches");
  CHECK(g_cov.handles_freed_early > 0 && g_cov.second_thread_handles > 0 && g_cov.next_begun_before_last_taken > 0 && g_cov.refusals > 0, "handle manners");
  CHECK(k.fills_off_thread > 0 && k.results_off_thread > 0 && k.tables_off_thread > 0 && k.slots_off_thread > 0, "engine calls from pool threads");
  printf("ok configurations=%zu sets=%llu tracks_compared=%llu state_checks=%llu refusals=%llu evictions_staged=%llu from_pool_threads=%llu eviction_commits=%llu waves=%llu rows_evicted_or_wasted=%llu "
         "driver_asleep=%llu driver_spinning=%llu taken_before_finish=%llu taken_after_finish=%llu scratch_sets=%llu/%llu flush_behind_launches=%llu freed_early=%llu second_thread=%llu "
         "begun_before_last_taken=%llu trackers=%llu\n",
         all.size(), (unsigned long long)g_cov.sets, (unsigned long long)g_cov.tracks_compared, (unsigned long long)g_cov.state_checks, (unsigned long long)g_cov.refusals, (unsigned long long)k.stages,
         (unsigned long long)k.stages_off_thread, (unsigned long long)k.commits, (unsigned long long)k.waves, (unsigned long long)k.rows_removed, (unsigned long long)g_cov.begins_driver_asleep,
         (unsigned long long)g_cov.begins_driver_spinning, (unsigned long long)g_cov.taken_before_finish.load(), (unsigned long long)g_cov.taken_after_finish.load(), (unsigned long long)g_cov.scratch_set[0],
         (unsigned long long)g_cov.scratch_set[1], (unsigned long long)g_cov.flush_behind_launches, (unsigned long long)g_cov.handles_freed_early, (unsigned long long)g_cov.second_thread_handles,
         (unsigned long long)g_cov.next_begun_before_last_taken, (unsigned long long)k.engines_created);
  return 0;
}
