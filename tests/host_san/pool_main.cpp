// pool_main.cpp — the facade's fork-join pool (similari_amd/csrc/sa_pool.h) in the scenarios a data race would need, for a thread or
// address sanitizer build.  The first part is the program of tests/test_pool.py; the rest drives the stop_ / gen_ hand-over on every path
// of loop(), both branches of the sleepers' handshake in run(), exceptions on both sides of one run, and plain per-job memory.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <exception>
#include <functional>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>
// (the program counts the two branches of run()'s handshake by looking at the sleepers' count right before a run)
#define private public
#include "sa_pool.h"
#undef private

#define CHECK(cond, ...) do { if (!(cond)) { printf("BAD " __VA_ARGS__); printf("\n"); fflush(stdout); return 1; } } while (0)

static void nap_us(int us) { std::this_thread::sleep_for(std::chrono::microseconds(us)); }

static int claims_and_jobs(int* allowed_out, int* pinned_out) {
  int allowed = 0;
  cpu_set_t set; CPU_ZERO(&set);
  if (sched_getaffinity(0, sizeof set, &set) == 0) allowed = CPU_COUNT(&set);
  SaPool a(2), b(2);
  SaPool* c = new SaPool(1);
  std::set<int> seen;
  size_t n = 0;
  for (const SaPool* p : {(const SaPool*)&a, (const SaPool*)&b, (const SaPool*)c})
    for (int cpu : p->claimed_cpus()) { seen.insert(cpu); ++n; }
  const bool pinned = !a.claimed_cpus().empty();
  CHECK(!(allowed >= 9 && !(pinned && a.claimed_cpus().size() == 3 && b.claimed_cpus().size() == 3 && c->claimed_cpus().size() == 2)), "sizes");
  CHECK(seen.size() == n, "overlap");
  CHECK(!(pinned && (a.next_cpu() != a.claimed_cpus().back())), "next");
  const std::vector<int> was = c->claimed_cpus();
  delete c;                               // its CPUs are free again: the next pool takes them
  SaPool d(1);
  CHECK(was.empty() || d.claimed_cpus() == was, "release");
  std::vector<std::atomic<int>> hits(64);
  for (int rep = 0; rep < 2000; ++rep) {
    const uint32_t jobs = 1 + rep % 64;
    for (auto& h : hits) h = 0;
    a.run(jobs, [&](uint32_t i) { hits[i].fetch_add(1); });
    for (uint32_t i = 0; i < 64; ++i) CHECK(hits[i] == (i < jobs ? 1 : 0), "job %u of %u", i, jobs);
  }
  // a job that throws: run() comes back (every worker has answered) and rethrows on the caller; the pool works afterwards
  for (uint32_t bad : {0u, 1u, 5u}) {
    bool caught = false;
    try { a.run(8, [&](uint32_t i) { if (i == bad) throw std::runtime_error("job failed"); }); } catch (const std::runtime_error&) { caught = true; }
    CHECK(caught, "exception of job %u lost", bad);
    for (auto& h : hits) h = 0;
    a.run(8, [&](uint32_t i) { hits[i].fetch_add(1); });
    for (uint32_t i = 0; i < 8; ++i) CHECK(hits[i] == 1, "run after an exception");
  }
  SaPool lazy(2, true, 0);   // spin_us = 0: the workers sleep at once
  for (int rep = 0; rep < 50; ++rep) {
    for (auto& h : hits) h = 0;
    lazy.run(6, [&](uint32_t i) { hits[i].fetch_add(1); });
    for (uint32_t i = 0; i < 6; ++i) CHECK(hits[i] == 1, "lazy pool");
  }
  *allowed_out = allowed;
  *pinned_out = (int)pinned;
  return 0;
}

// Pools created and destroyed: at once, right behind a run, and with the workers asleep — stop_ is a plain field read behind gen_.
static int create_destroy(int reps, unsigned* asleep_at_destroy) {
  for (int rep = 0; rep < reps; ++rep) {
    const uint32_t workers = 1 + (uint32_t)rep % 3;
    const bool pin = rep % 4 == 0;
    const int spin = rep % 2 ? 0 : 100;
    { SaPool p(workers, pin, spin); }
    {
      SaPool p(workers, pin, spin);
      std::vector<uint32_t> out(9, 0);
      p.run(9, [&](uint32_t i) { out[i] = i + 1; });
      for (uint32_t i = 0; i < 9; ++i) CHECK(out[i] == i + 1, "job %u of a short-lived pool", i);
    }
    {
      SaPool p(workers, pin, spin);
      if (rep % 2) { std::vector<uint32_t> out(5, 0); p.run(5, [&](uint32_t i) { out[i] = i; }); }
      for (int w = 0; w < 200 && p.sleepers_.load() != workers; ++w) nap_us(100);   // (until every worker has gone to sleep)
      if (p.sleepers_.load() == workers) ++*asleep_at_destroy;
    }
  }
  return 0;
}

// Runs spaced inside and outside the spin window, on a default pool and on one that never spins: the caller of run() must find the
// workers awake (no notify) and asleep (lock + notify), and every job runs exactly once either way.  The jobs write plain memory that
// the caller reads after run(): the release / acquire pair on the acknowledgement words is the only thing that orders them.
static int handshake(unsigned* found_awake, unsigned* found_asleep) {
  for (int kind = 0; kind < 2; ++kind) {
    SaPool p(3, kind == 0, kind == 0 ? -1 : 0);
    std::vector<uint64_t> in(64), out(64);
    for (int rep = 0; rep < 400; ++rep) {
      const uint32_t jobs = 2 + (uint32_t)rep % 62;
      for (uint32_t i = 0; i < jobs; ++i) { in[i] = (uint64_t)rep * 1000 + i; out[i] = 0; }   // plain stores before the run ...
      const int gap = rep % 8;
      if (gap == 7) nap_us(2500);        // far outside the spin window: asleep
      else if (gap == 6) nap_us(150);    // inside the default window, outside an empty one
      const uint32_t sleeping = p.sleepers_.load(std::memory_order_seq_cst);
      if (sleeping) ++*found_asleep; else ++*found_awake;
      p.run(jobs, [&](uint32_t i) { out[i] = in[i] * 3 + 1; });                               // ... plain loads and stores in the jobs ...
      for (uint32_t i = 0; i < jobs; ++i) CHECK(out[i] == in[i] * 3 + 1, "job %u of %u (rep %d, pool %d)", i, jobs, rep, kind);   // ... plain loads behind it
    }
  }
  return 0;
}

// One run in which the caller's share AND a worker's share throw: exactly one exception comes out, and the pool is clean afterwards.
static int both_throw(unsigned* from_caller, unsigned* from_worker) {
  SaPool p(2, false, -1);
  for (int rep = 0; rep < 200; ++rep) {
    int caught = 0;
    std::string what;
    try {
      p.run(6, [&](uint32_t i) {
        if (i == 0 || i == 3) throw std::runtime_error("caller's share");   // thread 0 = the caller: jobs 0 and 3
        if (i == 1 || i == 2) throw std::runtime_error("worker's share");   // workers 0 and 1
      });
    } catch (const std::runtime_error& ex) { ++caught; what = ex.what(); }
    CHECK(caught == 1, "%d exceptions out of one run", caught);
    if (what == "caller's share") ++*from_caller; else if (what == "worker's share") ++*from_worker; else CHECK(false, "a foreign exception");
    std::vector<uint32_t> out(7, 0);
    p.run(7, [&](uint32_t i) { out[i] = i + 10; });   // (no stale error_ is rethrown by the next run)
    for (uint32_t i = 0; i < 7; ++i) CHECK(out[i] == i + 10, "run after two exceptions");
  }
  // a worker's exception alone still arrives
  for (int rep = 0; rep < 50; ++rep) {
    bool caught = false;
    try { p.run(3, [&](uint32_t i) { if (i == 2) throw std::runtime_error("worker's share"); }); } catch (const std::runtime_error&) { caught = true; ++*from_worker; }
    CHECK(caught, "a worker's exception was lost");
  }
  return 0;
}

int main() {
  int allowed = 0, pinned = 0;
  if (claims_and_jobs(&allowed, &pinned)) return 1;
  unsigned asleep_at_destroy = 0, found_awake = 0, found_asleep = 0, from_caller = 0, from_worker = 0;
  const int reps = 300;
  if (create_destroy(reps, &asleep_at_destroy)) return 1;
  if (handshake(&found_awake, &found_asleep)) return 1;
  if (both_throw(&from_caller, &from_worker)) return 1;
  CHECK(asleep_at_destroy > 0, "no pool was destroyed with its workers asleep");
  CHECK(found_awake > 0 && found_asleep > 0, "the sleepers' handshake took one branch only: awake %u asleep %u", found_awake, found_asleep);
  CHECK(from_caller > 0 && from_worker > 0, "exceptions: caller's %u worker's %u", from_caller, from_worker);
  printf("ok allowed=%d pinned=%d pools=%d asleep_at_destroy=%u run_found_awake=%u run_found_asleep=%u rethrown_caller=%u rethrown_worker=%u\n",
         allowed, pinned, reps * 3, asleep_at_destroy, found_awake, found_asleep, from_caller, from_worker);
  return 0;
}
