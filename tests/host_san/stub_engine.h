// stub_engine.h — what the host-sanitizer programs read from the test-only engine (stub_engine.cpp).  TEST INFRASTRUCTURE ONLY.
#pragma once
#include <cstdint>

extern "C" {
// Process-wide counters of what the facade and the router made the stub do (every engine of the process adds to them).
struct stub_counters {
  uint64_t engines_created, engines_destroyed;
  uint64_t sets_begun;            // sa_batch_begin
  uint64_t scenes_associated;     // scenes through sa_batch_run*, sa_associate_batch
  uint64_t stages;                // sa_tracks_remove_stage
  uint64_t stages_off_thread;     // ... from a thread other than the one that called sa_batch_begin for the set (a pool thread)
  uint64_t commits;               // sa_tracks_remove_commit / _many that had something to take out
  uint64_t waves;                 // ... of two scenes or more
  uint64_t rows_removed;
  uint64_t fills_off_thread;      // sa_batch_fill from a thread other than the set's
  uint64_t results_off_thread;    // sa_batch_results from a thread other than the set's (pool thread, driver)
  uint64_t tables_off_thread;     // sa_tracks_apply_collect_table likewise
  uint64_t slots_off_thread;      // sa_tracks_apply_collect_slot likewise
};
void stub_read_counters(stub_counters* out);
}
