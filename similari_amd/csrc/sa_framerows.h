// sa_framerows.h — what sa_engine.hip and sa_framerows.hip share of include/similari_framerows.h: the host checks of a frame's row
// descriptor, its per-detection row table, and the one widen launch of an uploaded request set.
#pragma once
#include "sa_engine.h"
#include "../../include/similari_framerows.h"

extern "C" __attribute__((visibility("hidden"))) bool sa_in_device_block(const void* p, size_t bytes, int* device);   // sa_engine.hip

// One scene of the widen launch (blockIdx.y), in the bank's arena behind the scene descriptors.
struct SaWidenSlot {
  const char* base;        // sa_dev_rows.base
  uint64_t row_stride;     // elements
  const uint32_t* table;   // [n] source row of detection i, SA_ROW_NONE = no feature (the slot's part of the arena)
  float* dst;              // [n][D] f32: the slot's feat_raw
  uint32_t n;
  int32_t elem;            // SA_ELEM_*
};

// What the host checks of sa_framerows_check found out on the way.
struct SaFrameRows {
  bool in_place = false;     // f32, contiguous, no index, every detection present, 16-byte aligned: today's pointer route
  bool index_absent = false; // some index entry is SA_ROW_NONE
  uint32_t present = 0;      // detections with a feature
};

// The row is read with one 16-byte load per lane and step (the kernel's own test; sa_framerows_last counts by it).
__host__ __device__ inline bool sa_widen_row_is_wide(uint64_t addr, uint32_t D) { return ((addr & 15u) | (uint64_t)(D & 3u)) == 0; }
static inline uint32_t sa_widen_elem_bytes(int elem) { return elem == SA_ELEM_F32 ? 4u : 2u; }

// Every refusal of include/similari_framerows.h, on the host, before anything is staged.  device / D / visual: the engine's.
int sa_framerows_check(sa_engine* e, const char* what, int device, uint32_t D, bool visual, const sa_detections* d, const sa_dev_rows* r,
                       SaFrameRows* out);
// table[i] = the source row of detection i or SA_ROW_NONE; present (or nullptr) [i] = whether it has a feature
void sa_framerows_table(const sa_detections* d, const sa_dev_rows* r, uint32_t* table, uint8_t* present);
// k_widen_rows over n_slots scenes (slots: device address of their array), max_n = the largest SaWidenSlot::n; elem = the scenes' common
// element type, or -1 when they differ.  start / done (optional): stamped by the dispatch itself with its begin / carried as its
// completion signal.
hipError_t sa_launch_widen_rows(const SaWidenSlot* slots, uint32_t n_slots, uint32_t max_n, uint32_t D, int elem, hipStream_t st,
                                hipEvent_t start, hipEvent_t done);
