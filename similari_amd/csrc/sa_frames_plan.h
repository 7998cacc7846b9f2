// sa_frames_plan.h — where the scenes of one sa_own_areas_batch / sa_nms_batch call (include/similari_frames.h) lie in the call's one
// staging block, and the shape of its launches.  sa_own_areas / sa_nms are the plan of one scene: first = 0, count = n, mask_off = 0.
// Host arithmetic only, from the scenes' box counts: sa_engine.hip turns the result into one upload, the launches and one copy back,
// the kernels of sa_upkeep.hip read the segment table it fills, and tests/test_frames_plan.py compiles this header on the host.
#pragma once
#include <stdint.h>

#include <vector>

#define SA_FRAMES_MAX_SCENES 65535u   // the scene is a grid dimension of every launch (blockIdx.y / .z)
#define SA_FRAMES_NMS_MAX 16384u      // boxes of one scene that may reach the pair stage (SA_NMS_MAX: k_nms_sweep<4> holds 64 * 64 * 4 bits)
#define SA_FRAMES_SPILL_LIST 64u      // boxes per launch of the own-area spill path: they share one block of HBM scratch

// One scene of the call, as the device reads it: rows [first, first + count) of the staging block.  NMS: W = 64-bit words per mask
// row of the scene, mask_off = where its count x W mask words begin (in words).
struct SaFrameSeg {
  uint32_t first, count, W, pad;
  uint64_t mask_off;
};

struct SaFramesPlan {
  std::vector<SaFrameSeg> segs;
  uint32_t total = 0;        // rows of the staging block
  uint32_t max_count = 0;    // the largest scene: the inner grid dimension
  uint32_t max_W = 0;
  uint32_t sweep_S = 0;      // NMS: the k_nms_sweep<S> class of the call — 1, 2 or 4 words of removed-bitmap per lane — from the largest scene
  uint64_t mask_words = 0;   // NMS: words of all masks together
};

enum SaFramesRefusal { SA_FRAMES_FITS = 0, SA_FRAMES_TOO_MANY_SCENES, SA_FRAMES_SCENE_TOO_LARGE, SA_FRAMES_TOO_MANY_ROWS };

// counts[s]: boxes of scene s that reach the device (NMS: after the host filter).  A scene of no boxes keeps its entry (count 0: its
// blocks leave at once).  *bad_scene: the scene a refusal is about.
static inline SaFramesRefusal sa_frames_plan(uint32_t n_scenes, const uint32_t* counts, bool nms, SaFramesPlan* plan, uint32_t* bad_scene) {
  *plan = SaFramesPlan();
  *bad_scene = 0;
  if (n_scenes > SA_FRAMES_MAX_SCENES) return SA_FRAMES_TOO_MANY_SCENES;
  plan->segs.resize(n_scenes);
  uint64_t first = 0, words = 0;
  for (uint32_t s = 0; s < n_scenes; ++s) {
    const uint32_t n = counts[s];
    *bad_scene = s;
    if (nms && n > SA_FRAMES_NMS_MAX) return SA_FRAMES_SCENE_TOO_LARGE;
    if (first + n > 0xffffffffull) return SA_FRAMES_TOO_MANY_ROWS;
    SaFrameSeg& g = plan->segs[s];
    g.first = (uint32_t)first;
    g.count = n;
    g.W = nms ? (n + 63u) / 64u : 0u;
    g.pad = 0;
    g.mask_off = words;
    first += n;
    words += (uint64_t)n * g.W;
    if (n > plan->max_count) plan->max_count = n;
    if (g.W > plan->max_W) plan->max_W = g.W;
  }
  *bad_scene = 0;
  plan->total = (uint32_t)first;
  plan->mask_words = words;
  const uint32_t S = (plan->max_W + 63u) / 64u;
  plan->sweep_S = !nms || !S ? 0u : S <= 1u ? 1u : S <= 2u ? 2u : 4u;
  return SA_FRAMES_FITS;
}

// Own areas, the spill path: `spilled` boxes go in lists of SA_FRAMES_SPILL_LIST, one launch each.
static inline uint32_t sa_frames_spill_launches(uint32_t spilled) { return (spilled + SA_FRAMES_SPILL_LIST - 1u) / SA_FRAMES_SPILL_LIST; }
