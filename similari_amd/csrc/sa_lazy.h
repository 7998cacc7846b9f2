// sa_lazy.h — the positional stage's mode for a VisualSORT frame (no device code: host-only tests compile it on its own).
//   eager: the first phase's positional tiles evaluate every cell of the frame;
//   lazy:  the first phase evaluates none, and the one-workgroup tail evaluates the cells of the rows the visual vote leaves over
//          (k_assign_small<.., LAZY>), after the vote words are known.  Same edges, same results.
#pragma once
#include <stdint.h>
#include "../../include/similari_assoc.h"

// Lazy while every scene of the request set reported at most this many leftover rows (rows without a visual group) in its newest
// collected frame: the crossover between what the positional tiles cost the first phase (C2's k_frame_visual: 15.2 us eager, 13.0 lazy)
// and what the tail's lazy phase costs per leftover row (c2n, 250 of 1000 rows left over: k_assign_small 4.2 -> 45 us, ~0.16 us a row).
// A scene without a report yet counts as 0.
#define SA_LAZY_MAX_LEFT 14u

// possible: the frame takes the one-workgroup tail with one column per thread, single vote words, IoU (the only form with a lazy
// phase).  flags: sa_config.flags plus the engine's SA_POSITIONAL override.  max_left: the largest hint over the set's scenes.
static inline bool sa_lazy_positional(bool possible, uint32_t flags, uint32_t max_left) {
  if (!possible) return false;
  if (flags & SA_FLAG_LAZY_POSITIONAL) return true;             // wherever possible, whatever the hint (with SA_FLAG_TAP too: the lazy edges)
  if (flags & (SA_FLAG_EAGER_POSITIONAL | SA_FLAG_TAP)) return false;   // (the taps compare every cell's edge record by default)
  return max_left <= SA_LAZY_MAX_LEFT;
}
