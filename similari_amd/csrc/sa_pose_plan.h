// sa_pose_plan.h — where the scenes of one sa_points_associate_batch call (include/similari_pose_batch.h) lie in the call's arrays, and
// the shape of its tile launch.  Host arithmetic only, from the scenes' track and pose counts: sa_pose.hip turns the result into one
// upload of the segment table and three launches, the batch kernels read the table, and tests/test_pose_plan.py compiles this header
// on the host.
#pragma once
#include <stdint.h>

#include <vector>

#define SA_POSE_PLAN_SCENES 65535u       // SA_POSE_BATCH_SCENES: a block finds its scene by 16 steps of bisection
#define SA_POSE_PLAN_SIDE 2048u          // SA_POSE_MAX: poses or tracks of one scene (the LDS tables of the assignment)
#define SA_POSE_PLAN_CELLS (1ull << 27)  // SA_POSE_BATCH_CELLS: pairs of all scenes together (8 B of gain each)
#define SA_POSE_PLAN_TILE_M 16u          // the tile of k_pose_tile: poses x tracks
#define SA_POSE_PLAN_TILE_T 64u

// One scene of the call, as the device reads it.  Poses [pose0, pose0 + m) of the call's rows, results and bid words; columns
// [track0, track0 + n) of the call's slot table and factor; cells [cell0, cell0 + m * n) of the gains and the tap, leading dimension n;
// blocks [tile0, tile0 + ceil(m / 16) * tiles_x) of the tile launch, tiles_x = ceil(n / 64) of them side by side.
struct SaPoseSeg {
  uint32_t pose0, m, track0, n;
  uint64_t cell0;
  uint32_t tile0, tiles_x;
};

struct SaPosePlan {
  std::vector<SaPoseSeg> segs;
  uint32_t poses = 0, tracks = 0, tiles = 0;   // the totals
  uint64_t cells = 0;
};

enum SaPoseRefusal { SA_POSE_FITS = 0, SA_POSE_TOO_MANY_SCENES, SA_POSE_SCENE_TOO_LARGE, SA_POSE_TOO_MANY_POSES, SA_POSE_TOO_MANY_TRACKS, SA_POSE_TOO_MANY_CELLS };

// track_counts[s], pose_counts[s]: the tracks and the poses of scene s.  An empty scene (no poses, or no tracks) keeps its entry and
// has no tile.  side: the most poses or tracks a scene may have (the call passes SA_POSE_PLAN_SIDE; within it and SA_POSE_PLAN_SCENES the
// sums always fit 32 bits, and those two refusals only guard a caller of this function with a larger side).  *bad_scene: the scene a
// refusal is about — the first that is too large, or the one with which a sum crosses its limit.
static inline SaPoseRefusal sa_pose_plan(uint32_t n_scenes, const uint32_t* track_counts, const uint32_t* pose_counts, uint32_t side, SaPosePlan* plan,
                                         uint32_t* bad_scene) {
  *plan = SaPosePlan();
  *bad_scene = 0;
  if (n_scenes > SA_POSE_PLAN_SCENES) return SA_POSE_TOO_MANY_SCENES;
  plan->segs.resize(n_scenes);
  uint64_t poses = 0, tracks = 0, cells = 0, tiles = 0;
  for (uint32_t s = 0; s < n_scenes; ++s) {
    const uint32_t n = track_counts[s], m = pose_counts[s];
    *bad_scene = s;
    if (m > side || n > side) return SA_POSE_SCENE_TOO_LARGE;
    if (poses + m > 0xffffffffull) return SA_POSE_TOO_MANY_POSES;
    if (tracks + n > 0xffffffffull) return SA_POSE_TOO_MANY_TRACKS;
    if ((uint64_t)m * n > SA_POSE_PLAN_CELLS - cells) return SA_POSE_TOO_MANY_CELLS;   // (cells <= the cap: no wrap)
    SaPoseSeg& g = plan->segs[s];
    g.pose0 = (uint32_t)poses;
    g.m = m;
    g.track0 = (uint32_t)tracks;
    g.n = n;
    g.cell0 = cells;
    g.tile0 = (uint32_t)tiles;   // (at most 2^27 non-empty scenes' worth of cells, one tile has at least one: tiles <= 2^27)
    g.tiles_x = m ? (n + SA_POSE_PLAN_TILE_T - 1u) / SA_POSE_PLAN_TILE_T : 0u;
    poses += m;
    tracks += n;
    cells += (uint64_t)m * n;
    tiles += (uint64_t)((m + SA_POSE_PLAN_TILE_M - 1u) / SA_POSE_PLAN_TILE_M) * g.tiles_x;
  }
  *bad_scene = 0;
  plan->poses = (uint32_t)poses;
  plan->tracks = (uint32_t)tracks;
  plan->cells = cells;
  plan->tiles = (uint32_t)tiles;
  return SA_POSE_FITS;
}
