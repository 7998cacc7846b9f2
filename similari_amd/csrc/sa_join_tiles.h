// sa_join_tiles.h — which tiles the join's launch 1 runs (k_search_tile<EU, JOIN = true, COMPAT>, sa_gemm.hip), and how a workgroup index finds
// its tile.  Host and device; tests/test_join_tiles.py compiles it with the host compiler and walks every index.
//
// The store is contracted with itself: N observation slots on both sides, row tiles of BM slots, column tiles of BN = r * BM slots
// (64 x 64: r = 1; 32 x 128: r = 4).  Tile (i, j) — rows from m0 = i * BM, columns from n0 = j * BN — runs when it reaches the diagonal or
// lies above it: n0 + BN > m0, that is (j + 1) * r > i.  Column j therefore runs its first min(R, (j + 1) * r) row tiles, R = the row
// tile count: a true triangle for r = 1, a staircase with steps of r rows for r > 1.  Workgroups are numbered column by column, rows
// ascending inside a column, so the tiles before column j number r * j * (j + 1) / 2 whatever R is (only the last column is cut by R).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SA_JT_HD __host__ __device__ inline
#else
#define SA_JT_HD static inline
#endif

// tiles of R row tiles with r row tiles per column tile; 0 for R == 0
SA_JT_HD uint64_t sa_join_tile_count(uint32_t R, uint32_t r) {
  if (!R) return 0;
  const uint64_t C = ((uint64_t)R + r - 1) / r;   // column tiles
  return (uint64_t)r * (C * (C - 1) / 2) + R;
}

// what the rectangular grid of a search over the same rows launches
SA_JT_HD uint64_t sa_join_tile_rect(uint32_t R, uint32_t r) { return (uint64_t)R * (((uint64_t)R + r - 1) / r); }

// The grid that carries `tiles` workgroups.  One dimension of a dispatch holds fewer than 2^32 work-items — 2^24 workgroups of 256
// threads, 2^23 of 512 — and a join of 65535 x 32 observation slots has 5.4e8 tiles, so the grid is two-dimensional: gx = at most
// SA_JOIN_GRID_X workgroups across (2^25 work-items at 512 threads), gy = as many rows of them as the tiles need (at most 8193 at the
// largest extents), idx = blockIdx.x + gridDim.x * blockIdx.y, and the workgroups of the last row with idx >= tiles leave at once.
#define SA_JOIN_GRID_X 65536u
SA_JT_HD void sa_join_grid(uint64_t tiles, uint32_t* gx, uint32_t* gy) {
  *gx = (uint32_t)(tiles < SA_JOIN_GRID_X ? (tiles ? tiles : 1u) : SA_JOIN_GRID_X);
  *gy = (uint32_t)((tiles + *gx - 1) / *gx);
}
SA_JT_HD uint64_t sa_join_grid_index(uint32_t bx, uint32_t by, uint32_t gx) { return (uint64_t)by * gx + bx; }

// idx < sa_join_tile_count(R, r) -> row tile i, column tile j.  j is the largest column with r * j * (j + 1) / 2 <= idx: a float square
// root gives a first guess (idx stays below 2^30 at the extents a join admits, the root below 2^16, so the guess is off by one at
// most), integer steps settle it.
SA_JT_HD void sa_join_tile_decode(uint64_t idx, uint32_t r, uint32_t* i, uint32_t* j) {
  const uint64_t x = idx / r;   // j * (j + 1) / 2 <= x
  uint64_t c = (uint64_t)((__builtin_sqrtf(8.0f * (float)x + 1.0f) - 1.0f) * 0.5f);
  while (c * (c + 1) / 2 > x) --c;
  while ((c + 1) * (c + 2) / 2 <= x) ++c;
  *j = (uint32_t)c;
  *i = (uint32_t)(idx - (uint64_t)r * (c * (c + 1) / 2));
}
