// sa_vote_weight.h — what the two votes of a track search share on the device: the order of a ranked list and the weight of one
// pool block.  k_topn (sa_search.hip) and the BestFit stage (sa_bestfit.hip) include this one statement of them, so that a group
// weighs the same bits under either vote.
#pragma once
#include "sa_device.h"

constexpr uint32_t SA_VOTE_THREADS = 256;     // one workgroup per query row of grp, under either vote
constexpr uint32_t SA_VOTE_LDS_CAND = 2048;   // surviving groups of one query that a workgroup ranks from LDS; beyond, it re-reads grp

__device__ __forceinline__ bool ranks_before(double wa, uint64_t ia, double wb, uint64_t ib) { return wa > wb || (wa == wb && ia < ib); }

// sequential f64 sum of f64(f32(M - d)) over the kept (non-NaN) cells of one pool block, in row-major order — query observation outer,
// the order of Track::distances.  KK = Kp^2 is a power of two; from 64 cells on, sixteen 16-byte loads go out before the sums that use them.
__device__ __forceinline__ double block_weight(const float* __restrict__ c, uint32_t KK, float M) {
  double w = 0.0;
  if (KK >= 64) {
    constexpr uint32_t U = 16;
    for (uint32_t k = 0; k < KK; k += 4 * U) {
      float4 v[U];
#pragma unroll
      for (uint32_t u = 0; u < U; ++u) v[u] = *(const float4*)(c + k + 4 * u);
#pragma unroll
      for (uint32_t u = 0; u < U; ++u) {
        if (v[u].x == v[u].x) w += (double)(M - v[u].x);
        if (v[u].y == v[u].y) w += (double)(M - v[u].y);
        if (v[u].z == v[u].z) w += (double)(M - v[u].z);
        if (v[u].w == v[u].w) w += (double)(M - v[u].w);
      }
    }
  } else {
    for (uint32_t k = 0; k < KK; ++k) {
      const float d = c[k];
      if (d == d) w += (double)(M - d);
    }
  }
  return w;
}

// the same sum over the block read column by column: the order of Track::distances for the query whose observations are the block's
// columns (a join keeps one block per unordered pair of tracks, written by the lower slot as the query: include/similari_gallery.h).
// Eight strided loads go out before the sums that use them.
__device__ __forceinline__ double block_weight_t(const float* __restrict__ c, uint32_t Kp, float M) {
  double w = 0.0;
  if (Kp >= 8) {
    constexpr uint32_t U = 8;
    for (uint32_t o = 0; o < Kp; ++o)
      for (uint32_t i = 0; i < Kp; i += U) {
        float v[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) v[u] = c[(i + u) * Kp + o];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u)
          if (v[u] == v[u]) w += (double)(M - v[u]);
      }
  } else {
    for (uint32_t o = 0; o < Kp; ++o)
      for (uint32_t i = 0; i < Kp; ++i) {
        const float d = c[i * Kp + o];
        if (d == d) w += (double)(M - d);
      }
  }
  return w;
}
