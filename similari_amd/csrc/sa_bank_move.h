// sa_bank_move.h — what the steps behind a BestFit vote share on the device: the walk that resolves a winner's id to its slot, and
// the two ways a destination bank takes another bank's rows under a retention rule (include/similari_retain.h).  sa_absorb.hip feeds
// them the padded query rows of a search (k_absorb_match, k_absorb_move, k_absorb_move_best), sa_consolidate.hip another bank of the
// same store (k_consolidate_pair, k_consolidate_merge, k_consolidate_merge_best).  Device code only; every function is called by a
// whole wave, one wave per destination, `lane` its lane.
//
// Ownership, which both callers must give: the destination bank is read and written by this wave alone, the source rows are read by
// this wave and written by nobody while the launch runs.  s_feat / s_norm / s_qual carry no __restrict__ here, and the source
// pointers promise nothing either, so the source may be another bank of the same arrays.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sa_engine.h"   // SA_SEARCH_NONE

// The slot of the stored track whose id is w, SA_SEARCH_NONE if no slot holds it.  The wave walks s_ids, four loads in flight per
// lane; ids are unique, so at most one lane meets it, and the minimum over the wave is its slot.
__device__ __forceinline__ uint32_t sa_bank_find_slot(uint64_t w, const uint64_t* __restrict__ s_ids, uint32_t T, uint32_t lane) {
  constexpr uint32_t U = 4;
  uint32_t found = SA_SEARCH_NONE;
  for (uint32_t s0 = lane; s0 < T; s0 += U * 64u) {
    uint64_t id[U];
#pragma unroll
    for (uint32_t u = 0; u < U; ++u) id[u] = s0 + u * 64u < T ? s_ids[s0 + u * 64u] : 0ull;   // 0 is no id
#pragma unroll
    for (uint32_t u = 0; u < U; ++u)
      if (id[u] == w) found = s0 + u * 64u;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t x = __shfl_xor(found, o);
    found = x < found ? x : found;
  }
  return found;
}

// SA_KEEP_LATEST.  Rows are 16-byte pieces of a row of Dp floats as the movers of sa_merge.hip count it (sa_store::row_floats).  The
// destination bank — rows bank .. bank + Kp - 1 of s_feat — holds n0 rows (a created slot: none) and takes the source's n1 — rows
// qrow .. of q_feat — at capacity C: keep = min(n0 + n1, C), drop = n0 + n1 - keep; position j takes combined row drop + j — the
// bank's own row drop + j while that is below n0, else row drop + j - n0 of the source —, the row's norm moves with it, positions
// keep .. n0 - 1 (a created slot: keep .. Kp - 1) end zeroed with norm 0.  Returns keep.
// The bank shifts onto itself when drop > 0.  The one owning wave moves the rows in ascending j, and piece i of a row is read and
// written by the same lane (i % 64) in every iteration: position j is written in iteration j and read, as row drop + j', only in
// iteration j' = j - drop < j, earlier in that lane's program order.
__device__ __forceinline__ uint32_t sa_bank_take_latest(uint32_t lane, bool created, uint32_t n0, uint32_t n1, uint32_t C, uint32_t Kp,
                                                        uint32_t Dp, const float* q_feat, const float* q_norm, size_t qrow, float* s_feat,
                                                        float* s_norm, size_t bank) {
  const uint32_t tot = n0 + n1, keep = tot < C ? tot : C, drop = tot - keep;
  const uint32_t end = created ? Kp : (n0 > keep ? n0 : keep);
  for (uint32_t j = 0; j < end; ++j) {
    float4* to = (float4*)(s_feat + (bank + j) * Dp);
    if (j >= keep) {
      for (uint32_t i = lane; i < Dp / 4; i += 64u) to[i] = float4{0.f, 0.f, 0.f, 0.f};
      if (lane == 0) s_norm[bank + j] = 0.f;
      continue;
    }
    const uint32_t r = drop + j;
    if (r < n0) {
      if (drop == 0) continue;   // the row stays where it is
      const float4* from = (const float4*)(s_feat + (bank + r) * Dp);
      for (uint32_t i = lane; i < Dp / 4; i += 64u) to[i] = from[i];
      if (lane == 0) s_norm[bank + j] = s_norm[bank + r];
    } else {
      const float4* from = (const float4*)(q_feat + (qrow + (r - n0)) * Dp);
      for (uint32_t i = lane; i < Dp / 4; i += 64u) to[i] = from[i];
      if (lane == 0) s_norm[bank + j] = q_norm[qrow + (r - n0)];
    }
  }
  return keep;
}

// SA_KEEP_BEST.  The combined bank — the destination's n0 rows in bank order, then the source's n1 in their order — has tot = n0 + n1
// <= 2 K <= 64 observations, one per lane (K = 32: every lane, 63 included, so nothing here shifts a mask by the lane).  Lane i
// loads its observation's norm and quality, and its rank is the number of j with q_j > q_i plus the number of j < i with q_j == q_i:
// the place std::stable_sort with > gives it (sa_merge_plan.h; -0.0 == 0.0 in both compares, NaN was refused).  The ranks are a
// permutation of 0 .. tot - 1.  keep = min(tot, C); position p < keep takes the observation of rank p, found by a ballot and
// find-first, so its source row is wave-uniform; positions keep .. n0 - 1 (a created slot: keep .. KP - 1) end zeroed with norm 0 and
// quality +0.0.  Returns keep.
// Rows permute arbitrarily here, so sa_bank_take_latest's ascending order gives nothing.  Instead lane l owns the 16-byte pieces i =
// l, l + 64, .. of every row of the bank, and for each of its pieces it first loads that piece of the source of every retained
// position into registers (the loop over p is unrolled on KP, so the register index is static and only the address dynamic: 4 KP
// VGPRs, no scratch), then stores every position and zeroes the tail.  Within one piece all loads of a lane precede all of its stores
// — the bank pointers carry no __restrict__, so the compiler keeps that order —, a lane's other pieces are other addresses, and no
// lane touches another lane's pieces.  A bank's own row whose rank is its position is not written; it is the source of no other
// position.
// Norms and qualities move through the lane that holds the observation: lane i stores them at position rank_i.  Their loads come
// first in the wave's program order, and the store addresses depend on the rank, which depends — through the shuffles — on every
// lane's quality having arrived, the norms ahead of them.
typedef float v4f __attribute__((ext_vector_type(4)));   // a 16-byte piece as a register value

template <uint32_t KP>
__device__ __forceinline__ uint32_t sa_bank_take_best(uint32_t lane, bool created, uint32_t n0, uint32_t n1, uint32_t C, uint32_t Dp,
                                                      const float* q_feat, const float* q_norm, const float* q_qual, size_t qrow,
                                                      float* s_feat, float* s_norm, float* s_qual, size_t bank) {
  const uint32_t tot = n0 + n1, keep = tot < C ? tot : C;
  const uint32_t end = created ? KP : (n0 > keep ? n0 : keep);
  const bool have = lane < tot, own = lane < n0;
  float nv = 0.f, qv = 0.f;
  if (have) {
    nv = own ? s_norm[bank + lane] : q_norm[qrow + (lane - n0)];
    qv = own ? s_qual[bank + lane] : q_qual[qrow + (lane - n0)];
  }
  uint32_t rank = 0;
  for (uint32_t j = 0; j < tot; ++j) {
    const float qj = __shfl(qv, (int)j);
    rank += (qj > qv || (qj == qv && j < lane)) ? 1u : 0u;
  }
  // Position p < keep takes combined row r_p.  KP row addresses, or KP tests on keep and end, held across the piece loop would
  // outgrow the scalar registers.  So lane p (p < KP <= 32) keeps the address of position p's source — of the bank's row p itself where
  // nothing is to arrive, which makes every load of the piece loop unconditional — and two words say what is stored: moves, bit p: position
  // p is written from its source (a bank's own row whose rank is its position stays as it is); zeros, bit p: it is zeroed.  Every
  // turn of the piece loop reads all of them through an empty asm, which the compiler cannot hoist: an address is in scalar registers
  // only between its shuffle and its load, a test from its bit compare to its branch.
  uint32_t src = lane;   // lane p: the combined row that position p takes; no such observation (p >= tot): the bank's row p itself
#pragma unroll
  for (uint32_t p = 0; p < KP; ++p) {
    const unsigned long long b = __ballot(have && rank == p);
    if (b && lane == p) src = (uint32_t)__ffsll((long long)b) - 1u;
  }
  const bool fresh = src >= n0 && src < tot;   // a source row
  const float* mine = fresh ? q_feat + (qrow + (src - n0)) * Dp : s_feat + (bank + src) * Dp;
  const uint32_t moves = (uint32_t)__ballot(lane < keep && (fresh || src != lane));
  const uint32_t zeros = (uint32_t)__ballot(lane >= keep && lane < end);
  v4f* to = (v4f*)(s_feat + bank * Dp);
  const uint32_t pieces = Dp / 4;
  for (uint32_t i0 = 0; i0 < pieces; i0 += 64u) {   // every lane takes every turn: the shuffles below read lanes 0 .. KP - 1 of lo / hi
    const uint32_t i = i0 + lane;
    const bool on = i < pieces;
    uint32_t lo = (uint32_t)(uintptr_t)mine, hi = (uint32_t)((uintptr_t)mine >> 32), mv = moves, zr = zeros;
    asm volatile("" : "+v"(lo), "+v"(hi), "+v"(mv), "+v"(zr));
    mv = __builtin_amdgcn_readfirstlane(mv);
    zr = __builtin_amdgcn_readfirstlane(zr);
    v4f r[KP];
#pragma unroll
    for (uint32_t p = 0; p < KP; ++p) {
      const uintptr_t from = (uintptr_t)(uint32_t)__shfl((int)hi, (int)p) << 32 | (uint32_t)__shfl((int)lo, (int)p);
      r[p] = ((const __attribute__((address_space(1))) v4f*)from)[on ? i : 0u];   // (from an integer the pointer is generic; it is global memory)
    }
    if (!on) continue;
#pragma unroll
    for (uint32_t p = 0; p < KP; ++p) {
      if (mv >> p & 1u) to[p * pieces + i] = r[p];   // (Kp * Dp / 4 < 2^28)
      else if (zr >> p & 1u) to[p * pieces + i] = v4f{0.f, 0.f, 0.f, 0.f};
    }
  }
  if (have && rank < keep) {
    s_norm[bank + rank] = nv;
    s_qual[bank + rank] = qv;
  }
  if (lane >= keep && lane < end) {
    s_norm[bank + lane] = 0.f;
    s_qual[bank + lane] = 0.f;
  }
  return keep;
}
