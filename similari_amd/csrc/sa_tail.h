// sa_tail.h — what the one-workgroup assignment tail needs around its body; the body itself is sa_tail_body.h, shared by the stand-alone
// kernels (k_assign_small, sa_kernels.hip) and the last block of a one-launch lazy frame (k_frame_visual<.., HELP, TAIL>, sa_gemm.hip).
#pragma once
#include "sa_engine.h"
#include "sa_frame.h"
#include "sa_dense.h"
#include <type_traits>

#ifndef TAIL_STAMP   // (the in-kernel timeline of the stand-alone tail: sa_kernels.hip, -DSA_TAIL_TRACE)
#define TAIL_STAMP(k) do { } while (0)
#endif

// One 1024-thread workgroup per scene: edge lists -> LDS, components, solve, results.  The solver's duals / matches / search
// scratch live in LDS whenever the scene has at most 1024 tracks: every step of the shortest-path search is a chain of
// dependent accesses, ~10x cheaper in LDS than in L2.  VISUAL = the engine has a visual vote whose verdicts (row_has,
// vis_winner, col_excluded) must be honoured; plain SORT skips those loads altogether.
// Timeline at C3 (500 x 500 IoU, -DSA_TAIL_TRACE) before / after this version: scan 2.9 k cycles | pack + unite 8.1 k -> edge
// loads batched four at a time instead of one dependent round trip per edge | order rows inside components: 1024-key bitonic
// sort 6.8 k + link 0.7 k -> each row pushes itself on its root's LDS list, the solver thread orders the (short) list |
// solve 9.8 k | results 3.2 k.
// Workgroup barrier for phases that hand over LDS data only: __syncthreads() carries a workgroup-scope release, which on gfx9
// drains vmcnt as well (loads and stores share the counter) — every global load in flight would have to land before the
// barrier.  Here the long-latency loads (edge lists and track ids written by other XCDs: a trip to memory) are meant to stay in
// flight across the LDS phases, so only the LDS counter is drained.
__device__ __forceinline__ void sa_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// WORDS: the contraction's tiles reduced the BestFit vote into one 64-bit word per candidate and per track (SaParams::vote_words,
// visual_cosine_tile): thread q reads candidate q's word and track q's word, re-arms both, and the verdicts stay in registers
// (has / winner) and two LDS tables instead of going through k_bestfit_resolve's row_has / vis_winner / col_excluded — one
// dependent launch less per frame.
//
// The solve ("batched Jonker-Volgenant with per-row minima in LDS"):
//   1. greedy start, one thread per row, all rows at once: a row bids for the column of its heaviest usable edge (lowest column
//      on ties), a column goes to the lowest row that bids for it.  Under the duals u = -(heaviest gain), v = 0 those edges are
//      tight, so this is a feasible primal-dual start (what the shortest-path search would do for a row whose nearest column is
//      free, for every such row in ONE step).  In tracking frames almost every row keeps its bid.
//   2. the rows that lost their bid are the search roots of their connected component; every component that has any goes onto a
//      work queue;
//   3. the workgroup's 1024 / G groups of G lanes take components off the queue; a group orders the component's roots
//      (ascending: the canonical augmentation order) and runs sa_assign_component_coop<G> (sa_device.h): the search's two inner
//      loops — nearest labelled column, relax a row's edges — spread over the lanes, minima by lane reductions.
// A component of hundreds of rows (a crowd under a low IoU threshold) is then a few hundred microseconds of group work instead
// of seconds of one lane's dependent LDS chain; the usual one- and two-row components never reach step 3.
// Needs N <= SA_SMALL_N and T <= SA_SMALL_N (launcher; TC = 2: T <= SA_SMALL_T; wider frames: k_assign_small2, sa_kernels.hip): rows, columns and
// the usable edges (up to POOL of them; more stay in the HBM lists and are read from there) live in LDS.
// the dense solver (sa_dense.h): SA_DENSE_NT threads, each owning T / SA_DENSE_NT columns; components with at least SA_DENSE_MIN_ROOTS
// search roots on at least SA_DENSE_MIN_COLS columns (or whose edge lists stayed in HBM) go to it
#define SA_DENSE_NT 256
#define SA_DENSE_MIN_ROOTS 8u
#define SA_DENSE_MIN_COLS 128u
// The end of a scene's results, reported by the workgroup itself (done_seq != 0): every wave, when it has issued its last result, waits
// for its stores to be acknowledged (s_waitcnt vmcnt(0); the results are SYSTEM-scope stores — SA_OUT in k_assign_small —, acknowledged
// from the host's side of the link: a system-scope release per workgroup instead, i.e. an L2 write-back each, cost a 64-scene set
// 25 us) and counts itself in LDS; the wave that completes the count stores the launch's sequence number to the scene's completion word
// (a cache line of its own in the same block) — every result was acknowledged before that store was issued.  The host polls the word.
// Waves leave k_assign_small at three places; each of them reports.
__device__ __forceinline__ void sa_report_done(const SceneDev& S, uint64_t done_seq, uint32_t* s_done) {
  if (!done_seq) return;
  // (a workgroup-scope release alone is NOT that wait: the waves of a workgroup share their CU's memory pipeline, so the compiler
  // emits no s_waitcnt for it — measured: the word overtook the results)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) (expcnt / lgkmcnt untouched): this wave's stores have been acknowledged
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    const uint32_t before = atomicAdd(s_done, 1u);
    if (before + 1u == blockDim.x / WAVE) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // (the count seen: the other waves' acknowledgements are behind us)
      __hip_atomic_store(S.out_done, (unsigned long long)done_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}
// SA_OUT(ptr, val), for kernels with `done_seq` in scope (the tail's body, k_assign_small2) — a result on its way to the host's mapped
// block: with completion words as a SYSTEM-scope store — such a store is acknowledged when it has reached the host's memory, a plain
// one when the L2 has taken it (measured: behind plain stores the completion word overtook the results it announces, s_waitcnt vmcnt(0)
// or not); otherwise plain (the dispatch's own end-of-kernel release covers it)
#define SA_OUT(ptr, val)                                                                                             \
do {                                                                                                               \
  if (done_seq) __hip_atomic_store((ptr), (std::remove_cv_t<std::remove_reference_t<decltype(*(ptr))>>)(val), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); \
  else *(ptr) = (val);                                                                                             \
} while (0)
// TC: columns per thread — 1: T <= 1024; 2: T <= 2048 (a tracker loop's table once idle tracks linger: more tracks than detections is its
// normal state): every per-column array twice as long, the LDS edge pool given up for them (rows that lose their bid walk the HBM lists:
// rare in tracking frames); class words (SCN_WORDSK) with a register set per column — what keeps them out of k_assign_small2.
// LAZY: the frame's first phase computed no positional cells (SaParams::lazy_pos); this workgroup evaluates them itself, for the rows
// the visual vote leaves over only (see the lazy phase below).  Single vote words, IoU, TC = 1.
// FUSED: the body runs in the last-arriving block of the frame's ONE launch (k_frame_visual<.., HELP, TAIL>, sa_gemm.hip), behind the
// contraction's tiles of the same launch.  What those tiles wrote — the vote words, by 64-bit agent-scope atomic minima and nothing else —
// is fetched by 64-bit agent-scope atomic exchanges (the fetch and the re-arm in one operation, performed where the minima were: no fence
// on either side); everything else this instantiation loads was written before the launch.  The edge pool's gains live in `egain_ext`,
// the tile's LDS buffer, which is dead by then (POOL words of 8 bytes): the two kinds' LDS together stay under a CU's 160 KB.
//
// sa_tail_body.h is the kernel's statements, included INSIDE the kernel that runs them, with these names in scope:
//   VISUAL, WORDS, G, TC, LAZY, FUSED (constants), scenes, done_seq, p, egain_ext.
// Text, not a __device__ function: inlined from a function of its own the same statements are scheduled differently (a handful of
// instructions and the register numbering; measured on every form), and the stand-alone tails are to stay the kernels they were,
// instruction for instruction (scripts/kernel_identity.py).  Its `return`s leave the kernel: it is the last thing a kernel does.
