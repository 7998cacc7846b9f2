// sa_gemm.hip — the N x (T*K) feature-distance contraction of VisualSORT on gfx950.
//
// Reference: distance::cosine / distance::euclidean (src/distance.rs:9-47) evaluated for every
// (candidate, stored observation) pair by VisualMetric::visual_metric (visual_sort/metric.rs:200-225).
//
// cosine   : dot products on the f32 matrix cores — v_mfma_f32_32x32x2_f32, exact f32 (an fmaf chain),
//            157 TF/s peak; A = candidates [N][Dp], B = track bank [T*K][Dp], both k-contiguous, so the
//            contraction is C = A * B^T.  Block tile 128x128 (big frames) or 64x64 (small frames), 4 waves
//            as 2x2 per k-group, k staged 32 floats at a time through XOR-swizzled LDS, ds_read_b128
//            fragments (each lane takes 4 consecutive k of its row; the k-slot permutation is the same for A
//            and B, so the sum is unchanged).  Small frames cannot fill 256 CUs x 4 SIMDs with 32x32 wave
//            tiles, so the 64x64 kernel splits k across KG wave groups inside the block (each group owns its
//            LDS stage and accumulators; one LDS reduction at the end) — 2-4 waves per SIMD instead of 1.
//            The epilogue fuses everything the reference does per pair after the dot product:
//            d = dot / sqrt(n1*n2) with hoisted norms, is_ok threshold, distance_to_weight (1 - d), the
//            feature_can_be_used / minimal-track-length gates, compatible(), and the running maximum that
//            BestFitVoting needs (voting/best.rs:59-76).
// euclidean: sum (a-b)^2 directly on the VALU — the GEMM expansion |a|^2+|b|^2-2ab cancels catastrophically
//            on near-identical vectors, which are exactly the true matches (SURVEY §7 hard parts).
#include "sa_engine.h"
#include "sa_frame.h"
#include "sa_compat.h"
#include "sa_join_tiles.h"
#include "../../include/similari_f16.h"
#include "../../include/similari_i8.h"
#include <type_traits>
#ifdef SA_GEMM_TRACE   // (the tail behind a one-launch frame's tiles ends the block's timeline: stamp 5, in place of the tile's own exit)
#define TAIL_STAMP(k) do { if ((k) == 7 && g_trace_dev && threadIdx.x == 0) g_trace_dev[8 * blockIdx.x + 5] = __builtin_amdgcn_s_memtime(); } while (0)
#endif
#include "sa_tail.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
// Pointers that reach a kernel through the SceneDev descriptor are generic ("flat") to the compiler: their loads become
// flat_load, which counts on BOTH vmcnt and lgkmcnt — every s_waitcnt lgkmcnt for an LDS fragment then also drains the
// feature loads in flight and the software pipeline collapses (C2: 20 -> 41 us).  The feature operands are therefore
// re-typed as global-address-space pointers before the main loop.
#define SA_AS1 __attribute__((address_space(1)))
typedef const SA_AS1 float* gfloat_p;
typedef const SA_AS1 f32x4* gf32x4_p;

#define BK SA_BK

// In-kernel timeline (build with -DSA_GEMM_TRACE, run with SA_GEMM_TRACE=<launch #> to dump gpurun_out/gemm_trace.txt):
// s_memtime stamps per workgroup at  0 entry | 1 prologue done | 2 main loop done | 3 k-group reduction done |
// 4 epilogue stores issued | 5 exit.  Compiled out of the product.
#ifdef SA_GEMM_TRACE
#define SA_STAMP(tr, i) do { if ((tr) && threadIdx.x == 0) (tr)[i] = __builtin_amdgcn_s_memtime(); } while (0)
__device__ uint64_t* g_trace_dev;
#define SA_TRACE_PTR() (g_trace_dev ? g_trace_dev + 8 * (blockIdx.x + blockIdx.y * gridDim.x) : nullptr)
#else
#define SA_STAMP(tr, i) do { } while (0)
#define SA_TRACE_PTR() nullptr
#endif

static inline uint32_t cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// XCD-aware tile order.  Workgroups of a launch go round-robin over the 8 XCDs (workgroup b -> XCD b % 8), each with an L2 of its own:
// with tiles numbered row by row, every XCD's L2 ends up pulling the WHOLE candidate panel and its share of the track panel out of
// HBM (C2: 19.9 MB measured for 4.1 MB of operands).  Instead XCD x takes the x-th CONTIGUOUS chunk of a tile numbering that walks
// the grid in bands of W tile columns (row by row inside a band): its tiles form a compact block of about W x chunk / W tiles that
// shares W column panels and chunk / W row panels (C2, 16 x 16 tiles, chunk 32, W 4: 8 x 4 tiles = 1.5 MB per XCD instead of 2.25).
// MEASURED (round 4, SA_FLAG_XCD_TILES; profiles/r04_*): FETCH_SIZE of the C2 launch 19.1 -> 15.3 MB, the frame no faster (20.42 against
// 20.48 us; the launch itself 17.6 against 16.5 us between its own timestamps), c2b's stand-alone contraction 92.3 -> 91.0 us, C5's
// 634 -> 657 us (bands of 12 x 128 tracks x 16 KB overflow the 4 MB L2 that a row-by-row walk keeps one candidate panel in): the HBM
// traffic is not what bounds these launches (1.1 TB/s at C5).  Since round 4 the FUSED first phase numbers its contraction tiles this way
// by default (the same speed on every workload that takes it, a fifth fewer L2 fills; SA_FLAG_ROW_TILES: row by row); the stand-alone
// contraction stays row by row (SA_FLAG_XCD_TILES: this order there too).
// b in [0, 8 chunk) -> tile number t = (b % 8) chunk + b / 8 (t >= tiles: an idle workgroup); t -> (row, column).
struct XcdOrder { uint32_t chunk, W; };
static inline XcdOrder xcd_order(uint32_t gx, uint32_t gy, bool row_major = false) {
  XcdOrder o;
  const uint32_t tiles = gx * gy;
  if (row_major || tiles >= (1u << 24)) { o.chunk = tiles; o.W = 0; return o; }  // the default: W = 0 -> workgroup b is tile b, row by row
  o.chunk = (tiles + 7u) / 8u;
  uint32_t w = 1;
  while ((w + 1) * (w + 1) <= o.chunk) ++w;   // ~ sqrt(chunk): square-ish blocks
  o.W = w < gx ? w : gx;
  if (o.W == 0) o.W = 1;
  // (the kernels take the pair packed as chunk << 8 | W: any band width is a valid one — 255 at most; a grid beyond 2^24 chunks — half
  // a million tracks against as many detections — falls back to the row-by-row numbering, which the launchers handle with W = 0)
  if (o.W > 255u) o.W = 255u;
  if (o.chunk >= (1u << 24)) { o.chunk = tiles; o.W = 0; }
  return o;
}
__device__ __forceinline__ bool xcd_tile(uint32_t b, uint32_t gx, uint32_t gy, uint32_t chunk, uint32_t W, uint32_t* bx, uint32_t* by) {
  if (W == 0) {  // row-major numbering (chunk = tiles)
    if (b >= gx * gy) return false;
    *bx = b % gx; *by = b / gx;
    return true;
  }
  const uint32_t t = (b & 7u) * chunk + (b >> 3);
  if (t >= gx * gy || (b >> 3) >= chunk) return false;
  const uint32_t band = t / (W * gy), t2 = t - band * W * gy;
  const uint32_t wb = gx - band * W < W ? gx - band * W : W;
  *by = t2 / wb;
  *bx = band * W + t2 % wb;
  return true;
}

// Physical float offset of logical 16-byte chunk `kc` (0..7) of row `row` in a [rows][32] f32 LDS tile.
// XOR with (row>>1)&7: with a 128-B row stride, the 16 rows one ds_read_b128 lane group touches land on
// 16 distinct 16-B slots of the 256-B bank row (conflict-free); see MI355X_MICROARCH.md §LDS.
__device__ __forceinline__ uint32_t lds_off(uint32_t row, uint32_t kc) { return row * BK + ((kc ^ ((row >> 1) & 7u)) << 2); }

struct GemmCols {   // per-lane column metadata kept in registers through the epilogue
  float nb;         // squared norm of the stored feature
  bool ok;          // feature present, track long enough, epoch distance within max_idle_epochs
  float cmax;       // max_dist of the spatio-temporal constraint that applies to this column's epoch distance; < 0 = none
  sa_geo g;
};

// Dp is a multiple of 32, so a 32-float chunk is either entirely inside a row or absent; rows past the
// matrix edge are clamped to the last row (their results are never stored) — no branches around the loads.
//
// Pipeline per k-group (256 threads, 2 LDS stages of (BM+BN) x 32 floats), ONE barrier per 32-deep chunk.
// f32 MFMA is slow (64 cycles per 32x32x2 on a SIMD), so LDS and L2 bandwidth are never the limit; what costs is every
// cycle a wave spends issuing something else while its matrix pipe is free.  Iteration c is therefore laid out as four
// k-steps (8 floats of k each), each one a straight run of 4*TM*TN MFMAs with the other work of the iteration placed
// in their shadow (an MFMA takes 4 cycles to issue and 64 to execute; the wave keeps issuing meanwhile):
//     k-step kk:  MFMAs on fragment buffer kk&1
//                 | ds_read the fragments of k-step kk+1 into the other fragment buffer
//                 | a quarter of: ds_write chunk c+1 (already in registers) to the other LDS stage, then re-issue those
//                   registers' global loads for chunk c+2
// Only the fragment read of k-step 0 (right after the barrier) is exposed; the co-resident workgroup covers it.
// The body is branch-free (three specialisations: steady state / last-but-one chunk / last chunk) so that the whole
// iteration is ONE scheduling region, pinned with sched_group_barrier; measured against the same loop with the loads and
// stores hoisted to the top of the iteration (what the compiler does on its own): 110 -> see profiles/.
// NORM: also accumulate, per lane, the sum of squares of the A fragments it multiplies (its half of the k values of row
// wm*32 + lr, this k-group's chunks) into nsq[0] — the raw-feature mode of the fused frame launch has no pre-computed norms.
template <int BM, int BN, int KG, bool NORM = false>
__device__ __forceinline__ void gemm_mainloop(gfloat_p A, gfloat_p B, uint32_t M,
                                              uint32_t Ncols, uint32_t Dp, uint32_t m0, uint32_t n0, float* lds,
                                              f32x16 (&acc)[BM / 64][BN / 64], uint64_t* tr = nullptr, float* nsq = nullptr) {
  constexpr int TM = BM / 64, TN = BN / 64;
  constexpr int A_CH = BM * 8 / 256, B_CH = BN * 8 / 256;  // 16-B chunks per thread per stage
  constexpr int L_CH = A_CH + B_CH;                          // 4 (64x64) .. 8 (128x128): a multiple of 4 or exactly 6
  constexpr int STAGE = (BM + BN) * BK;                     // floats per LDS stage
  const uint32_t tid = threadIdx.x;
  // k-group of this wave (0 when KG == 1).  readfirstlane: the value is wave-uniform, and telling the compiler so keeps
  // every branch of the main loop scalar — with a divergent-looking branch it parks the 16-64 accumulator registers
  // in VGPRs and copies them to and from the matrix-core register file on EVERY chunk (128 v_accvgpr moves + a
  // pipeline drain per 64 MFMAs in the 128x128 kernel).
  const uint32_t kg = KG == 1 ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 8));
  const uint32_t ltid = tid & 255u, lane = tid & 63u, w4 = (tid >> 6) & 3u;
  float* base = lds + kg * 2 * STAGE;
  const uint32_t wm = w4 >> 1, wn = w4 & 1u;
  const uint32_t lr = lane & 31u, lh = lane >> 5;
  const uint32_t nchunks = Dp / BK;
  const uint32_t niter = (nchunks + KG - 1) / KG;
  // entries 0..A_CH-1 belong to A, the rest to B
  uint32_t goff[L_CH], soff[L_CH];
#pragma unroll
  for (int r = 0; r < L_CH; ++r) {
    const bool isA = r < A_CH;
    uint32_t c = ltid + 256u * (isA ? r : r - A_CH), row = c >> 3, kc = c & 7u;
    uint32_t gr = (isA ? m0 : n0) + row;
    const uint32_t lim = isA ? M : Ncols;
    gr = gr < lim ? gr : lim - 1;
    goff[r] = gr * Dp + kc * 4u;
    soff[r] = (isA ? 0 : BM * BK) + lds_off(row, kc);
  }
  // Two register sets: the rows of chunk i+1 are written to LDS from set (i+1)&1, which is then reloaded with chunk i+3 —
  // whatever place inside the iteration the scheduler gives a load, it has at least one whole iteration to land (with
  // one set, loads that sink to the end of an iteration are consumed 5 MFMAs later: a full L2 round trip exposed per
  // chunk, 28 us instead of 15 at C2).
  f32x4 rg[2][L_CH];
  auto gload_set = [&](int set, uint32_t k0) {
#pragma unroll
    for (int r = 0; r < L_CH; ++r) rg[set][r] = *(gf32x4_p)((r < A_CH ? A : B) + (size_t)(goff[r] + k0));
  };
#pragma unroll
  for (int m = 0; m < TM; ++m)
#pragma unroll
    for (int n = 0; n < TN; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;

  uint32_t aoff[TM], boff[TN];
#pragma unroll
  for (int m = 0; m < TM; ++m) aoff[m] = wm * (BM / 2) + m * 32 + lr;
#pragma unroll
  for (int n = 0; n < TN; ++n) boff[n] = wn * (BN / 2) + n * 32 + lr;

  // chunks of this group: local index i <-> chunk i*KG + kg, i < mine
  const uint32_t mine = kg < nchunks ? (nchunks - kg + KG - 1) / KG : 0u;
  if (mine > 0) {
    gload_set(0, kg * BK);
#pragma unroll
    for (int r = 0; r < L_CH; ++r) *(f32x4*)(base + soff[r]) = rg[0][r];
  }
  if (mine > 1) gload_set(1, (kg + KG) * BK);
  if (mine > 2) gload_set(0, (kg + 2 * KG) * BK);
  __syncthreads();
  SA_STAMP(tr, 1);

  // One iteration.  SET = (i+1)&1; STORE: chunk i+1 exists (set -> other LDS stage); LOAD: chunk i+3 exists (global -> set).
  // The iteration's ONE barrier sits between its third and fourth k-step: the rows of chunk i+1 go to the other LDS stage during
  // k-steps 0-2 (which also fetch the fragments of k-steps 1-3 from this stage), every wave then meets at the barrier with the
  // MFMAs of k-step 2 still queued on its matrix pipe, and k-step 3 — running on fragments already in registers — fetches the
  // FIRST fragments of chunk i+1 from the stage that has just become visible.  With the barrier at the end of the iteration
  // that first fetch came after it, its LDS latency exposed on an idle pipe once per chunk (one wave per SIMD: 1560 cycles per
  // chunk for 1024 of MFMA work).
  f32x4 fa[2][TM], fb[2][TN];
  if (mine > 0) {
#pragma unroll
    for (int m = 0; m < TM; ++m) fa[0][m] = *(const f32x4*)(base + lds_off(aoff[m], lh));
#pragma unroll
    for (int n = 0; n < TN; ++n) fb[0][n] = *(const f32x4*)(base + BM * BK + lds_off(boff[n], lh));
  }
  auto body = [&](uint32_t it, auto set_tag, auto store_tag, auto load_tag) {
    constexpr int SET = decltype(set_tag)::value;
    constexpr bool STORE = decltype(store_tag)::value, LOAD = decltype(load_tag)::value;
    const float* As = base + (it & 1u) * STAGE;
    const float* Bs = As + BM * BK;
    float* nxt = base + ((it + 1u) & 1u) * STAGE;
    const uint32_t k3 = ((it + 3u) * KG + kg) * BK;
    auto kstep = [&](auto kk_tag) {
      constexpr int kk = decltype(kk_tag)::value;
      constexpr int cur = kk & 1, nx = cur ^ 1;
      if constexpr (kk < 3) {
#pragma unroll
        for (int m = 0; m < TM; ++m) fa[nx][m] = *(const f32x4*)(As + lds_off(aoff[m], (kk + 1) * 2 + lh));
#pragma unroll
        for (int n = 0; n < TN; ++n) fb[nx][n] = *(const f32x4*)(Bs + lds_off(boff[n], (kk + 1) * 2 + lh));
      } else if constexpr (STORE) {
#pragma unroll
        for (int m = 0; m < TM; ++m) fa[nx][m] = *(const f32x4*)(nxt + lds_off(aoff[m], lh));
#pragma unroll
        for (int n = 0; n < TN; ++n) fb[nx][n] = *(const f32x4*)(nxt + BM * BK + lds_off(boff[n], lh));
      }
      // this k-step's share of the register -> LDS -> register hand-over of the staged rows: the LDS stores in k-steps 0-2
      // (they must be visible at the barrier), each register's reload from global memory right after its store
      constexpr int lo_of[5] = {0, (L_CH + 2) / 3, (2 * L_CH + 2) / 3, L_CH, L_CH};
      constexpr int lo = lo_of[kk], hi = lo_of[kk + 1];
#pragma unroll
      for (int r = lo; r < hi; ++r) {
        if constexpr (STORE) *(f32x4*)(nxt + soff[r]) = rg[SET][r];
        if constexpr (LOAD) rg[SET][r] = *(gf32x4_p)((r < A_CH ? A : B) + (size_t)(goff[r] + k3));
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
          for (int n = 0; n < TN; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur][m][e], fb[cur][n][e], acc[m][n], 0, 0, 0);
      if constexpr (NORM) {
#pragma unroll
        for (int e = 0; e < 4; ++e) nsq[0] += fa[cur][0][e] * fa[cur][0][e];
      }
      // pin the interleave: one side instruction in the shadow of each of the first MFMAs of the k-step
      constexpr int NM = 4 * TM * TN;
      constexpr int nrd = (kk < 3 || STORE) ? TM + TN : 0, nst = STORE ? hi - lo : 0, nld = LOAD ? hi - lo : 0;
      constexpr int used = nrd + nst + nld;
#pragma unroll
      for (int i = 0; i < nrd; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); }
#pragma unroll
      for (int i = 0; i < (nst > nld ? nst : nld); ++i) {
        if (i < nst) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x200, 1, 0); }
        if (i < nld) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); }
      }
      if constexpr (used < NM) __builtin_amdgcn_sched_group_barrier(0x008, NM - used, 0);
    };
    kstep(std::integral_constant<int, 0>{});
    kstep(std::integral_constant<int, 1>{});
    kstep(std::integral_constant<int, 2>{});
    __syncthreads();
    kstep(std::integral_constant<int, 3>{});
  };
  using T_ = std::true_type;
  using F_ = std::false_type;
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  uint32_t it = 0;
  // steady state two iterations per trip, so that the register set is a compile-time constant (set of iteration i = (i+1)&1)
  for (; it + 4 < mine; it += 2) {
    body(it, S1{}, T_{}, T_{});
    body(it + 1, S0{}, T_{}, T_{});
  }
  for (; it < mine; ++it) {  // at most 4 iterations left; `it` is even on entry
    const bool st = it + 1 < mine, ld = it + 3 < mine;
    if (it & 1u) {
      if (ld) body(it, S0{}, T_{}, T_{});
      else if (st) body(it, S0{}, T_{}, F_{});
      else body(it, S0{}, F_{}, F_{});
    } else {
      if (ld) body(it, S1{}, T_{}, T_{});
      else if (st) body(it, S1{}, T_{}, F_{});
      else body(it, S1{}, F_{}, F_{});
    }
  }
  for (; it < niter; ++it) __syncthreads();  // a group that ran out of chunks still meets the others at the barrier
  SA_STAMP(tr, 2);
}

// Ring variant (KG == 0 in the kernel templates): ONE wave per SIMD, a 3-stage LDS ring, nothing left for a partner wave
// to cover.  Used where a frame yields about one workgroup per CU (C2: 16 x 16 tiles of 64x64 on 256 CUs), so that the
// k-group trick above would put the two waves of a SIMD behind the SAME barrier — they then stall together (measured:
// 2583 cycles per iteration against 2048 of MFMA work).  Here a wave's own instruction stream keeps its matrix pipe fed:
//     iteration c:  MFMAs of chunk c from stage c%3, fragments double-buffered in registers
//                   | ds_write chunk c+2 (registers, loaded two iterations ago) -> stage (c+2)%3
//                   | re-issue those registers' global loads for chunk c+4
//                   | during the LAST k-step: ds_read the first fragments of chunk c+1 (stage (c+1)%3, complete since the
//                     previous barrier) — so nothing but the barrier itself sits between two chunks' MFMAs.
// Hazards: stage (c+2)%3 was last read in iteration c-1, and every wave has passed that iteration's barrier.
template <int BM, int BN>
__device__ __forceinline__ void gemm_mainloop_ring(gfloat_p A, gfloat_p B, uint32_t M,
                                                   uint32_t Ncols, uint32_t Dp, uint32_t m0, uint32_t n0, float* lds,
                                                   f32x16 (&acc)[BM / 64][BN / 64], uint64_t* tr = nullptr) {
  constexpr int TM = BM / 64, TN = BN / 64;
  constexpr int A_CH = BM * 8 / 256, B_CH = BN * 8 / 256, L_CH = A_CH + B_CH;
  constexpr int STAGE = (BM + BN) * BK;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w4 = tid >> 6;
  const uint32_t wm = w4 >> 1, wn = w4 & 1u, lr = lane & 31u, lh = lane >> 5;
  const uint32_t nchunks = Dp / BK;
  uint32_t goff[L_CH], soff[L_CH];
#pragma unroll
  for (int r = 0; r < L_CH; ++r) {
    const bool isA = r < A_CH;
    uint32_t c = tid + 256u * (isA ? r : r - A_CH), row = c >> 3, kc = c & 7u;
    uint32_t gr = (isA ? m0 : n0) + row;
    const uint32_t lim = isA ? M : Ncols;
    gr = gr < lim ? gr : lim - 1;
    goff[r] = gr * Dp + kc * 4u;
    soff[r] = (isA ? 0 : BM * BK) + lds_off(row, kc);
  }
  f32x4 rg[2][L_CH];
#pragma unroll
  for (int m = 0; m < TM; ++m)
#pragma unroll
    for (int n = 0; n < TN; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;
  uint32_t aoff[TM], boff[TN];
#pragma unroll
  for (int m = 0; m < TM; ++m) aoff[m] = wm * (BM / 2) + m * 32 + lr;
#pragma unroll
  for (int n = 0; n < TN; ++n) boff[n] = wn * (BN / 2) + n * 32 + lr;

  // prologue: chunks 0 and 1 -> stages 0 and 1; chunks 2 and 3 -> register sets 0 and 1
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if ((uint32_t)c < nchunks) {
#pragma unroll
      for (int r = 0; r < L_CH; ++r) rg[c & 1][r] = *(gf32x4_p)((r < A_CH ? A : B) + (size_t)(goff[r] + c * BK));
      if (c < 2) {
#pragma unroll
        for (int r = 0; r < L_CH; ++r) *(f32x4*)(lds + c * STAGE + soff[r]) = rg[c & 1][r];
      }
    }
  __syncthreads();
  SA_STAMP(tr, 1);
  f32x4 fa[2][TM], fb[2][TN];
#pragma unroll
  for (int m = 0; m < TM; ++m) fa[0][m] = *(const f32x4*)(lds + lds_off(aoff[m], lh));
#pragma unroll
  for (int n = 0; n < TN; ++n) fb[0][n] = *(const f32x4*)(lds + BM * BK + lds_off(boff[n], lh));

  // PAR: parity of the iteration (selects the register set); STORE: chunk c+2 exists; LOAD: chunk c+4 exists;
  // NEXT: chunk c+1 exists (prefetch its first fragments)
  auto body = [&](uint32_t c, uint32_t st, auto par_tag, auto store_tag, auto load_tag, auto next_tag) {
    constexpr int PAR = decltype(par_tag)::value;
    constexpr bool STORE = decltype(store_tag)::value, LOAD = decltype(load_tag)::value, NEXT = decltype(next_tag)::value;
    const uint32_t st1 = st == 2 ? 0u : st + 1u, st2 = st == 0 ? 2u : st - 1u;  // (c+1)%3, (c+2)%3
    const float* As = lds + st * STAGE;
    const float* Bs = As + BM * BK;
    const float* An = lds + st1 * STAGE;
    const float* Bn = An + BM * BK;
    float* wr = lds + st2 * STAGE;
    const uint32_t k4 = (c + 4u) * BK;
    auto kstep = [&](auto kk_tag) {
      constexpr int kk = decltype(kk_tag)::value;
      constexpr int cur = kk & 1, nx = cur ^ 1;
      if constexpr (kk < 3) {
#pragma unroll
        for (int m = 0; m < TM; ++m) fa[nx][m] = *(const f32x4*)(As + lds_off(aoff[m], (kk + 1) * 2 + lh));
#pragma unroll
        for (int n = 0; n < TN; ++n) fb[nx][n] = *(const f32x4*)(Bs + lds_off(boff[n], (kk + 1) * 2 + lh));
      } else if constexpr (NEXT) {
#pragma unroll
        for (int m = 0; m < TM; ++m) fa[nx][m] = *(const f32x4*)(An + lds_off(aoff[m], lh));
#pragma unroll
        for (int n = 0; n < TN; ++n) fb[nx][n] = *(const f32x4*)(Bn + lds_off(boff[n], lh));
      }
      constexpr int lo_of[5] = {0, (L_CH + 3) / 4, (L_CH + 1) / 2, (3 * L_CH + 3) / 4, L_CH};
      constexpr int lo = lo_of[kk], hi = lo_of[kk + 1];
#pragma unroll
      for (int r = lo; r < hi; ++r) {
        if constexpr (STORE) *(f32x4*)(wr + soff[r]) = rg[PAR][r];
        if constexpr (LOAD) rg[PAR][r] = *(gf32x4_p)((r < A_CH ? A : B) + (size_t)(goff[r] + k4));
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
          for (int n = 0; n < TN; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur][m][e], fb[cur][n][e], acc[m][n], 0, 0, 0);
      constexpr int NM = 4 * TM * TN;
      constexpr int nrd = (kk < 3 || NEXT) ? TM + TN : 0, nst = STORE ? hi - lo : 0, nld = LOAD ? hi - lo : 0;
      constexpr int used = nrd + nst + nld;
#pragma unroll
      for (int i = 0; i < nrd; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); }
#pragma unroll
      for (int i = 0; i < (nst > nld ? nst : nld); ++i) {
        if (i < nst) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x200, 1, 0); }
        if (i < nld) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); }
      }
      if constexpr (used < NM) __builtin_amdgcn_sched_group_barrier(0x008, NM - used, 0);
    };
    kstep(std::integral_constant<int, 0>{});
    kstep(std::integral_constant<int, 1>{});
    kstep(std::integral_constant<int, 2>{});
    kstep(std::integral_constant<int, 3>{});
  };
  using T_ = std::true_type;
  using F_ = std::false_type;
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
  uint32_t c = 0, st = 0;
  auto adv = [&]() { ++c; st = st == 2 ? 0u : st + 1u; __syncthreads(); };
  // steady state, two iterations per trip so that the register-set parity is static
  while (c + 5 < nchunks) { body(c, st, P0{}, T_{}, T_{}, T_{}); adv(); body(c, st, P1{}, T_{}, T_{}, T_{}); adv(); }
  // c is even here.  Remaining chunks: at most 5.
  if (c + 4 < nchunks) { body(c, st, P0{}, T_{}, T_{}, T_{}); adv(); }          // c+4 exists
  // from here no more loads; parity alternates from (c & 1)
  while (c < nchunks) {
    const bool store = c + 2 < nchunks, next = c + 1 < nchunks;
    if (c & 1u) {
      if (store) body(c, st, P1{}, T_{}, F_{}, T_{});
      else if (next) body(c, st, P1{}, F_{}, F_{}, T_{});
      else body(c, st, P1{}, F_{}, F_{}, F_{});
    } else {
      if (store) body(c, st, P0{}, T_{}, F_{}, T_{});
      else if (next) body(c, st, P0{}, F_{}, F_{}, T_{});
      else body(c, st, P0{}, F_{}, F_{}, F_{});
    }
    adv();
  }
  SA_STAMP(tr, 2);
}

// (fragment order: sa_engine.h, sa_frag_index)
__global__ void k_frag_reorder(const float* __restrict__ src, uint32_t rows, uint32_t Dp, float* __restrict__ dst) {
  // one thread per 16-byte piece of the destination; rows past the end repeat the last row (never stored by the consumers)
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)((rows + 31u) / 32u * 32u) * Dp / 4u;
  if (i >= total) return;
  const uint32_t lane = (uint32_t)(i & 63u);
  const size_t blk = i >> 6;
  const uint32_t kb = (uint32_t)(blk % (Dp >> 3)), rb = (uint32_t)(blk / (Dp >> 3));
  uint32_t r = rb * 32u + (lane & 31u);
  r = r < rows ? r : rows - 1;
  ((f32x4*)dst)[i] = *(const f32x4*)(src + (size_t)r * Dp + kb * 8u + (lane >> 5) * 4u);
}
hipError_t sa_launch_frag_reorder(const float* src, uint32_t rows, uint32_t dp, float* dst, hipStream_t st) {
  const size_t total = (size_t)((rows + 31u) / 32u * 32u) * dp / 4u;
  hipLaunchKernelGGL(k_frag_reorder, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, src, rows, dp, dst);
  return hipGetLastError();
}

template <int I, int N, typename F>
__device__ __forceinline__ void sa_static_for(F&& f) {
  if constexpr (I < N) { f(std::integral_constant<int, I>{}); sa_static_for<I + 1, N>(f); }
}

// k-split main loop of the 64 x 64 tile (KS): NO LDS stage and NO barrier between the first load and the last matrix instruction.
// A lone wave per SIMD pays ~25 matrix-pipe cycles for every LDS or memory instruction it issues (scripts/micro/mfma_side_mix.hip);
// the staged loop above issues 16 of them per 16 matrix instructions (8 ds_read_b128, 4 ds_write_b128, 4 global loads).  Here wave
// (wm, kg) owns tile rows wm 32 .. +31, ALL 64 tile columns, and every second 8-deep k-step (kg = its parity): a 32 x 64 wave tile of
// two independent accumulators whose operands come straight from memory into registers — per k-step one dwordx4 of A (its 32 rows,
// row-major: 32 B out of 32 lines) and two of B (row-major likewise, or BFRAG: the fragment-order copy of the bank, one contiguous
// kilobyte each) for 8 matrix instructions: 6 side instructions per 16 instead of 16.  NBUF register buffers: the loads of step
// j + NBUF - 1 are issued under the matrix instructions of step j.  The two k-halves of a 32 x 32 quadrant meet through LDS once, at
// the end (each wave ships the quadrant it does not keep: 4 KB): wave (wm, x) leaves with rows wm 32.., columns x 32.. in the
// standard 32 x 32 accumulator layout — what the epilogues of this file expect from wave (wm, wn = x).
// NORM: *nsq = the squared norm of row wm 32 + lr of A (both lane halves, both k-halves), complete.
template <int NBUF, bool NORM, bool BFRAG, bool AFRAG = false>
__device__ __forceinline__ void gemm_mainloop_ks(gfloat_p A, gfloat_p B, uint32_t M, uint32_t Ncols, uint32_t Dp, uint32_t m0,
                                                 uint32_t n0, float* lds, f32x16& out, uint64_t* tr = nullptr, float* nsq = nullptr,
                                                 uint32_t yield_every = 0) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t w4 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)) & 3u;
  const uint32_t wm = w4 >> 1, kg = w4 & 1u, lr = lane & 31u, lh = lane >> 5;
  // Buffer loads: a resource descriptor per operand (base = the tile's first row, range = what is left of the matrix behind it), a
  // 32-bit byte offset per lane (constant), and the position along k in the instruction's SCALAR offset — no vector arithmetic and no
  // 64-bit address in the loop, and rows past the matrix edge need no clamp: they are out of range and read as zero.
  const uint32_t Mp = AFRAG ? (M + 31u) / 32u * 32u : M, Np = BFRAG ? (Ncols + 31u) / 32u * 32u : Ncols;
  const uint32_t nb0 = BFRAG ? (n0 & ~31u) : n0;
  auto left = [&](uint32_t rows) { const uint64_t b = (uint64_t)rows * Dp * 4u; return (uint32_t)(b < 0xffffffffull ? b : 0xffffffffull); };
  const __amdgpu_buffer_rsrc_t RA = __builtin_amdgcn_make_buffer_rsrc((void*)(A + (size_t)m0 * Dp), 0, (int)left(Mp - m0), 0x00020000);
  const __amdgpu_buffer_rsrc_t RB = __builtin_amdgcn_make_buffer_rsrc((void*)(B + (size_t)nb0 * Dp), 0, (int)left(Np - nb0), 0x00020000);
  const uint32_t oa = AFRAG ? (wm * 32u * Dp + lane * 4u) * 4u : ((wm * 32u + lr) * Dp + lh * 4u) * 4u;  // (m0 is a multiple of 64)
  uint32_t ob[2];
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    // (fragment order: the tile's first column need not start a block of 32 rows — the whole-track tiles of deeper banks start anywhere;
    // a wave-load then covers two runs of a kilobyte instead of one)
    const uint32_t rr = (n0 - nb0) + n * 32u + lr;
    ob[n] = BFRAG ? ((rr >> 5) * (Dp >> 3) * 256u + lh * 128u + (rr & 31u) * 4u) * 4u : ((n * 32u + lr) * Dp + lh * 4u) * 4u;
  }
  const uint32_t mine = Dp >> 4;  // k-steps of this wave: global step s = 2 j + kg (Dp is a multiple of 32)
  f32x16 acc0, acc1;
#pragma unroll
  for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; }
  f32x4 fa[NBUF], fb[NBUF][2];
  float ns = 0.f;
  auto load = [&](auto buf_tag, uint32_t j) {  // (a step past the end reads the next rows' bytes or zeros: never multiplied)
    constexpr int buf = decltype(buf_tag)::value;
    const uint32_t s = 2u * j + kg;
    fa[buf] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(RA, (int)oa, (int)(s * (AFRAG ? 1024u : 32u)), 0));
#pragma unroll
    for (int n = 0; n < 2; ++n)
      fb[buf][n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(RB, (int)ob[n], (int)(s * (BFRAG ? 1024u : 32u)), 0));
  };
  auto compute = [&](auto buf_tag) {
    constexpr int buf = decltype(buf_tag)::value;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[buf][e], fb[buf][0][e], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[buf][e], fb[buf][1][e], acc1, 0, 0, 0);
    }
    if constexpr (NORM) {
#pragma unroll
      for (int e = 0; e < 4; ++e) ns += fa[buf][e] * fa[buf][e];
    }
  };
  auto step = [&](auto b_tag, uint32_t j) {  // step j on buffer b; the loads of step j + NBUF - 1 go to the buffer step j - 1 has just left
    constexpr int b = decltype(b_tag)::value;
    load(std::integral_constant<int, (b + NBUF - 1) % NBUF>{}, j + NBUF - 1);
    compute(b_tag);
    // three loads spread over the step: a matrix instruction has to be presented well before the pipe is free for it, so only a few
    // cycles of other instructions fit between two of them for nothing
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
    // (the fused launch: the waves of the positional tiles on this SIMD issue nothing while this wave presents matrix instructions)
    if (yield_every && (j % yield_every) == 0) __builtin_amdgcn_s_sleep(1);
  };
  // prologue: steps 0 .. NBUF-2 in flight
  // (in STEP order, pinned: the wait in front of a step's first matrix instruction counts the loads issued after that step's own, and
  // the loop header's count is the smaller of the two ways in — a prologue that issues buffer 0 last would drain every trip)
  sa_static_for<0, NBUF - 1>([&](auto b) { load(b, (uint32_t)decltype(b)::value); __builtin_amdgcn_sched_barrier(0); });
  SA_STAMP(tr, 1);
  uint32_t j = 0;
  for (; j + NBUF <= mine; j += NBUF) sa_static_for<0, NBUF>([&](auto b) { step(b, j + decltype(b)::value); });
  const uint32_t rem = mine - j;
  sa_static_for<0, NBUF>([&](auto b) { if ((uint32_t)decltype(b)::value < rem) step(b, j + decltype(b)::value); });
  SA_STAMP(tr, 2);
  // the two k-halves of every quadrant meet: wave (wm, x) keeps columns x 32 .. and ships the other accumulator to wave (wm, 1 - x)
  f32x4* red = (f32x4*)lds;                 // [4 waves][4][64 lanes] f32x4 = 16 KB
  float* rn = lds + 4 * 4 * 64 * 4;         // [4 waves][32] squared-norm halves
  if (kg == 0) {
#pragma unroll
    for (int g = 0; g < 4; ++g) red[(w4 * 4 + g) * 64 + lane] = f32x4{acc1[4 * g], acc1[4 * g + 1], acc1[4 * g + 2], acc1[4 * g + 3]};
  } else {
#pragma unroll
    for (int g = 0; g < 4; ++g) red[(w4 * 4 + g) * 64 + lane] = f32x4{acc0[4 * g], acc0[4 * g + 1], acc0[4 * g + 2], acc0[4 * g + 3]};
  }
  if constexpr (NORM) {
    ns += __shfl_xor(ns, 32);
    if (lh == 0) rn[w4 * 32 + lr] = ns;
  }
  __syncthreads();
  const uint32_t pw = w4 ^ 1u;
  // (a + b is the same f32 whichever wave adds: both orders give the k-half 0 + k-half 1 sum)
  if (kg == 0) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 o = red[(pw * 4 + g) * 64 + lane];
#pragma unroll
      for (int c = 0; c < 4; ++c) out[4 * g + c] = acc0[4 * g + c] + o[c];
    }
  } else {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 o = red[(pw * 4 + g) * 64 + lane];
#pragma unroll
      for (int c = 0; c < 4; ++c) out[4 * g + c] = o[c] + acc1[4 * g + c];
    }
  }
  if constexpr (NORM) *nsq = rn[(wm * 2) * 32 + lr] + rn[(wm * 2 + 1) * 32 + lr];
  __syncthreads();  // the epilogue reuses this LDS
}

// The k-split loop for a 64 x 96 tile (the fused first phase of frames whose 64 x 64 tiles would be one and a half rounds of the chip:
// sa_launch_frame_visual): wave (wm, kg) owns tile rows wm 32 .. +31, ALL 96 columns (three accumulators) and every second 8-deep k-step —
// one gather of A and three fragment-order loads of B per 12 matrix instructions.  Wave (wm, x) leaves with columns x 32 .. +31 in the
// standard 32 x 32 accumulator (`out`: what wave (wm, wn = x) of a 64 x 64 tile holds) and with HALF of the third column block: accumulator
// registers 8 x .. 8 x + 7 of columns 64 .. 95 (`out2`; register r <-> tile row wm 32 + acc_row(r, lane half)).  Every cell is
// (k-half 0) + (k-half 1), each half accumulated over the same k-steps in the same order as gemm_mainloop_ks: the 64 x 64 tiling's bits.
// LDS: [4 waves][6][64] f32x4 of exchange (24 KB) + [4][32] squared-norm halves.
constexpr uint32_t SA_KS96_RED = 4u * 6u * 64u * 4u;
constexpr uint32_t SA_KS96_LDS = SA_KS96_RED + 4u * 32u;
template <int NBUF, bool NORM>
__device__ __forceinline__ void gemm_mainloop_ks96(gfloat_p A, gfloat_p B, uint32_t M, uint32_t Ncols, uint32_t Dp, uint32_t m0, uint32_t n0,
                                                   float* lds, f32x16& out, float (&out2)[8], uint64_t* tr = nullptr, float* nsq = nullptr,
                                                   uint32_t yield_every = 0) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t w4 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)) & 3u;
  const uint32_t wm = w4 >> 1, kg = w4 & 1u, lr = lane & 31u, lh = lane >> 5;
  const uint32_t Np = (Ncols + 31u) / 32u * 32u;   // (n0 is a multiple of 96: it starts a block of 32 rows of the twin)
  auto left = [&](uint32_t rows) { const uint64_t b = (uint64_t)rows * Dp * 4u; return (uint32_t)(b < 0xffffffffull ? b : 0xffffffffull); };
  const __amdgpu_buffer_rsrc_t RA = __builtin_amdgcn_make_buffer_rsrc((void*)(A + (size_t)m0 * Dp), 0, (int)left(M - m0), 0x00020000);
  const __amdgpu_buffer_rsrc_t RB = __builtin_amdgcn_make_buffer_rsrc((void*)(B + (size_t)n0 * Dp), 0, (int)left(Np - n0), 0x00020000);
  const uint32_t oa = ((wm * 32u + lr) * Dp + lh * 4u) * 4u;
  uint32_t ob[3];
#pragma unroll
  for (int n = 0; n < 3; ++n) ob[n] = ((uint32_t)n * (Dp >> 3) * 256u + lh * 128u + lr * 4u) * 4u;
  const uint32_t mine = Dp >> 4;
  f32x16 acc0, acc1, acc2;
#pragma unroll
  for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; acc2[e] = 0.f; }
  f32x4 fa[NBUF], fb[NBUF][3];
  float ns = 0.f;
  auto load = [&](auto buf_tag, uint32_t j) {
    constexpr int buf = decltype(buf_tag)::value;
    const uint32_t s = 2u * j + kg;
    fa[buf] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(RA, (int)oa, (int)(s * 32u), 0));
#pragma unroll
    for (int n = 0; n < 3; ++n) fb[buf][n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(RB, (int)ob[n], (int)(s * 1024u), 0));
  };
  auto compute = [&](auto buf_tag) {
    constexpr int buf = decltype(buf_tag)::value;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[buf][e], fb[buf][0][e], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[buf][e], fb[buf][1][e], acc1, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[buf][e], fb[buf][2][e], acc2, 0, 0, 0);
    }
    if constexpr (NORM) {
#pragma unroll
      for (int e = 0; e < 4; ++e) ns += fa[buf][e] * fa[buf][e];
    }
  };
  auto step = [&](auto b_tag, uint32_t j) {
    constexpr int b = decltype(b_tag)::value;
    load(std::integral_constant<int, (b + NBUF - 1) % NBUF>{}, j + NBUF - 1);
    compute(b_tag);
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 3, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 3, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 3, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
    if (yield_every) {
      const uint32_t ev = yield_every & 255u, amt = yield_every >> 8;
      if ((j % ev) == 0) { if (amt <= 1) __builtin_amdgcn_s_sleep(1); else if (amt == 2) __builtin_amdgcn_s_sleep(2); else if (amt == 3) __builtin_amdgcn_s_sleep(3); else __builtin_amdgcn_s_sleep(4); }   // (yield_every: period | naps of 64 cycles << 8)
    }
  };
  sa_static_for<0, NBUF - 1>([&](auto b) { load(b, (uint32_t)decltype(b)::value); __builtin_amdgcn_sched_barrier(0); });
  SA_STAMP(tr, 1);
  uint32_t j = 0;
  for (; j + NBUF <= mine; j += NBUF) sa_static_for<0, NBUF>([&](auto b) { step(b, j + decltype(b)::value); });
  const uint32_t rem = mine - j;
  sa_static_for<0, NBUF>([&](auto b) { if ((uint32_t)decltype(b)::value < rem) step(b, j + decltype(b)::value); });
  SA_STAMP(tr, 2);
  f32x4* red = (f32x4*)lds;           // [4 waves][6][64 lanes]
  float* rn = lds + SA_KS96_RED;      // [4 waves][32]
  if (kg == 0) {
#pragma unroll
    for (int g = 0; g < 4; ++g) red[(w4 * 6 + g) * 64 + lane] = f32x4{acc1[4 * g], acc1[4 * g + 1], acc1[4 * g + 2], acc1[4 * g + 3]};
#pragma unroll
    for (int g = 0; g < 2; ++g) red[(w4 * 6 + 4 + g) * 64 + lane] = f32x4{acc2[8 + 4 * g], acc2[9 + 4 * g], acc2[10 + 4 * g], acc2[11 + 4 * g]};
  } else {
#pragma unroll
    for (int g = 0; g < 4; ++g) red[(w4 * 6 + g) * 64 + lane] = f32x4{acc0[4 * g], acc0[4 * g + 1], acc0[4 * g + 2], acc0[4 * g + 3]};
#pragma unroll
    for (int g = 0; g < 2; ++g) red[(w4 * 6 + 4 + g) * 64 + lane] = f32x4{acc2[4 * g], acc2[4 * g + 1], acc2[4 * g + 2], acc2[4 * g + 3]};
  }
  if constexpr (NORM) {
    ns += __shfl_xor(ns, 32);
    if (lh == 0) rn[w4 * 32 + lr] = ns;
  }
  __syncthreads();
  const uint32_t pw = w4 ^ 1u;
  if (kg == 0) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 o = red[(pw * 6 + g) * 64 + lane];
#pragma unroll
      for (int c = 0; c < 4; ++c) out[4 * g + c] = acc0[4 * g + c] + o[c];
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const f32x4 o = red[(pw * 6 + 4 + g) * 64 + lane];
#pragma unroll
      for (int c = 0; c < 4; ++c) out2[4 * g + c] = acc2[4 * g + c] + o[c];
    }
  } else {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 o = red[(pw * 6 + g) * 64 + lane];
#pragma unroll
      for (int c = 0; c < 4; ++c) out[4 * g + c] = o[c] + acc1[4 * g + c];
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const f32x4 o = red[(pw * 6 + 4 + g) * 64 + lane];
#pragma unroll
      for (int c = 0; c < 4; ++c) out2[4 * g + c] = o[c] + acc2[8 + 4 * g + c];
    }
  }
  if constexpr (NORM) *nsq = rn[(wm * 2) * 32 + lr] + rn[(wm * 2 + 1) * 32 + lr];
  __syncthreads();  // the epilogue reuses this LDS
}

// The k-split loop for the 64 x 128 tile: wave (wm, kg) owns tile rows wm 32 .. +31, ALL 128 columns (four accumulators) and every second
// 8-deep k-step — one row-major gather of A and four fragment-order loads of B per 16 matrix instructions (the direct loop's 32 x 64 wave
// tiles: 6 per 16, and every fragment loaded by two waves), nothing loaded twice.  Wave (wm, x) keeps columns x 64 .. +63 and ships its other
// two accumulators to wave (wm, 1 - x) through LDS (8 KB per wave): it leaves with acc[0][0..1] as the 2 x 2 wave layout of the epilogues has them.
// Two blocks per CU (150 VGPRs + 64 AGPRs as the compiler allots them).  Asked for three waves per SIMD (__launch_bounds__(256, 3): 162
// registers, nothing spilled) the kernel is SLOWER — C5 645 us per frame against 616, c2b on this tile 119 against 107: like the direct
// loop's tiles (three resident beat four), fewer co-resident operand streams keep their lines in L1.
template <int NBUF>
__device__ __forceinline__ void gemm_mainloop_ks128(gfloat_p A, gfloat_p B, uint32_t M, uint32_t Ncols, uint32_t Dp, uint32_t m0,
                                                    uint32_t n0, float* lds, f32x16 (&out)[1][2], uint64_t* tr = nullptr) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t w4 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)) & 3u;
  const uint32_t wm = w4 >> 1, kg = w4 & 1u, lr = lane & 31u, lh = lane >> 5;
  const uint32_t Np = (Ncols + 31u) / 32u * 32u, nb0 = n0 & ~31u;
  auto left = [&](uint32_t rows) { const uint64_t b = (uint64_t)rows * Dp * 4u; return (uint32_t)(b < 0xffffffffull ? b : 0xffffffffull); };
  const __amdgpu_buffer_rsrc_t RA = __builtin_amdgcn_make_buffer_rsrc((void*)(A + (size_t)m0 * Dp), 0, (int)left(M - m0), 0x00020000);
  const __amdgpu_buffer_rsrc_t RB = __builtin_amdgcn_make_buffer_rsrc((void*)(B + (size_t)nb0 * Dp), 0, (int)left(Np - nb0), 0x00020000);
  const uint32_t oa = ((wm * 32u + lr) * Dp + lh * 4u) * 4u;
  uint32_t ob[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const uint32_t rr = (n0 - nb0) + n * 32u + lr;
    ob[n] = ((rr >> 5) * (Dp >> 3) * 256u + lh * 128u + (rr & 31u) * 4u) * 4u;
  }
  const uint32_t mine = Dp >> 4;
  f32x16 acc[4];
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[n][e] = 0.f;
  f32x4 fa[NBUF], fb[NBUF][4];
  auto load = [&](auto buf_tag, uint32_t j) {
    constexpr int buf = decltype(buf_tag)::value;
    const uint32_t s = 2u * j + kg;
    fa[buf] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(RA, (int)oa, (int)(s * 32u), 0));
#pragma unroll
    for (int n = 0; n < 4; ++n) fb[buf][n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(RB, (int)ob[n], (int)(s * 1024u), 0));
  };
  auto step = [&](auto b_tag, uint32_t j) {
    constexpr int b = decltype(b_tag)::value;
    load(std::integral_constant<int, (b + NBUF - 1) % NBUF>{}, j + NBUF - 1);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[b][e], fb[b][n][e], acc[n], 0, 0, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    sa_static_for<0, 4>([&](auto) { __builtin_amdgcn_sched_group_barrier(0x008, 3, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); });
    __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
  };
  sa_static_for<0, NBUF - 1>([&](auto b) { load(b, (uint32_t)decltype(b)::value); __builtin_amdgcn_sched_barrier(0); });
  SA_STAMP(tr, 1);
  uint32_t j = 0;
  for (; j + NBUF <= mine; j += NBUF) sa_static_for<0, NBUF>([&](auto b) { step(b, j + decltype(b)::value); });
  const uint32_t rem = mine - j;
  sa_static_for<0, NBUF>([&](auto b) { if ((uint32_t)decltype(b)::value < rem) step(b, j + decltype(b)::value); });
  SA_STAMP(tr, 2);
  f32x4* red = (f32x4*)lds;   // [4 waves][2 accumulators][4][64 lanes] f32x4 = 32 KB
  auto ship = [&](const f32x16& a, uint32_t slot) {
#pragma unroll
    for (int g = 0; g < 4; ++g) red[((w4 * 2u + slot) * 4u + g) * 64u + lane] = f32x4{a[4 * g], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]};
  };
  if (kg == 0) { ship(acc[2], 0); ship(acc[3], 1); } else { ship(acc[0], 0); ship(acc[1], 1); }
  __syncthreads();
  const uint32_t pw = w4 ^ 1u;
  auto take = [&](const f32x16& mine_, uint32_t slot, f32x16& dst, bool mine_first) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 o = red[((pw * 2u + slot) * 4u + g) * 64u + lane];
#pragma unroll
      for (int c = 0; c < 4; ++c) dst[4 * g + c] = mine_first ? mine_[4 * g + c] + o[c] : o[c] + mine_[4 * g + c];
    }
  };
  // (k-half 0 + k-half 1 whichever wave adds)
  if (kg == 0) { take(acc[0], 0, out[0][0], true); take(acc[1], 1, out[0][1], true); }
  else { take(acc[2], 0, out[0][0], false); take(acc[3], 1, out[0][1], false); }
  __syncthreads();
}

// The same idea for the wider tiles (128x128, 64x128, 128x64: 2 x 2 waves, each a (BM/2) x (BN/2) wave tile over the WHOLE k range): operands
// straight from memory — A row-major, B from the bank's fragment-order twin — TM + TN buffer loads per 8-deep k-step for 4 TM TN matrix
// instructions, no LDS stage, no barrier, no reduction.  The two waves of a wave row (column) load the same A (B) fragments: twice the
// L1 traffic of the staged loop, none of its LDS instructions.
template <int BM, int BN, int NBUF>
__device__ __forceinline__ void gemm_mainloop_direct(gfloat_p A, gfloat_p B, uint32_t M, uint32_t Ncols, uint32_t Dp, uint32_t m0, uint32_t n0,
                                                     f32x16 (&acc)[BM / 64][BN / 64], uint64_t* tr = nullptr) {
  constexpr int TM = BM / 64, TN = BN / 64;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t w4 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)) & 3u;
  const uint32_t wm = w4 >> 1, wn = w4 & 1u, lr = lane & 31u, lh = lane >> 5;
  const uint32_t Np = (Ncols + 31u) / 32u * 32u, nb0 = n0 & ~31u;
  auto left = [&](uint32_t rows) { const uint64_t b = (uint64_t)rows * Dp * 4u; return (uint32_t)(b < 0xffffffffull ? b : 0xffffffffull); };
  const __amdgpu_buffer_rsrc_t RA = __builtin_amdgcn_make_buffer_rsrc((void*)(A + (size_t)m0 * Dp), 0, (int)left(M - m0), 0x00020000);
  const __amdgpu_buffer_rsrc_t RB = __builtin_amdgcn_make_buffer_rsrc((void*)(B + (size_t)nb0 * Dp), 0, (int)left(Np - nb0), 0x00020000);
  uint32_t oa[TM], ob[TN];
#pragma unroll
  for (int m = 0; m < TM; ++m) oa[m] = ((wm * (BM / 2) + m * 32u + lr) * Dp + lh * 4u) * 4u;
#pragma unroll
  for (int n = 0; n < TN; ++n) {
    const uint32_t rr = (n0 - nb0) + wn * (BN / 2) + n * 32u + lr;
    ob[n] = ((rr >> 5) * (Dp >> 3) * 256u + lh * 128u + (rr & 31u) * 4u) * 4u;
  }
  const uint32_t steps = Dp >> 3;
#pragma unroll
  for (int m = 0; m < TM; ++m)
#pragma unroll
    for (int n = 0; n < TN; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;
  f32x4 fa[NBUF][TM], fb[NBUF][TN];
  auto load = [&](auto buf_tag, uint32_t s) {
    constexpr int buf = decltype(buf_tag)::value;
#pragma unroll
    for (int m = 0; m < TM; ++m) fa[buf][m] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(RA, (int)oa[m], (int)(s * 32u), 0));
#pragma unroll
    for (int n = 0; n < TN; ++n) fb[buf][n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(RB, (int)ob[n], (int)(s * 1024u), 0));
  };
  auto step = [&](auto b_tag, uint32_t s) {
    constexpr int b = decltype(b_tag)::value;
    load(std::integral_constant<int, (b + NBUF - 1) % NBUF>{}, s + NBUF - 1);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int m = 0; m < TM; ++m)
#pragma unroll
        for (int n = 0; n < TN; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[b][m][e], fb[b][n][e], acc[m][n], 0, 0, 0);
    // the step's loads spread evenly over its 4 TM TN matrix instructions
    constexpr int NM = 4 * TM * TN, NL = TM + TN, GAP = NM / NL;
    sa_static_for<0, NL>([&](auto i) {
      __builtin_amdgcn_sched_group_barrier(0x008, decltype(i)::value == 0 ? 1 : GAP, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    });
    __builtin_amdgcn_sched_group_barrier(0x008, NM - 1 - (NL - 1) * GAP, 0);
  };
  sa_static_for<0, NBUF - 1>([&](auto b) { load(b, (uint32_t)decltype(b)::value); __builtin_amdgcn_sched_barrier(0); });
  SA_STAMP(tr, 1);
  uint32_t s = 0;
  for (; s + NBUF <= steps; s += NBUF) sa_static_for<0, NBUF>([&](auto b) { step(b, s + decltype(b)::value); });
  const uint32_t rem = steps - s;
  sa_static_for<0, NBUF>([&](auto b) { if ((uint32_t)decltype(b)::value < rem) step(b, s + decltype(b)::value); });
  SA_STAMP(tr, 2);
}

// k-group reductions (64x64 tile only: one 32x32 accumulator per wave).  Every group parks its 16 partial
// sums per lane in LDS as red[group][reg][thread] (conflict-free: consecutive lanes, consecutive words).
//  * kgroup_reduce_spread: group g then owns registers [g*16/KG, (g+1)*16/KG) of every wave tile and sums them
//    over the groups in group order — the epilogue work is spread over all 4*KG waves.
template <int KG>
__device__ __forceinline__ void kgroup_reduce_spread(const f32x16& acc, float* lds, float (&out)[16 / KG]) {
  constexpr int R = 16 / KG;
  if constexpr (KG == 1) {
#pragma unroll
    for (int i = 0; i < 16; ++i) out[i] = acc[i];
  } else {
    const uint32_t tid = threadIdx.x, kg = tid >> 8, ltid = tid & 255u;
    float* red = lds;
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(kg * 16 + r) * 256 + ltid] = acc[r];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const uint32_t r = kg * R + i;
      float sum = red[r * 256 + ltid];
#pragma unroll
      for (int g = 1; g < KG; ++g) sum += red[(g * 16 + r) * 256 + ltid];
      out[i] = sum;
    }
    __syncthreads();
  }
}

// Row of accumulator register r for lane half lh in a 32x32 MFMA tile (C/D layout, cdna_hip_programming.md §3)
__device__ __forceinline__ uint32_t acc_row(uint32_t r, uint32_t lh) { return (r & 3u) + 8u * (r >> 2) + 4u * lh; }

// Running maximum of the present weights (BestFitVoting's max_dist, voting/best.rs:59-76) WITHOUT atomics: a register-level
// wave reduction (DPP / ds_swizzle), the wave maxima through one LDS word each and one barrier, then every workgroup stores
// its maximum into its own slot of S.vis_max_key (slot = tile index inside the scene; the host puts the tile grid into the
// descriptor).  k_bestfit_tile folds the slots.  Device-scope atomics on shared words serialise on this chip
// (MI355X_MICROARCH.md "fanin"): one per wave on one word cost 45 us at 4096 waves; sharded 64 ways, one per wave (2048)
// still +8.7 us and one per workgroup (256) +1.1 us on the C2 kernel.  Key 0 = "no weight" (reads back as -1.0).
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  auto mx = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
  v = mx(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true));    // xor 1
  v = mx(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true));    // xor 2
  v = mx(v, (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (4 << 10) | 0x1F));     // xor 4
  v = mx(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, true));   // row_ror:8 = xor 8
  v = mx(v, (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (16 << 10) | 0x1F));    // xor 16
  return mx((uint32_t)__builtin_amdgcn_readlane((int)v, 0), (uint32_t)__builtin_amdgcn_readlane((int)v, 32));
}
__device__ __forceinline__ void block_max_key(uint32_t SA_G* slots, uint32_t slot, uint32_t kmax) {
  __shared__ uint32_t s_wmax[16];
  const uint32_t m = wave_max_u32(kmax);
  const uint32_t wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63u) == 0) s_wmax[wave] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t b = 0;
    for (uint32_t w = 0; w < nw; ++w) b = s_wmax[w] > b ? s_wmax[w] : b;
    slots[slot] = b;
  }
}

// Everything the reference does per (candidate, observation) pair after the dot product.  compatible() (sort.rs:250-270)
// compares the candidate's epoch — the same for every row of a scene-frame — with the track's, so its epoch part and the
// choice of the constraint (spatio_temporal_constraints.rs:48-59) are per-COLUMN facts, folded into GemmCols before the
// main loop; what is left per cell is dist_in_2r <= max_dist when a constraint applies.
// Bit c of the result: cell c of this lane fails the spatio-temporal constraint of its column (dist_in_2r > max_dist).  One
// pass, entered only when some lane of the wave has a constrained column at all.
template <int CELLS, typename RowGeo>
__device__ __forceinline__ uint32_t constraint_mask(const GemmCols& col, RowGeo row_geo) {
  uint32_t failed = 0;
  if (__ballot(col.cmax >= 0.0f) != 0ull) {
    if (col.cmax >= 0.0f) {
#pragma unroll
      for (int c = 0; c < CELLS; ++c) failed |= (sa_dist_in_2r(*row_geo(c), col.g) <= col.cmax) ? 0u : (1u << c);
    }
  }
  return failed;
}
// A candidate's row operands in raw-feature mode (the fused first phase: nothing the preparation blocks write may be read): what
// frame_prep_block derives for it (visual_sort/simple_api.rs:130-170, metric.rs:227-249).  FETCH issues the loads — which of them by the
// scene's flags alone, none behind a branch on a loaded value — and the values are turned into geometry and the feature_can_be_used gate
// BEHIND the main loop: with the gate's short-circuit chain in front of it (present? -> quality -> own area) the tile's first wave
// started its loop a memory round trip late, and the other three waited for it at the exchange.
struct RawRow { float xc, yc, aspect, height, q, oa; uint32_t fp; };
__device__ __forceinline__ RawRow raw_row_fetch(const SceneDev& S, uint32_t gi) {
  RawRow r;
  const BoxRaw br = sa_ldg(S.c_raw + gi);
  r.xc = br.box.xc; r.yc = br.box.yc; r.aspect = br.box.aspect; r.height = br.box.height;
  r.fp = (S.flags & SCN_HAS_FPRESENT) ? (uint32_t)S.c_fpresent_in[gi] : 1u;
  r.q = (S.flags & SCN_HAS_QUALITY) ? S.c_quality[gi] : 1.0f;
  r.oa = (S.flags & SCN_HAS_OWN) ? S.c_own[gi] : __builtin_nanf("");
  return r;
}
__device__ __forceinline__ bool raw_row_usable(const SceneDev& S, const SaParams& p, const RawRow& r, sa_geo* g) {
  g->xc = r.xc; g->yc = r.yc; g->r = sa_radius(r.aspect, r.height); g->hha = r.height * r.height * r.aspect;
  const bool perc_ok = !(r.oa == r.oa) || r.oa >= p.visual_minimal_own_area_use;
  return (S.flags & SCN_HAS_FEATS) != 0 && r.fp != 0 && sa_area(r.aspect, r.height) >= p.visual_minimal_area && r.q >= p.visual_minimal_quality_use && perc_ok;
}
// EU: distance::euclidean (distance.rs:9-19) on the matrix cores.  sqrt(|a|^2 + |b|^2 - 2 a.b) cancels on near-identical vectors —
// exactly the true matches — so a cell whose expansion is not trustworthy to 1e-5 relative, d^2 < rho (|a|^2 + |b|^2) with
// rho = 5e-3 sqrt(Dp) (twice the largest error of the f32 expansion seen over 10^6 pairs, scripts/euclid_error_model.py), is FLAGGED
// instead of evaluated (*flagged; false for the cosine metric — only the cell loops look at it): the tile recomputes it afterwards as the direct sum of
// (a - b)^2 (euclid_fixup).  In tracking frames that is about one cell per candidate; everything else rides the contraction at the
// cosine kernel's speed.
template <bool EU>
__device__ __forceinline__ float visual_cell(const SaParams& p, float dot, float na, bool cons_failed, const GemmCols& col,
                                             uint32_t* kmax, bool* flagged) {
  // Straight-line on purpose: with a short-circuit chain (usable? column ok? ...) the compiler sinks every operand load into the
  // branch that first needs it, and the row operands come from LDS — each cell then pays two or three LDS round trips one after
  // the other.  na = squared norm of the candidate's feature, NaN when feature_can_be_used() says no (the distance is then NaN
  // and fails is_ok like any NaN).  The spatio-temporal constraint, rare and expensive, is evaluated by the caller in a pass of
  // its own (constraint_mask) and arrives as one bit: a branch per cell made every cell a basic block of its own, and a lone
  // wave then walks 16 dependent chains (multiply, v_rsq, multiply, compare, key ...) one after the other — 4 k cycles.
  const bool ok0 = col.ok && !cons_failed;
  bool ok = ok0;
  float w;
  if constexpr (EU) {
    const float s = na + col.nb;
    const float d2 = s - 2.0f * dot;
    const bool f = ok0 & (d2 < p.eu_rho * s);        // NaN norms (unusable candidate): never flagged, never present
    *flagged = f;
    const float d = __fsqrt_rn(d2 < 0.0f ? 0.0f : d2);  // NaN stays NaN
    ok = ok & !f & (d <= p.visual_threshold);         // VisualSortMetricType::is_ok for Euclidean (NaN fails)
    w = d;                                            // distance_to_weight: the distance itself
  } else {
    // divided / (f1_divisor * f2_divisor).sqrt(): v_rsq_f32 + multiply, <= 2 ulp from the reference's sqrt + divide,
    // two orders of magnitude inside the 1e-5 gate and ~25 instructions cheaper per cell
    const float d = dot * __frsqrt_rn(na * col.nb);
    ok = ok & (d >= p.visual_threshold);  // VisualSortMetricType::is_ok (NaN fails)
    w = 1.0f - d;                         // distance_to_weight
    *flagged = false;
  }
  const uint32_t key = ok ? sa_f32_key(w) : 0u;
  *kmax = key > *kmax ? key : *kmax;
  return ok ? w : __builtin_nanf("");
}

// ---- The fused epilogue, piece by piece.  Every tile form below (visual_cosine_tile, visual_tile96, visual_tile_helped, visual_ktile)
// is a prologue, a main loop of its own, its own hand-over of the accumulators, and calls of these.  The gates (column ok, row usable,
// constraint) and the lowest-column rule of the row scan are written here and nowhere else.  The lowest-row rule of the column minima is
// written here (vote_cells, col_min_fold) and in two more places, both in visual_cosine_tile: the cell loop of its wider tiles, which
// walks two columns per lane with the row operands shared between them, and the sink of its euclidean fix-up (one recomputed cell into
// the column's slot). ----

// Where the epilogue keeps its tables: offsets in floats from the start of the tile's LDS (the main loop's stages or exchange lie under
// them and are dead by then).  CK = false: no column minima (the whole-track tile, whose key tile holds the cells' weights instead).
constexpr uint32_t key_stride(int BN) { return (uint32_t)BN + 4u; }   // row stride of the key tile (words)
constexpr uint32_t flag_words(int BN) { return (uint32_t)BN / 32u; }  // EU: words of flag bits per tile row
constexpr uint32_t FL_CAP = 255;   // EU: the flagged cells as a list too (a tracking frame has a handful per tile); entry [FL_CAP] = their count
struct EpiLds {
  int BM, BN, KG;
  bool CK;
  constexpr uint32_t na() const { return 0u; }                                       // [BM] squared norm of the row, NaN where feature_can_be_used says no
  constexpr uint32_t geo() const { return 2u * BM; }                                 // [BM] sa_geo
  constexpr uint32_t np() const { return 6u * BM; }                                  // [KG][BM] raw mode: squared-norm partials of the k-groups
  constexpr uint32_t ck() const { return (6u + KG) * BM; }                           // [BN] PART: (weight key << 32) | row, minimum per column
  constexpr uint32_t key() const { return ck() + (CK ? 2u * BN : 0u); }              // [64][key_stride] PART: order-preserving keys of 64 tile rows
  constexpr uint32_t flag() const { return key() + 64u * key_stride(BN); }           // [64][flag_words] EU: cells of the current 64-row pass to recompute directly
  constexpr uint32_t flist() const { return flag() + 64u * flag_words(BN); }         // [FL_CAP + 1] EU: the same cells as a list
  constexpr uint32_t end() const { return flist() + FL_CAP + 1u; }
  constexpr uint32_t floats(bool keys, bool eu) const { return eu ? end() : keys ? flag() : key(); }
};
struct EpiTile {   // the same as pointers (visual_tile_helped, whose helper waves fill the tables beside the exchange, places them itself)
  float* na; sa_geo* g; float* np; unsigned long long* ck; uint32_t* key; uint32_t* flag; uint32_t* flist;
};
__device__ __forceinline__ EpiTile epi_tile(EpiLds L, float* lds) {
  return EpiTile{lds + L.na(), (sa_geo*)(lds + L.geo()), lds + L.np(), (unsigned long long*)(lds + L.ck()), (uint32_t*)(lds + L.key()),
                 (uint32_t*)(lds + L.flag()), (uint32_t*)(lds + L.flist())};
}

// Column operands of bank row gj (in_range: the lane has one).  They are fetched BEFORE the contraction, like the row operands: their
// L2/HBM latency (a chain of dependent loads that used to sit, fully exposed, between the last MFMA and the first store: ~2 us of a 18 us
// kernel at C2) disappears behind the main loop.
__device__ __forceinline__ GemmCols tile_col_fetch(const SceneDev& S, const SaParams& p, uint32_t gj, bool in_range) {
  GemmCols c;
  c.ok = false;
  c.nb = 0.f;
  c.cmax = -1.0f;
  c.g = sa_geo{0.f, 0.f, 0.f, 0.f};
  if (in_range) {
    // independent loads, no short-circuit: one round trip instead of a chain of three
    const uint32_t t = gj / S.K;
    const float nb = S.t_fnorm[gj];
    const uint8_t pres = S.t_fpresent[gj];
    const uint32_t cnt = S.t_fcount[t];
    const uint64_t te = S.t_epoch[t];
    c.g = sa_ldg(S.t_geo + t);
    c.nb = nb;
    const uint64_t delta = S.epoch > te ? S.epoch - te : te - S.epoch;
    c.ok = (pres != 0) & (cnt >= p.min_track_len) & (p.max_idle >= delta);
    // (the FIRST constraint whose window holds the track's age — as a chain of selects from the last one down: a `break` on the loaded
    // epoch would hold every wave of the tile in front of its main loop for the load)
    for (uint32_t i = p.cons.n; i-- > 0;) c.cmax = p.cons.delta[i] >= delta ? p.cons.max_dist[i] : c.cmax;
  }
  return c;
}

// Row operands: thread r < BM holds tile row r from before the main loop (loads only; RAW: raw_row_usable behind it) and hands it to the
// other threads through LDS afterwards.
struct TileRow { RawRow raw; sa_geo g; float na, us; bool in; };
template <bool RAW>
__device__ __forceinline__ TileRow tile_row_fetch(const SceneDev& S, uint32_t BM, uint32_t m0) {
  TileRow r{RawRow{0.f, 0.f, 1.f, 1.f, 0.f, 0.f, 0u}, sa_geo{0.f, 0.f, 0.f, 0.f}, 0.f, 0.f, false};
  const uint32_t gi = m0 + threadIdx.x;
  r.in = threadIdx.x < BM && gi < S.N;
  if (r.in) {
    if constexpr (RAW) r.raw = raw_row_fetch(S, gi);
    else {
      r.na = S.c_fnorm[gi];
      r.us = S.c_usable[gi] ? 1.f : 0.f;
      r.g = sa_ldg(S.c_geo + gi);
    }
  }
  return r;
}
__device__ __forceinline__ float gated_norm(float usable, float na) { return usable != 0.f ? na : __builtin_nanf(""); }  // the feature_can_be_used gate rides in the norm
// ... behind the main loop (and the k-group reduction, which uses the same LDS): geometry and gated norms of the tile's rows into E.g / E.na.
// RAW: nsq = what the main loop accumulated of the squared norm of row wm 32 + lr (FOLDED: lane halves and k-halves already summed);
// the k-groups' partials meet in E.np.  Two barriers (one when the norms come pre-computed); E.na / E.g are complete on return.
template <int BM, int KG, bool RAW, bool FOLDED>
__device__ __forceinline__ void tile_rows_to_lds(const SceneDev& S, const SaParams& p, TileRow row, float nsq, const EpiTile& E) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w4 = (tid >> 6) & 3u, kg = KG == 1 ? 0u : tid >> 8;
  if constexpr (RAW) { if (row.in) row.us = raw_row_usable(S, p, row.raw, &row.g) ? 1.f : 0.f; }
  if (tid < (uint32_t)BM) {
    E.g[tid] = row.g;
    if constexpr (!RAW) E.na[tid] = gated_norm(row.us, row.na);
  }
  if constexpr (RAW) {
    // the two halves of a row's k values sit in lanes lr and lr + 32; the waves wn = 0 / 1 of a group hold the same rows
    if constexpr (!FOLDED) nsq += __shfl_xor(nsq, 32);
    if ((w4 & 1u) == 0 && (lane >> 5) == 0) E.np[kg * BM + (w4 >> 1) * 32 + (lane & 31u)] = nsq;
  }
  __syncthreads();
  if constexpr (RAW) {
    if (tid < (uint32_t)BM) {
      float s = E.np[tid];
#pragma unroll
      for (int g2 = 1; g2 < KG; ++g2) s += E.np[g2 * BM + tid];
      E.na[tid] = gated_norm(row.us, s);
    }
    __syncthreads();
  }
}

// EU: the flag words and the list of one 64-row pass, emptied (before a barrier that the caller has anyway).
template <int BN, int NT>
__device__ __forceinline__ void flags_reset(const EpiTile& E) {
  for (uint32_t i = threadIdx.x; i < 64u * flag_words(BN); i += NT) E.flag[i] = 0u;
  if (threadIdx.x == 0) E.flist[FL_CAP] = 0u;
}
// ... cell (lrow, lc) of the pass registered for the direct recompute
template <int BN>
__device__ __forceinline__ void flag_cell(const EpiTile& E, uint32_t lrow, uint32_t lc) {
  atomicOr(&E.flag[lrow * flag_words(BN) + (lc >> 5)], 1u << (lc & 31u));
  const uint32_t pos = atomicAdd(&E.flist[FL_CAP], 1u);
  if (pos < FL_CAP) E.flist[pos] = (lrow << 8) | lc;
}
// ... and a lane's cells out of the mask tile_cells returns.  (The flagged cells are REGISTERED behind the cell loop: with the LDS atomics
// inside it every cell was a basic block of its own and the lone wave walked 16 dependent chains one after the other — the euclidean
// cells 6.2 k cycles against the cosine ones' 3.2 k.)
template <int BN>
__device__ __forceinline__ void flag_cells(const EpiTile& E, uint32_t fmask, uint32_t row0, uint32_t lc) {
  if (__ballot(fmask != 0u) != 0ull) {  // (a tracking frame: about one cell per candidate — most waves skip this)
    while (fmask) {
      const uint32_t i = (uint32_t)__builtin_ctz(fmask);
      fmask &= fmask - 1u;
      flag_cell<BN>(E, row0 + 8u * (i >> 2) + (i & 3u), lc);
    }
  }
}

// The cells of one lane in one column: R accumulator values (dot(i), i < R) of a 32 x 32 wave tile.  Registers 4g .. 4g+3 hold four
// consecutive tile rows (acc_row) — row0 + 8g .. +3 with row0 the row of the lane's first register — so the row operands are one
// 16-byte LDS read per group of four cells, all issued before the first cell is evaluated.  sink(li, gi, w) takes cell i = tile row li,
// candidate gi (rows / columns past the edge: ok = false, w = NaN).  Returns (EU) the mask of the cells to recompute directly.
template <int R, bool EU, typename Dot, typename Sink>
__device__ __forceinline__ uint32_t tile_cells(const SaParams& p, const EpiTile& E, uint32_t row0, uint32_t m0, uint32_t N, const GemmCols& col,
                                               Dot dot, uint32_t* kmax, Sink sink) {
  static_assert(R % 4 == 0, "whole groups of four accumulator registers");
  constexpr int G = R / 4;
  f32x4 nav[G];
#pragma unroll
  for (int g = 0; g < G; ++g) nav[g] = *(const f32x4*)(E.na + row0 + 8u * g);
  const uint32_t cfail = constraint_mask<R>(col, [&](int c) { return E.g + row0 + 8u * (c >> 2) + (c & 3); });
  uint32_t fmask = 0;  // EU: bit i = cell i of this lane goes to the direct recompute
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const uint32_t li = row0 + 8u * (i >> 2) + (i & 3);
    const uint32_t gi = m0 + li;
    bool flagged;
    const float w = visual_cell<EU>(p, dot(i), nav[i >> 2][i & 3], (cfail >> i) & 1u, col, kmax, &flagged);
    if constexpr (EU) fmask |= (flagged && gi < N) ? (1u << i) : 0u;
    sink(li, gi, w);
  }
  return fmask;
}
// Column minima: in-lane over the rows a lane holds (vote_cells), the two lane halves by one exchange, the waves stacked on each other by
// a 64-bit LDS minimum into the column's slot.
__device__ __forceinline__ void col_min_fold(unsigned long long* slot, uint32_t ckey, uint32_t crow, uint32_t lh) {
  unsigned long long cb = ((unsigned long long)ckey << 32) | crow;
  const unsigned long long ob = __shfl_xor(cb, 32);
  cb = ob < cb ? ob : cb;
  if (lh == 0 && (uint32_t)(cb >> 32) != 0xffffffffu) atomicMin(slot, cb);
}
// ... of a vote tile (PART): the cells' order-preserving keys go to the key tile (tile column lc), the column's minimum over the lane's
// rows — lowest row on ties — to E.ck[lc].
template <int BN, int R, bool EU, typename Dot>
__device__ __forceinline__ uint32_t vote_cells(const SaParams& p, const EpiTile& E, uint32_t row0, uint32_t lc, uint32_t m0, uint32_t N,
                                               const GemmCols& col, Dot dot, uint32_t* kmax) {
  uint32_t ckey = 0xffffffffu, crow = 0;
  const uint32_t fmask = tile_cells<R, EU>(p, E, row0, m0, N, col, dot, kmax, [&](uint32_t li, uint32_t gi, float w) {
    const uint32_t key = (w == w && gi < N) ? sa_f32_key(w) : 0xffffffffu;
    E.key[li * key_stride(BN) + lc] = key;
    if (key < ckey) { ckey = key; crow = gi; }  // rows ascend with i: the lowest row wins ties
  });
  col_min_fold(E.ck + lc, ckey, crow, (threadIdx.x >> 5) & 1u);
  return fmask;
}

// PART: the order-preserving keys of 64 tile rows at a time go to an LDS tile; after a barrier every row is scanned by TPR threads
// (contiguous column segments, running minimum with the lowest column on ties, then a few DPP exchanges between the threads of a row)
// and its partial goes straight to memory (the caller's sink: thread seg == 0 of the row holds the result, key 0xffffffff = no weight).
// (A first version reduced every accumulator register across the wave with DPP + ballot: 30 instructions per cell, 10.7 k cycles of
// epilogue for the one-k-group tile where each lane holds 16 cells.)
struct RowBest { uint32_t row, seg, key, col; };   // row of the key tile, the thread's place in its row, lightest key and its tile column
template <int BN, int TPR>
__device__ __forceinline__ RowBest row_scan(const uint32_t* s_key) {
  static_assert((TPR == 4 || TPR == 8) && BN % (4 * TPR) == 0, "a quad or two per row, whole 16-byte reads per thread");
  constexpr uint32_t CPT = BN / TPR;  // columns per thread
  const uint32_t rr = threadIdx.x / TPR, seg = threadIdx.x % TPR;
  const uint32_t* kp = s_key + rr * key_stride(BN) + seg * CPT;
  uint32_t bk = 0xffffffffu, bc = 0;
  // (unrolled up to the six 16-byte reads of the 96-column tile; the 128-column tiles' eight would hold 32 registers beside the next
  // pass's accumulators: a loop there, as it always was)
  constexpr int UNROLL = CPT <= 24 ? CPT / 4 : 1;
#pragma unroll UNROLL
  for (uint32_t c4 = 0; c4 < CPT; c4 += 4) {
    const uint4 v = *(const uint4*)(kp + c4);
    if (v.x < bk) { bk = v.x; bc = c4; }
    if (v.y < bk) { bk = v.y; bc = c4 + 1; }
    if (v.z < bk) { bk = v.z; bc = c4 + 2; }
    if (v.w < bk) { bk = v.w; bc = c4 + 3; }
  }
  bc += seg * CPT;
  auto take = [&](uint32_t ok, uint32_t oc) { if (ok < bk || (ok == bk && oc < bc)) { bk = ok; bc = oc; } };
  take((uint32_t)__builtin_amdgcn_mov_dpp((int)bk, 0xB1, 0xF, 0xF, true), (uint32_t)__builtin_amdgcn_mov_dpp((int)bc, 0xB1, 0xF, 0xF, true));
  take((uint32_t)__builtin_amdgcn_mov_dpp((int)bk, 0x4E, 0xF, 0xF, true), (uint32_t)__builtin_amdgcn_mov_dpp((int)bc, 0x4E, 0xF, 0xF, true));
  if constexpr (TPR == 8) take(__shfl_xor(bk, 4), __shfl_xor(bc, 4));  // the other quad of the 8-thread group
  return RowBest{rr, seg, bk, bc};
}
// ... into the vote word of candidate gi (the caller: thread seg == 0, gi < N)
__device__ __forceinline__ void vote_row(const SceneDev& S, uint32_t gi, uint32_t n0, const RowBest& b) {
  if (b.key != 0xffffffffu)
    __hip_atomic_fetch_min(S.row_best + gi, ((unsigned long long)b.key << 32) | (n0 + b.col), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The tile's column minima into the vote words of its tracks: complete since the barrier of the last row pass.
// (blockDim.x, not the tile's thread count as a template parameter: with the constant the 64 x 96 kernel, at its 128-register limit,
// keeps one more register across its main loop and spills it)
template <int BN>
__device__ __forceinline__ void flush_col_best(const SceneDev& S, const unsigned long long* s_ck, uint32_t n0) {
  for (uint32_t i = threadIdx.x; i < (uint32_t)BN; i += blockDim.x) {
    const uint32_t gj = n0 + i;
    if (gj >= S.TK) continue;
    const unsigned long long k2 = s_ck[i];
    if (k2 != ~0ull) __hip_atomic_fetch_min(S.col_best + gj, k2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// EU: the flagged cells of a 64-row pass, recomputed as the direct sum of (a - b)^2: a wave per cell, the lanes along k (16-byte loads of
// both rows, L2-resident: the tile has just streamed them), a wave reduction, one result per cell — lane 0 hands it to
// sink(lrow, lc, gi, w): w = the distance, NaN when it fails is_ok.  row_of(lrow) = the candidate of row lrow of the pass; A = the
// candidates' rows; TWIN: the track's row out of the fragment-order twin the tile has just streamed (k-split / direct loops: L2-resident;
// the row-major bank is cold there, a trip to memory per flagged cell).  A tile with more than 64 such cells reports the frame as
// ill-conditioned for the expansion (S.stats[0], read by the host after the frame: it switches the scene's engine to the vector-pipe
// kernel for a while); the answers of THIS frame are exact either way.
template <int BN, bool TWIN, typename RowOf, typename Sink>
__device__ __forceinline__ void euclid_fixup(const SceneDev& S, const SaParams& p, const EpiTile& E, const float SA_G* A, uint32_t n0, RowOf row_of, Sink sink) {
  __syncthreads();  // flag words / list (and the keys / weights / matrix cells of the pass) complete
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  auto recompute = [&](uint32_t lrow, uint32_t lc) {
    const uint32_t gi = row_of(lrow), gj = n0 + lc;
    const float SA_G* a = A + (size_t)gi * S.Dp;
    const float SA_G* b = TWIN ? S.t_ffrag + sa_frag_index(gj, 0, S.Dp) : S.t_feat + (size_t)gj * S.Dp;
    float acc2 = 0.f;
    for (uint32_t k = lane * 4u; k < S.Dp; k += 256u) {
      const f32x4 x = *(const f32x4 SA_G*)(a + k), y = *(const f32x4 SA_G*)(b + (TWIN ? (size_t)(k >> 3) * 256u + ((k >> 2) & 1u) * 128u : (size_t)k));
      const float d0 = x[0] - y[0], d1 = x[1] - y[1], d2 = x[2] - y[2], d3 = x[3] - y[3];
      acc2 += d0 * d0; acc2 += d1 * d1; acc2 += d2 * d2; acc2 += d3 * d3;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc2 += __shfl_xor(acc2, o);
    if (lane == 0) {
      const float d = __fsqrt_rn(acc2);
      sink(lrow, lc, gi, d <= p.visual_threshold ? d : __builtin_nanf(""));
    }
  };
  const uint32_t nf = (uint32_t)__builtin_amdgcn_readfirstlane((int)E.flist[FL_CAP]);
  if (nf <= FL_CAP) {
    // the usual case: a handful of cells, dealt round-robin to the waves straight from the list
    for (uint32_t i = wave; i < nf; i += nw) {
      const uint32_t ent = (uint32_t)__builtin_amdgcn_readfirstlane((int)E.flist[i]);
      recompute(ent >> 8, ent & 255u);
    }
  } else {
    // more than the list holds (an ill-conditioned frame): every wave walks the flag words of its rows
    for (uint32_t lrow = wave; lrow < 64u; lrow += nw)
      for (uint32_t wd = 0; wd < flag_words(BN); ++wd) {
        uint32_t bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)E.flag[lrow * flag_words(BN) + wd]);
        while (bits) {
          const uint32_t lc = wd * 32u + (uint32_t)__builtin_ctz(bits);
          bits &= bits - 1u;
          recompute(lrow, lc);
        }
      }
  }
  if (nf > 64u && threadIdx.x == 0) S.stats[0] = 1u;  // more than 1.5 % of a tile's cells: the frame is ill-conditioned for the expansion
}

// One tile of the fused visual cost kernel.  RAW (the heterogeneous frame launch, k_frame_visual): the frame-preparation
// blocks run BESIDE this tile, not before it, so nothing they produce may be read — the candidate features come straight
// from the uploaded rows (their length is a multiple of 32: no padding needed), their squared norms are accumulated from
// the A fragments inside the main loop, and the row's geometry / feature_can_be_used gate are derived from the raw box.
//
// PART (bank depth 1 only): instead of the N x T weight matrix the tile emits what k_bestfit_tile would derive from it — per row
// the lightest weight over the tile's columns (lowest column on ties), per column the lightest over its rows (lowest row) — as
// the BestFit partials k_bestfit_resolve folds.  BestFit ranks groups by W = sum_k f64(max_dist - w_k); with one observation per
// track that is decreasing in w, so the heaviest group of a row or column is its lightest weight and max_dist (known only when
// every tile is done) is needed neither here nor in k_bestfit_resolve, which folds the partials on the weights.  Where two
// DIFFERENT weights round to the same f32 difference from max_dist the reference would fall back on the index order; they
// differ by < 6e-8, four hundred times below the 1e-5 the feature distances themselves are good for.  One launch
// (k_bestfit_tile) and the write + re-read of the matrix disappear; the parity taps re-run the contraction with PART = false.
// LDS floats a contraction tile needs: its main loop's (SaTileForm, sa_tile_plan.h) and what the
// fused epilogue lays out in the same buffer afterwards (EpiLds): row operands, PART / EU: column minima + a 64-row key tile, EU: flag words + list.
constexpr uint32_t gemm_lds_floats(SaTileForm F, bool PART, bool EU) {
  const uint32_t loop = F.loop_lds_floats(), epi = EpiLds{F.bm, F.bn, F.kg, true}.floats(PART || EU, EU);
  uint32_t m = loop > epi ? loop : epi;
  // the direct loop's 64 x 128 tile (85 VGPRs: four blocks per CU by registers) is held to THREE blocks per CU by its LDS footprint: measured at
  // C5 (5000 x 2000 x 4096), four resident tiles 714 us, three 631, two 655 (the staged loop: 657) — a fourth tile's operand streams thrash the L1
  if (F.loop == SaLoop::direct && F.bm == 64 && F.bn == 128 && m < 12288u) m = 12288u;
  return (m + 63u) & ~63u;
}
template <int BM, int BN, SaLoop LOOP, int KG, bool RAW, bool PART, bool EU = false>
__device__ __forceinline__ void visual_cosine_tile(const SceneDev& S, const SaParams& p, uint32_t bx, uint32_t by, float* lds) {
  constexpr SaTileForm F{BM, BN, LOOP, KG};
  constexpr bool KSPLIT = LOOP == SaLoop::ksplit;   // gemm_mainloop_ks: the bank read in fragment order, no LDS stage
  constexpr bool TWIN = LOOP != SaLoop::staged && LOOP != SaLoop::ring;   // ... as the direct loop and the 64 x 128 tile's k-split loop read it
  static_assert(LOOP != SaLoop::ks128 || (BM == 64 && BN == 128 && !RAW), "k-split 64 x 128");
  constexpr int NT = F.threads();        // threads of the block
  uint64_t* tr = SA_TRACE_PTR();
  SA_STAMP(tr, 0);
  const uint32_t N = S.N, TK = S.TK;
  const uint32_t m0 = by * BM, n0 = bx * BN;
  if (m0 >= N || n0 >= TK) return;
  const uint32_t key_slot = by * ((TK + BN - 1) / BN) + bx;  // < S.nkeys = tiles of THIS scene
  constexpr int TM = BM / 64, TN = BN / 64;
  static_assert(KG == 1 || (TM == 1 && TN == 1), "k-groups only with the 64x64 tile");
  static_assert(!RAW || (TM == 1 && TN == 1 && LOOP != SaLoop::ring), "raw mode: 64x64 tiles with k-groups");
  static_assert(!KSPLIT || (TM == 1 && TN == 1), "k-split: 64x64 tiles");
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w4 = (tid >> 6) & 3u, kg = TWIN ? 0u : tid >> 8;
  const uint32_t wm = w4 >> 1, wn = w4 & 1u, lr = lane & 31u, lh = lane >> 5;
  static_assert(BM <= 256, "one thread per tile row");
  const TileRow row = tile_row_fetch<RAW>(S, BM, m0);
  GemmCols col[TN];
#pragma unroll
  for (int n = 0; n < TN; ++n) {
    const uint32_t gj = n0 + wn * (BN / 2) + n * 32 + lr;
    col[n] = tile_col_fetch(S, p, gj, gj < TK);
  }

  f32x16 acc[TM][TN];
  float nsq = 0.f;
  if constexpr (KSPLIT) gemm_mainloop_ks<4, RAW, true>((gfloat_p)(RAW ? S.c_feat_raw : (const float SA_G*)S.c_feat), (gfloat_p)S.t_ffrag, N, TK, S.Dp, m0, n0, lds, acc[0][0], tr, &nsq, RAW ? p.ks_yield : 0u);
  else if constexpr (LOOP == SaLoop::ks128) gemm_mainloop_ks128<3>((gfloat_p)S.c_feat, (gfloat_p)S.t_ffrag, N, TK, S.Dp, m0, n0, lds, acc, tr);
  else if constexpr (LOOP == SaLoop::direct) gemm_mainloop_direct<BM, BN, 4>((gfloat_p)S.c_feat, (gfloat_p)S.t_ffrag, N, TK, S.Dp, m0, n0, acc, tr);
  else if constexpr (LOOP == SaLoop::ring) gemm_mainloop_ring<BM, BN>((gfloat_p)S.c_feat, (gfloat_p)S.t_feat, N, TK, S.Dp, m0, n0, lds, acc, tr);
  else if constexpr (RAW) gemm_mainloop<BM, BN, KG, true>((gfloat_p)S.c_feat_raw, (gfloat_p)S.t_feat, N, TK, S.Dp, m0, n0, lds, acc, tr, &nsq);
  else gemm_mainloop<BM, BN, KG>((gfloat_p)S.c_feat, (gfloat_p)S.t_feat, N, TK, S.Dp, m0, n0, lds, acc, tr);

  constexpr int R = 16 / KG;
  float part[TM == 1 && TN == 1 ? R : 1];
  if constexpr (TM == 1 && TN == 1) kgroup_reduce_spread<KG>(acc[0][0], lds, part);
  SA_STAMP(tr, 3);

  // ---- fused epilogue: row metadata through LDS, column metadata in registers ----
  constexpr EpiLds L{BM, BN, KG, true};
  static_assert(L.floats(PART || EU, EU) <= gemm_lds_floats(F, PART, EU), "the epilogue's tables must fit the tile's LDS");
  const EpiTile E = epi_tile(L, lds);
  constexpr uint32_t KS = key_stride(BN);
  if constexpr (EU) flags_reset<BN, NT>(E);
  if constexpr (PART) {
    for (uint32_t i = tid; i < (uint32_t)BN; i += NT) E.ck[i] = ~0ull;
  }
  tile_rows_to_lds<BM, KG, RAW, KSPLIT>(S, p, row, nsq, E);
  uint32_t kmax = 0;  // order-preserving key of the largest present weight seen by this lane
  auto rows_to_partials = [&](uint32_t m) {
    if constexpr (PART) {
      __syncthreads();  // the key tile (and, in the last pass, the column minima) complete
      const RowBest b = row_scan<BN, NT / 64>(E.key);
      const uint32_t gi = m0 + (b.row >> 5) * (BM / 2) + m * 32 + (b.row & 31u);
      if (b.seg != 0 || gi >= N) return;
      if (p.vote_words) vote_row(S, gi, n0, b);
      else {
        const bool has = b.key != 0xffffffffu;
        S.row_part_w[(size_t)bx * S.N + gi] = has ? (double)sa_key_f32(b.key) : -1.0;
        S.row_part_t[(size_t)bx * S.N + gi] = has ? (int32_t)(n0 + b.col) : -1;
      }
    }
  };
  // EU: the flagged cells of the 64-row pass `m` recomputed — into the key tile and the column minima (PART) or the weight matrix.
  auto fixup = [&](uint32_t m) {
    if constexpr (EU) {
      euclid_fixup<BN, TWIN>(S, p, E, RAW ? S.c_feat_raw : (const float SA_G*)S.c_feat, n0,
        [&](uint32_t lrow) { return m0 + (lrow >> 5) * (BM / 2) + m * 32 + (lrow & 31u); },
        [&](uint32_t lrow, uint32_t lc, uint32_t gi, float w) {
          if constexpr (PART) {
            E.key[lrow * KS + lc] = w == w ? sa_f32_key(w) : 0xffffffffu;
            if (w == w) atomicMin(&E.ck[lc], ((unsigned long long)sa_f32_key(w) << 32) | gi);
          } else {
            const uint32_t key = w == w ? sa_f32_key(w) : 0u;
            S.vis[(size_t)gi * TK + n0 + lc] = w;
            kmax = key > kmax ? key : kmax;
          }
        });
      if (m + 1 < (uint32_t)TM) {  // the next pass reuses the flag words and the list
        __syncthreads();
        flags_reset<BN, NT>(E);
        __syncthreads();
      }
    }
  };
  if constexpr (TM == 1 && TN == 1) {
    // k-group kg owns registers kg R .. kg R + R - 1 of every wave tile (kgroup_reduce_spread)
    const uint32_t lc = wn * 32 + lr, gj = n0 + lc, row0 = wm * 32 + 8u * (kg * (R / 4)) + 4u * lh;
    auto dot = [&](int i) { return part[i]; };
    if constexpr (PART) {
      const uint32_t fmask = vote_cells<BN, R, EU>(p, E, row0, lc, m0, N, col[0], dot, &kmax);
      if constexpr (EU) flag_cells<BN>(E, fmask, row0, lc);   // (BM = 64: the tile row is the pass row)
      SA_STAMP(tr, 6);
      fixup(0);
      rows_to_partials(0);
      SA_STAMP(tr, 7);
    } else {
      const uint32_t fmask = tile_cells<R, EU>(p, E, row0, m0, N, col[0], dot, &kmax, [&](uint32_t, uint32_t gi, float w) {
        if (gi < N && gj < TK) S.vis[(size_t)gi * TK + gj] = w;
      });
      if constexpr (EU) flag_cells<BN>(E, fmask, row0, lc);
      fixup(0);
    }
  } else {
    // the wider tiles: TM passes of 64 rows, a lane's 16 rows against its TN columns in each
    uint32_t ckey[TN], crow[TN];
#pragma unroll
    for (int n = 0; n < TN; ++n) { ckey[n] = 0xffffffffu; crow[n] = 0; }
#pragma unroll
    for (int m = 0; m < TM; ++m) {
      f32x4 nav[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) nav[g] = *(const f32x4*)(E.na + wm * (BM / 2) + m * 32 + 8 * g + 4 * lh);
      uint32_t cfail[TN];
#pragma unroll
      for (int n = 0; n < TN; ++n)
        cfail[n] = constraint_mask<16>(col[n], [&](int c) { return E.g + wm * (BM / 2) + m * 32 + acc_row(c, lh); });
      uint32_t fmask[TN] = {};  // EU: bit r = the lane's cell in row r of column n goes to the direct recompute
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const uint32_t lrow = wm * 32 + acc_row(r, lh);          // row of the 64-row key tile of this pass
        const uint32_t li = wm * (BM / 2) + m * 32 + acc_row(r, lh);
        const uint32_t gi = m0 + li;
#pragma unroll
        for (int n = 0; n < TN; ++n) {
          const uint32_t lc = wn * (BN / 2) + n * 32 + lr, gj = n0 + lc;
          bool flagged;
          const float w = visual_cell<EU>(p, acc[m][n][r], nav[r >> 2][r & 3], (cfail[n] >> r) & 1u, col[n], &kmax, &flagged);
          if constexpr (EU) fmask[n] |= (flagged && gi < N) ? (1u << r) : 0u;
          if constexpr (PART) {
            const uint32_t key = (w == w && gi < N) ? sa_f32_key(w) : 0xffffffffu;
            E.key[lrow * KS + lc] = key;
            if (key < ckey[n]) { ckey[n] = key; crow[n] = gi; }
          } else {
            if (gi < N && gj < TK) S.vis[(size_t)gi * TK + gj] = w;
          }
        }
      }
      if constexpr (EU) {
#pragma unroll
        for (int n = 0; n < TN; ++n) flag_cells<BN>(E, fmask[n], wm * 32 + 4 * lh, wn * (BN / 2) + n * 32 + lr);
      }
      if constexpr (PART) {
        if (m + 1 == TM) {
#pragma unroll
          for (int n = 0; n < TN; ++n) col_min_fold(E.ck + wn * (BN / 2) + n * 32 + lr, ckey[n], crow[n], lh);
        }
        fixup(m);
        rows_to_partials(m);
        if (m + 1 < TM) __syncthreads();  // the next pass overwrites the key tile
      } else fixup(m);
    }
  }
  if constexpr (PART) {
    // column partials, in k_bestfit_tile's layout with this plan's tile grid (S.CT = column tiles, S.RT = row tiles): complete
    // since the barrier of the last row pass.  (No max_dist slot in this mode: k_bestfit_resolve compares the weights themselves.)
    if (p.vote_words) flush_col_best<BN>(S, E.ck, n0);
    else
      for (uint32_t i = tid; i < (uint32_t)BN; i += NT) {
        const uint32_t gj = n0 + i;
        if (gj >= TK) continue;
        const unsigned long long k2 = E.ck[i];
        const bool has = k2 != ~0ull;
        S.col_part_w[(size_t)by * TK + gj] = has ? (double)sa_key_f32((uint32_t)(k2 >> 32)) : -1.0;
        S.col_part_q[(size_t)by * TK + gj] = has ? (uint32_t)k2 : SA_NONE;
      }
  }
  SA_STAMP(tr, 4);
  if constexpr (!PART) block_max_key(S.vis_max_key, key_slot, kmax);
  SA_STAMP(tr, 5);
}

// A 64 x 96 tile of the fused first phase: cosine, one observation per track, the BestFit vote reduced into the vote words (raw candidate
// rows: visual_cosine_tile's RAW / PART mode).  For frames whose 64 x 64 tiles would be one and
// a half rounds of the chip — 1000 detections against 1100 .. 1536 tracks: 272 .. 384 tiles, every CU that gets two of them runs twice as
// long as the others — 256 tiles of one and a half times the work each leave nothing unbalanced (sa_launch_frame_visual picks the form).
// Wave (wm, x) evaluates its 32 x 32 block of columns x 32 .. (16 cells per lane) and eight rows' worth of columns 64 .. 95 (8 cells).
constexpr EpiLds LDS96{64, 96, 1, true};
__device__ __forceinline__ void visual_tile96(const SceneDev& S, const SaParams& p, uint32_t bx, uint32_t by, float* lds) {
  constexpr int BM = 64, BN = 96, NT = 256;   // (threads of the block: k_frame_visual holds this tile to one k-group)
  uint64_t* tr = SA_TRACE_PTR();
  SA_STAMP(tr, 0);
  const uint32_t N = S.N, TK = S.TK;
  const uint32_t m0 = by * BM, n0 = bx * BN;
  if (m0 >= N || n0 >= TK) return;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w4 = (tid >> 6) & 3u;
  const uint32_t wm = w4 >> 1, wn = w4 & 1u, lr = lane & 31u, lh = lane >> 5;
  const TileRow row = tile_row_fetch<true>(S, BM, m0);
  const uint32_t lc0 = wn * 32u + lr, lc1 = 64u + lr;   // the lane's column of the 32 x 32 block, and of columns 64 .. 95
  const GemmCols col0 = tile_col_fetch(S, p, n0 + lc0, n0 + lc0 < TK), col1 = tile_col_fetch(S, p, n0 + lc1, n0 + lc1 < TK);
  f32x16 acc;
  float acc2[8];
  float nsq = 0.f;
  gemm_mainloop_ks96<3, true>((gfloat_p)S.c_feat_raw, (gfloat_p)S.t_ffrag, N, TK, S.Dp, m0, n0, lds, acc, acc2, tr, &nsq, p.ks_yield);
  SA_STAMP(tr, 3);
  const EpiTile E = epi_tile(LDS96, lds);
  for (uint32_t i = tid; i < (uint32_t)BN; i += NT) E.ck[i] = ~0ull;
  tile_rows_to_lds<BM, 1, true, true>(S, p, row, nsq, E);
  uint32_t kmax = 0;
  // the 32 x 32 block: registers 4g .. 4g+3 = tile rows wm 32 + 8g + 4 lh .. +3
  vote_cells<BN, 16, false>(p, E, wm * 32 + 4u * lh, lc0, m0, N, col0, [&](int i) { return acc[i]; }, &kmax);
  // this wave's half of columns 64 .. 95: accumulator registers 8 wn .. 8 wn + 7 (the column's other rows: wave (wm, 1 - wn) and the other wave row)
  vote_cells<BN, 8, false>(p, E, wm * 32 + 16u * wn + 4u * lh, lc1, m0, N, col1, [&](int i) { return acc2[i]; }, &kmax);
  SA_STAMP(tr, 6);
  __syncthreads();  // the key tile and the column minima complete
  const RowBest b = row_scan<BN, NT / 64>(E.key);   // four threads per row, 24 columns each
  if (b.seg == 0 && m0 + b.row < N) vote_row(S, m0 + b.row, n0, b);
  SA_STAMP(tr, 7);
  flush_col_best<BN>(S, E.ck, n0);
  SA_STAMP(tr, 4);
  SA_STAMP(tr, 5);
}

// The 64 x 64 tile of a LAZY first phase (no positional tiles, no preparation blocks: the launch is this tile and nothing else) with
// helper waves: cosine, one observation per track, the vote into the vote words — visual_cosine_tile's RAW / PART mode.
// A lone wave per SIMD spends ~8 k of a ~28 k-cycle tile life with its matrix pipe idle (profiles/r08_a_gemm_trace.txt):
// operand round trips in front of the first matrix instruction and dependent VALU / LDS chains behind the last, which no other block on
// the CU can cover.  Here a block holds 512 threads:
//   waves 0-3 (matrix): gemm_mainloop_ks<4, true, true> as in the one-wave form, and nothing in front of it;
//   waves 4-7 (helpers): meanwhile fetch and derive every row and column operand of the epilogue into LDS the exchange does not touch,
//                        then wait at the exchange's barriers — they never issue a matrix instruction;
//   all eight: the epilogue, half a 32 x 32 quadrant each (matrix wave w keeps accumulator registers 0 .. 7 of its quadrant and hands
//              8 .. 15 to helper w + 4 through LDS: kgroup_reduce_spread<2>'s layout, 8 cells per lane), then the row scan over 512 threads.
// LDS (floats): [0, 4224) the exchange, then [0, 2048) the hand-over | [2048, 6400) the key tile | [6400, 7424) the operands.
// TAIL: the block holds 1024 threads, the size the one-workgroup tail behind it is written for (k_frame_visual<.., HELP, TAIL>).  Waves 8-15
// (spare) take the helper side of every barrier and do no cell or scan work: the vote words are those of the 512-thread form, bit for bit.
constexpr uint32_t HELP_LDS_FLOATS = 7424;
template <bool TAIL = false>
__device__ __forceinline__ void visual_tile_helped(const SceneDev& S, const SaParams& p, uint32_t bx, uint32_t by, float* lds) {
  constexpr int BM = 64, BN = 64;
  uint64_t* tr = SA_TRACE_PTR();
  SA_STAMP(tr, 0);
  const uint32_t N = S.N, TK = S.TK;
  const uint32_t m0 = by * BM, n0 = bx * BN;
  if (m0 >= N || n0 >= TK) return;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, lr = lane & 31u, lh = lane >> 5;
  const uint32_t w8 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));   // wave-uniform: the two roles branch on scalars
  const uint32_t q = w8 & 3u, half = w8 >> 2;                  // the wave's quadrant (wm, wn) = (q >> 1, q & 1) and its half of it
  const uint32_t wm = q >> 1, wn = q & 1u;
  f32x4* s_hand = (f32x4*)lds;                                 // [4 quadrants][2][64 lanes] accumulator registers 8 .. 15
  float* s_us = lds + 6400;                                    // [BM] feature_can_be_used of the row (1 / 0)
  float* s_col = lds + 6784;                                   // [BN][8] nb, ok, cmax, -, geometry (GemmCols)
  EpiTile E{};                                                 // (np, flag, flist stay null: no k-groups and cosine only — k_frame_visual asserts !EU for HELP)
  E.key = (uint32_t*)(lds + 2048);                             // [64][key_stride] order-preserving keys of the tile's cells
  E.na = lds + 6464;                                           // [BM] squared norm of the row, NaN where the gate says no
  E.g = (sa_geo*)(lds + 6528);                                 // [BM]
  E.ck = (unsigned long long*)(lds + 7296);                    // [BN] (weight key << 32) | row, minimum per column
  static_assert(2048 + 64 * key_stride(BN) <= 6400 && 7296 + 2 * BN <= HELP_LDS_FLOATS && 4 * 4 * 64 * 4 + 4 * 32 <= 2048 + 64 * key_stride(BN), "the tile's LDS");
  f32x4 part[2];                                               // this wave's 8 cells: registers 8 half .. 8 half + 7 of the quadrant
  if (half == 0) {
    __builtin_amdgcn_s_setprio(1);                             // the matrix waves win the vector issue port while they share it
    f32x16 acc;
    float nsq = 0.f;
    gemm_mainloop_ks<4, true, true>((gfloat_p)S.c_feat_raw, (gfloat_p)S.t_ffrag, N, TK, S.Dp, m0, n0, lds, acc, tr, &nsq);
    __builtin_amdgcn_s_setprio(0);
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      s_hand[(q * 2 + g) * 64 + lane] = f32x4{acc[8 + 4 * g], acc[9 + 4 * g], acc[10 + 4 * g], acc[11 + 4 * g]};
      part[g] = f32x4{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
    }
    if (wn == 0 && lh == 0) E.na[wm * 32 + lr] = gated_norm(s_us[wm * 32 + lr], nsq);   // (the helpers wrote the gate before the exchange)
  } else {
    const uint32_t ht = tid - 256u;
    if (TAIL && w8 >= 8u) {   // (a spare wave: the barriers only)
    } else if (ht < (uint32_t)BM) {
      // row operands (what frame_prep_block derives for the candidate)
      float us = 0.f;
      sa_geo g{0.f, 0.f, 0.f, 0.f};
      if (m0 + ht < N) us = raw_row_usable(S, p, raw_row_fetch(S, m0 + ht), &g) ? 1.f : 0.f;
      s_us[ht] = us;
      E.g[ht] = g;
    } else if (ht < (uint32_t)(BM + BN)) {
      const uint32_t c = ht - BM;
      const GemmCols col = tile_col_fetch(S, p, n0 + c, n0 + c < TK);
      *(f32x4*)(s_col + 8 * c) = f32x4{col.nb, col.ok ? 1.f : 0.f, col.cmax, 0.f};
      *(sa_geo*)(s_col + 8 * c + 4) = col.g;
    } else if (ht < (uint32_t)(BM + 2 * BN)) {
      E.ck[ht - BM - BN] = ~0ull;
    }
    __syncthreads();   // gemm_mainloop_ks: the two k-halves meet
    __syncthreads();   // gemm_mainloop_ks: the exchange buffer is free
  }
  __syncthreads();     // the hand-over and the gated norms complete
  if constexpr (TAIL) {
    if (w8 >= 8u) {      // a spare wave: the key tile's barrier, and out (flush_col_best is threads 0 .. 63's)
      __syncthreads();
      return;
    }
  }
  if (half != 0) {
#pragma unroll
    for (int g = 0; g < 2; ++g) part[g] = s_hand[(q * 2 + g) * 64 + lane];
  }
  SA_STAMP(tr, 3);
  // the cells: registers 4g .. 4g+3 of this half = tile rows wm 32 + 8 (2 half + g) + 4 lh .. +3
  const uint32_t lc = wn * 32 + lr;
  GemmCols col;
  {
    const f32x4 c0 = *(const f32x4*)(s_col + 8 * lc);
    col.nb = c0[0];
    col.ok = c0[1] != 0.f;
    col.cmax = c0[2];
    col.g = *(const sa_geo*)(s_col + 8 * lc + 4);
  }
  uint32_t kmax = 0;
  vote_cells<BN, 8, false>(p, E, wm * 32 + 16u * half + 4u * lh, lc, m0, N, col, [&](int i) { return part[i >> 2][i & 3]; }, &kmax);
  SA_STAMP(tr, 6);
  __syncthreads();  // the key tile and the column minima complete
  const RowBest b = row_scan<BN, 8>(E.key);   // eight threads per row, 8 columns each
  if (b.seg == 0 && m0 + b.row < N) vote_row(S, m0 + b.row, n0, b);
  SA_STAMP(tr, 7);
  flush_col_best<BN>(S, E.ck, n0);
  SA_STAMP(tr, 4);
  SA_STAMP(tr, 5);
}

// Deeper banks (K = 2 .. SA_CLS_MAXK observations per track) WITHOUT the N x T x K weight matrix and without k_bestfit_tile: the
// whole-track tile of the fused frame launch.  A 64-column tile of the contraction holds the observations of floor(64 / K) WHOLE
// tracks (its first column is bank row bx floor(64 / K) K: the B operand stays one contiguous run of rows; the 64 mod K columns left
// over are computed and ignored — 1 of 64 at K = 3, 4 at K = 5), so every BestFit group (candidate, track) of the tile is complete
// inside it: the cells' weights go to an LDS tile instead of memory, and one thread per group adds the present ones up (f64, k
// ascending like the reference's sum) and counts them.  BestFit ranks a group by W = sum_k f64(max_dist - w_k) and max_dist is known
// only when every tile is done — but among groups with the SAME count c the heaviest is the one with the smallest sum.  So the tile
// reduces its groups per count class: 64-bit LDS minima of (order-preserving key of the f32 sum << 32 | index: lowest index on ties,
// as the reference orders exact ties) per row and per track, folded into the class words S.row_cls / S.col_cls with 64-bit atomic
// minima; the one-workgroup tail, which folds max_dist anyway, compares a row's (track's) class winners by W = c max_dist - sum.
// (W differs from the reference's sum of f32 differences by <= c/2 ulp of max_dist, 2e-7: the distances themselves are good to 1e-5.)
// The tiles stay as many and as independent as before (three per CU in flight at C2's size — a version that kept one 64 x 64 tile of
// (candidate, track) pairs per workgroup and ran the main loop K times lost exactly that: 44.7 us against 38.6 for the first phase).
// RAW rows only (the fused launch); EU: the flagged cells are recomputed directly (euclid_fixup), into the LDS tile.
template <bool EU, bool KSL = false>
__device__ __forceinline__ void visual_ktile(const SceneDev& S, const SaParams& p, uint32_t bx, uint32_t by, float* lds) {
  constexpr int BM = 64, BN = 64, NT = 256;   // (threads of the block: k_frame_visual holds this tile to one k-group)
  const uint32_t N = S.N, T = S.T, K = S.K, TK = S.TK;
  const uint32_t TPT = 64u / K, used = TPT * K;       // whole tracks per tile, columns they occupy
  const uint32_t m0 = by * BM, t0 = bx * TPT, n0 = t0 * K;
  if (m0 >= N || t0 >= T) return;
  const uint32_t key_slot = by * ((T + TPT - 1) / TPT) + bx;  // < S.nkeys (tiles of this scene in this mode)
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w4 = (tid >> 6) & 3u;
  const uint32_t wm = w4 >> 1, wn = w4 & 1u, lr = lane & 31u, lh = lane >> 5;
  const TileRow row = tile_row_fetch<true>(S, BM, m0);
  const uint32_t lc = wn * 32 + lr;
  const GemmCols col = tile_col_fetch(S, p, n0 + lc, lc < used && n0 + lc < TK);   // (columns past the tile's tracks: col.ok = false)
  f32x16 acc[1][1];
  float nsq = 0.f;
  if constexpr (KSL) gemm_mainloop_ks<4, true, true>((gfloat_p)S.c_feat_raw, (gfloat_p)S.t_ffrag, N, TK, S.Dp, m0, n0, lds, acc[0][0], nullptr, &nsq);
  else gemm_mainloop<BM, BN, 1, true>((gfloat_p)S.c_feat_raw, (gfloat_p)S.t_feat, N, TK, S.Dp, m0, n0, lds, acc, nullptr, &nsq);
  constexpr EpiLds L{BM, BN, 1, false};   // (no column minima; the key tile holds the cells' weights: f32 bits, NaN = absent)
  constexpr uint32_t KS = key_stride(BN);
  const EpiTile E = epi_tile(L, lds);
  uint32_t* s_w = E.key;
  unsigned long long* s_rc = (unsigned long long*)(lds + L.end());         // [64][K] row class words of the tile
  unsigned long long* s_cc = s_rc + 64 * SA_CLS_MAXK;                      // [TPT][K] track class words of the tile
  static_assert(L.end() + 2 * 64 * SA_CLS_MAXK + 2 * 64 <= 2 * (BM + BN) * BK, "the epilogue's tables must fit the stages");
  if constexpr (EU) flags_reset<BN, NT>(E);
  for (uint32_t i = tid; i < 64u * K; i += blockDim.x) s_rc[i] = ~0ull;
  if (tid < used) s_cc[tid] = ~0ull;
  tile_rows_to_lds<BM, 1, true, KSL>(S, p, row, nsq, E);
  uint32_t kmax = 0;
  const uint32_t row0 = wm * 32 + 4u * lh;
  const uint32_t fmask = tile_cells<16, EU>(p, E, row0, m0, N, col, [&](int i) { return acc[0][0][i]; }, &kmax, [&](uint32_t li, uint32_t gi, float w) {
    s_w[li * KS + lc] = __float_as_uint(gi < N ? w : __builtin_nanf(""));
  });
  if constexpr (EU) {
    flag_cells<BN>(E, fmask, row0, lc);
    euclid_fixup<BN, KSL>(S, p, E, S.c_feat_raw, n0, [&](uint32_t li) { return m0 + li; }, [&](uint32_t li, uint32_t lc2, uint32_t, float w) {
      const uint32_t key = w == w ? sa_f32_key(w) : 0u;
      s_w[li * KS + lc2] = __float_as_uint(w);
      kmax = key > kmax ? key : kmax;
    });
  }
  __syncthreads();  // the weight tile (and the reset class words) complete
  // one thread per group (row-major over the tile's tracks: a wave's LDS reads fall K words apart, conflict-free)
  const uint32_t mv = p.min_votes > 1u ? p.min_votes : 1u;
  for (uint32_t g2 = tid; g2 < 64u * TPT; g2 += blockDim.x) {
    const uint32_t grow = g2 / TPT, tr = g2 % TPT;
    const uint32_t gi = m0 + grow, gt = t0 + tr;
    if (gi >= N || gt >= T) continue;
    const uint32_t* wp = s_w + grow * KS + tr * K;
    double sum = 0.0;
    uint32_t cnt = 0;
    for (uint32_t k = 0; k < K; ++k) {
      const float w = __uint_as_float(wp[k]);
      if (w == w) { sum += (double)w; ++cnt; }
    }
    if (cnt >= mv) {
      const unsigned long long key = (unsigned long long)sa_f32_key((float)sum) << 32;
      atomicMin(&s_rc[grow * K + cnt - 1u], key | gt);
      atomicMin(&s_cc[tr * K + cnt - 1u], key | gi);
    }
  }
  __syncthreads();
  for (uint32_t i = tid; i < 64u * K; i += blockDim.x) {
    const unsigned long long v = s_rc[i];
    const uint32_t gi = m0 + i / K;
    if (v != ~0ull && gi < N) __hip_atomic_fetch_min(S.row_cls + (size_t)gi * K + i % K, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid < used) {
    const unsigned long long v = s_cc[tid];
    const uint32_t gt = t0 + tid / K;
    if (v != ~0ull && gt < T) __hip_atomic_fetch_min(S.col_cls + (size_t)gt * K + tid % K, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  block_max_key(S.vis_max_key, key_slot, kmax);
}

// (Tile order: row by row.  An XCD-aware band order — each XCD's L2 keeping one set of candidate panels — was measured at C5 with bands
// of 1, 2 and 4 tile rows: no difference, the 114 MB working set sits in the 256 MB Infinity Cache and the fabric keeps up.)
template <int BM, int BN, SaLoop LOOP, int KG, bool PART = false, bool EU = false>
__global__ __launch_bounds__((SaTileForm{BM, BN, LOOP, KG}.threads()), (SaTileForm{BM, BN, LOOP, KG}.min_blocks_per_cu())) void k_visual_cosine(const SceneDev* __restrict__ scenes, SaParams p, uint32_t gx, uint32_t gy,
                                                                          uint32_t xo_) {
  __shared__ __attribute__((aligned(16))) float lds[gemm_lds_floats(SaTileForm{BM, BN, LOOP, KG}, PART, EU)];
  const SceneDev S = scenes[blockIdx.z];  // by value: wave-uniform SGPRs, cannot alias the stores below
  uint32_t bx, by;  // XCD-aware tile order (xcd_order): a 1-D grid of 8 chunk workgroups per scene
  if (!xcd_tile(blockIdx.x, gx, gy, xo_ >> 8, xo_ & 255u, &bx, &by)) return;
  visual_cosine_tile<BM, BN, LOOP, KG, false, PART, EU>(S, p, bx, by, lds);
}
// The whole first phase of a VisualSORT frame in ONE heterogeneous launch: blockIdx.x <
//   n_gemm            : a 64x64 tile of the feature contraction (matrix cores; raw-feature mode, see visual_cosine_tile)
//   n_gemm + n_prep   : a frame-preparation block (padded features + norms for the upkeep and the taps, vote-state reset)
//   ...               : a 16x256 positional tile (f64 VALU + LDS: pair pre-filter, disjointness proofs, polygon clipping, edges)
// The three kinds are independent of each other, so the positional tiles and the preparation blocks fill the issue slots and
// the LDS the MFMA-bound contraction leaves idle on every CU instead of costing two more dependent launches.  Tiles are
// dispatched in blockIdx order: the contraction's (longest) first.  All kinds share ONE static LDS buffer (a kernel's
// static LDS is the sum of its arrays: separate arrays would cut the residency to one block per CU and serialise the kinds).
// HELP: a lazy frame's launch of contraction tiles alone, 512-thread blocks with helper waves (visual_tile_helped).
// TAIL: ... and the whole frame in this ONE launch: 1024-thread blocks, and the scene's LAST-ARRIVING block runs the one-workgroup tail
// (sa_tail.h) behind its tile.  Nobody waits, nobody spins, nobody fences:
//   every block   its tile's last vote-word atomic acknowledged (s_waitcnt vmcnt(0), every wave), a barrier, then ONE lane takes a ticket:
//                 a relaxed agent-scope add on shard blockIdx.x % 16 of the scene's ticket block (SA_TICKET_*: 16 shards + a top word, a
//                 128-byte line each — 256 blocks retiring onto ONE word would queue ~70 ns apiece at the memory side) and, where that add
//                 completes its shard, a second one on the top word;
//   the last one  the block whose top add completes the count: every tile's minima were acknowledged before the adds that lead up to
//                 its own, so the exchanges by which the tail fetches (and re-arms) the words see them all.  It zeroes the ticket
//                 block for the next frame (agent-scope stores; the kernel boundary stands between them and the next frame's adds).
//                 This two-level ticket (last arriver read from the value the TOP add returns, after a shard add) is NOT one of the
//                 hand-offs whose fence-free use has been measured elsewhere: those detect the last add on ONE unsharded counter, or poll
//                 sharded ones.  It rests on reasoning, not on a published guarantee: a tile's minima are acknowledged before its shard
//                 add is issued, the top add is issued only after the shard add has RETURNED, and minima, adds and exchanges are all
//                 atomics performed at the one coherence point of the device's memory side.  Whoever changes its shape has to redo
//                 that argument (and tests/test_one_launch.py holds both forms to the same vote words bit for bit).
// The vote words are the only bytes that cross workgroups in the launch, touched by 64-bit agent-scope atomics on both sides.  A block
// without a tile (idle in its XCD chunk, or past a smaller scene's edge) goes straight to the ticket.  px | py << 32 = done_seq here
// (no positional tiles in a HELP launch).  LDS: the tile's 29.7 KB (the tail's edge-gain pool inside them) + the tail's 120 KB: one block per CU.
template <bool PART, bool EU = false, bool KP = false, bool KSL = false, bool W96 = false, bool HELP = false, bool TAIL = false>
__global__ __launch_bounds__(TAIL ? SA_SMALL_N : HELP ? 512 : 256, W96 ? 4 : 1) void k_frame_visual(const SceneDev* __restrict__ scenes, SaParams p, uint32_t gx, uint32_t gy,
                                                           uint32_t px, uint32_t py, uint32_t nprep_, uint32_t xo_) {
  // nprep_: preparation blocks of the launch; bit 31: they run their RESET half only, bit 30: the positional tiles also feed the
  // many-workgroup tail (row-major edge lists, row duals, union-find: UNION) — frames beyond the one-workgroup tail's 1024 x 1024
  // bit 29: the positional tiles are 16 x 256 (launches whose blocks would not all be resident with 16 x 128 tiles: sa_launch_frame_visual)
  const uint32_t nprep = nprep_ & 0x1fffffffu;
  const bool prep_light = (nprep_ >> 31) != 0, uni = ((nprep_ >> 30) & 1u) != 0, wide = ((nprep_ >> 29) & 1u) != 0;
  using FusedPos = PosSmem<2, 64>;  // the wide, proof-filtered positional tile of this launch (sa_frame.h)
  using FusedPosW = PosSmem<4, 64>; // ... and its 16 x 256 form
  static_assert(sizeof(FusedPos) <= sizeof(float) * 2 * 128 * BK, "the positional tile must fit one k-group's stages");
  constexpr uint32_t POS_LDS = (sizeof(FusedPosW) + 15u) & ~15u;
  constexpr SaTileForm F{64, 64, KSL ? SaLoop::ksplit : SaLoop::staged, 1, KSL};   // the launch's contraction tile (one k-group: see sa_launch_frame_visual)
  constexpr uint32_t LDSP = (POS_LDS + 3u) / 4u > (uint32_t)(2 * (64 + 64) * BK) ? (POS_LDS + 3u) / 4u : (uint32_t)(2 * (64 + 64) * BK);
  constexpr uint32_t LDSF = HELP ? HELP_LDS_FLOATS : LDSP;
  __shared__ __attribute__((aligned(16))) float lds[LDSF];   // (35.6 KB with the 16 x 256 positional tile: four blocks per CU as before; HELP: 29.7 KB)
  static_assert(gemm_lds_floats(F, PART, EU) <= LDSF, "the contraction tile must fit the launch's LDS");
  static_assert(!W96 || (KSL && PART && !EU && !KP && SA_KS96_LDS <= LDSF && LDS96.flag() <= LDSF), "the 64 x 96 tile: cosine vote-word frames on the k-split loop");
  static_assert(!HELP || (PART && !EU && !KP && KSL && !W96), "helper waves: cosine vote-word tiles on the k-split loop");
  static_assert(!TAIL || (HELP && HELP_LDS_FLOATS * sizeof(float) >= 3072 * sizeof(int64_t)), "the tail behind helped tiles, its edge-gain pool inside their LDS");
  const SceneDev S = scenes[blockIdx.z];  // by value: wave-uniform SGPRs, cannot alias the stores below
  if constexpr (HELP) {   // (contraction tiles only)
    uint32_t tbx, tby;
    if (xcd_tile(blockIdx.x, gx, gy, xo_ >> 8, xo_ & 255u, &tbx, &tby)) visual_tile_helped<TAIL>(S, p, tbx, tby, lds);
    if constexpr (TAIL) {
      __shared__ uint32_t s_last;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's vote-word atomics have been acknowledged
      __syncthreads();                                    // ... and every wave's (the tile's LDS is dead from here on)
      if (threadIdx.x == 0) {
        uint32_t SA_G* const tk = S.stats + SA_TICKET_WORD0;
        const uint32_t shard = blockIdx.x % SA_TICKET_SHARDS;
        const uint32_t in_shard = (gridDim.x - shard + SA_TICKET_SHARDS - 1u) / SA_TICKET_SHARDS;   // blocks b of the scene with b % 16 == shard
        const uint32_t shards = gridDim.x < SA_TICKET_SHARDS ? gridDim.x : SA_TICKET_SHARDS;
        uint32_t last = 0u;
        if (__hip_atomic_fetch_add(tk + shard * SA_TICKET_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == in_shard)
          last = __hip_atomic_fetch_add(tk + SA_TICKET_SHARDS * SA_TICKET_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == shards ? 1u : 0u;
        s_last = last;
      }
      __syncthreads();
      if (!s_last) return;
      if (threadIdx.x <= SA_TICKET_SHARDS) __hip_atomic_store(S.stats + SA_TICKET_WORD0 + threadIdx.x * SA_TICKET_STRIDE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      // the tail (sa_tail.h): k_assign_small<true, true, 64, 1, true>'s statements, FUSED
      constexpr bool VISUAL = true, WORDS = true, LAZY = true, FUSED = true;
      constexpr int G = 64, TC = 1;
      const uint64_t done_seq = (uint64_t)px | ((uint64_t)py << 32);
      int64_t* const egain_ext = (int64_t*)lds;
#include "sa_tail_body.h"
    }
    return;
  }
  // Contraction tiles first in blockIdx order: the dispatcher hands blocks out in that order, breadth-first over the CUs, so
  // every CU starts with (at most) one contraction tile and fills its remaining slots with the other kinds.  Interleaving the
  // kinds (one contraction tile every k blocks) was measured: 32-50 us instead of 22.6; the other kinds FIRST (so that the positional tiles of a
  // frame with several rounds of contraction tiles do not queue behind them): C2 16.8 -> 17.5 us, three observations per track 40.9 -> 48.1.
  // xo_ = XcdOrder: chunk << 8 | W — the contraction's tiles in XCD-aware order (8 chunk workgroup slots, the last few possibly idle)
  uint32_t b = blockIdx.x;
  const uint32_t xchunk = xo_ >> 8, xW = xo_ & 255u;
  if (b < (xW ? 8u * xchunk : xchunk)) {
    uint32_t tbx, tby;
    if (!xcd_tile(b, gx, gy, xchunk, xW, &tbx, &tby)) return;
    if constexpr (W96) visual_tile96(S, p, tbx, tby, lds);         // (gx counts tiles of 96 columns here)
    else if constexpr (KP) visual_ktile<EU, KSL>(S, p, tbx, tby, lds);  // (gx counts tiles of floor(64 / K) whole tracks here)
    else visual_cosine_tile<F.bm, F.bn, F.loop, F.kg, true, PART, EU>(S, p, tbx, tby, lds);
    return;
  }
  b -= xW ? 8u * xchunk : xchunk;
  // the other two kinds are 256-thread units, one per block (threadIdx.x >> 8 is 0 here; the expressions are kept as the kernels have
  // always been compiled: the compiler does not fold them, and dropping them moves the register allocation of the whole kernel)
  const uint32_t unit = b + (threadIdx.x >> 8), tid = threadIdx.x & 255u;
#ifdef SA_GEMM_TRACE
  uint64_t* tr2 = g_trace_dev && blockIdx.x < 65536 ? g_trace_dev + 8 * blockIdx.x : nullptr;  // entry / exit of the other kinds
  if (tr2 && threadIdx.x == 0) { tr2[0] = __builtin_amdgcn_s_memtime(); tr2[1] = unit < nprep ? 2 : 1; }
#endif
  // preparation blocks (short) before the positional tiles (long): the tiles alone fill every slot the contraction leaves, and
  // preparation blocks queued behind them started only when the first tiles retired — the last thing to finish in the launch
  if (unit < nprep) frame_prep_block(S, p, unit, tid, prep_light);
  else if (unit - nprep < px * py) {
    unsigned char* pl = (unsigned char*)lds + (threadIdx.x >> 8) * POS_LDS;
    if (wide) positional_tile<false, true, 4, false, true, 64, true>(S, p, (unit - nprep) % px, (unit - nprep) / px, pl, tid);   // (never with the many-workgroup tail's extras)
    else if (uni) positional_tile<false, true, 2, true, true, 64, true>(S, p, (unit - nprep) % px, (unit - nprep) / px, pl, tid);
    else positional_tile<false, true, 2, false, true, 64, true>(S, p, (unit - nprep) % px, (unit - nprep) / px, pl, tid);
  }
#ifdef SA_GEMM_TRACE
  if (tr2 && threadIdx.x == 0) tr2[5] = __builtin_amdgcn_s_memtime();
#endif
}

// Direct sum (a-b)^2 on the vector pipe.  A 512-thread block computes 32 rows x 128 columns: wave w owns rows 4w .. 4w+3, lane l
// the columns l and l + 64 — 8 cells per thread, two partial sums per cell (even / odd k) so that every step is one packed
// subtract and one packed fused multiply-add (v_pk_add_f32 / v_pk_fma_f32: two f32 per lane per issue, 4-5 cycles per wave
// instruction measured, scripts/micro/pk_fma_rate.hip; the pipe's 157 TF/s is quoted on these).  What bounds such a kernel is
// operand delivery, not arithmetic: the first version (64 x 64 tile, 4 x 4 cells per thread, both operands through LDS) needs
// 8 ds_read_b128 per 64 packed instructions — exactly the 128 B/clk the LDS has when the vector pipe runs at full rate, so
// neither did (61.7 us at C2's size with scalar arithmetic, 38.7 packed; two LDS stages with fragment prefetch: 49.5).  Here the
// A operand never touches LDS or a vector register: a wave's 4 rows are the same for all its lanes, so their k-runs come through
// the SCALAR cache (s_load_dwordx8 from the constant address space) and enter the packed subtract as SGPR pairs (inline asm:
// left to itself the compiler subtracts the halves separately); only B goes through LDS, four ds_read_b128 per 64 packed
// instructions.  (Eight rows per wave halve that again but need 128 SGPRs for the two operand buffers: spilled through
// v_writelane.)  Eight waves per block: two per SIMD even when the frame is one block per CU.  Column stores of a wave cover
// 256-byte row segments.  35.3 us at C2's size (0.28 of the vector peak); with the scalar loads or the LDS reads taken out
// (wrong answers) 25.5 either way — what is left over the ~16 us of issue time is the two operand streams' round trips, which
// share one counter (lgkmcnt) and can only be awaited together; one column per lane (four waves per SIMD) 37.0, 4-float steps 35.7.
constexpr int EU_C = 2;                                          // columns per lane
constexpr int EU_BM = 32, EU_BN = 64 * EU_C, EU_R = 4, EU_THREADS = 512;  // EU_R rows per wave, EU_BM / EU_R waves
constexpr int EU_LDS_FLOATS = 2 * EU_BN * BK;
typedef const f32x4 __attribute__((address_space(4)))* kf32x4_p;
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef const f32x8 __attribute__((address_space(4)))* kf32x8_p;
__device__ __forceinline__ void euclid_mainloop(gfloat_p A, gfloat_p B, uint32_t M,
                                                uint32_t Ncols, uint32_t Dp, uint32_t m0, uint32_t n0, float* lds,
                                                float (&acc)[EU_R][EU_C]) {
  constexpr int STAGE = EU_BN * BK;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  f32x2 acc2[EU_R][EU_C];
#pragma unroll
  for (int i = 0; i < EU_R; ++i)
#pragma unroll
    for (int j = 0; j < EU_C; ++j) acc2[i][j] = f32x2{0.f, 0.f};
  // B rows of this block: 128 columns x 32 k per chunk = 1024 16-byte pieces, two per thread
  constexpr int NL = EU_BN * 8 / EU_THREADS;  // 16-byte pieces per thread per chunk
  gfloat_p pb[NL];
  uint32_t so[NL];
#pragma unroll
  for (int r = 0; r < NL; ++r) {
    const uint32_t c = tid + 512u * r, row = c >> 3, kc = c & 7u;
    uint32_t gb = n0 + row;
    gb = gb < Ncols ? gb : Ncols - 1;
    pb[r] = B + (size_t)gb * Dp + kc * 4u;
    so[r] = lds_off(row, kc);
  }
  // A rows of this wave (rows past the edge are clamped; their results are never stored)
  kf32x4_p ka[EU_R];
#pragma unroll
  for (int i = 0; i < EU_R; ++i) {
    uint32_t ga = m0 + (uint32_t)EU_R * w + i;
    ga = ga < M ? ga : M - 1;
    ka[i] = (kf32x4_p)(uintptr_t)(A + (size_t)ga * Dp);
  }
  const uint32_t nchunks = Dp / BK;
  f32x4 rb[NL];
#pragma unroll
  for (int r = 0; r < NL; ++r) rb[r] = *(gf32x4_p)pb[r];
#pragma unroll
  for (int r = 0; r < NL; ++r) *(f32x4*)(lds + so[r]) = rb[r];
  if (nchunks > 1) {
#pragma unroll
    for (int r = 0; r < NL; ++r) rb[r] = *(gf32x4_p)(pb[r] + BK);
  }
  __syncthreads();
  // one step = 8 k: four rows' runs as s_load_dwordx8 (32 SGPRs per buffer), two ds_read_b128 per column, 16 * EU_C packed
  // subtract / multiply-add pairs — long enough (~300 cycles) to cover the LDS and scalar-cache round trips of the next step's
  // operands, which share one counter (lgkmcnt) and can only be awaited together
  f32x4 fb[2][EU_C][2];
  f32x8 sa[2][EU_R];
  auto fetch = [&](auto buf_tag, const float* Bs, uint32_t k8) {  // k8 = index of the 8-float run along k (global)
    constexpr int buf = decltype(buf_tag)::value;
#pragma unroll
    for (int j = 0; j < EU_C; ++j)
#pragma unroll
      for (int h = 0; h < 2; ++h) fb[buf][j][h] = *(const f32x4*)(Bs + lds_off(lane + 64u * j, (2u * k8 + h) & 7u));
#pragma unroll
    for (int i = 0; i < EU_R; ++i) sa[buf][i] = ((kf32x8_p)ka[i])[k8];
  };
  auto compute = [&](auto cur_tag) {
    constexpr int cur = decltype(cur_tag)::value;
#pragma unroll
    for (int e = 0; e < 8; e += 2)
#pragma unroll
      for (int i = 0; i < EU_R; ++i)
#pragma unroll
        for (int j = 0; j < EU_C; ++j) {
          // a - b as ONE packed instruction with the SGPR pair as a source (left to itself the compiler subtracts the two
          // halves separately: 96 instructions per step instead of 64)
          const f32x2 av = f32x2{sa[cur][i][e], sa[cur][i][e + 1]};
          const f32x2 bv = f32x2{fb[cur][j][e >> 2][e & 3], fb[cur][j][e >> 2][(e & 3) + 1]};
          f32x2 df;
          asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(df) : "s"(av), "v"(bv));
          acc2[i][j] = __builtin_elementwise_fma(df, df, acc2[i][j]);
        }
  };
  using B0 = std::integral_constant<int, 0>;
  using B1 = std::integral_constant<int, 1>;
  fetch(B0{}, lds, 0);
  for (uint32_t c = 0; c < nchunks; ++c) {
    const float* Bs = lds + (c & 1u) * STAGE;
    float* nxt = lds + ((c + 1u) & 1u) * STAGE;
    const bool store = c + 1 < nchunks, load = c + 2 < nchunks;
    // two steps per trip of a ROLLED loop: the operand buffers stay compile-time constants, and the scheduler cannot hoist a
    // whole chunk's reads to the top
#pragma unroll 1
    for (uint32_t ks = 0; ks < 4; ks += 2) {
      fetch(B1{}, Bs, c * 4u + ks + 1);
      compute(B0{});
      if (ks == 0 && store) {
#pragma unroll
        for (int r = 0; r < NL; ++r) *(f32x4*)(nxt + so[r]) = rb[r];
        if (load) {
#pragma unroll
          for (int r = 0; r < NL; ++r) rb[r] = *(gf32x4_p)(pb[r] + (c + 2) * BK);
        }
      }
      if (ks + 2 < 4) fetch(B0{}, Bs, c * 4u + ks + 2);
      compute(B1{});
    }
    __syncthreads();  // the other stage is complete, and everyone is done reading this one
    if (store) fetch(B0{}, nxt, (c + 1) * 4u);
  }
#pragma unroll
  for (int i = 0; i < EU_R; ++i)
#pragma unroll
    for (int j = 0; j < EU_C; ++j) acc[i][j] = acc2[i][j][0] + acc2[i][j][1];
}

__global__ __launch_bounds__(EU_THREADS) void k_visual_euclid(const SceneDev* __restrict__ scenes, SaParams p) {
  constexpr int BM = EU_BM, BN = EU_BN;
  const SceneDev S = scenes[blockIdx.z];  // by value: wave-uniform SGPRs, cannot alias the stores below
  const uint32_t N = S.N, TK = S.TK, K = S.K;
  const uint32_t m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  if (m0 >= N || n0 >= TK) return;
  __shared__ __attribute__((aligned(16))) float lds[EU_LDS_FLOATS];
  float acc[EU_R][EU_C];
  euclid_mainloop((gfloat_p)S.c_feat, (gfloat_p)S.t_feat, N, TK, S.Dp, m0, n0, lds, acc);
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  const float nanv = __builtin_nanf("");
  const uint64_t epoch = S.epoch;
  uint32_t kmax = 0;
  // vote words (SaParams::vote_words; one observation per track, frame up to 1024 x 1024): no weight matrix — every row's and every
  // column's lightest weight, (order-preserving key << 32) | index, goes into S.row_best / S.col_best by 64-bit atomic minima, as
  // from the cosine contraction's epilogue.  Rows: a wave holds whole row segments (64 lanes x EU_C columns), so one wave
  // reduction per row; columns: in-lane over the wave's rows, then the eight waves meet in LDS (the stages are free now).
  const bool words = p.vote_words != 0;
  unsigned long long* s_col = (unsigned long long*)lds;
  unsigned long long cbest[EU_C];
#pragma unroll
  for (int j = 0; j < EU_C; ++j) cbest[j] = ~0ull;
  if (words) {
    __syncthreads();  // every wave is done with the stages
    for (uint32_t i = tid; i < (uint32_t)EU_BN; i += EU_THREADS) s_col[i] = ~0ull;
    __syncthreads();
  }
  // the two columns of this lane: their gates once, not once per row
  bool col_ok[EU_C];
  sa_geo tg[EU_C];
  uint64_t tep[EU_C];
#pragma unroll
  for (int j = 0; j < EU_C; ++j) {
    const uint32_t gj = n0 + lane + 64u * j;
    col_ok[j] = false;
    if (gj < TK) {
      const uint32_t t = gj / K;
      col_ok[j] = S.t_fpresent[gj] && S.t_fcount[t] >= p.min_track_len;
      tg[j] = sa_ldg(S.t_geo + t);
      tep[j] = S.t_epoch[t];
    }
  }
#pragma unroll
  for (int i = 0; i < EU_R; ++i) {
    const uint32_t gi = m0 + (uint32_t)EU_R * w + i;
    if (gi >= N) continue;
    const bool us = S.c_usable[gi] != 0;
    const sa_geo cg = sa_ldg(S.c_geo + gi);
#pragma unroll
    for (int j = 0; j < EU_C; ++j) {
      const uint32_t gj = n0 + lane + 64u * j;
      if (gj >= TK) continue;
      float out = nanv;
      if (us && col_ok[j] && sa_compatible(cg, epoch, tg[j], tep[j], p.max_idle, p.cons)) {
        const float d = sqrtf(acc[i][j]);
        if (d <= p.visual_threshold) {
          out = d;
          const uint32_t key = sa_f32_key(out);
          kmax = key > kmax ? key : kmax;
        }
      }
      if (!words) S.vis[(size_t)gi * TK + gj] = out;
      else acc[i][j] = out;
    }
  }
  if (!words) {
    block_max_key(S.vis_max_key, blockIdx.y * ((TK + BN - 1) / BN) + blockIdx.x, kmax);
    return;
  }
#pragma unroll
  for (int i = 0; i < EU_R; ++i) {
    const uint32_t gi = m0 + (uint32_t)EU_R * w + i;  // wave-uniform
    unsigned long long rbest = ~0ull;
    if (gi < N) {
#pragma unroll
      for (int j = 0; j < EU_C; ++j) {
        const uint32_t gj = n0 + lane + 64u * j;
        const float o = acc[i][j];
        if (gj < TK && o == o) {
          const unsigned long long k = (unsigned long long)sa_f32_key(o) << 32;
          rbest = (k | gj) < rbest ? (k | gj) : rbest;        // lowest column on ties
          cbest[j] = (k | gi) < cbest[j] ? (k | gi) : cbest[j];  // rows ascend with i: lowest row on ties
        }
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(rbest, o);
      rbest = other < rbest ? other : rbest;
    }
    if (lane == 0 && rbest != ~0ull) __hip_atomic_fetch_min(S.row_best + gi, rbest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
#pragma unroll
  for (int j = 0; j < EU_C; ++j)
    if (cbest[j] != ~0ull) atomicMin(&s_col[lane + 64u * j], cbest[j]);
  __syncthreads();
  for (uint32_t i = tid; i < (uint32_t)EU_BN; i += EU_THREADS) {
    const unsigned long long v = s_col[i];
    if (v != ~0ull && n0 + i < TK) __hip_atomic_fetch_min(S.col_best + n0 + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- standalone distance matrix (sa_feature_distance_matrix): no gating, plain d ----
template <int BM, int BN, SaLoop LOOP, int KG, bool BFRAG, bool AFRAG>
__global__ __launch_bounds__((SaTileForm{BM, BN, LOOP, KG}.threads())) void k_cosine_matrix(const float* __restrict__ A, const float* __restrict__ an,
                                                            const float* __restrict__ B, const float* __restrict__ bn,
                                                            uint32_t M, uint32_t Ncols, uint32_t Dp, float* __restrict__ out) {
  const uint32_t m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  uint64_t* tr = SA_TRACE_PTR();
  SA_STAMP(tr, 0);
  constexpr int TM = BM / 64, TN = BN / 64;
  // the k-split main loop (gemm_mainloop_ks) with B row-major / in fragment order / A in fragment order as well (the
  // stand-alone matrix entry point's measurement plans: sa_feature_distance_matrix reorders the operands it is asked to)
  constexpr bool KS = LOOP == SaLoop::ksplit;
  static_assert(KG == 1 || (TM == 1 && TN == 1), "k-groups only with the 64x64 tile");
  static_assert(!KS || (TM == 1 && TN == 1), "k-split only with the 64x64 tile");
  // (no zero-length array under the direct loop; the k-split loop keeps the two stages' 32 KB it has always been compiled with here)
  __shared__ __attribute__((aligned(16))) float lds[LOOP == SaLoop::direct ? 64 : KS ? 2 * (BM + BN) * BK : SaTileForm{BM, BN, LOOP, KG}.loop_lds_floats()];
  f32x16 acc[TM][TN];
  if constexpr (LOOP == SaLoop::ks128) gemm_mainloop_ks128<3>((gfloat_p)A, (gfloat_p)B, M, Ncols, Dp, m0, n0, lds, acc, tr);
  else if constexpr (LOOP == SaLoop::direct) gemm_mainloop_direct<BM, BN, 4>((gfloat_p)A, (gfloat_p)B, M, Ncols, Dp, m0, n0, acc, tr);
  else if constexpr (KS) gemm_mainloop_ks<4, false, BFRAG, AFRAG>((gfloat_p)A, (gfloat_p)B, M, Ncols, Dp, m0, n0, lds, acc[0][0], tr);
  else if constexpr (LOOP == SaLoop::ring) gemm_mainloop_ring<BM, BN>((gfloat_p)A, (gfloat_p)B, M, Ncols, Dp, m0, n0, lds, acc, tr);
  else gemm_mainloop<BM, BN, KG>((gfloat_p)A, (gfloat_p)B, M, Ncols, Dp, m0, n0, lds, acc, tr);
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w4 = (tid >> 6) & 3u, kg = tid >> 8;
  const uint32_t wm = w4 >> 1, wn = w4 & 1u, lr = lane & 31u, lh = lane >> 5;
  if constexpr (TM == 1 && TN == 1) {
    constexpr int R = 16 / KG;
    float part[R];
    kgroup_reduce_spread<KG>(acc[0][0], lds, part);
    SA_STAMP(tr, 3);
    const uint32_t gj = n0 + wn * 32 + lr;
    const float nb = bn[gj < Ncols ? gj : Ncols - 1];
    float na[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      uint32_t gi = m0 + wm * 32 + acc_row(kg * R + i, lh);
      na[i] = an[gi < M ? gi : M - 1];
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      uint32_t gi = m0 + wm * 32 + acc_row(kg * R + i, lh);
      if (gi < M && gj < Ncols) out[(size_t)gi * Ncols + gj] = part[i] / sqrtf(na[i] * nb);
    }
  } else {
    float nb[TN];
#pragma unroll
    for (int n = 0; n < TN; ++n) {
      uint32_t gj = n0 + wn * (BN / 2) + n * 32 + lr;
      nb[n] = bn[gj < Ncols ? gj : Ncols - 1];
    }
    float na[TM][16];
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        uint32_t gi = m0 + wm * (BM / 2) + m * 32 + acc_row(r, lh);
        na[m][r] = an[gi < M ? gi : M - 1];
      }
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        uint32_t gi = m0 + wm * (BM / 2) + m * 32 + acc_row(r, lh);
        if (gi >= M) continue;
#pragma unroll
        for (int n = 0; n < TN; ++n) {
          uint32_t gj = n0 + wn * (BN / 2) + n * 32 + lr;
          if (gj < Ncols) out[(size_t)gi * Ncols + gj] = acc[m][n][r] / sqrtf(na[m][r] * nb[n]);
        }
      }
  }
  SA_STAMP(tr, 4);
}

__global__ __launch_bounds__(EU_THREADS) void k_euclid_matrix(const float* __restrict__ A, const float* __restrict__ B, uint32_t M,
                                                       uint32_t Ncols, uint32_t Dp, float* __restrict__ out) {
  const uint32_t m0 = blockIdx.y * EU_BM, n0 = blockIdx.x * EU_BN;
  __shared__ __attribute__((aligned(16))) float lds[EU_LDS_FLOATS];
  float acc[EU_R][EU_C];
  euclid_mainloop((gfloat_p)A, (gfloat_p)B, M, Ncols, Dp, m0, n0, lds, acc);
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
#pragma unroll
  for (int i = 0; i < EU_R; ++i) {
    const uint32_t gi = m0 + (uint32_t)EU_R * w + i;
    if (gi >= M) continue;
#pragma unroll
    for (int j = 0; j < EU_C; ++j) {
      const uint32_t gj = n0 + lane + 64u * j;
      if (gj < Ncols) out[(size_t)gi * Ncols + gj] = sqrtf(acc[i][j]);
    }
  }
}

#ifdef SA_GEMM_TRACE
// dumps the stamps of the PREVIOUS launches when the call counter reaches $SA_GEMM_TRACE
static void sa_trace_hook(hipStream_t st, uint32_t nb) {
  static uint64_t* buf = nullptr;
  static int calls = 0;
  const char* env = getenv("SA_GEMM_TRACE");
  if (!env) return;
  if (!buf) {
    hipMalloc(&buf, 8 * 8 * 65536);
    hipMemset(buf, 0, 8 * 8 * 65536);
    hipMemcpyToSymbol(HIP_SYMBOL(g_trace_dev), &buf, sizeof(void*));
  }
  if (++calls != atoi(env)) return;
  hipStreamSynchronize(st);
  if (nb > 65536) nb = 65536;
  uint64_t* h = (uint64_t*)malloc((size_t)nb * 64);
  hipMemcpy(h, buf, (size_t)nb * 64, hipMemcpyDeviceToHost);
  if (FILE* f = fopen("gpurun_out/gemm_trace.txt", "w")) {
    for (uint32_t i = 0; i < nb; ++i)
      if (h[i * 8])
        fprintf(f, "%u %llu %llu %llu %llu %llu %llu %llu %llu\n", i, (unsigned long long)h[i * 8], (unsigned long long)h[i * 8 + 1],
                (unsigned long long)h[i * 8 + 2], (unsigned long long)h[i * 8 + 3], (unsigned long long)h[i * 8 + 4],
                (unsigned long long)h[i * 8 + 5], (unsigned long long)h[i * 8 + 6], (unsigned long long)h[i * 8 + 7]);
    fclose(f);
  }
  free(h);
}
#else
static inline void sa_trace_hook(hipStream_t, uint32_t) {}
#endif

// Tile extents the visual cost kernel will use for a batch with these maxima (the host needs them for the per-scene number of
// max-key slots, SceneDev::nkeys).
void sa_visual_tile(int visual_kind, bool eu_mfma, uint32_t maxN, uint32_t maxTK, uint32_t ns, uint32_t Dp, int32_t plan_override, uint32_t* bm, uint32_t* bn) {
  *bm = 64; *bn = 64;
  if (visual_kind == SA_VIS_EUCLIDEAN && !eu_mfma) { *bm = EU_BM; *bn = EU_BN; return; }  // k_visual_euclid's block tile (vis_max_key slots)
  if ((visual_kind != SA_VIS_COSINE && visual_kind != SA_VIS_EUCLIDEAN) || !maxN || !maxTK) return;
  const SaTileForm f = sa_tile_form(SaTileUse::cosine, tile_plan(maxN, maxTK, ns, Dp, plan_override));
  *bm = f.bm; *bn = f.bn;
}

// The fused first phase (k_frame_visual) applies when the contraction runs as 64 x 64 tiles — frames of up to two tiles per compute
// unit, where the other two kinds of work are a sizeable part of the frame and a dependent launch (~4 us) is a sizeable part of
// either — and the feature length needs no padding; any N, T: with more than 1024 detections or tracks the positional tiles of the
// launch feed the many-workgroup tail (UNION) instead of the one-workgroup one.  Where it does not apply, the frame's plan
// (sa_frame_plan) runs k_frame + k_visual_cost instead.
// (and with it, for banks of 2 .. SA_CLS_MAXK observations, the whole-track tiles and their class words)
bool sa_frame_visual_ok(uint32_t ns, uint32_t maxN, uint32_t maxT, uint32_t K, uint32_t D, const SaParams& p, bool class_words) {
  const uint32_t maxTK = maxT * K;
  const bool eu = p.visual_kind == SA_VIS_EUCLIDEAN && p.eu_mfma;
  if ((p.visual_kind != SA_VIS_COSINE && !eu) || !maxN || !maxTK || D != p.Dp) return false;
  // every plan of the 64 x 64 family: the launch runs one-k-group 64 x 64 tiles whatever the stand-alone kernel would do (frames of
  // several rounds of tiles — deeper banks: 1000 x 5000 columns at five observations per track — gain as well: 107.2 -> 102.5 us)
  if (sa_plan_is_64x64(tile_plan(maxN, maxTK, ns, p.Dp, p.gemm_plan))) return true;
  // deeper banks with class words: the whole-track tiles (64 x 64) replace THREE launches of the other family's path (positional
  // tiles, the contraction on wider tiles, k_bestfit_tile) — C2's frame with two observations per track: 42.9 us there.  (Only
  // with class words: the matrix mode's per-tile slots are laid out by the engine for the plan's own tile grid.)
  if (class_words && K >= 2 && K <= SA_CLS_MAXK) return true;
  // a frame of at most two 64 x 64 tiles per compute unit that the plan would give wider tiles (1000 detections x 1500 tracks: 64 x 128):
  // one launch less and the positional tiles beside the contraction weigh more than the wider tile's shorter main loop.  Vote-word
  // frames only (p.vote_words: the matrix mode's per-tile slots follow the plan's own grid).
  return p.gemm_plan < 0 && p.vote_words && K == 1 && (size_t)cdiv(maxN, 64) * cdiv(maxTK, 64) * ns <= 512;
}
// The launch's shape: its contraction tiles (their form and grid, XCD-aware numbering included) and its preparation blocks.
struct FvShape { bool kpass, eu, w96, help; uint32_t gx, gy, prep_blocks, xo_, n_gemm; };
static FvShape fv_shape(uint32_t ns, uint32_t maxN, uint32_t maxT, uint32_t K, const SaParams& p, const SaFramePlan& plan) {
  FvShape s{};
  const bool partials = plan.partials;
  s.kpass = plan.vote == SaVote::class_words;
  s.eu = p.visual_kind == SA_VIS_EUCLIDEAN && p.eu_mfma;
  const uint32_t maxTK = maxT * K;
  s.gy = cdiv(maxN, 64);
  // Tiles of 64 x 96 where they take fewer rounds of the chip's 256 CUs than 64 x 64 ones cost (one and a half times the work each): the
  // frames between one and one and a half rounds of 64 x 64 tiles — c2t, 1000 x 1500: 384 tiles, half the CUs with two; 256 of 64 x 96.
  // Cosine frames that vote through the vote words (visual_tile96); sa_config.gemm_plan = 19 + 1 pins the form (tests).
  if (!s.kpass && !s.eu && partials && p.vote_words && K == 1 && !p.staged_loop) {
    const size_t t64 = (size_t)cdiv(maxTK, 64) * s.gy * ns, t96 = (size_t)cdiv(maxTK, 96) * s.gy * ns;
    s.w96 = sa_plan_pins_w96(p.gemm_plan) || (p.gemm_plan < 0 && ((t96 + 255) / 256) * 3 < ((t64 + 255) / 256) * 2);
  }
  s.gx = s.kpass ? cdiv(maxT, 64u / K) : s.w96 ? cdiv(maxTK, 96) : cdiv(maxTK, 64);
  // preparation blocks: all of them (one wave per feature row: N / 4), the reset half only (one thread per row / column), or none
  s.prep_blocks = cdiv(maxN + maxT + 1, 256);
  if (plan.prep == SaPrep::all && cdiv(maxN, 4) > s.prep_blocks) s.prep_blocks = cdiv(maxN, 4);
  if (plan.prep == SaPrep::none) s.prep_blocks = 0;
  // (the fused launch numbers its contraction tiles in XCD-aware order by default: the same speed on every workload that takes it —
  // C2 20.3, c2t 36.1 / 36.4, c2k3 46.7 / 46.6, c2d 80.9, c2e 23.4 us either way — for a fifth fewer L2 fills; SA_FLAG_ROW_TILES: row by row)
  const XcdOrder xo = xcd_order(s.gx, s.gy, p.row_major_tiles == 2u);
  s.xo_ = (xo.chunk << 8) | xo.W;
  s.n_gemm = xo.W ? 8u * xo.chunk : xo.chunk;
  // a lazy frame whose launch is the contraction's tiles alone: the 512-thread tile with helper waves (visual_tile_helped)
  s.help = !s.kpass && !s.eu && !s.w96 && partials && p.lazy_pos && p.vote_words && K == 1 && !p.staged_loop && s.prep_blocks == 0;
  return s;
}
bool sa_frame_visual_helped(uint32_t ns, uint32_t maxN, uint32_t maxT, uint32_t K, const SaParams& p, const SaFramePlan& plan, uint32_t* blocks) {
  const FvShape s = fv_shape(ns, maxN, maxT, K, p, plan);
  *blocks = s.n_gemm * ns;
  return s.help;
}
hipError_t sa_launch_frame_visual(const SceneDev* scenes, uint32_t ns, uint32_t maxN, uint32_t maxT, uint32_t K, const SaParams& p_in,
                                  hipStream_t st, const SaFramePlan& plan, uint64_t done_seq) {
  const bool partials = plan.partials, kpass = plan.vote == SaVote::class_words, general_tail = plan.tail == SaTail::general;
  // The matrix waves of a one-observation cosine frame sleep 64 cycles after every k-step (SA_FLAG_NO_YIELD: never): while a wave presents
  // matrix instructions back to back, the positional tiles' waves on its SIMD issue no vector instruction at all (NOTES), and with the
  // k-split loop the contraction's tile retires ~3-6 k cycles BEFORE the positional tiles that end the launch — 32 naps hand them ~2 k
  // cycles of the port at the same cost to the tile that can afford it: C2 first phase -1.5 .. -5 % over three visits (c2n -1.5 %); euclidean
  // frames (a longer epilogue: +2.5 %) and deeper banks (several matrix waves per SIMD: no difference) do not take it.
  SaParams p_ = p_in;
  // A lazy frame (SaParams::lazy_pos) has no positional tiles in this launch: nothing to hand issue slots to, no naps.
  p_.ks_yield = (p_in.no_yield || p_in.lazy_pos || kpass || (p_in.visual_kind == SA_VIS_EUCLIDEAN && p_in.eu_mfma)) ? 0u : 1u;

  const SaParams& p = p_;
  const FvShape shape = fv_shape(ns, maxN, maxT, K, p, plan);
  const bool eu = shape.eu, w96 = shape.w96;
  const uint32_t gx = shape.gx, gy = shape.gy, prep_blocks = shape.prep_blocks, xo_ = shape.xo_, n_gemm = shape.n_gemm;
  const uint32_t py = p.lazy_pos ? 0u : cdiv(maxN, POS_TI);   // (lazy: the contraction's tiles and the preparation blocks only)
  if (plan.one_launch && !shape.help) return hipErrorInvalidValue;   // (the tail rides behind the helped tiles only: sa_one_launch)
  // (their matrix waves nap 128 cycles per k-step of 12 matrix instructions — such a frame brings three positional tiles per CU, which
  // end the launch: c2t first phase 24.4-25.0 us without naps, 23.9-24.3 with 64 cycles, 22.7-23.1 with 128, 23.0-23.2 with 192, 24.6 with
  // 256.  As compiled: with the nap's length chosen by a two-way branch instead of the loop's four-way one the 128-cycle form read 24.0 —
  // the scalar instructions between two k-steps are part of the gap the positional waves get)
  if (w96 && p_.ks_yield) p_.ks_yield = 1u | (2u << 8);
  uint32_t px = cdiv(maxT, 128);
  // Positional tiles of 16 x 256 where the launch's blocks would not all be resident with 16 x 128 (four blocks per CU: 1024) — deeper
  // banks, request sets of several scenes: a tile that has to wait for a place starts when the first contraction tiles retire.  Measured,
  // first phase: c2k3 37.1 -> 35.5 us, c2bk3 262 -> 253, c2d 69.3 -> 68.5.  Not where the tiles also feed the many-workgroup tail (row
  // duals, union-find: a 16 x 256 tile of THAT kind is a longer chain than two rounds of 16 x 128 — c2t 27.0 -> 29.2 us).
  const bool wide_pos = !general_tail && (size_t)(n_gemm + px * py + prep_blocks) * ns > 1024u;
  if (wide_pos) px = cdiv(maxT, 256);
  sa_trace_hook(st, n_gemm + px * py + prep_blocks);
  // One k-group (256-thread blocks, 32 KB of LDS for every kind of block: five blocks per CU).  With two k-groups the
  // contraction alone is faster (15 vs 20 us) but every block of the launch then owns 512 threads and 64 KB — a kernel's LDS is
  // per launch, not per block — so only two blocks fit a CU, and even with two positional / preparation units side by side in
  // each 512-thread block the latency-bound tiles, which want four or five blocks in flight per CU, queue: 30 us for the launch
  // against 22.7 (raising the contraction's wave priority changes nothing).
  const dim3 grid(n_gemm + px * py + prep_blocks, 1, ns);
  const uint32_t np = prep_blocks | (plan.prep == SaPrep::reset ? 0x80000000u : 0u) | (general_tail ? 0x40000000u : 0u) | (wide_pos ? 0x20000000u : 0u);
  // the contraction tiles' main loop: k-split over the bank's fragment-order twin by default, the LDS-staged loop with SA_FLAG_STAGED_LOOP
#define SA_FV(PART_, EU_, KP_) do { if (p.staged_loop) SA_LAUNCH((k_frame_visual<PART_, EU_, KP_, false>), grid, dim3(256), 0, st, scenes, p, gx, gy, px, py, np, xo_); \
                                    else SA_LAUNCH((k_frame_visual<PART_, EU_, KP_, true>), grid, dim3(256), 0, st, scenes, p, gx, gy, px, py, np, xo_); } while (0)
  if (kpass) {
    if (eu) SA_FV(false, true, true);
    else SA_FV(false, false, true);
    return hipGetLastError();
  }
  if (eu) {
    if (partials) SA_FV(true, true, false);
    else SA_FV(false, true, false);
  } else if (w96) SA_LAUNCH((k_frame_visual<true, false, false, true, true>), grid, dim3(256), 0, st, scenes, p, gx, gy, px, py, np, xo_);
  else if (shape.help && plan.one_launch)
    // ... and the tail behind them in the same launch: 1024-thread blocks, the scene's last-arriving block runs it (px, py: done_seq)
    SA_LAUNCH((k_frame_visual<true, false, false, true, false, true, true>), grid, dim3(SA_SMALL_N), 0, st, scenes, p, gx, gy, (uint32_t)done_seq,
              (uint32_t)(done_seq >> 32), np, xo_);
  else if (shape.help) SA_LAUNCH((k_frame_visual<true, false, false, true, false, true>), grid, dim3(512), 0, st, scenes, p, gx, gy, px, py, np, xo_);
  else if (partials) SA_FV(true, false, false);
  else SA_FV(false, false, false);
#undef SA_FV
  return hipGetLastError();
}

// The stand-alone launchers: ONE dispatch from the table row an entry point resolved (sa_tile_plan.h: what the plan numbers mean, which
// rows each entry point runs, tile_plan() + loop_plan() and their measurements) to the kernel of that row's form.  f(row constant) is
// compiled for the rows entry point U leaves alone — the kernels it instantiates — and for no others.
template <SaTileUse U, int I = 0, class Fn>
static inline void tile_dispatch(int row, Fn&& f) {
  constexpr int P = SA_TILE_PLANS[I].plan;
  if constexpr (sa_tile_row(U, P) == P) { if (row == P) return f(std::integral_constant<int, P>{}); }
  if constexpr (I + 1 < sizeof(SA_TILE_PLANS) / sizeof(SA_TILE_PLANS[0])) tile_dispatch<U, I + 1>(row, f);
}
// (the tiles of the stand-alone contraction in XCD-aware order)
template <SaTileUse U, bool PART, bool EU>
static void launch_contraction(uint32_t maxTK, uint32_t maxN, uint32_t ns, hipStream_t st, const SceneDev* scenes, const SaParams& p) {
  tile_dispatch<U>(sa_tile_resolve(U, maxN, maxTK, ns, p.Dp, p.gemm_plan, p.staged_loop != 0), [&](auto row) {
    constexpr SaTileForm F = sa_tile_form(U, decltype(row)::value);
    const uint32_t gx = cdiv(maxTK, F.bn), gy = cdiv(maxN, F.bm);
    const XcdOrder xo = xcd_order(gx, gy, p.row_major_tiles != 0);
    SA_LAUNCH((k_visual_cosine<F.bm, F.bn, F.loop, F.kg, PART, EU>), dim3(xo.W ? 8u * xo.chunk : xo.chunk, 1, ns), dim3(F.threads()), 0, st, scenes, p, gx, gy, (xo.chunk << 8) | xo.W);
  });
}
hipError_t sa_launch_visual(const SceneDev* scenes, uint32_t ns, uint32_t maxN, uint32_t maxTK, const SaParams& p,
                            hipStream_t st, bool partials) {
  if (!maxN || !maxTK) return hipSuccess;
  sa_trace_hook(st, cdiv(maxTK, 64) * cdiv(maxN, 64));
  const bool eu = p.visual_kind == SA_VIS_EUCLIDEAN && p.eu_mfma, cosine = p.visual_kind == SA_VIS_COSINE;
  if (eu && partials) launch_contraction<SaTileUse::euclid, true, true>(maxTK, maxN, ns, st, scenes, p);
  else if (eu) launch_contraction<SaTileUse::euclid, false, true>(maxTK, maxN, ns, st, scenes, p);
  else if (cosine && partials) launch_contraction<SaTileUse::cosine_partials, true, false>(maxTK, maxN, ns, st, scenes, p);
  else if (cosine) launch_contraction<SaTileUse::cosine, false, false>(maxTK, maxN, ns, st, scenes, p);
  else SA_LAUNCH(k_visual_euclid, dim3(cdiv(maxTK, EU_BN), cdiv(maxN, EU_BM), ns), dim3(EU_THREADS), 0, st, scenes, p);
  return hipGetLastError();
}

hipError_t sa_launch_distance_matrix(int kind, const float* a, const float* an, const float* b, const float* bn,
                                     uint32_t n, uint32_t t, uint32_t dp, float* out, hipStream_t st, int32_t plan_override) {
  if (!n || !t) return hipSuccess;
  sa_trace_hook(st, cdiv(t, 64) * cdiv(n, 64));
  // (cosine: b = the bank in fragment order where the form says so: sa_launch_frag_reorder; a as well)
  if (kind != SA_VIS_COSINE) hipLaunchKernelGGL(k_euclid_matrix, dim3(cdiv(t, EU_BN), cdiv(n, EU_BM)), dim3(EU_THREADS), 0, st, a, b, n, t, dp, out);
  else tile_dispatch<SaTileUse::matrix>(sa_tile_resolve(SaTileUse::matrix, n, t, 1, dp, plan_override, false), [&](auto row) {
    constexpr SaTileForm F = sa_tile_form(SaTileUse::matrix, decltype(row)::value);
    hipLaunchKernelGGL((k_cosine_matrix<F.bm, F.bn, F.loop, F.kg, F.b_frag, F.a_frag>), dim3(cdiv(t, F.bn), cdiv(n, F.bm)), dim3(F.threads()), 0, st, a, an, b, bn, n, t, dp, out);
  });
  return hipGetLastError();
}

// ---- track search: the contraction with a group epilogue (include/similari_search.h, launch 1) ----
// Rows are query observations (Kp per query track), columns stored observations (Kp per stored track).  Kp divides 32, so every
// Kp x Kp group of one query track and one stored track lies inside one tile of either kernel (64 x 64 cosine, 32 x 128 euclidean):
// the epilogue never combines across workgroups.  It stages the tile's distances in LDS (the main loop's stages are free by then),
// then: the self pair and absent cells are skipped; the tile's maximum of the remaining distances goes into the call's M by one
// device-scope atomicMax per workgroup on the order-preserving key; the kept cells of each group are counted (LDS atomics); the
// tile's surviving groups reserve their pool blocks with ONE atomicAdd on the cursor, record them in grp and write their cells
// (NaN where not kept).  Blocks past the pool are not written; the cursor counts on, and the host reruns with a pool that large.
// A stored track marked in a.s_out is withdrawn for the call (sa_store_search_stored): it pairs with no query, as the self pair.
//
// JOIN (the store against itself, rows and columns are the same slots, q and t are slot numbers): a group (q, t) is handled
// only when q < t, and stands for (t, q) as well — the distances are symmetric to the bit — so it counts, raises M and takes ONE pool
// block, whose number goes to grp[q][t] and grp[t][q]; launch 2 reads it row-major for q and column by column for t.  The tap gets
// both mirrored sets of cells.  A diagonal group (q == t) is a self pair: no group, cells to the tap.  Groups below the diagonal
// inside a tile that runs are left to the tile that holds their mirror.
//
// COMPAT (include/similari_attrs.h): liveness is a property of a group.  It is evaluated once per group (sa_compat.h) and
// kept in the top bits of the group's counter word — counts never exceed Kp^2 <= 1024, block numbers inside a tile never 4096 —
// before the cell loop; the cells of a group that is not live neither raise M nor count.  In a join a group carries one bit per
// direction: it counts once, raises M and takes ONE block if either direction is live, and its block number goes to grp[q][t] only if
// q -> t is live and to grp[t][q] only if t -> q is (SA_SEARCH_NONE otherwise).  The tap still gets every cell.
constexpr uint32_t SA_LIVE_FWD = 0x80000000u, SA_LIVE_BWD = 0x40000000u, SA_LIVE_BITS = SA_LIVE_FWD | SA_LIVE_BWD;

// the live bits of group (gq, gt), 0 for a group the tile does not own (out of range; in a join, on or below the diagonal)
template <bool JOIN>
__device__ __forceinline__ uint32_t compat_group_bits(const SaSearchArgs& a, const SaCompatArgs& c, uint32_t gq, uint32_t gt) {
  if (gq >= a.Q || gt >= a.T || (JOIN && gq >= gt)) return 0u;
  const sa_track_attrs qa = c.q_attrs[gq], ta = c.s_attrs[gt];
  uint32_t bits = sa_compat_live(c.flags, c.ready_at, qa, ta) ? SA_LIVE_FWD : 0u;
  if (JOIN && sa_compat_live(c.flags, c.ready_at, ta, qa)) bits |= SA_LIVE_BWD;
  return bits;
}

// Before the main loop of a compat tile without the tap: one workgroup-wide OR over the live bits of its groups.  When none is live
// the tile writes SA_SEARCH_NONE to exactly the grp words its epilogue would have written, counts itself in ctrl[2], adds nothing to M
// and the caller returns — without having read a feature row or a norm.  The decision is uniform: every thread takes the same branch.
template <int BM, int BN, int NT, bool JOIN>
__device__ __forceinline__ bool compat_tile_dead(const SaSearchArgs& a, const SaCompatArgs& c, uint32_t m0, uint32_t n0) {
  if (a.cells) return false;
  const uint32_t tid = threadIdx.x, lg = a.lgK;
  const uint32_t GC = (uint32_t)BN >> lg, G = ((uint32_t)BM >> lg) * GC;
  const uint32_t q0 = m0 >> lg, t0 = n0 >> lg;
  uint32_t any = 0;
  for (uint32_t g = tid; g < G; g += NT) any |= compat_group_bits<JOIN>(a, c, q0 + g / GC, t0 + g % GC);
  if (__syncthreads_or((int)(any != 0))) return false;
  for (uint32_t g = tid; g < G; g += NT) {
    const uint32_t gq = q0 + g / GC, gt = t0 + g % GC;
    if (gq >= a.Q || gt >= a.T) continue;
    if (!JOIN || gq <= gt) a.grp[(size_t)gq * a.T + gt] = SA_SEARCH_NONE;
    if (JOIN && gq < gt) a.grp[(size_t)gt * a.T + gq] = SA_SEARCH_NONE;
  }
  if (tid == 0) atomicAdd(a.ctrl + 2, 1u);
  return true;
}

template <int BM, int BN, int NT, bool JOIN = false, bool COMPAT = false>
__device__ __forceinline__ void search_epilogue(const SaSearchArgs& a, const SaCompatArgs& c, float* lds, uint32_t m0, uint32_t n0) {
  static_assert(NT % BN == 0, "a thread's cells must share one column");
  static_assert(!COMPAT || (BM * BN <= 4096), "a block number inside a tile must stay below the live bits");
  constexpr uint32_t CELLS = BM * BN;
  __shared__ uint32_t s_wmax[NT / 64], s_n, s_base;
  const uint32_t tid = threadIdx.x, lg = a.lgK, Kp = a.Kp;
  const uint32_t GC = (uint32_t)BN >> lg, G = ((uint32_t)BM >> lg) * GC;
  uint32_t* cnt = (uint32_t*)(lds + CELLS);   // [G] kept cells, then the group's pool block
  const uint32_t rows = a.Q << lg, cols = a.T << lg;
  const float nanv = __builtin_nanf("");
  const uint32_t q0 = m0 >> lg, t0 = n0 >> lg;
  for (uint32_t g = tid; g < G; g += NT) cnt[g] = COMPAT ? compat_group_bits<JOIN>(a, c, q0 + g / GC, t0 + g % GC) : 0u;
  if (tid == 0) s_n = 0;
  __syncthreads();
  const uint32_t j = tid % BN, gj = n0 + j;
  const bool col_in = gj < cols;
  const uint32_t t = gj >> lg, kb = gj & (Kp - 1u);
  const uint32_t t_nobs = col_in ? a.s_nobs[t] : 0u;
  const uint64_t t_id = col_in ? a.s_ids[t] : 0ull;
  const bool t_out = !JOIN && col_in && a.s_out && a.s_out[t];
  uint32_t kmax = 0;   // 0: no distance (below the key of any float)
  for (uint32_t c = tid; c < CELLS; c += NT) {
    const uint32_t i = c / BN, gi = m0 + i;
    if (!col_in || gi >= rows) continue;
    const uint32_t q = gi >> lg, ka = gi & (Kp - 1u);
    if (JOIN && q > t) continue;
    const float d = lds[c];
    const bool present = ka < a.q_nobs[q] && kb < t_nobs;
    if (a.cells && ka < a.K && kb < a.K) {
      a.cells[(((size_t)q * a.K + ka) * a.T + t) * a.K + kb] = present ? d : nanv;
      if (JOIN && q < t) a.cells[(((size_t)t * a.K + kb) * a.T + q) * a.K + ka] = present ? d : nanv;
    }
    if (!present || (JOIN ? q == t : a.q_ids[q] == t_id || t_out) || d >= a.keep_below) continue;
    if (COMPAT && !(cnt[(i >> lg) * GC + (j >> lg)] & SA_LIVE_BITS)) continue;   // the top bits do not change under the counting
    if (d == d) {
      const uint32_t key = sa_f32_key(d);
      kmax = key > kmax ? key : kmax;
    }
    if (d <= a.max_distance) atomicAdd(&cnt[(i >> lg) * GC + (j >> lg)], 1u);
  }
  const uint32_t wm = wave_max_u32(kmax);
  if ((tid & 63u) == 0) s_wmax[tid >> 6] = wm;
  __syncthreads();   // the counts and the wave maxima are complete
  if (tid == 0) {
    uint32_t b = 0;
    for (uint32_t w = 0; w < (uint32_t)NT / 64; ++w) b = s_wmax[w] > b ? s_wmax[w] : b;
    if (b) atomicMax(a.ctrl + 1, b);
  }
  for (uint32_t g = tid; g < G; g += NT) {
    const uint32_t gq = q0 + g / GC, gt = t0 + g % GC;
    uint32_t v = SA_SEARCH_NONE;
    if (COMPAT) {   // no live bit: nothing was counted; a surviving group keeps its bits beside its number inside the tile
      const uint32_t w = cnt[g];
      if (gq < a.Q && gt < a.T && (w & ~SA_LIVE_BITS) >= a.min_votes) v = atomicAdd(&s_n, 1u) | (w & SA_LIVE_BITS);
    } else if (gq < a.Q && gt < a.T && cnt[g] >= a.min_votes) v = atomicAdd(&s_n, 1u);   // JOIN: cnt is 0 unless gq < gt, min_votes >= 1
    cnt[g] = v;
  }
  __syncthreads();
  if (tid == 0) s_base = s_n ? atomicAdd(a.ctrl, s_n) : 0u;
  __syncthreads();
  for (uint32_t g = tid; g < G; g += NT) {
    const uint32_t gq = q0 + g / GC, gt = t0 + g % GC;
    if (gq >= a.Q || gt >= a.T) continue;
    const uint32_t w = cnt[g];
    const uint32_t v = w == SA_SEARCH_NONE ? SA_SEARCH_NONE : s_base + (COMPAT ? w & ~SA_LIVE_BITS : w);
    const bool fwd = !COMPAT || w == SA_SEARCH_NONE || (w & SA_LIVE_FWD), bwd = !COMPAT || w == SA_SEARCH_NONE || (w & SA_LIVE_BWD);
    if (!JOIN || gq <= gt) a.grp[(size_t)gq * a.T + gt] = fwd ? v : SA_SEARCH_NONE;
    if (JOIN && gq < gt) a.grp[(size_t)gt * a.T + gq] = bwd ? v : SA_SEARCH_NONE;
    cnt[g] = v;
  }
  __syncthreads();
  if (s_n == 0) return;
  for (uint32_t c = tid; c < CELLS; c += NT) {
    const uint32_t i = c / BN, gi = m0 + i;
    if (!col_in || gi >= rows) continue;
    const uint32_t slot = cnt[(i >> lg) * GC + (j >> lg)];
    if (slot == SA_SEARCH_NONE || slot >= a.pool_cap) continue;
    const uint32_t q = gi >> lg, ka = gi & (Kp - 1u);
    const float d = lds[c];
    const bool kept = ka < a.q_nobs[q] && kb < t_nobs && !(d >= a.keep_below) && d <= a.max_distance;
    a.pool[(size_t)slot * Kp * Kp + ka * Kp + kb] = kept ? d : nanv;
  }
}

// cosine: gemm_mainloop<64, 64, 1> on row-major operands, d = dot / sqrt(|a|^2 |b|^2) as k_cosine_matrix computes it.  gemm_mainloop
// forms its element offsets (row * Dp + k) in 32 bits, which a store of 2^32 floats and more would wrap: the tile hands it operands that
// start at its own first rows (64-bit offsets), so only in-tile offsets — below 64 Dp — reach the loop (sa_search_limits.h).
__device__ __forceinline__ uint32_t cdiv_dev(uint32_t a, uint32_t b) { return (a + b - 1u) / b; }

template <bool JOIN, bool COMPAT = false>
__device__ __forceinline__ void search_cosine_tile(const SaSearchArgs& a, const SaCompatArgs& c, uint32_t m0, uint32_t n0) {
  constexpr int BM = 64, BN = 64;
  if (COMPAT && compat_tile_dead<BM, BN, 256, JOIN>(a, c, m0, n0)) return;
  const uint32_t M = a.Q << a.lgK, N = a.T << a.lgK;
  __shared__ __attribute__((aligned(16))) float lds[2 * (BM + BN) * BK];
  f32x16 acc[1][1];
  gemm_mainloop<BM, BN, 1>((gfloat_p)(a.q_feat + (size_t)m0 * a.Dp), (gfloat_p)(a.s_feat + (size_t)n0 * a.Dp), M - m0, N - n0, a.Dp, 0u, 0u,
                           lds, acc);
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w4 = tid >> 6;
  const uint32_t wm = w4 >> 1, wn = w4 & 1u, lr = lane & 31u, lh = lane >> 5;
  const uint32_t j = wn * 32 + lr, gj = n0 + j;
  const float nb = a.s_norm[gj < N ? gj : N - 1];
  __syncthreads();   // every wave is done with the stages
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const uint32_t i = wm * 32 + acc_row(r, lh), gi = m0 + i;
    const float na = a.q_norm[gi < M ? gi : M - 1];
    lds[i * BN + j] = acc[0][0][r] / sqrtf(na * nb);
  }
  __syncthreads();
  search_epilogue<BM, BN, 256, JOIN, COMPAT>(a, c, lds, m0, n0);
}

// euclidean: euclid_mainloop, the direct sum (a - b)^2 of k_euclid_matrix
template <bool JOIN, bool COMPAT = false>
__device__ __forceinline__ void search_euclid_tile(const SaSearchArgs& a, const SaCompatArgs& c, uint32_t m0, uint32_t n0) {
  if (COMPAT && compat_tile_dead<EU_BM, EU_BN, EU_THREADS, JOIN>(a, c, m0, n0)) return;
  const uint32_t M = a.Q << a.lgK, N = a.T << a.lgK;
  __shared__ __attribute__((aligned(16))) float lds[EU_LDS_FLOATS];
  float acc[EU_R][EU_C];
  euclid_mainloop((gfloat_p)a.q_feat, (gfloat_p)a.s_feat, M, N, a.Dp, m0, n0, lds, acc);
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < EU_R; ++i)
#pragma unroll
    for (int j = 0; j < EU_C; ++j) lds[(EU_R * w + i) * EU_BN + lane + 64u * j] = sqrtf(acc[i][j]);
  __syncthreads();
  search_epilogue<EU_BM, EU_BN, EU_THREADS, JOIN, COMPAT>(a, c, lds, m0, n0);
}

// ---- the tile kernel: k_search_tile<EU, JOIN, COMPAT> ----
// What it receives: SaSearchArgs and nothing else, or — under a rule — SaSearchArgs then SaCompatArgs.
template <bool COMPAT>
struct SaTileArgs {
  SaSearchArgs a;
  SaCompatArgs c;
  __device__ __forceinline__ const SaCompatArgs& rule() const { return c; }
};
template <>
struct SaTileArgs<false> {
  SaSearchArgs a;
  __device__ __forceinline__ SaCompatArgs rule() const { return SaCompatArgs{}; }
};

// A search runs the rectangle, tile (blockIdx.y, blockIdx.x).  A join runs the same bodies on the store against itself: the workgroup
// index (over a two-dimensional grid: sa_join_tiles.h) is decoded to a tile on or above the diagonal, and the last grid row's workgroups
// past the tile count leave at once.  (The origin is found here and not in a helper of its own, and the bodies are called from here and
// not through one: either costs the join kernels the instruction-for-instruction identity with the forms they had under eight names.)
template <bool EU, bool JOIN, bool COMPAT>
__global__ __launch_bounds__(EU ? EU_THREADS : 256) void k_search_tile(SaTileArgs<COMPAT> k) {
  static_assert(EU_BN % EU_BM == 0, "the staircase of sa_join_tiles.h needs whole row tiles per column tile");
  constexpr uint32_t BM = EU ? (uint32_t)EU_BM : 64u, BN = EU ? (uint32_t)EU_BN : 64u;
  uint32_t ti = blockIdx.y, tj = blockIdx.x;
  if (JOIN) {
    const uint64_t idx = sa_join_grid_index(blockIdx.x, blockIdx.y, gridDim.x);
    if (idx >= sa_join_tile_count(cdiv_dev(k.a.T << k.a.lgK, BM), BN / BM)) return;
    sa_join_tile_decode(idx, BN / BM, &ti, &tj);
  }
  if constexpr (EU) search_euclid_tile<JOIN, COMPAT>(k.a, k.rule(), ti * BM, tj * BN);
  else search_cosine_tile<JOIN, COMPAT>(k.a, k.rule(), ti * BM, tj * BN);
}

template <bool EU, bool JOIN>
static hipError_t launch_search_tile(dim3 grid, const SaSearchArgs& a, const SaCompatArgs* c, hipStream_t st) {
  const dim3 block(EU ? EU_THREADS : 256);
  if (c) hipLaunchKernelGGL((k_search_tile<EU, JOIN, true>), grid, block, 0, st, SaTileArgs<true>{a, *c});
  else hipLaunchKernelGGL((k_search_tile<EU, JOIN, false>), grid, block, 0, st, SaTileArgs<false>{a});
  return hipGetLastError();
}

// ---- bf16 rows (include/similari_bf16.h): k_search_tile_bf16<JOIN, COMPAT> ----
// The cosine tile of a bf16 store: the same 64 x 64 tile, 256 threads, 2 x 2 waves of one 32 x 32 accumulator, the same write of the
// distances to LDS and the same epilogue as search_cosine_tile; only the main loop is new.  v_mfma_f32_32x32x16_bf16 takes from lane l
// row (l & 31), k = 8 (l >> 5) + j, j = 0 .. 7, of either operand: 16 contiguous bytes of a row-major bf16 row.  A fragment is
// therefore ONE 16-byte global load, with no transposition and no LDS stage, and the loop is a ring of BF_RING chunks of 32 k (two
// k-steps: an A and a B fragment each) in registers — the loads of chunk c + BF_RING are issued right behind the MFMAs of chunk c,
// so BF_RING - 1 chunks are in flight under every MFMA.  The two waves
// that share a row panel read it twice; the second read is an L1 / L2 hit.  C/D of this instruction is the layout acc_row describes
// (it does not depend on the input type), products of bf16 values are exact in f32, and A and B take the same k from the same lane,
// so the cell of (row i, column j) and the cell of (row j, column i) sum the same products in the same order: symmetric to the bit,
// as the join needs it.
// Operands start at the tile's first rows (64-bit offsets); inside the tile, offsets stay below 64 Dp elements.  Edge rows are clamped
// to the last row of their side, never read past the array.  Dp is a multiple of 32, so a chunk is whole; padding columns are zero
// (k_pad_rows, sa_devrows.hip).
//
// f16 rows (include/similari_f16.h) run the same body: v_mfma_f32_32x32x16_f16 has the operand and C/D layout of the bf16 instruction
// and products of f16 values (11 x 11 significant bits) are exact in f32 as well.  ELEM picks the instruction, nothing else.
//
// EU (f16 rows only): the euclidean distance as sqrt(|a|^2 + |b|^2 - 2 a.b) off the same loop.  The expansion cancels on near-identical
// rows, so a cell with d2 < rho s (s = |a|^2 + |b|^2, rho = x.rho: 5e-3 sqrt(Dp), the rule of visual_cell<EU>) is FLAGGED and recomputed
// as the direct sum of (a - b)^2 before the epilogue reads the tile.  Unlike a tracking frame, a search flags whole Kp x Kp groups (a
// query track and its stored twin) and, in a gallery of near-identical rows, whole tiles.  So the flagged cells go into a list in the
// upper half of the tile's LDS — free until the epilogue lays its group words there — that holds all 4096 cells of the tile: it
// cannot overflow and there is no second path.  A wave ballots each of its 16 accumulator registers into one flag word per row segment
// (32 columns of a row), reserves that many entries with one LDS atomic and its flagged lanes write their cells behind one another.
// The list is then dealt to the 32 groups of 8 lanes of the workgroup, a cell per group and turn: lane u of a group takes the 16-byte
// pieces u, u + 8, .. of both rows (L2-resident, the tile has just streamed them), sums (a_k - b_k)^2 in f32 in that fixed order, and
// three xor steps fold the group.  (a - b)^2 == (b - a)^2 and the order depends on k alone, so cell (i, j) and cell (j, i) get the
// same bits by either route, and a duplicate pair gives exactly 0.  A NaN never flags.  Rows and columns past the edge never flag.
// The tile's flagged cells and the tile itself are counted in x.ctr[0] and x.ctr[1] by one two-lane vector atomic.
//
// i8 rows (include/similari_i8.h; cosine only) run the same loop byte for byte: a 64-byte chunk of a row is 64 codes, consumed by two
// steps of v_mfma_i32_32x32x32_i8, whose operands are 16 bytes per lane as well — a 16-byte unit holds 16 elements in place of 8, so a
// row is Dp / 16 units and nch = Dp >> 6 (Dp is a multiple of 64).  Lane half lh of step s holds bytes 32 s + 16 lh .. + 15 of the
// chunk for A and for B alike: which 16 k's of the step the instruction pairs with a lane half does not matter to a dot product as long
// as both operands take the same bytes from the same lane and the halves cover the step.  The accumulators are i32 and exact
// (127^2 Dp < 2^31 for Dp <= 131072); C/D is the layout of acc_row, so the epilogue converts each and divides as the other forms do.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef const SA_AS1 u32x4* gu32x4_p;
constexpr int BF_RING = 4;

template <int ELEM, bool EU, bool JOIN, bool COMPAT = false>
__device__ __forceinline__ void search_tile_h16(const SaSearchArgs& a, const SaCompatArgs& c, const SaExpandArgs& x, uint32_t m0, uint32_t n0) {
  static_assert(ELEM == SA_ELEM_BF16 || ELEM == SA_ELEM_F16 || ELEM == SA_ELEM_I8, "16-bit rows or int8 codes");
  static_assert(!EU || ELEM == SA_ELEM_F16, "a bf16 store and an i8 store are cosine only");
  constexpr bool I8 = ELEM == SA_ELEM_I8;
  constexpr uint32_t LGU = I8 ? 4u : 3u;   // log2 of the elements of a 16-byte unit
  using elem_t = std::conditional_t<I8, uint8_t, uint16_t>;
  using acc_t = std::conditional_t<I8, i32x16, f32x16>;
  constexpr int BM = 64, BN = 64;
  if (COMPAT && compat_tile_dead<BM, BN, 256, JOIN>(a, c, m0, n0)) return;
  __shared__ uint32_t s_nf;   // EU: flagged cells of the tile
  if (EU && threadIdx.x == 0) s_nf = 0;
  const uint32_t M = a.Q << a.lgK, N = a.T << a.lgK, Dp = a.Dp;
  __shared__ __attribute__((aligned(16))) float lds[2 * BM * BN];   // the tile's distances, then the epilogue's group words (Kp = 1: one per cell)
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w4 = tid >> 6;
  const uint32_t wm = w4 >> 1, wn = w4 & 1u, lr = lane & 31u, lh = lane >> 5;
  const uint32_t ra = wm * 32 + lr, rb = wn * 32 + lr;   // this lane's operand rows inside the tile, clamped at the edge
  const uint32_t ca = m0 + ra < M ? ra : M - 1 - m0, cb = n0 + rb < N ? rb : N - 1 - n0;
  // 16-byte units: a row is Dp / 8 of them (i8: Dp / 16), this lane's fragment of k-step s of chunk ch is unit 4 ch + 2 s + lh of its row
  gu32x4_p pa = (gu32x4_p)((const SA_AS1 elem_t*)a.q_feat + (size_t)m0 * Dp) + (ca * (Dp >> LGU) + lh);
  gu32x4_p pb = (gu32x4_p)((const SA_AS1 elem_t*)a.s_feat + (size_t)n0 * Dp) + (cb * (Dp >> LGU) + lh);
  const uint32_t nch = Dp >> (LGU + 2u);
  u32x4 fa[BF_RING][2], fb[BF_RING][2];   // slot r holds chunk ch + r, ch a multiple of BF_RING
  auto load = [&](int r, uint32_t ch) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      fa[r][s] = pa[4 * ch + 2 * s];
      fb[r][s] = pb[4 * ch + 2 * s];
    }
  };
  acc_t acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0;
  auto mfma = [&](int r) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
      if constexpr (I8)
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4, fa[r][s]), __builtin_bit_cast(i32x4, fb[r][s]), acc, 0, 0, 0);
      else if constexpr (ELEM == SA_ELEM_F16)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fa[r][s]), __builtin_bit_cast(f16x8, fb[r][s]), acc, 0, 0, 0);
      else
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[r][s]), __builtin_bit_cast(bf16x8, fb[r][s]), acc, 0, 0, 0);
  };
  uint32_t ch = 0;
  if (nch >= 2 * BF_RING) {
    // Steady state: every chunk of a ring turn has a successor BF_RING chunks on.  The prologue and the body are free of branches, so
    // that the loop is ONE block and the compiler counts its waits (vmcnt(13) / vmcnt(14) ahead of an MFMA: the three younger
    // chunks stay in flight); with a guard around each load the counts merge to vmcnt(0) and every chunk drains the ring.
    // (sched_barrier: left alone, the scheduler issues the prologue's loads youngest chunk first and gathers a turn's loads behind its
    // MFMAs, and the turn then opens with vmcnt(0) all the same)
#pragma unroll
    for (int r = 0; r < BF_RING; ++r) {
      load(r, r);
      __builtin_amdgcn_sched_barrier(0);
    }
    for (; ch + 2 * BF_RING <= nch; ch += BF_RING) {
#pragma unroll
      for (int r = 0; r < BF_RING; ++r) {
        mfma(r);
        load(r, ch + r + BF_RING);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < BF_RING; ++r)
      if ((uint32_t)r < nch) load(r, r);
  }
  // the last turns (fewer than 2 BF_RING chunks; all of a short row): guarded, uniform branches (nch is a kernel argument's)
  for (; ch < nch; ch += BF_RING) {
#pragma unroll
    for (int r = 0; r < BF_RING; ++r) {
      if (ch + r >= nch) break;
      mfma(r);
      if (ch + r + BF_RING < nch) load(r, ch + r + BF_RING);
    }
  }
  const uint32_t j = wn * 32 + lr, gj = n0 + j;
  const float nb = a.s_norm[gj < N ? gj : N - 1];
  if constexpr (!EU) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint32_t i = wm * 32 + acc_row(r, lh), gi = m0 + i;
      const float na = a.q_norm[gi < M ? gi : M - 1];
      lds[i * BN + j] = (float)acc[r] / sqrtf(na * nb);   // i8: the exact integer converted once; a no-op otherwise
    }
    __syncthreads();
  } else {
    uint32_t* list = (uint32_t*)(lds + BM * BN);   // [BM * BN] the flagged cells, i * BN + j each
    __syncthreads();                               // s_nf is zero
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const uint32_t i = wm * 32 + acc_row(r, lh), gi = m0 + i;
      const float na = a.q_norm[gi < M ? gi : M - 1];
      const float s = na + nb, d2 = s - 2.0f * acc[r];
      const bool f = gi < M && gj < N && d2 < x.rho * s;   // a NaN compares false
      lds[i * BN + j] = sqrtf(d2 < 0.0f ? 0.0f : d2);      // NaN stays NaN
      const unsigned long long word = __ballot(f);         // two flag words: columns wn 32 .. + 31 of rows acc_row(r, 0) and acc_row(r, 1)
      if (word) {                                          // uniform
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(&s_nf, (uint32_t)__popcll(word));
        at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
        if (f) list[at + (uint32_t)__popcll(word & ((1ull << lane) - 1ull))] = i * BN + j;
      }
    }
    __syncthreads();   // the tile, the list and its length are complete
    const uint32_t nf = s_nf;
    if (nf) {
      gu32x4_p qa = (gu32x4_p)((const SA_AS1 uint16_t*)a.q_feat + (size_t)m0 * Dp);
      gu32x4_p qb = (gu32x4_p)((const SA_AS1 uint16_t*)a.s_feat + (size_t)n0 * Dp);
      const uint32_t sub = lane & 7u, units = Dp >> 3;
      for (uint32_t e = tid >> 3; e < nf; e += 32u) {
        const uint32_t cell = list[e];   // a flagged cell lies inside both edges: no clamping
        gu32x4_p ra = qa + (cell >> 6) * units, rb = qb + (cell & 63u) * units;
        float sum = 0.0f;
        for (uint32_t u = sub; u < units; u += 8u) {
          const f16x8 va = __builtin_bit_cast(f16x8, ra[u]), vb = __builtin_bit_cast(f16x8, rb[u]);
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float d = (float)va[k] - (float)vb[k];
            sum += d * d;
          }
        }
        sum += __shfl_xor(sum, 1);
        sum += __shfl_xor(sum, 2);
        sum += __shfl_xor(sum, 4);
        if (sub == 0) lds[cell] = sqrtf(sum);
      }
      if (tid < 2) atomicAdd(x.ctr + tid, tid ? 1ull : (unsigned long long)nf);
      __syncthreads();   // the recomputed cells are in the tile; the list is dead
    }
  }
  search_epilogue<BM, BN, 256, JOIN, COMPAT>(a, c, lds, m0, n0);
}

// the grid and the decoding of a join's workgroup index are those of k_search_tile<false, JOIN, COMPAT>
template <bool JOIN, bool COMPAT>
__global__ __launch_bounds__(256) void k_search_tile_bf16(SaTileArgs<COMPAT> k) {
  constexpr uint32_t BM = 64u, BN = 64u;
  uint32_t ti = blockIdx.y, tj = blockIdx.x;
  if (JOIN) {
    const uint64_t idx = sa_join_grid_index(blockIdx.x, blockIdx.y, gridDim.x);
    if (idx >= sa_join_tile_count(cdiv_dev(k.a.T << k.a.lgK, BM), BN / BM)) return;
    sa_join_tile_decode(idx, BN / BM, &ti, &tj);
  }
  search_tile_h16<SA_ELEM_BF16, false, JOIN, COMPAT>(k.a, k.rule(), SaExpandArgs{}, ti * BM, tj * BN);
}

// i8 rows: the same tiles and the same arguments (Dp counts elements, a multiple of 64)
template <bool JOIN, bool COMPAT>
__global__ __launch_bounds__(256) void k_search_tile_i8(SaTileArgs<COMPAT> k) {
  constexpr uint32_t BM = 64u, BN = 64u;
  uint32_t ti = blockIdx.y, tj = blockIdx.x;
  if (JOIN) {
    const uint64_t idx = sa_join_grid_index(blockIdx.x, blockIdx.y, gridDim.x);
    if (idx >= sa_join_tile_count(cdiv_dev(k.a.T << k.a.lgK, BM), BN / BM)) return;
    sa_join_tile_decode(idx, BN / BM, &ti, &tj);
  }
  search_tile_h16<SA_ELEM_I8, false, JOIN, COMPAT>(k.a, k.rule(), SaExpandArgs{}, ti * BM, tj * BN);
}

// f16 rows: the same tiles, either metric; the expansion's rho and counters ride behind the arguments of the other forms
template <bool COMPAT>
struct SaTileArgsF16 {
  SaTileArgs<COMPAT> t;
  SaExpandArgs x;
};

template <bool EU, bool JOIN, bool COMPAT>
__global__ __launch_bounds__(256) void k_search_tile_f16(SaTileArgsF16<COMPAT> k) {
  constexpr uint32_t BM = 64u, BN = 64u;
  uint32_t ti = blockIdx.y, tj = blockIdx.x;
  if (JOIN) {
    const uint64_t idx = sa_join_grid_index(blockIdx.x, blockIdx.y, gridDim.x);
    if (idx >= sa_join_tile_count(cdiv_dev(k.t.a.T << k.t.a.lgK, BM), BN / BM)) return;
    sa_join_tile_decode(idx, BN / BM, &ti, &tj);
  }
  search_tile_h16<SA_ELEM_F16, EU, JOIN, COMPAT>(k.t.a, k.t.rule(), k.x, ti * BM, tj * BN);
}

template <bool JOIN>
static hipError_t launch_search_tile_bf16(dim3 grid, const SaSearchArgs& a, const SaCompatArgs* c, hipStream_t st) {
  if (c) hipLaunchKernelGGL((k_search_tile_bf16<JOIN, true>), grid, dim3(256), 0, st, SaTileArgs<true>{a, *c});
  else hipLaunchKernelGGL((k_search_tile_bf16<JOIN, false>), grid, dim3(256), 0, st, SaTileArgs<false>{a});
  return hipGetLastError();
}

template <bool JOIN>
static hipError_t launch_search_tile_i8(dim3 grid, const SaSearchArgs& a, const SaCompatArgs* c, hipStream_t st) {
  if (c) hipLaunchKernelGGL((k_search_tile_i8<JOIN, true>), grid, dim3(256), 0, st, SaTileArgs<true>{a, *c});
  else hipLaunchKernelGGL((k_search_tile_i8<JOIN, false>), grid, dim3(256), 0, st, SaTileArgs<false>{a});
  return hipGetLastError();
}

template <bool EU, bool JOIN>
static hipError_t launch_search_tile_f16(dim3 grid, const SaSearchArgs& a, const SaCompatArgs* c, const SaExpandArgs& x, hipStream_t st) {
  if (c) hipLaunchKernelGGL((k_search_tile_f16<EU, JOIN, true>), grid, dim3(256), 0, st, SaTileArgsF16<true>{{a, *c}, x});
  else hipLaunchKernelGGL((k_search_tile_f16<EU, JOIN, false>), grid, dim3(256), 0, st, SaTileArgsF16<false>{{a}, x});
  return hipGetLastError();
}

hipError_t sa_launch_search_tiles(int kind, bool join, const SaSearchArgs& a, const SaCompatArgs* c, hipStream_t st, SaSearchTiles* out,
                                  int elem, const SaExpandArgs* x) {
  const bool eu = kind != SA_VIS_COSINE, bf16 = elem == SA_ELEM_BF16, f16 = elem == SA_ELEM_F16, i8 = elem == SA_ELEM_I8;
  if (eu && (bf16 || i8)) return hipErrorInvalidValue;
  if (!bf16 && !f16 && !i8 && elem != SA_ELEM_F32) return hipErrorInvalidValue;
  if (i8 && ((a.Dp & 63u) || a.Dp > SA_I8_MAX_FEATURE_LEN)) return hipErrorInvalidValue;   // whole 64-byte chunks; 127^2 Dp < 2^31
  if (eu && f16 && !(x && x->ctr)) return hipErrorInvalidValue;
  const uint32_t M = a.Q << a.lgK, N = a.T << a.lgK;
  const uint32_t bm = eu && !f16 ? (uint32_t)EU_BM : 64u, bn = eu && !f16 ? (uint32_t)EU_BN : 64u;   // the vector-pipe tile is the f32 store's alone
  dim3 grid(cdiv(N, bn), cdiv(M, bm));
  out->tiles = out->tiles_rect = M && N ? (uint64_t)grid.x * grid.y : 0;
  if (join) {
    out->tiles = sa_join_tile_count(cdiv(N, bm), bn / bm);   // up to 5.4e8 (N <= 65535 * 32, sa_search_limits.h): more than one grid dimension holds
    out->tiles_rect = sa_join_tile_rect(cdiv(N, bm), bn / bm);
    if (N && a.Q != a.T) return hipErrorInvalidValue;
    sa_join_grid(out->tiles, &grid.x, &grid.y);
  }
  if (!M || !N) return hipSuccess;
  if (bf16) return join ? launch_search_tile_bf16<true>(grid, a, c, st) : launch_search_tile_bf16<false>(grid, a, c, st);
  if (i8) return join ? launch_search_tile_i8<true>(grid, a, c, st) : launch_search_tile_i8<false>(grid, a, c, st);
  if (f16 && eu) return join ? launch_search_tile_f16<true, true>(grid, a, c, *x, st) : launch_search_tile_f16<true, false>(grid, a, c, *x, st);
  if (f16) return join ? launch_search_tile_f16<false, true>(grid, a, c, SaExpandArgs{}, st) : launch_search_tile_f16<false, false>(grid, a, c, SaExpandArgs{}, st);
  if (eu) return join ? launch_search_tile<true, true>(grid, a, c, st) : launch_search_tile<true, false>(grid, a, c, st);
  return join ? launch_search_tile<false, true>(grid, a, c, st) : launch_search_tile<false, false>(grid, a, c, st);
}
