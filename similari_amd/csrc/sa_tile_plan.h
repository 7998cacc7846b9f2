// sa_tile_plan.h — which tile and main loop a launch of the feature contraction runs (sa_gemm.hip), and what the plan numbers
// (sa_config.gemm_plan - 1) mean: ONE table, read by every entry point (no device code: host-only tests compile it on its own).
#pragma once
#include <cstddef>
#include <cstdint>

constexpr int SA_BK = 32;   // floats of k per step of every main loop

enum class SaLoop : uint8_t {
  staged,      // gemm_mainloop: both operands through XOR-swizzled LDS, two stages per k-group
  ring,        // gemm_mainloop_ring: one k-group, three stages
  ksplit,      // gemm_mainloop_ks (64 x 64): no LDS stage, the waves split k and exchange quadrants; operands row-major or in fragment order
  direct,      // gemm_mainloop_direct (the wider tiles): no LDS in the main loop; B in fragment order
  ks128,       // gemm_mainloop_ks128: the 64 x 128 tile's k-split loop (32 KB exchange); B in fragment order
};

struct SaTileForm {
  int bm, bn; SaLoop loop; int kg;   // kg: k-groups of 256 threads (the staged loop on 64 x 64 tiles; 1 everywhere else)
  bool b_frag, a_frag;               // the launch reads B / A in fragment order (sa_frag_index; B: the bank's fragment-order twin)
  constexpr uint32_t threads() const { return 256u * (uint32_t)kg; }
  constexpr uint32_t loop_lds_floats() const {   // (the k-split loop: four waves' 64 x 4 quadrant exchange + 4 x 32 norm partials)
    return loop == SaLoop::direct ? 0u : loop == SaLoop::ks128 ? 8192u : loop == SaLoop::ksplit ? 4u * 4u * 64u * 4u + 4u * 32u
         : (uint32_t)((loop == SaLoop::ring ? 3 : kg * 2) * (bm + bn) * SA_BK);
  }
  constexpr int min_blocks_per_cu() const { return loop == SaLoop::direct && bm == 128 && bn == 128 ? 2 : 1; }   // (__launch_bounds__)
  constexpr bool is_64x64() const { return bm == 64 && bn == 64; }
};

// The plan numbers.  Every number not listed is plan 1.  (10 / 13 / 17: the stand-alone matrix entry point's measurement plans —
// sa_feature_distance_matrix reorders the operands the form asks for.)
struct SaTilePlan { int plan; SaTileForm form; };
constexpr SaTilePlan SA_TILE_PLANS[] = {
  {0, {128, 128, SaLoop::staged, 1}},
  {1, {64, 64, SaLoop::staged, 1}},
  {2, {64, 64, SaLoop::staged, 2}},
  {4, {64, 64, SaLoop::staged, 4}},
  {5, {64, 128, SaLoop::staged, 1}},
  {6, {128, 64, SaLoop::staged, 1}},
  {7, {64, 64, SaLoop::ring, 1}},
  {8, {128, 128, SaLoop::ring, 1}},
  {9, {64, 64, SaLoop::ksplit, 1}},               // B row-major in the distance matrix; the frame's entry points read the twin (sa_tile_form)
  {10, {64, 64, SaLoop::ksplit, 1, true}},        // distance matrix only
  {13, {64, 64, SaLoop::ksplit, 1, true, true}},  // distance matrix only
  {15, {128, 128, SaLoop::direct, 1, true}},
  {16, {64, 128, SaLoop::direct, 1, true}},
  {17, {128, 64, SaLoop::direct, 1, true}},       // distance matrix only
  {18, {64, 128, SaLoop::ks128, 1, true}},
};
// 19: as 9, and pins the fused first phase's 64 x 96 tiles (sa_launch_frame_visual; tests)
constexpr bool sa_plan_pins_w96(int32_t plan_override) { return plan_override == 19; }

// The entry points of the contraction: the stand-alone kernel's weight matrix, its BestFit vote (partials / vote words), the euclidean
// expansion through it, and the stand-alone distance matrix.
enum class SaTileUse : uint8_t { cosine, cosine_partials, euclid, matrix };

// The table row an entry point runs for a plan number.  An entry point instantiates exactly the rows this leaves alone.
constexpr int sa_tile_row(SaTileUse u, int plan) {
  if (u == SaTileUse::cosine_partials) plan = plan == 4 ? 2 : plan == 7 ? 1 : plan == 8 ? 0 : plan;   // (four k-groups and the ring are weight-matrix tuning)
  // euclidean distances through the contraction: the one-k-group plans of every tile size (the k-group and ring plans are cosine tuning)
  if (u == SaTileUse::euclid) plan = plan == 8 ? 0 : (plan == 2 || plan == 4 || plan == 7) ? 1 : plan;
  if (u != SaTileUse::matrix && (plan == 10 || plan == 13 || plan == 17)) return 1;
  for (const SaTilePlan& r : SA_TILE_PLANS) if (r.plan == plan) return plan;
  return 1;
}
// ... and its form there (the frame's kernels read the bank through its fragment-order twin whenever the loop can: plan 9 too)
constexpr SaTileForm sa_tile_form(SaTileUse u, int plan) {
  SaTileForm f = SA_TILE_PLANS[1].form;
  for (const SaTilePlan& r : SA_TILE_PLANS) if (r.plan == sa_tile_row(u, plan)) f = r.form;
  if (u != SaTileUse::matrix && f.loop == SaLoop::ksplit) f.b_frag = true;
  return f;
}

// Tile plans: 0 = 128x128, 5 = 64x128, 6 = 128x64 (4 waves, one k-group), 1/2/4 = 64x64 with 1/2/4 k-groups.
// The contraction is matrix-core bound once every SIMD holds >= 2 waves, so a CU's time is (tiles it receives) x (tile
// area); the plan minimises ceil(tiles / 256 CUs) x area x (1 + 16/BM + 16/BN) — the last factor is the measured cost of
// the shorter MFMA runs between barriers on narrower tiles.  C5 (2000 x 5000): 128x128 gives 640 tiles = 2.5 per CU
// (3 rounds of 16384 cells), 64x128 gives 1280 = 5 per CU (5 rounds of 8192 cells) — 17 % less work on the critical CU.
// Frames that fit in one round of 64x64 tiles split k over 2 or 4 wave groups inside each workgroup so that every SIMD
// still holds 2-4 waves.
static inline int tile_plan(uint32_t M, uint32_t Ncols, uint32_t ns, uint32_t Dp, int32_t plan_override = -1) {
  if (sa_plan_pins_w96(plan_override)) return 9;   // (the fused first phase's 64 x 96 tiles pinned — everything else sees the 64 x 64 k-split plan)
  if (plan_override >= 0) return plan_override;    // sa_config.gemm_plan: tuning / tests
  const auto cdiv = [](uint32_t a, uint32_t b) { return (a + b - 1) / b; };
  struct Cand { int plan, bm, bn; };
  const Cand cands[4] = {{0, 128, 128}, {5, 64, 128}, {6, 128, 64}, {1, 64, 64}};
  int best = 1;
  double best_cost = 1e300;
  for (const Cand& c : cands) {
    const size_t tiles = (size_t)cdiv(M, c.bm) * cdiv(Ncols, c.bn) * ns;
    const double rounds = (double)((tiles + 255) / 256);
    const double cost = rounds * c.bm * c.bn * (1.0 + 16.0 / c.bm + 16.0 / c.bn);
    if (cost < best_cost) { best_cost = cost; best = c.plan; }
  }
  if (best != 1) return best;
  const size_t b64 = (size_t)cdiv(M, 64) * cdiv(Ncols, 64) * ns;
  const uint32_t nchunks = Dp / SA_BK;
  // two k-groups per tile only while a CU holds ONE tile (a lone wave per SIMD loses a third of the matrix pipe to its own LDS and memory
  // instructions, scripts/micro/mfma_side_mix.hip); from two co-resident tiles on, the second wave is there anyway and the split only adds the
  // reduction: 512 tiles (1000 x 2000 columns) 25.5 us with one group against 27.1 with two, 752 tiles (1000 x 3000) 33.0 against 40.3
  if (b64 <= 320 && nchunks >= 8) return 2;
  return 1;
}

// tile_plan() chooses among the tile SIZES; unless a plan is pinned or SA_FLAG_STAGED_LOOP is set, the frame's entry points then run
// 128x128 / 64x128 / 64x64 on the direct / k-split / k-split loops (measured on the stand-alone contraction, 4096 x 2048 x 512:
// 93.6 -> 74.6 us; 1000 x 1000 x 512: 15.0 -> 12.9; C5's frame with the 64x128 tile staged / direct / k-split: 657 / 632-642 / 617-619 us;
// 128x64 stays staged: two row-major gathers per fragment-order load are what the direct loop is worst at).
static inline int loop_plan(int plan, int32_t plan_override, bool staged_loop) {
  if (plan_override >= 0 || staged_loop) return plan;
  return plan == 0 ? 15 : plan == 5 ? 18 : (plan == 1 || plan == 2) ? 9 : plan;
}

// What an entry point launches for a request set of these maxima (M x Ncols cells per scene, ns scenes, Dp floats of k): the row of
// the table — the compile-time dispatch of sa_gemm.hip switches on it; sa_tile_form() of it is the form.  (The distance matrix keeps
// tile_plan()'s own staged choice: its operands are row-major unless a plan asks otherwise.)
static inline int sa_tile_resolve(SaTileUse u, uint32_t M, uint32_t Ncols, uint32_t ns, uint32_t Dp, int32_t plan_override, bool staged_loop) {
  const int plan = tile_plan(M, Ncols, ns, Dp, plan_override);
  return sa_tile_row(u, u == SaTileUse::matrix ? plan : loop_plan(plan, plan_override, staged_loop));
}
// The frame's tile extents (sa_visual_tile) are sa_tile_form(cosine, tile_plan()): its three entry points agree on them, and the main
// loop does not change them.  The 64 x 64 family (sa_frame_visual_ok): a plan of the table that the stand-alone contraction itself
// runs on 64 x 64 tiles — not the numbers it merely folds onto plan 1.
constexpr bool sa_plan_is_64x64(int plan) { return sa_tile_row(SaTileUse::cosine, plan) == plan && sa_tile_form(SaTileUse::cosine, plan).is_64x64(); }
