// sa_plan.h — which launches a frame of a request set runs, decided once per frame on the host (no device code: host-only tests compile
// it on its own).  bank_prepare plans, enqueue_frame carries the plan out, the taps and the graph key read it (the lazy mode: sa_lazy.h).
#pragma once
#include "sa_lazy.h"

#define SA_SMALL_N 1024   // reach of the one-workgroup assignment tail (SaTail)
#define SA_SMALL_T 2048
#define SA_CLS_MAXK 8u    // deepest bank the class words serve

// How the BestFit vote reaches the assignment tail.  Vote words: the first phase reduces the vote into one 64-bit word per candidate and
// per track (atomic minima, free at tile retirement: scripts/micro/atomic_min.hip) and the tail reads them — the one-workgroup tail its
// two words per thread, the many-workgroup tail in its label kernel (k_assign_label<WORDS>) — no resolve launch, whatever the frame size.
enum class SaVote : uint8_t {
  resolve,      // per-tile partials or the weight matrix, then k_bestfit_resolve (SA_FLAG_SEPARATE_RESOLVE, and where no words apply)
  cell_words,   // one observation per track: the cost kernel itself, (key32 << 32 | index)
  tile_words,   // deeper banks through the weight matrix: k_bestfit_tile, (key54 << 10 | index) — a 10-bit index: frames up to 1024 x 1024
  class_words,  // deeper banks (2 .. SA_CLS_MAXK observations) through the whole-track tiles of the fused first phase: CLASS words (no
                // weight matrix, no k_bestfit_tile) wherever that launch applies
};
// The frame-preparation blocks of the first phase.  A LEAN frame leaves their candidate half out (C2: 23.0 -> 20.8 us per frame).  It
// derives the candidates' geometry / usability / padded features + norms; the positional tiles and the raw-row contraction derive what
// they need from the uploaded records themselves and, with vote words, nothing of the resolve kernel's state is touched — so on such
// frames nothing reads it.  What does (sa_tracks_apply's feature-bank step, the visual tap) calls ensure_prepped first.  The other half
// — the reset of the many-workgroup tail's per-row / per-column state — the one-workgroup tail does not need either (its state lives in
// LDS).  SA_FLAG_NEVER_LEAN: never lean.
enum class SaPrep : uint8_t {
  none,   // positional tiles only (a lean frame on the one-workgroup tail)
  all,    // positional tiles + preparation blocks
  only,   // preparation blocks only (what a lean frame left out, on demand: ensure_prepped)
  reset,  // positional tiles + the preparation blocks' RESET half only (a lean frame on the many-workgroup tail: a dozen blocks, not N / 4)
};
enum class SaTail : uint8_t {
  small,       // k_assign_small, one workgroup per scene, one column per thread: N, T <= SA_SMALL_N
  small_tc2,   // k_assign_small<.., TC = 2>, two columns per thread: N <= SA_SMALL_N, T <= SA_SMALL_T
  small2,      // k_assign_small2, two rows and two columns per thread: N, T <= SA_SMALL_T
  small2_1x4,  // k_assign_small2<.., 1, 4>, one row and four columns per thread: N <= SA_SMALL_N, T <= 2 SA_SMALL_T
  general,     // k_assign_label + k_assign_solve, many workgroups per scene
};

struct SaFramePlan {
  SaVote vote; SaPrep prep; SaTail tail;
  bool eu_mfma;        // the euclidean distances go through the matrix-core contraction
  bool partials;       // the contraction votes itself (no weight matrix): cosine or matrix-core euclidean, bank depth 1
  bool fused;          // the heterogeneous first phase (k_frame_visual), else k_frame + the stand-alone contraction
  bool lazy_possible;  // the frame's form has a lazy positional phase (sa_lazy_positional)
  bool lazy;           // ... and takes it: settled at launch time by the scenes' hints (bank_launch)
  bool reports_left;   // the tail writes each scene's leftover rows into out_stats[2] (k_assign_small with vote words, TC = 1)
  bool one_launch;     // a lazy frame whose tail rides in the first phase's launch, run by the scene's last-arriving block
                       // (k_frame_visual<.., HELP, TAIL>): settled with `lazy` at launch time (sa_one_launch)
};

struct SaPlanInputs {
  int32_t positional_kind, visual_kind;
  uint32_t flags, K, maxN, maxT;   // sa_config.flags, bank depth, the request set's largest scene
  bool bf_partials, bf_words_euclid, bf_tile_forced, eu_mfma_ok;  // the engine's capabilities (sa_engine)
  bool all_feats, backing_off;   // every scene of the set brings features; a scene of the set is backing off the euclidean expansion
  bool (*visual_ok)(const void* ctx, bool eu_mfma, bool vote_words, bool class_words);   // sa_frame_visual_ok (sa_gemm.hip) of this frame
  const void* ctx;
  uint32_t n_cu = 0;      // compute units of the device
  bool profile = false;   // the engine is being profiled kernel by kernel
};

static inline SaFramePlan sa_frame_plan(const SaPlanInputs& in) {
  const uint32_t f = in.flags;
  const bool visual = in.visual_kind != SA_VIS_NONE, general = (f & SA_FLAG_GENERAL_TAIL) != 0, small = in.maxN <= SA_SMALL_N && in.maxT <= SA_SMALL_N;
  SaFramePlan pl{};   // (vote: resolve)
  pl.eu_mfma = in.visual_kind == SA_VIS_EUCLIDEAN && in.eu_mfma_ok && !(f & SA_FLAG_EUCLID_VALU) && (!in.backing_off || (f & SA_FLAG_EUCLID_MFMA));
  pl.partials = in.bf_partials || (pl.eu_mfma && in.bf_words_euclid);
  if (visual && !(f & SA_FLAG_SEPARATE_RESOLVE)) {
    if (pl.partials || in.bf_words_euclid) pl.vote = SaVote::cell_words;
    else if (small && !general) pl.vote = SaVote::tile_words;
    if (pl.vote != SaVote::cell_words && in.K >= 2 && in.K <= SA_CLS_MAXK && !(f & SA_FLAG_SEPARATE_FRAME) && !in.bf_tile_forced &&
        in.all_feats && in.visual_ok(in.ctx, pl.eu_mfma, false, true))
      pl.vote = SaVote::class_words;
  }
  // (SA_FLAG_GENERAL_TAIL: the many-workgroup tail on small frames too — both tails must agree with the oracle.  Tile words: small frames only)
  if (general) pl.tail = SaTail::general;
  else if (in.maxN > SA_SMALL_N) pl.tail = in.maxN <= SA_SMALL_T && in.maxT <= SA_SMALL_T ? SaTail::small2 : SaTail::general;
  else if (in.maxT > SA_SMALL_T) pl.tail = in.maxT <= 2u * SA_SMALL_T ? SaTail::small2_1x4 : SaTail::general;
  else pl.tail = in.maxT > SA_SMALL_N ? SaTail::small_tc2 : SaTail::small;
  // Fused: contraction + positional tiles + preparation blocks in ONE launch (sa_frame_visual_ok).  Else (SA_FLAG_SEPARATE_FRAME too) k_frame,
  // then the stand-alone contraction, which reads the padded features, norms and gates: no lean frame there.
  pl.fused = pl.vote == SaVote::class_words ||
             (visual && !(f & SA_FLAG_SEPARATE_FRAME) && in.all_feats && in.visual_ok(in.ctx, pl.eu_mfma, pl.vote == SaVote::cell_words, false));
  const bool lean = !(f & SA_FLAG_NEVER_LEAN) && (!visual || (pl.vote != SaVote::resolve && pl.fused));
  pl.prep = !lean ? SaPrep::all : pl.tail == SaTail::general ? SaPrep::reset : SaPrep::none;
  pl.reports_left = visual && pl.vote != SaVote::resolve && pl.tail == SaTail::small;
  // (cosine only: a euclidean first phase ends with the flagged-cell recompute, not the positional tiles — c2e 22.1 us eager, 22.3 lazy)
  pl.lazy_possible = in.visual_kind == SA_VIS_COSINE && pl.vote == SaVote::cell_words && in.positional_kind == SA_POS_IOU && pl.tail == SaTail::small;
  return pl;
}

// One launch for a lazy frame.  helped: the first phase's launch is the helped contraction tiles and nothing else (sa_frame_visual_helped,
// sa_gemm.hip), blocks: how many of them the request set brings.  A block of that form holds 1024 threads and ~150 KB of LDS — one per
// compute unit: beyond the device's compute units they would queue behind each other.  A profiled engine keeps the two launches (figures
// per kernel need two kernels); SA_FLAG_SEPARATE_TAIL: always two (A/B, tests).  Asked for by SA_FLAG_ONE_LAUNCH: measured at C2
// the form is 0.1-0.2 us a step slower than the two launches, so it is nobody's default (NOTES section 0e).
static inline bool sa_one_launch(const SaFramePlan& pl, const SaPlanInputs& in, bool helped, uint32_t blocks) {
  return (in.flags & SA_FLAG_ONE_LAUNCH) && pl.fused && pl.lazy && pl.tail == SaTail::small && helped && !in.profile && !(in.flags & SA_FLAG_SEPARATE_TAIL) && blocks <= in.n_cu;
}
