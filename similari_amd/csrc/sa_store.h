// sa_store.h — the feature store as its three host files see it: sa_search.hip (the store itself, sa_store_search_topn, launch 2),
// sa_gallery.hip (searches whose queries are stored tracks: include/similari_gallery.h) and sa_merge.hip (bank upkeep on the device:
// include/similari_merge.h), sa_attrs.hip (track attributes and what the *_compat calls share: include/similari_attrs.h) and
// sa_bestfit.hip (the BestFit vote as the second stage of a search: include/similari_bestfit.h), sa_devrows.hip (the one fill of padded rows, from
// the host or from device memory: include/similari_devrows.h) and sa_absorb.hip (a frame's tracks absorbed behind the vote: include/similari_absorb.h,
// under either retention rule: include/similari_retain.h) and sa_handover.hip (tracks handed from one store to another, the one-launch
// removal: include/similari_handover.h) and sa_consolidate.hip (a store's mutual best pairs merged behind the vote of its join:
// include/similari_consolidate.h) and sa_waste.hip (tracks that leave the engine's table enter a store: include/similari_waste.h).
// Private to the library.
#pragma once
#include "sa_engine.h"
#include "sa_search_limits.h"
#include "../../include/similari_attrs.h"
#include "../../include/similari_bestfit.h"
#include "../../include/similari_bf16.h"
#include "../../include/similari_f16.h"
#include "../../include/similari_devrows.h"
#include "../../include/similari_absorb.h"
#include "../../include/similari_retain.h"
#include "../../include/similari_i8.h"
#include "../../include/similari_handover.h"
#include "../../include/similari_consolidate.h"
#include "../../include/similari_waste.h"

#include <functional>
#include <unordered_map>
#include <vector>

constexpr uint32_t SA_TOPN_MAX = 64;

struct sa_store {
  sa_engine* e = nullptr;   // nullptr: the engine was destroyed first (sa_store_orphan)
  bool broken = false;      // a device call failed half-way through an upsert or remove: host tables and device arrays may disagree
  int device = 0;
  hipStream_t st = nullptr;
  int32_t kind = SA_VIS_COSINE;
  int32_t elem = SA_ELEM_F32;                     // the element type of feat, q_feat and the merge's staging rows (sa_bf16.hip), set once at creation
  uint32_t D = 0, Dp = 0, K = 1, Kp = 1, lgK = 0;
  uint32_t T = 0, cap = 0;                        // tracks, track capacity of the device arrays
  std::vector<uint64_t> ids;                      // slot -> id (the column order of a search)
  std::vector<uint32_t> nobs;                     // slot -> observations
  std::vector<float> qual;                        // [T * Kp] slot * Kp + k -> quality of observation k (0 past nobs and after an upsert)
  std::vector<sa_track_attrs> attrs;              // slot -> attributes ({0, 0, 0} until sa_store_set_attrs)
  bool attrs_dirty = true;                        // the table changed since d_attrs was written (only a *_compat search uploads it)
  bool qual_dirty = true;                         // qual changed since d_qual was written (only a SA_KEEP_BEST absorb uploads it): every writer of qual sets it
  std::unordered_map<uint64_t, uint32_t> slot_of;
  DevBuf feat, norm, d_ids, d_nobs;               // [cap * Kp][Dp] of elem, [cap * Kp] f32, [cap], [cap]
  DevBuf stage, up_slots;                         // a host-fed call's rows as the caller passed them ([rows read][D] f32: sa_rows_fill); an upsert's slots
  DevBuf q_feat, q_norm, q_ids, q_nobs;
  DevBuf d_attrs, q_attrs;                        // [cap] mirror of attrs, [Q] the queries' attributes: *_compat searches only
  DevBuf g_slots, s_out;                          // sa_store_search_stored: the queried slots [n], the withdrawn mark per stored track [T]
  DevBuf grp, pool, wscr, ctrl, cells, o_n, o_id, o_w;
  DevBuf fit, o_trk;                              // a BestFit search: col_key [T], col_q [T], {groups, claimed}; the tracks the rows name [Q][topn]
  uint32_t h_fit[2] = {0, 0};                     // groups, claimed as the last run counted them
  sa_bestfit_stats fit_last{};                    // sa_store_bestfit_last
  DevBuf m_new_feat, m_new_norm;                  // sa_merge.hip: appended rows, padded with norms
  DevBuf m_rows, m_moves, m_feat, m_norm;         // the plan's rewritten rows and net moves, the staging rows between gather and scatter
  sa_merge_stats merge_last{};
  uint32_t pool_cap = 0;                          // blocks of Kp * Kp floats
  uint32_t h_ctrl[3] = {0, 0, 0};                 // cursor, key of M, tiles skipped (a *_compat search)
  hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // call, launch 1, stage 2, end; [4], [5]: between the BestFit launches; [6], [7]: around an absorb's step
  sa_search_stats last{};
  uint64_t join_tiles = 0, join_tiles_rect = 0;   // launch 1 of the last join (sa_store_join_last)
  uint32_t join_blocks = 0;
  sa_compat_stats compat_last{};                  // launch 1 of the last *_compat search (sa_store_compat_last)
  DevBuf expand;                                  // an f16 euclidean store: [2] u64 the expansion's counters of launch 1 (SaExpandArgs::ctr)
  uint64_t h_expand[2] = {0, 0};
  sa_expand_stats expand_last{};                  // sa_store_expand_last (sa_f16.hip)
  DevBuf dr_table;                                // [rows] u32 the source row of each destination row, where the host names it (sa_rows_fill)
  sa_devrows_stats devrows_last{};                // sa_store_devrows_last
  DevBuf ab_slot, ab_cap;                         // an absorb (sa_absorb.hip): [Q] u32 the matched slot, then the destination slot, of each query; [Q] u32 the capacities
  sa_absorb_stats absorb_last{};                  // sa_store_absorb_last
  DevBuf d_qual, ab_qual;                         // [cap * Kp] f32 mirror of qual; [Q][Kp] f32 the qualities of an absorb's query rows: a SA_KEEP_BEST absorb only
  uint32_t retain_keep = 0;                       // sa_store_retain_last: the rule of the last absorb,
  uint64_t retain_upload = 0;                     // and the bytes of d_qual it uploaded
  hipEvent_t hev[4] = {nullptr, nullptr, nullptr, nullptr};   // sa_handover.hip, created on first use: around the fill of a hand-over into this store; around a timed compaction of this store
  sa_handover_stats handover_last{};              // sa_store_handover_last
  sa_consolidate_stats consolidate_last{};        // sa_store_consolidate_last (sa_consolidate.hip; its step keeps each track's partner slot in ab_slot, [T] u32)
  DevBuf w_rows, w_meta, w_table, w_feat;         // a waste (sa_waste.hip): [n] u32 the leaving rows of the engine's tables; [n] u32 counts then [n][Kp] f32 qualities; [n][Kp] u32 the row table; [n][Kp][engine Dp] f32 the captured rows
  hipEvent_t wev[2] = {nullptr, nullptr};         // ... around the capture launches, created on first use
  sa_waste_stats waste_last{};                    // sa_store_waste_last

  // A padded row in bytes, and in floats as the row movers count it (k_gather, k_merge_*: 16-byte pieces of a row of "Dp floats";
  // a bf16 or f16 row of Dp elements is a row of Dp / 2 floats to them, an i8 row — Dp a multiple of 64 — a row of Dp / 4: a multiple
  // of 16 each).  The host paths branch on elem here, where the store is created (Dp), where sa_rows_fill picks the instance
  // of k_pad_rows and sa_store_search_run the tile launcher, and where sa_store_fetch widens, nowhere else.  No mover does arithmetic on a norm:
  // norms are copied as 32-bit words, so the f32(integer) norms of an i8 store pass through them unchanged.
  bool half_rows() const { return elem == SA_ELEM_BF16 || elem == SA_ELEM_F16; }
  bool expands() const { return elem == SA_ELEM_F16 && kind == SA_VIS_EUCLIDEAN; }   // launch 1 is the expansion with its fix-up
  uint32_t elem_bytes() const { return elem == SA_ELEM_I8 ? 1u : half_rows() ? 2u : 4u; }
  size_t row_bytes() const { return (size_t)Dp * elem_bytes(); }
  uint32_t row_floats() const { return Dp / (4u / elem_bytes()); }

  // The slot table (sa_search.hip): T, ids, nobs, qual, qual_dirty, attrs, attrs_dirty and slot_of change together, through these three only.
  uint32_t slot_append(uint64_t id);              // a new track takes the next slot: no observations, qualities 0, attributes {0, 0, 0}
  void slot_move(uint32_t from, uint32_t to);     // slot `from` takes the place of `to`, whose id has left slot_of already
  void slot_truncate(uint32_t T1);                // the table shrinks to its first T1 slots
};

struct SaBestFit;   // the BestFit vote of a search (below)

// Where the feature rows of a call come from, in one of four forms:
//   HOST    f32 rows [sum n_obs][D] in the caller's host memory, as the calls of similari_search.h .. similari_bestfit.h take them
//           (base; null only where no row is read);
//   DEVICE  a *_dev call (include/similari_devrows.h): the caller's descriptor of rows in device memory, unchecked and possibly null
//           until sa_rows_check accepted it;
//   STORE   a hand-over (include/similari_handover.h, sa_handover.hip): rows of another store.  `table` names, per destination row of
//           the call ([n][Kp] of the store that reads them), the source's observation slot (slot << lgK) + k, SA_SEARCH_NONE for an
//           absent row.  The caller checked the source store and built the table from its host tables; only
//           sa_store_search_topn_impl and sa_store_absorb_impl take this form;
//   OWN     a waste (include/similari_waste.h, sa_waste.hip): f32 rows the library owns, base + r * stride elements is row r of a
//           staging block in device memory.  A search or an absorb reads d_table, on the device already: per destination row
//           [n][Kp] the block's row, SA_SEARCH_NONE for an absent one.  An append reads `table`, on the host: the block's row of
//           each new row, in the order of the call's rows.
struct SaRowSource {
  enum Kind { HOST, DEVICE, STORE, OWN };
  Kind kind = HOST;
  const void* base = nullptr;
  uint64_t stride = 0;
  const sa_dev_rows* dev = nullptr;
  const sa_store* store = nullptr;
  const std::vector<uint32_t>* table = nullptr;
  const uint32_t* d_table = nullptr;
  static SaRowSource of_host(const float* feats) { return SaRowSource{HOST, feats}; }
  static SaRowSource of_device(const sa_dev_rows* rows) { return SaRowSource{DEVICE, nullptr, 0, rows}; }
  static SaRowSource of_store(const sa_store* src, const std::vector<uint32_t>* table) { return SaRowSource{STORE, nullptr, 0, nullptr, src, table}; }
  static SaRowSource of_own(const void* base, uint64_t stride, const uint32_t* d_table, const std::vector<uint32_t>* table) {
    return SaRowSource{OWN, base, stride, nullptr, nullptr, table, d_table};
  }
};

// A source resolved for one call (sa_rows_prepare): what the one launch of sa_rows_fill reads — `rows` destination rows, row
// d_table[r] of each at base + d_table[r] * stride elements of type elem.
struct SaRows {
  const SaRowSource* src = nullptr;
  uint32_t rows = 0;
  size_t total = 0;                               // the rows that are read (the others are absent)
  int elem = SA_ELEM_F32;
  const void* base = nullptr;                     // nullptr: no row is read
  uint64_t stride = 0;
  const uint32_t* d_table = nullptr;
  const std::vector<uint32_t>* table = nullptr;   // the fill uploads it to d_table (dr_table) first; nullptr: d_table is the source's own
  std::vector<uint32_t> built;                    // ... where the call builds it (HOST, DEVICE)
};

#define SA_HIPCHK(e, call)                                                                                                  \
  do {                                                                                                                      \
    hipError_t _h = (call);                                                                                                 \
    if (_h != hipSuccess) return sa_engine_fail((e), SA_ERR_HIP, "%s failed: %s (%d)", #call, hipGetErrorString(_h), (int)_h); \
  } while (0)

// every entry point but destroy: a live, consistent store whose engine has drained
int sa_store_enter(sa_store* s, const char* what);
// the device arrays hold T1 tracks: capacity doubles, the rows stored so far move along (a failed allocation leaves the store as it was)
int sa_store_reserve(sa_store* s, uint64_t T1);
// d_ids / d_nobs from the host tables, queued on the store's stream
int sa_store_upload_table(sa_store* s);
// ---- the one way a store fills padded rows (sa_devrows.hip) ----
// The source's own refusal, at its place among a call's checks: every check of include/similari_devrows.h for a descriptor
// (sa_devrows_check), "null <name>" for host rows that are missing; the other two forms were checked by whoever built them.
// total == 0: nothing is read and nothing is looked at.
int sa_rows_check(sa_store* s, const char* what, const SaRowSource& src, size_t total, const char* name);
int sa_devrows_check(sa_store* s, const char* what, const sa_dev_rows* r, size_t total);
// The source row of each of n * Kp destination rows: observation k of track i -> row i * Kp + k; SA_SEARCH_NONE: an absent row.
void sa_devrows_table(uint32_t n, const uint32_t* n_obs, const uint32_t* index, uint32_t Kp, std::vector<uint32_t>& table);
// Everything of a fill that can fail without the device, behind the call's checks (the tables are sized by what the extent check
// accepted) and before it records ev[0]: the row table — banked: [n][Kp] for tracks of n_obs observations, as an upsert, a search
// and an absorb lay them; otherwise one row per observation, `total` of them, as an append stages them — and the buffers (dr_table
// for a table that goes up, `stage` for host rows, which go up as they are and are then an f32 block the library owns).
int sa_rows_prepare(sa_store* s, const SaRowSource& src, uint32_t n, const uint32_t* n_obs, size_t total, bool banked, SaRows& R);
// The uploads and ONE launch on the store's stream: R.rows padded rows of the store's element type into dst with their squared norms
// (row r -> slots[r / K] * K + r % K, or r).  k_pad_rows<source elem, store elem>; between two stores of one element type
// k_handover_rows, which copies rows and norm words (sa_handover.hip).  Stats: devrows_last for a descriptor; rows and launches_fill
// of handover_last, with hev[0] and hev[1] around the launch, for a store; none for host rows and rows the library owns.
int sa_rows_fill(sa_store* s, const SaRows& R, uint32_t K, const uint32_t* slots, void* dst, float* norms);
// ---- tracks handed from one store to another (sa_handover.hip) ----
// The two halves of sa_rows_fill that are the hand-over's: its stats and hev[0] ahead of the launch, and k_handover_rows from the
// banks of `from`, a store of s's element type, into [rows] padded rows of s's query side.
int sa_handover_fill_begin(sa_store* s, const std::vector<uint32_t>& table);
int sa_handover_copy(sa_store* s, const sa_store* from, const uint32_t* d_table, uint32_t rows, void* dst, float* norms);
// The tracks at `slots` (distinct, in call order) leave the store as sa_store_remove would take them one by one: the host tables
// move first, then the net moves of sa_merge_compaction run in ONE launch and the tables go up; the call waits.  timed: hev[2],
// hev[3] around the launch, *ms its time.  A device failure leaves the store broken.  Nothing to remove: nothing is queued.
int sa_store_remove_slots(sa_store* s, const std::vector<uint32_t>& slots, bool timed, uint32_t* launches, uint32_t* moved, double* ms);
// k_merge_compact (sa_merge.hip) for n net moves, which this uploads into m_moves first: queued on the store's stream
struct SaMergeMove;
int sa_store_launch_compact(sa_store* s, const SaMergeMove* moves, size_t n);
// the bodies of sa_store_upsert and sa_store_append (sa_search.hip, sa_merge.hip)
int sa_store_upsert_impl(sa_store* s, const char* what, uint32_t n, const uint64_t* ids, const uint32_t* n_obs, const SaRowSource& src);
int sa_store_append_impl(sa_store* s, const char* what, uint32_t keep, uint32_t n, const uint64_t* ids, const uint32_t* n_obs,
                         const SaRowSource& src, const float* quality, const uint32_t* capacity);
// sa_engine.hip: is [p, p + bytes) inside a block registered with sa_device_block_register?  *device: the block's
extern "C" __attribute__((visibility("hidden"))) bool sa_in_device_block(const void* p, size_t bytes, int* device);

// sa_store_create with an element type (sa_search.hip; sa_store_create_elem of sa_bf16.hip and sa_store_create_i8 of sa_i8.hip check
// what is theirs and call it)
int sa_store_create_as(sa_engine* e, const sa_store_options* o, int32_t elem, const char* what, sa_store** out);
// The ids of one call: none is 0 ("id 0 at <index>"), none comes twice.  slots (or nullptr: no look-up) takes each id's slot,
// SA_SEARCH_NONE for an id the store does not hold.  each(index): what the call site checks besides, run element by element behind the
// two shared checks (slots[index] is set by then), so that a call with several bad elements reports the first.
int sa_store_check_ids(sa_store* s, const char* what, uint32_t n, const uint64_t* ids, uint32_t* slots,
                       const std::function<int(uint32_t)>& each = nullptr);
// topn, max_distance and keep_below as every search accepts them
int sa_store_check_params(sa_store* s, const sa_topn_params* p, const char* what);
// The buffers both launches of a search of Q queries write (grp, ctrl, the outputs, the tap, a first pool), then — once the caller
// has recorded ev[0] and queued whatever fills the query side — the launches themselves, the pool's growth with its single rerun,
// the stats and the copies out.  join: the queries are the store (Q == T, q_* of the launch = the store's arrays, launch 1 runs the
// tiles on or above the diagonal only); s_out: the withdrawn mark per stored track, or nullptr.
// fit: nullptr — the vote is TopN, stage 2 is k_topn —, or the BestFit vote (SaBestFit below).
int sa_store_search_buffers(sa_store* s, uint32_t Q, uint32_t topn, bool tap, bool join, const SaBestFit* fit = nullptr);
// compat: nullptr (the plain calls), or the rule of a *_compat call as sa_store_check_compat accepted it: launch 1 is then the
// COMPAT form of the same tile, fed with q_attrs (a join: d_attrs) and d_attrs.
int sa_store_search_run(sa_store* s, const sa_topn_params* p, const char* what, uint32_t Q, bool join, const uint8_t* s_out,
                        uint32_t* out_n, uint64_t* out_winner, double* out_weight, float* out_cells, const sa_compat* compat = nullptr,
                        const SaBestFit* fit = nullptr);

// ---- the BestFit vote (sa_bestfit.hip): stage 2 of a search in place of k_topn ----
// What a search carries when its vote is BestFit.  out_winner of the call then takes the claim's outcome (o_id on the device),
// out_track — or nullptr — the stored ids the rows name (o_trk).
struct SaAbsorbStep;
struct SaBestFit {
  uint64_t* out_track = nullptr;
  const SaAbsorbStep* step = nullptr;   // the search is the first half of an absorb (sa_absorb.hip): what it adds to the body
};
// What sa_store_search_topn_impl, sa_store_join_topn_impl (a consolidation, sa_consolidate.hip) and sa_store_search_run call when the
// search carries a step.  check: the absorb's own refusals, behind
// the search's checks of its query list (host only).  prepare: behind every check and before anything is launched — the extent and
// the reservation for T + Q tracks, the step's buffers.  queue(voted): the step's launches on the store's stream, behind the vote of
// the run that fits the pool (voted) or — an empty store, nothing was searched — behind the padded queries; the caller waits.
struct SaAbsorbStep {
  std::function<int()> check, prepare;
  std::function<int(bool)> queue;
};
// fit (16 B per stored track and the two counters) and o_trk, sized for this call
int sa_bestfit_buffers(sa_store* s, uint32_t Q, uint32_t topn);
// the per-column state and the counters as a run finds them: no claim anywhere.  Queued at the start of every run, the rerun included.
int sa_bestfit_reset(sa_store* s);
// k_fit_weigh, k_fit_claim, k_fit_rank on the store's stream, ev[4] and ev[5] between them; q_ids: the queries' ids on the device
int sa_bestfit_launch(sa_store* s, bool join, uint32_t Q, uint32_t topn, const uint64_t* q_ids);

// ---- what the *_compat calls share (sa_attrs.hip) ----
// the rule itself: struct_size, known flag bits, DISJOINT without QUERY_FIRST; merge: ONLY_READY is refused too
int sa_store_check_compat(sa_store* s, const sa_compat* c, const char* what, bool merge);
// d_attrs holds the table (uploaded on the store's stream only if it changed since the last time); stats of the last compat search zeroed
int sa_store_compat_begin(sa_store* s);

// What the three searches do before they fill the query side, in this order: a live store (sa_store_enter), the rule
// (sa_store_check_compat) if the call has one, the params, the stats of the last compat search zeroed, bad_flags == 0 ("unknown flag
// bits"), Q == 0: done; no null_arg and no null output ("null argument"), no stray_attrs, queries() — the call's own checks of its query list, or
// nullptr —, the extent, the stats of the last search zeroed, and an empty store: done, the outputs of Q queries zeroed.  join: Q is
// the store's T, and an empty store leaves the outputs alone.  *run: the launches are to follow (false with SA_OK: the call is done).
struct SaSearchCall {
  const char* what = nullptr;
  const sa_topn_params* p = nullptr;
  bool ruled = false;                  // a *_compat call: compat is its rule, unchecked and possibly null
  const sa_compat* compat = nullptr;
  uint32_t bad_flags = 0;              // the bits of the call's flag word that it does not know
  bool join = false;
  uint32_t Q = 0;                      // queries (ignored by a join)
  bool null_arg = false;               // one of the call's own input pointers is null
  bool stray_attrs = false;            // query attributes came without a rule (a BestFit call, whose rule may be null)
  uint32_t* out_n = nullptr;
  uint64_t* out_winner = nullptr;
  double* out_weight = nullptr;
  const SaBestFit* fit = nullptr;      // the vote is BestFit: its stats are zeroed with the search's, its out_track with the outputs
};
int sa_store_search_begin(sa_store* s, const SaSearchCall& c, const std::function<int()>& queries, bool* run);

// The bodies behind a plain call, its *_compat twin and its *_bestfit form (fit; the vote is TopN without).  ruled == false: the plain call, which neither reads nor uploads attributes
// (compat is nullptr).  ruled: compat is the caller's rule, unchecked and possibly null; the body validates it right after it entered.
int sa_store_search_topn_impl(sa_store* s, const char* what, const sa_topn_params* p, bool ruled, const sa_compat* compat, uint32_t nq,
                              const uint64_t* q_ids, const uint32_t* q_n_obs, const SaRowSource& q_src, const sa_track_attrs* q_attrs,
                              uint32_t* out_n, uint64_t* out_winner, double* out_weight, float* out_cells, const SaBestFit* fit = nullptr);
int sa_store_search_stored_impl(sa_store* s, const char* what, const sa_topn_params* p, bool ruled, const sa_compat* compat, uint32_t flags,
                                uint32_t n, const uint64_t* ids, uint32_t* out_n, uint64_t* out_winner, double* out_weight, float* out_cells,
                                const SaBestFit* fit = nullptr);
int sa_store_join_topn_impl(sa_store* s, const char* what, const sa_topn_params* p, bool ruled, const sa_compat* compat, uint32_t* out_n,
                            uint64_t* out_winner, double* out_weight, float* out_cells, const SaBestFit* fit = nullptr);
int sa_store_merge_impl(sa_store* s, const char* what, bool ruled, const sa_compat* compat, uint32_t keep, uint32_t n_dst,
                        const uint64_t* dst_ids, const uint32_t* n_src, const uint64_t* src_ids, const uint32_t* capacity);
// the body of the absorb calls (sa_absorb.hip): the BestFit search of sa_store_search_topn_impl with the step behind its vote
int sa_store_absorb_impl(sa_store* s, const char* what, uint32_t keep, const sa_topn_params* p, const sa_compat* c, uint32_t nq,
                         const uint64_t* q_ids, const uint32_t* q_n_obs, const SaRowSource& src, const sa_track_attrs* q_attrs,
                         const float* quality, const uint32_t* capacity, uint32_t* out_n, uint64_t* out_winner, uint64_t* out_track,
                         double* out_weight, uint64_t* out_dest);
