// sa_merge_plan.h — which observation lands in which slot when banks are appended to or merged (include/similari_merge.h), and
// which tracks move when the merged-away ones leave.  Host arithmetic only, from ids, counts and qualities: sa_merge.hip turns the
// result into three launches, and tests/test_merge_plan.py compiles this header on the host against tests/merge_ref.py.
//
// A row is named by a 32-bit source word: a stored observation slot t * Kp + k (at most 2^31 - 1 of them, sa_search_limits.h), a
// staged new row (SA_MERGE_STAGED | index) or no row at all (SA_MERGE_ZERO: the slot ends zeroed, as an upsert leaves it).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#define SA_MERGE_STAGED 0x80000000u
#define SA_MERGE_ZERO 0xffffffffu

struct SaMergeObs {   // one observation of the concatenated bank: where its row lies, and its quality
  uint32_t src;
  float quality;
};
struct SaMergeRow {   // stored observation slot dst takes the row src names
  uint32_t dst, src;
};
struct SaMergeMove {  // the whole track at slot from moves to slot to
  uint32_t from, to;
};

// The retention rule over a concatenated bank of n observations: the indices kept, in their new order.  keep: 0 the last
// min(n, C) in their order; 1 stable by quality descending, the first min(n, C) (-0.0 == 0.0; no NaN: the caller refuses it).
static inline std::vector<uint32_t> sa_merge_select(uint32_t keep, uint32_t C, const std::vector<SaMergeObs>& bank) {
  const uint32_t n = (uint32_t)bank.size(), m = n < C ? n : C;
  std::vector<uint32_t> idx(n);
  std::iota(idx.begin(), idx.end(), 0u);
  if (keep == 0) return std::vector<uint32_t>(idx.end() - m, idx.end());
  std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return bank[a].quality > bank[b].quality; });
  idx.resize(m);
  return idx;
}

// One destination bank at stored slot `slot` that held old_n observations (fresh: the slot is new and holds anything, every one of
// its Kp rows is written).  bank: its own observations first (src = slot * Kp + k), then the sources' or the staged ones.  Appends the
// rows that change to `rows` — an observation that stays where it is costs nothing, slots from the new count up to the old one are
// zeroed — and writes the qualities of the new bank to quality_out[Kp] (0 past the count).  Returns the new count.
static inline uint32_t sa_merge_plan_bank(uint32_t keep, uint32_t C, uint32_t Kp, uint32_t slot, uint32_t old_n, bool fresh,
                                          const std::vector<SaMergeObs>& bank, std::vector<SaMergeRow>& rows, float* quality_out) {
  const std::vector<uint32_t> sel = sa_merge_select(keep, C, bank);
  const uint32_t m = (uint32_t)sel.size(), base = slot * Kp;
  for (uint32_t k = 0; k < m; ++k) {
    const SaMergeObs& o = bank[sel[k]];
    quality_out[k] = o.quality;
    if (fresh || o.src != base + k) rows.push_back({base + k, o.src});
  }
  for (uint32_t k = m; k < Kp; ++k) {
    quality_out[k] = 0.f;
    if (fresh || k < old_n) rows.push_back({base + k, SA_MERGE_ZERO});
  }
  return m;
}

// sa_store_remove(removed) in call order on a store of T tracks moves the last track into each hole in turn.  perm[p] = the original
// slot of the track that ends at slot p (T - removed.size() entries); moves = the entries with perm[p] != p.  Every move reads an
// original slot >= the final count and writes one below it, and no source repeats: a track moves only while it is the last one, which
// at the time of a removal lies at or beyond the final count, and so did wherever it came from.  The moves are independent.
static inline void sa_merge_compaction(uint32_t T, const std::vector<uint32_t>& removed, std::vector<uint32_t>& perm,
                                       std::vector<SaMergeMove>& moves) {
  std::vector<uint32_t> at(T), pos(T);   // at[p]: original slot now at p; pos[o]: where original slot o is now
  std::iota(at.begin(), at.end(), 0u);
  std::iota(pos.begin(), pos.end(), 0u);
  uint32_t n = T;
  for (const uint32_t o : removed) {
    const uint32_t p = pos[o], last = n - 1;
    if (p != last) {
      at[p] = at[last];
      pos[at[p]] = p;
    }
    --n;
  }
  at.resize(n);
  perm.swap(at);
  moves.clear();
  for (uint32_t p = 0; p < n; ++p)
    if (perm[p] != p) moves.push_back({perm[p], p});
}
