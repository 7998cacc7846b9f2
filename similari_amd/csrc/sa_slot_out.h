// sa_slot_out.h — the result block of one slot of a request set: mapped pinned memory that the assignment tail writes through its
// device view and the host reads in place.  This header is the layout's only home (host only, no HIP include):
//   ids[n] u64 | votes[n] u8 | (8-byte aligned) stats[4] u32 | winning columns[n] i32 | ... | completion word u64
// n = the slot's candidates, counted as 1 for an empty frame.  The completion word lies on a 128-byte line of its own behind the RESERVED
// extent (Slot::N_res): it moves only when that grows, and is cleared wherever it lands (a slot's earlier launches stored older sequence numbers).
#pragma once
#include <cstddef>
#include <cstdint>

namespace sa_slot_out {
enum Stat : uint32_t {   // the words of stats[4] (the fourth is spare)
  STAT_EUCLID_ILL = 0,   // a euclidean frame reported itself ill-conditioned for the matrix-core expansion
  STAT_GAVE_UP = 1,      // the assignment tail gave up waiting for its row workgroups: the frame's results are not valid
  STAT_LEFTOVER = 2,     // rows the visual vote left over (the next frame's positional mode goes by it)
  STAT_WORDS = 4
};
inline size_t count(size_t n) { return n ? n : 1; }
inline size_t ids_off(size_t) { return 0; }
inline size_t votes_off(size_t n) { return count(n) * 8; }
inline size_t stats_off(size_t n) { return (count(n) * 9 + 7) & ~(size_t)7; }
inline size_t cols_off(size_t n) { return stats_off(n) + STAT_WORDS * sizeof(uint32_t); }
inline size_t done_off(size_t n_res) { return (count(n_res) * 13 + 48 + 127) & ~(size_t)127; }   // (of the reserved count, like the size)
inline size_t bytes(size_t n_res) { return done_off(n_res) + 128; }
inline uint64_t* done_word(void* base, size_t off) { return (uint64_t*)((uint8_t*)base + off); }   // (off: done_off when the block was laid out)

// One block as its owner sees it: base = the host pointer, or the block's device view (then only the addresses are used).
struct View {
  uint8_t* base;
  size_t n;
  View(void* base_, size_t n_) : base((uint8_t*)base_), n(n_) {}
  uint64_t* ids() const { return (uint64_t*)(base + ids_off(n)); }
  uint8_t* votes() const { return base + votes_off(n); }
  uint32_t* stats() const { return (uint32_t*)(base + stats_off(n)); }
  int32_t* cols() const { return (int32_t*)(base + cols_off(n)); }
  bool gave_up() const { return n && stats()[STAT_GAVE_UP]; }   // (an empty frame runs no tail)
};
}  // namespace sa_slot_out
