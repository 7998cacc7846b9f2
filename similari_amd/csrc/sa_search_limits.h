// sa_search_limits.h — the extents a track search can index.  Host arithmetic only: sa_search.hip refuses a store or a search beyond them
// with SA_ERR_UNSUPPORTED, and tests/test_search_limits.py compiles this header on the host and probes its edges.
//
// Launch 1 (sa_gemm.hip: k_search_tile) numbers observation slots in 32 bits — stored t * Kp + k, query q * Kp + a —
// tiles the query slots over the grid's y extent (65535 tiles of 32 rows on the euclidean kernel), and counts pool blocks in 32 bits with
// UINT32_MAX meaning "no group".  Element offsets into the feature rows are 64-bit: each tile reads from its own base row, and inside a
// tile (at most 64 rows) row * Dp + k stays below 2^32 for every feature length accepted here.
#pragma once
#include <stdint.h>

#define SA_STORE_MAX_FEATURE_LEN (1u << 24)          // D; Dp = D rounded up to 32, and 64 * Dp <= 2^30
#define SA_STORE_MAX_SLOTS 0x7fffffffull             // stored observation slots T * Kp
#define SA_SEARCH_MAX_QUERY_SLOTS (65535ull * 32ull) // query observation slots Q * Kp of one search
#define SA_SEARCH_MAX_PAIRS 0xfffffffeull            // (query, stored track) pairs Q * T of one search: pool blocks stay below UINT32_MAX

enum SaSearchExtent { SA_EXTENT_OK = 0, SA_EXTENT_FEATURE_LEN, SA_EXTENT_STORED, SA_EXTENT_QUERIES, SA_EXTENT_PAIRS };

// stored_tracks / queries: T and Q (queries = 0: a store alone); Kp: observation slots per track (a power of two, 1..32)
static inline int sa_search_extent(uint64_t stored_tracks, uint64_t queries, uint32_t Kp, uint32_t feature_len) {
  if (feature_len > SA_STORE_MAX_FEATURE_LEN) return SA_EXTENT_FEATURE_LEN;
  if (stored_tracks > SA_STORE_MAX_SLOTS || stored_tracks * Kp > SA_STORE_MAX_SLOTS) return SA_EXTENT_STORED;
  if (queries > SA_SEARCH_MAX_QUERY_SLOTS || queries * Kp > SA_SEARCH_MAX_QUERY_SLOTS) return SA_EXTENT_QUERIES;
  if (queries * stored_tracks > SA_SEARCH_MAX_PAIRS) return SA_EXTENT_PAIRS;
  return SA_EXTENT_OK;
}

static inline const char* sa_search_extent_text(int x) {
  switch (x) {
    case SA_EXTENT_FEATURE_LEN: return "feature_len above 2^24";
    case SA_EXTENT_STORED: return "more than 2^31 - 1 stored observation slots (tracks x the next power of two >= max_observations)";
    case SA_EXTENT_QUERIES: return "more than 65535 x 32 query observation slots in one search";
    case SA_EXTENT_PAIRS: return "2^32 - 1 or more (query, stored track) pairs in one search";
    default: return "ok";
  }
}
