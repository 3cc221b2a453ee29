// spring_amd/csrc/unbwt_plan.h -- the parts of the inverse block-sort stage (unbwt.hip) that are
// plain arithmetic: the head rule of the sublists, the bound on the ranking rounds, the workspace a sub-batch needs and
// the cut of a batch into sub-batches.  Shared by host and device; compiles as plain C++ (tests/test_unbwt_cpu.py).
#ifndef SPRING_UNBWT_PLAN_H_
#define SPRING_UNBWT_PLAN_H_

#include <stdint.h>

#include "bwt_plan.h"

namespace unbwt {

constexpr uint64_t MAX_SEGMENT = bwt::MAX_SEGMENT;
constexpr uint64_t MAX_ROWS = 0x7fff0000ull;        // rows of a sub-batch (bytes + one per segment): a row fits 31 bits
constexpr uint64_t MAX_SUB_SEGMENTS = 1ull << 24;   // segments of a sub-batch: segment | byte is half a sort word
// per byte: two 64-bit sort words (the first array becomes the LF words), the sort's own storage, and two 8-byte
// ranking words per head at the closest head spacing
constexpr uint64_t SORT_TMP_PER_POS = 16;
constexpr uint64_t BYTES_PER_POS = 16 + SORT_TMP_PER_POS + 2;
// per segment: its extra row in the arrays above, two heads of its own (row 0 and the primary row) twice, the flags
constexpr uint64_t BYTES_PER_SEG = 96;
constexpr int LOG_K_MIN = 4, LOG_K_MAX = 10, LOG_K_DEFAULT = 6;   // a head about every 2^LOG_K rows
constexpr uint32_t DIST_CLAMP = 0x7fffffffu;        // distances saturate here: above every segment's length

// A fixed mixer of 32 bits (two multiply-xorshift rounds); only its low bits are used.
BWT_HD inline uint32_t mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// The head rule.  Rows are numbered through the sub-batch (segment s owns rows off[s] + s .. off[s + 1] + s).  Every
// block of K = 2^log_k consecutive rows has exactly one regular head, at a place inside the block that the mixer
// picks from the block's number: the heads need no list and no scan (head h is in block h), a run of consecutive rows
// meets one within 2K - 1 rows, and no period of the input lines up with them.  Row 0 of a segment is always a head
// (the walk starts there) and so is its primary row (the walk ends there); these two have slots of their own behind the
// regular ones.
BWT_HD inline uint32_t head_row(uint32_t block, int log_k) { return (block << log_k) + (mix(block) & ((1u << log_k) - 1)); }
BWT_HD inline bool is_regular_head(uint32_t row, int log_k) { return head_row(row >> log_k, log_k) == row; }
BWT_HD inline bool is_head(uint32_t row, uint32_t row_in_segment, int log_k) {
  return row_in_segment == 0 || is_regular_head(row, log_k);
}
BWT_HD inline uint64_t regular_heads(uint64_t rows, int log_k) { return (rows + ((uint64_t)1 << log_k) - 1) >> log_k; }
// heads a segment of n bytes can have on its path: its regular ones (its n + 1 rows touch at most this many blocks),
// row 0 and the primary row
BWT_HD inline uint64_t max_heads_of_segment(uint64_t n, int log_k) { return ((n + 1) >> log_k) + 2 + 2; }

// Pointer-doubling rounds after which every head on a path of at most `heads` heads points at the path's end: after r
// rounds a pointer spans 2^r hops, so ceil(log2(heads)) suffice; one more is kept in hand.
BWT_HD inline int rank_rounds(uint64_t heads) { return bwt::bits_for(heads ? heads : 1) + 1; }

// the share of the workspace budget a sub-batch of m bytes in s segments takes
BWT_HD inline uint64_t workspace_need(uint64_t m, uint64_t s) { return m * BYTES_PER_POS + s * BYTES_PER_SEG; }

// The cut of bwt::plan_sub_batches with this stage's charge and row limit: whole consecutive segments, greedily.
// first[] receives the first segment of every sub-batch and then S (room for S + 1 entries).  Returns the number of
// sub-batches, or -1 - s when segment s alone does not fit.
inline int64_t plan_sub_batches(const uint64_t *off, uint64_t S, uint64_t budget, uint64_t *first) {
  uint64_t nb = 0, s0 = 0;
  for (uint64_t s = 0; s < S; s++) {
    const uint64_t len = off[s + 1] - off[s];
    if (len > MAX_SEGMENT || len + 1 > MAX_ROWS || workspace_need(len, 1) > budget) return -1 - (int64_t)s;
    const uint64_t m = off[s + 1] - off[s0], k = s + 1 - s0;
    if (s > s0 && (m + k > MAX_ROWS || k > MAX_SUB_SEGMENTS || workspace_need(m, k) > budget)) {
      first[nb++] = s0;
      s0 = s;
    }
  }
  if (S) first[nb++] = s0;
  first[nb] = S;
  return (int64_t)nb;
}

}  // namespace unbwt
#endif
