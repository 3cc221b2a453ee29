// spring_amd/csrc/qlfc_plan.h -- the arithmetic of the QLFC stage that host and device share:
// chunk counts, slot numbering, events of a run, workspace need.  Internal to the library.
#ifndef SPRING_QLFC_PLAN_H_
#define SPRING_QLFC_PLAN_H_

#include <stdint.h>

#include "qlfc_params.h"

#ifdef __HIPCC__
#define QLFC_HD __host__ __device__ __forceinline__
#else
#define QLFC_HD inline
#endif

namespace qlfc {

constexpr uint64_t MAX_SEGMENT = 1ull << 30;
constexpr uint32_t TILE = 256;            // runs of a tile of the rank pass
constexpr uint32_t PAY_SLACK = 264;       // bytes a chunk's payload area is longer than the chunk
constexpr uint32_t INF = 0xffffffffu;

// families of predictors, in the order of qlfc_params.h
enum Family { RANK_TOP, RANK_EXP, RANK_MAN, RANK_ESC, RUN_TOP, RUN_EXP, RUN_MAN };
enum Kind { CHAR, STATE, STATIC };

// A slot is one predictor of one chunk: class (3 * family + kind) << 19 | index.  The index of a family's slot is
// hi << (8 + lo_bits) | who << lo_bits | lo: who = the run's byte (CHAR), the context state (STATE) or 0 (STATIC);
// lo = the position in the unary exponent or the bit-tree context; hi = the exponent a mantissa belongs to.
constexpr int CLASS_SHIFT = 19;
constexpr int SLOT_BITS = 24;
QLFC_HD int lo_bits(int family) {
  return family == RANK_EXP ? 3 : family == RANK_MAN || family == RANK_ESC ? 8 : family == RUN_EXP || family == RUN_MAN ? 5 : 0;
}
QLFC_HD uint32_t slot(int family, int kind, uint32_t who, uint32_t hi, uint32_t lo) {
  const int lb = lo_bits(family);
  return (uint32_t)(3 * family + kind) << CLASS_SHIFT | hi << (8 + lb) | who << lb | lo;
}

// bsc_coder_num_blocks (coder.cpp:52-59)
QLFC_HD uint32_t num_chunks(uint64_t n) { return n < 256 * 1024 ? 1 : n < 4 * 1024 * 1024 ? 2 : n < 16 * 1024 * 1024 ? 4 : 8; }

// floor(log2 n); -1 for 0 (bsc_log2 and bsc_log2_256)
QLFC_HD int log2i(uint32_t n) { return n ? 31 - __builtin_clz(n) : -1; }

// maxRank of a chunk with nsym distinct symbols (qlfc.cpp:457, :505)
QLFC_HD int max_rank(uint32_t nsym) { return nsym < 256 ? log2i(nsym - 1) : 7; }

// The decisions of one run.  escape: avgRank >= 32 in front of it.
QLFC_HD uint32_t rank_events(uint32_t rank, bool escape, int maxrank) {
  if (escape) return (uint32_t)(maxrank + 1);
  if (rank == 1) return 1;
  const int e = log2i(rank);
  return 1 + (uint32_t)(e - 1) + (e < maxrank ? 1 : 0) + (uint32_t)e;
}
QLFC_HD uint32_t run_events(uint32_t run) { return run == 1 ? 1 : 1 + 2 * (uint32_t)log2i(run); }

// Workspace of a sub-batch before its events are known: per byte the head flag and its scan (8), the payload area (1),
// per run -- at most one per byte -- start, symbol, rank, two table indexes, flags, event offset (15) and the tile
// table (4);
// per segment eight chunks' tables and payload slack.
constexpr uint64_t BYTE_NEED = 30, SEGMENT_NEED = 8 * (256 + 64 + PAY_SLACK), FIXED_NEED = 1 << 20;
inline uint64_t workspace_need(uint64_t bytes, uint64_t segments) { return bytes * BYTE_NEED + segments * SEGMENT_NEED + FIXED_NEED; }
// per event: keys and values of three slots, twice (the sort's two sides: 72), bit, three values, probability (11);
// the rest of EVENT_NEED is for the sort's own storage
constexpr uint64_t EVENT_ARRAYS = 83, EVENT_NEED = 160;

// How many segments from `first` on fit the budget (at least 1 if the first one fits alone, else 0); a sub-batch stays
// below 2^32 - 2^16 positions.
inline uint64_t take_segments(const uint64_t *off, uint64_t S, uint64_t first, uint64_t budget) {
  uint64_t k = 0;
  while (first + k < S) {
    const uint64_t bytes = off[first + k + 1] - off[first];
    if (bytes > 0xffff0000ull || workspace_need(bytes, k + 1) > budget) break;
    k++;
  }
  return k;
}

}  // namespace qlfc
#endif
