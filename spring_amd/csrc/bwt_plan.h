// spring_amd/csrc/bwt_plan.h -- the parts of the block-sort stage (bwt.hip) that are plain
// arithmetic: libbsc's secondary-index stride, the layout of the first sort key, the workspace a sub-batch needs and
// the cut of a batch into sub-batches.  Shared by host and device; compiles as plain C++ (tests/test_bwt_cpu.py).
#ifndef SPRING_BWT_PLAN_H_
#define SPRING_BWT_PLAN_H_

#include <stdint.h>

#ifdef __HIPCC__
#define BWT_HD __host__ __device__
#else
#define BWT_HD
#endif

namespace bwt {

constexpr uint64_t MAX_SEGMENT = 1ull << 30;        // bsc_compress refuses more
constexpr uint64_t MAX_POSITIONS = 0x7fff0000ull;   // positions of a sub-batch: they and their ranks + 1 fit 31 bits
constexpr uint64_t MAX_SUB_SEGMENTS = 1ull << 24;   // segments of a sub-batch: leaves four bytes in the first key
constexpr uint64_t BYTES_PER_POS = 72;              // two 64-bit keys, six 32-bit words, 24 bytes of the sort's own
constexpr uint64_t BYTES_PER_POS_RUNS = 76;         // ... and the hop word of the run-aware keys
constexpr uint64_t BYTES_PER_SEG = 16;
constexpr int VALID_BITS = 3;
constexpr int SIDE_BITS = 1;
constexpr int MAX_RUN_BITS = 20;                    // the widest run-length field of any run-key layout
constexpr int MIN_RUN_BITS = 16;

// smallest b with 2^b >= x (x >= 1)
BWT_HD inline int bits_for(uint64_t x) {
  int b = 0;
  for (int k = 0; k < 64 && ((uint64_t)1 << b) < x; k++) b++;
  return b;
}

// divsufsort.c:1704-1712: the distance between two sampled suffixes of a block of n bytes
BWT_HD inline uint32_t index_step(uint32_t n) {
  uint32_t mod = n / 8;
  mod |= mod >> 1; mod |= mod >> 2; mod |= mod >> 4; mod |= mod >> 8; mod |= mod >> 16;
  mod >>= 1;
  return mod + 1;
}
BWT_HD inline uint32_t num_indexes(uint32_t n) { return n ? (uint8_t)((n - 1) / index_step(n)) : 0; }

// The first key of a position: segment (seg_bits) | the next key_bytes bytes big-endian, zero behind the segment's end |
// how many of them exist (VALID_BITS).  Equal bytes with fewer of them valid is the shorter suffix: it sorts first.
struct KeyLayout {
  int seg_bits, key_bytes, total_bits;
};
BWT_HD inline KeyLayout key_layout(uint64_t sub_segments) {
  KeyLayout k;
  k.seg_bits = bits_for(sub_segments ? sub_segments : 1);
  k.key_bytes = (64 - VALID_BITS - k.seg_bits) / 8;
  if (k.key_bytes > 7) k.key_bytes = 7;
  k.total_bits = k.seg_bits + 8 * k.key_bytes + VALID_BITS;
  return k;
}

// The first key with run-aware keys on ("Run-aware first keys"): segment (seg_bits) | the next
// key_bytes bytes | VALID_BITS | side (1 bit) | the run's length or its complement (run_bits).  The run field keeps 20
// bits while four text bytes still fit beside it (up to 256 segments in a sub-batch), 16 above: four text bytes up to
// 4096 segments, three up to 2^20, two up to MAX_SUB_SEGMENTS.
struct RunKeyLayout {
  int seg_bits, key_bytes, run_bits, total_bits;
};
BWT_HD inline RunKeyLayout run_key_layout(uint64_t sub_segments) {
  RunKeyLayout k;
  k.seg_bits = bits_for(sub_segments ? sub_segments : 1);
  const int fixed = VALID_BITS + SIDE_BITS;
  k.run_bits = (64 - fixed - MAX_RUN_BITS - k.seg_bits) / 8 >= 4 ? MAX_RUN_BITS : MIN_RUN_BITS;
  k.key_bytes = (64 - fixed - k.run_bits - k.seg_bits) / 8;
  if (k.key_bytes > 4) k.key_bytes = 4;
  k.total_bits = k.seg_bits + 8 * k.key_bytes + fixed + k.run_bits;
  return k;
}

// the share of the workspace budget a sub-batch of m bytes in s segments takes; run_keys: with the hop word
BWT_HD inline uint64_t workspace_need(uint64_t m, uint64_t s, bool run_keys = false) {
  return m * (run_keys ? BYTES_PER_POS_RUNS : BYTES_PER_POS) + s * BYTES_PER_SEG;
}

// sort rounds a sub-batch whose longest segment has n bytes can take, the first sort included
BWT_HD inline int max_rounds(uint64_t n) { return bits_for(n ? n : 1) + 2; }

// Cuts segments [0, S) (off: S + 1 offsets) into sub-batches of whole consecutive segments, greedily: first[] receives
// the first segment of every sub-batch and then S (room for S + 1 entries).  Returns the number of sub-batches, or
// -1 - s when segment s alone does not fit.
inline int64_t plan_sub_batches(const uint64_t *off, uint64_t S, uint64_t budget, uint64_t *first, bool run_keys = false) {
  uint64_t nb = 0, s0 = 0;
  for (uint64_t s = 0; s < S; s++) {
    const uint64_t len = off[s + 1] - off[s];
    if (len > MAX_SEGMENT || len > MAX_POSITIONS || workspace_need(len, 1, run_keys) > budget) return -1 - (int64_t)s;
    const uint64_t m = off[s + 1] - off[s0], k = s + 1 - s0;
    if (s > s0 && (m > MAX_POSITIONS || k > MAX_SUB_SEGMENTS || workspace_need(m, k, run_keys) > budget)) {
      first[nb++] = s0;
      s0 = s;
    }
  }
  if (S) first[nb++] = s0;
  first[nb] = S;
  return (int64_t)nb;
}

}  // namespace bwt
#endif
