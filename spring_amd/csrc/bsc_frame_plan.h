// spring_amd/csrc/bsc_frame_plan.h -- the arithmetic of the BSC framing stage (bsc_frame.hip) that
// host and device share and that a host program can check without a GPU (tests/test_bsc_cpu.py): the store rule of
// bsc_compress, Adler-32 by tiles, the block header, the piece numbering and the offsets of both file framings.
// Plain C++; no HIP call.
#ifndef SPRING_BSC_FRAME_PLAN_H_
#define SPRING_BSC_FRAME_PLAN_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define BSCF_HD __host__ __device__
#else
#define BSCF_HD
#endif

namespace bscf {

constexpr uint32_t MOD = 65521;          // adler32.cpp: BASE
constexpr uint32_t HEADER = 28;          // LIBBSC_HEADER_SIZE
constexpr uint32_t INDEX_MIN = 65536;    // libbsc.cpp:270: below it the secondary indexes are dropped
constexpr int32_t MODE = 1 | (1 << 5);   // LIBBSC_BLOCKSORTER_BWT + (LIBBSC_CODER_QLFC_STATIC << 5), no LZP
constexpr uint32_t TILE = 4096;          // bytes a workgroup sums: 256 lanes, one aligned 16-byte word each

enum Outcome { CODED = 0, STORED_SMALL = 1, STORED_CODER = 2, STORED_NO_GAIN = 3 };
enum Framing { BLOCKS = 0, BSC_FILE = 1, STR_ARRAY = 2 };

// ---------------------------------------------------------------- the store rule (libbsc.cpp:237, :270, :282)
BSCF_HD inline uint32_t kept_indexes(uint64_t n, uint32_t k) { return n < INDEX_MIN ? 0 : k; }

// status: the coder's (0 coded, else not compressible); r: its bytes; k: the block sort's num_indexes
BSCF_HD inline int outcome(uint64_t n, int32_t status, uint64_t r, uint32_t k) {
  if (n <= HEADER) return STORED_SMALL;
  if (status != 0) return STORED_CODER;
  if (r + 1 + 4 * (uint64_t)kept_indexes(n, k) >= n) return STORED_NO_GAIN;
  return CODED;
}

// the block with its header
BSCF_HD inline uint64_t block_bytes(uint64_t n, int oc, uint64_t r, uint32_t k) {
  return HEADER + (oc == CODED ? r + 1 + 4 * (uint64_t)kept_indexes(n, k) : n);
}

// ---------------------------------------------------------------- Adler-32 by tiles
// A sum is the pair (a, b) of adler32.cpp, both below MOD; its value is b << 16 | a.  The empty sum is (1, 0).
struct Sum {
  uint32_t a, b;
};
BSCF_HD inline uint32_t value(Sum s) { return s.b << 16 | s.a; }

// A tile of len <= TILE bytes d[0 .. len): bytes = sum of d[i], weighted = sum of (len - i) * d[i].  At len = 4096 of
// 0xFF these are 1 044 480 and 2 139 617 280: both fit 32 bits, and so does weighted + len.
BSCF_HD inline Sum tile_sum(uint32_t bytes, uint32_t weighted, uint32_t len) {
  return Sum{(1 + bytes) % MOD, (len + weighted) % MOD};
}

// The sum of L followed by R, R of lenR bytes: a = aL + aR - 1, b = bL + bR + lenR (aL - 1), all mod MOD.  lenR is
// reduced before the multiply, so the product stays below 2^32.
BSCF_HD inline Sum combine(Sum L, Sum R, uint64_t lenR) {
  const uint32_t al = (L.a + MOD - 1) % MOD;
  const uint32_t shift = (uint32_t)(lenR % MOD) * al % MOD;
  return Sum{(al + R.a) % MOD, (L.b + R.b + shift) % MOD};
}

// The tiles of a segment at byte address addr: tile t is what the segment has of the aligned window
// [(addr & ~15) + t TILE, + TILE).  The first tile is short by the segment's misalignment.
BSCF_HD inline uint64_t num_tiles(uint64_t addr, uint64_t len) { return len ? ((addr & 15) + len + TILE - 1) / TILE : 0; }
// bytes [lo, hi) of the segment
BSCF_HD inline void tile_range(uint64_t addr, uint64_t len, uint64_t t, uint64_t *lo, uint64_t *hi) {
  const uint64_t h = addr & 15, a = t * TILE, b = a + TILE;
  *lo = a > h ? a - h : 0;
  *hi = b - h < len ? b - h : len;
}

BSCF_HD inline uint32_t adler_bytes(const uint8_t *d, uint32_t n) {   // short inputs only: the 24 bytes of a header
  uint32_t a = 1, b = 0;
  for (uint32_t i = 0; i < n; i++) {
    a = (a + d[i]) % MOD;
    b = (b + a) % MOD;
  }
  return b << 16 | a;
}

// ---------------------------------------------------------------- the block header (libbsc.cpp:82-88, :294-300)
BSCF_HD inline void put32(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}
// The first 20 bytes: sizes, mode, primary index, the sum of the input.
BSCF_HD inline void header_front(uint8_t *h, uint64_t n, int oc, uint64_t r, uint32_t k, int32_t primary, uint32_t adler_in) {
  put32(h + 0, (uint32_t)block_bytes(n, oc, r, k));
  put32(h + 4, (uint32_t)n);
  put32(h + 8, oc == CODED ? (uint32_t)MODE : 0);
  put32(h + 12, oc == CODED ? (uint32_t)primary : 0);
  put32(h + 16, adler_in);
}
// The last 8: the sum of the body, then the sum of the 24 bytes in front.
BSCF_HD inline void header_back(uint8_t *h, uint32_t adler_body) {
  put32(h + 20, adler_body);
  put32(h + 24, adler_bytes(h, 24));
}

// ---------------------------------------------------------------- framing (bsc.cpp:156, :368; bsc_str_array.cpp:206, :451)
BSCF_HD inline uint32_t file_header_bytes(int framing) { return framing == BLOCKS ? 0 : 4; }
BSCF_HD inline uint32_t cut_header_bytes(int framing) { return framing == BSC_FILE ? 10 : framing == STR_ARRAY ? 2 : 0; }
// h: cut_header_bytes(framing) bytes.  offset: the cut's first byte in its file's input.
BSCF_HD inline void cut_header(uint8_t *h, int framing, uint64_t offset) {
  if (framing == BSC_FILE) {
    put32(h, (uint32_t)offset);
    put32(h + 4, (uint32_t)(offset >> 32));
    h += 8;
  }
  if (framing != BLOCKS) h[0] = h[1] = 1;   // recordSize 1, LIBBSC_CONTEXTS_FOLLOWING
}

// The output is a list of pieces in the order of their bytes: per file its header, then per block of the file
//   0  cut header + block header   from the block's META_BYTES of meta
//   1  coded bytes or the input
//   2  the kept indexes (coded only)
//   3  their count (coded only)     byte META_COUNT of the meta
// A piece may be empty.  Block j of file f is pieces f + 1 + 4 j ..; the header of file f, whose first block is j0, is
// piece f + 4 j0.
constexpr uint32_t BLOCK_PIECES = 4, META_BYTES = 48, META_COUNT = 42;
BSCF_HD inline uint64_t piece_of_file(uint64_t f, uint64_t first_block) { return f + BLOCK_PIECES * first_block; }
BSCF_HD inline uint64_t piece_of_block(uint64_t j, uint64_t f) { return f + 1 + BLOCK_PIECES * j; }
BSCF_HD inline void piece_lengths(uint64_t *len, int framing, uint64_t n, int oc, uint64_t r, uint32_t k) {
  len[0] = cut_header_bytes(framing) + HEADER;
  len[1] = oc == CODED ? r : n;
  len[2] = oc == CODED ? 4 * (uint64_t)kept_indexes(n, k) : 0;
  len[3] = oc == CODED ? 1 : 0;
}

// What the device's scan over the piece lengths gives, on the host: file_off[F + 1], block_off[B] (the block's header)
// from the size of every block (block_bytes) and file_first[F + 1].
inline void layout(int framing, const uint64_t *size, const uint64_t *file_first, uint64_t F, uint64_t *file_off,
                   uint64_t *block_off) {
  uint64_t at = 0;
  for (uint64_t f = 0; f < F; f++) {
    file_off[f] = at;
    at += file_header_bytes(framing);
    for (uint64_t j = file_first[f]; j < file_first[f + 1]; j++) {
      at += cut_header_bytes(framing);
      block_off[j] = at;
      at += size[j];
    }
  }
  file_off[F] = at;
}

}  // namespace bscf
#endif
