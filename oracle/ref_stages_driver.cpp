// oracle/ref_stages_driver.cpp -- TEST INFRASTRUCTURE.
//
// Command-line drivers around the REAL reference stages, whole: spring::reorder_main<N> (reorder.h: reorder()'s loop,
// writetofile) and spring::encoder_main<N> (encoder.h: encode<>(), encoder.cpp whole incl. pack_compress_seq with the real
// BSC_compress).  oracle/Makefile takes both headers by line range into generated TUs under oracle/_ref/gen/ (never
// committed) and leaves out ONE thing: the lines that construct Boost gzip filters (Boost is not available).  In their
// place the same file names are opened as plain std::ofstream / std::ifstream, so the four intermediate files
// (read_rev.txt.<t>, tempflag.txt.<t>, temppos.txt.<t>, read_lengths.bin.<t>) go to disk and come back UNCOMPRESSED.
// Nothing from the reference is copied here; this file only calls it.  One source, two programs:
//
//   -DREF_STAGE_REORDER:  ref_reorder <dir> <max_readlen> <n1> <n2>
//       <dir> holds input_clean_1.dna (n1 reads) and, when n2 > 0, input_clean_2.dna (n2 reads).  Runs
//       reorder_main<N> with num_thr = 1 and leaves its files (the four above uncompressed).
//   -DREF_STAGE_ENCODER:  ref_encoder <dir> <max_readlen> <num_thr> <num_reads> <num_reads_clean>
//       <dir> holds the reorder stage's file set (the four above uncompressed), input_N.dna and read_order_N.bin.
//       Runs encoder_main<N>, then inflates each read_seq.bin.<t>.bsc with the real BSC_decompress into
//       read_seq.bin.<t>.raw and removes the .bsc.
//
// N (the bitset size) is chosen by the limb count: 2 bits per base for reorder, 3 for the encoder, every max_readlen from
// 1 to 511.  Anything else exits non-zero.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#if defined(REF_STAGE_REORDER)
#include "reorder_whole.gen.h"
#define STAGE_MAIN spring::reorder_main
#define BITS_PER_BASE 2
#elif defined(REF_STAGE_ENCODER)
#include "encoder_whole.gen.h"
#include "libbsc/bsc.h"
#define STAGE_MAIN spring::encoder_main
#define BITS_PER_BASE 3
#else
#error "define REF_STAGE_REORDER or REF_STAGE_ENCODER"
#endif

#define LIMBS(W) \
  case W:        \
    STAGE_MAIN<64 * W>(dir, cp); \
    return 0;

static int run_stage(const std::string &dir, const spring::compression_params &cp) {
  if (cp.max_readlen < 1 || cp.max_readlen > 511) return 2;
  switch ((BITS_PER_BASE * cp.max_readlen + 63) / 64) {
    LIMBS(1) LIMBS(2) LIMBS(3) LIMBS(4) LIMBS(5) LIMBS(6) LIMBS(7) LIMBS(8)
    LIMBS(9) LIMBS(10) LIMBS(11) LIMBS(12) LIMBS(13) LIMBS(14) LIMBS(15) LIMBS(16)
#if BITS_PER_BASE == 3
    LIMBS(17) LIMBS(18) LIMBS(19) LIMBS(20) LIMBS(21) LIMBS(22) LIMBS(23) LIMBS(24)
#endif
  }
  return 2;
}

static bool number(const char *s, unsigned long long max, unsigned long long *out) {
  char *end = nullptr;
  if (!*s || *s == '-') return false;
  *out = strtoull(s, &end, 10);
  return *end == 0 && *out <= max;
}

int main(int argc, char **argv) {
  spring::compression_params cp;
  memset(&cp, 0, sizeof(cp));
  unsigned long long v[4];
#if defined(REF_STAGE_REORDER)
  if (argc != 5 || !number(argv[2], 511, &v[0]) || !number(argv[3], UINT32_MAX, &v[1]) ||
      !number(argv[4], UINT32_MAX, &v[2]) || v[1] + v[2] > UINT32_MAX) {
    fprintf(stderr, "usage: ref_reorder <dir> <max_readlen 1..511> <n1> <n2>\n");
    return 2;
  }
  cp.max_readlen = (uint32_t)v[0];
  cp.num_reads_clean[0] = (uint32_t)v[1];
  cp.num_reads_clean[1] = (uint32_t)v[2];
  cp.num_reads = cp.num_reads_clean[0] + cp.num_reads_clean[1];
  cp.paired_end = v[2] != 0;
  cp.num_thr = 1;
  return run_stage(argv[1], cp);
#else
  if (argc != 6 || !number(argv[2], 511, &v[0]) || !number(argv[3], 64, &v[1]) || v[1] < 1 ||
      !number(argv[4], UINT32_MAX, &v[2]) || !number(argv[5], v[2], &v[3])) {
    fprintf(stderr, "usage: ref_encoder <dir> <max_readlen 1..511> <num_thr 1..64> <num_reads> <num_reads_clean>\n");
    return 2;
  }
  cp.max_readlen = (uint32_t)v[0];
  cp.num_thr = (int)v[1];
  cp.num_reads = (uint32_t)v[2];
  cp.num_reads_clean[0] = (uint32_t)v[3];
  int rc = run_stage(argv[1], cp);
  if (rc != 0) return rc;
  fflush(stdout);
  for (int t = 0; t < cp.num_thr; t++) {
    const std::string base = std::string(argv[1]) + "/read_seq.bin." + std::to_string(t);
    spring::bsc::BSC_decompress((base + ".bsc").c_str(), (base + ".raw").c_str());
    if (remove((base + ".bsc").c_str()) != 0) return 1;
  }
  return 0;
#endif
}
