// oracle/ref_streams_driver.cpp -- TEST INFRASTRUCTURE.
//
// Command-line driver around the REAL reference writer of the per-block read streams,
// spring::reorder_compress_streams (reorder_compress_streams.cpp, compiled whole where it lies, no Boost) and the
// REAL spring::bsc::BSC_decompress, built by oracle/Makefile into oracle/_ref/ref_streams.  Nothing from the
// reference is copied here; this file only calls it.  tests/test_models_vs_ref.py uses it to pin
// tests/streams_model.py::write_streams, tests/golden/make_ref_golden.py to record fixtures for the GPU tests.
//
//   ref_streams <dir> <num_reads> <paired_end> <preserve_order> <num_reads_per_block> <num_thr>
//
// <dir> holds the encoder's file set (read_pos.bin, read_noise.txt, read_noisepos.bin, read_rev.txt,
// read_lengths.bin, read_unaligned.txt, read_unaligned.txt.count = u64 total bases of the unaligned reads, and
// read_order.bin when paired_end or preserve_order).  The real function consumes them and leaves
// read_*.{txt,bin}.<b>.bsc; every one of these is then inflated with the real decompressor into the raw block file
// read_*.{txt,bin}.<b> and the .bsc removed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <dirent.h>

#include "libbsc/bsc.h"
#include "reorder_compress_streams.h"
#include "util.h"

int main(int argc, char **argv) {
  if (argc != 7) {
    fprintf(stderr, "usage: ref_streams <dir> <num_reads> <paired_end> <preserve_order> <num_reads_per_block> <num_thr>\n");
    return 2;
  }
  const std::string dir = argv[1];
  spring::compression_params cp;
  memset(&cp, 0, sizeof(cp));
  cp.num_reads = (uint32_t)strtoull(argv[2], nullptr, 10);
  cp.paired_end = atoi(argv[3]) != 0;
  cp.preserve_order = atoi(argv[4]) != 0;
  cp.num_reads_per_block = (int)strtol(argv[5], nullptr, 10);
  cp.num_thr = atoi(argv[6]);
  if (cp.num_reads_per_block <= 0 || cp.num_thr <= 0) return 2;
  spring::reorder_compress_streams(dir, cp);
  std::vector<std::string> packed;
  DIR *d = opendir(dir.c_str());
  if (!d) return 1;
  while (struct dirent *e = readdir(d)) {
    const std::string f = e->d_name;
    if (f.size() > 4 && f.compare(f.size() - 4, 4, ".bsc") == 0) packed.push_back(f);
  }
  closedir(d);
  for (const std::string &f : packed) {
    const std::string in = dir + "/" + f, out = in.substr(0, in.size() - 4);
    spring::bsc::BSC_decompress(in.c_str(), out.c_str());
    if (remove(in.c_str()) != 0) return 1;
  }
  return 0;
}
