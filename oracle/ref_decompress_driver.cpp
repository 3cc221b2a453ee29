// oracle/ref_decompress_driver.cpp -- TEST INFRASTRUCTURE.
//
// Command-line driver around the REAL reference decompressor of short reads, spring::decompress_short
// (decompress.cpp, compiled whole where it lies, no Boost), built by oracle/Makefile into oracle/_ref/ref_decompress.
// write_fastq_block (util.cpp:56-111) is taken by line range into a generated TU under oracle/_ref/gen/ (never
// committed) with ONE thing left out, its gzip branch (util.cpp:71-109, Boost): in its place stands a line that throws,
// so a gzip_flag run fails loudly.  reverse_complement, decompress_id_block and modify_id come from the util.cpp line
// ranges the other drivers already use, BSC_decompress / BSC_str_array_decompress from the real libbsc.  Nothing from
// the reference is copied here; this file only calls it.  tests/test_models_vs_ref_decompress.py uses it to pin
// tests/streams_model.py::read_block and tests/fastq_out_model.py, tests/golden/make_ref_golden.py to record fixtures,
// tests/test_gpu_vs_ref_decompress.py to let the real decompressor read what the GPU stages wrote.
//
//   ref_decompress pack <dir>
//       Turns a directory of RAW files into what decompress_short expects: every file read_*.<n> (the per-block
//       streams read_flag.txt.<b> ... and the 2-bit packed consensus read_seq.bin.<t>; names ending in .bsc or .tail
//       are left alone) goes through the real BSC_compress into <name>.bsc and is removed, as reorder_compress_streams
//       and pack_compress_seq do.  Quality and id block files are not touched: they come from the real
//       reorder_compress_quality_id (libref_qualid.so).
//   ref_decompress run <dir> <out1> <out2> <num_reads> <paired_end> <preserve_order> <preserve_quality> <preserve_id>
//                      <paired_id_code> <paired_id_match> <num_reads_per_block> <enc_num_thr> <num_thr> <start_num> <end_num>
//       decompress_short(dir, out1, out2, cp, num_thr, start_num, end_num, false, 0).  The range must satisfy what
//       spring.cpp:352-358 lets through, 0 <= start_num < end_num <= units; anything else exits with 2.  A reference
//       exception exits with 3.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <vector>
#include <dirent.h>

#include "decompress.h"
#include "libbsc/bsc.h"
#include "util.h"

static bool number(const char *s, unsigned long long max, unsigned long long *out) {
  char *end = nullptr;
  if (!*s || *s == '-') return false;
  *out = strtoull(s, &end, 10);
  return *end == 0 && *out <= max;
}

static bool ends_with(const std::string &f, const char *tail) {
  const size_t n = strlen(tail);
  return f.size() >= n && f.compare(f.size() - n, n, tail) == 0;
}

static int pack(const std::string &dir) {
  std::vector<std::string> raw;
  DIR *d = opendir(dir.c_str());
  if (!d) return 1;
  while (struct dirent *e = readdir(d)) {
    const std::string f = e->d_name;
    if (f.compare(0, 5, "read_") == 0 && !ends_with(f, ".bsc") && !ends_with(f, ".tail")) raw.push_back(f);
  }
  closedir(d);
  for (const std::string &f : raw) {
    const std::string in = dir + "/" + f;
    spring::bsc::BSC_compress(in.c_str(), (in + ".bsc").c_str());
    if (remove(in.c_str()) != 0) return 1;
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && strcmp(argv[1], "pack") == 0) return pack(argv[2]);
  unsigned long long v[12];
  bool ok = argc == 17 && strcmp(argv[1], "run") == 0;
  if (ok) {
    static const unsigned long long max[12] = {UINT32_MAX, 1, 1, 1, 1, 255, 1, INT32_MAX, 64, 64, UINT32_MAX, UINT32_MAX};
    for (int i = 0; i < 12; i++) ok = ok && number(argv[5 + i], max[i], &v[i]);
  }
  if (ok) {
    const unsigned long long units = v[1] ? v[0] / 2 : v[0];
    ok = v[7] >= 1 && v[8] >= 1 && v[9] >= 1 && v[10] < v[11] && v[11] <= units;
  }
  if (!ok) {
    fprintf(stderr,
            "usage: ref_decompress pack <dir>\n"
            "       ref_decompress run <dir> <out1> <out2> <num_reads> <paired_end> <preserve_order> <preserve_quality>\n"
            "                          <preserve_id> <paired_id_code> <paired_id_match> <num_reads_per_block> <enc_num_thr>\n"
            "                          <num_thr> <start_num> <end_num>     (0 <= start_num < end_num <= units)\n");
    return 2;
  }
  spring::compression_params cp;
  memset(&cp, 0, sizeof(cp));
  cp.num_reads = (uint32_t)v[0];
  cp.paired_end = v[1] != 0;
  cp.preserve_order = v[2] != 0;
  cp.preserve_quality = v[3] != 0;
  cp.preserve_id = v[4] != 0;
  cp.paired_id_code = (uint8_t)v[5];
  cp.paired_id_match = v[6] != 0;
  cp.num_reads_per_block = (int)v[7];
  cp.num_thr = (int)v[8];
  try {
    spring::decompress_short(argv[2], argv[3], argv[4], cp, (int)v[9], (uint64_t)v[10], (uint64_t)v[11], false, 0);
  } catch (std::exception &e) {
    fprintf(stderr, "ref_decompress: %s\n", e.what());
    return 3;
  }
  return 0;
}
