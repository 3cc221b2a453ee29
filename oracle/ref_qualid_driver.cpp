// oracle/ref_qualid_driver.cpp -- TEST INFRASTRUCTURE.
//
// C-ABI driver around the REAL reference code of the quality / id stage, built by oracle/Makefile into
// oracle/_ref/libref_qualid.so: reorder_compress_quality_id.cpp compiled whole where it lies, the real
// BSC_str_array_decompress (libbsc/bsc_str_array.cpp), and util.cpp:113-267 taken by line range (compress_id_block,
// decompress_id_block, quantize_quality, generate_illumina_binning_table, generate_binary_binning_table,
// find_id_pattern, check_id_pattern, modify_id) with the id and qvz codecs they call.  None of these uses Boost.
// Nothing from the reference is copied here; this file only calls it.  tests/test_models_vs_ref.py uses it to pin
// tests/qualid_model.py and spring_quality_table, tests/golden/make_ref_golden.py to record fixtures.
//
// Lines travel as one buffer and count + 1 byte offsets.  A reference exception is returned as -1.
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "libbsc/bsc.h"
#include "reorder_compress_quality_id.h"
#include "util.h"

namespace {
long pack(const std::vector<std::string> &v, char *out, long cap, uint64_t *off) {
  long o = 0;
  for (size_t i = 0; i < v.size(); i++) {
    if (off) off[i] = (uint64_t)o;
    if (o + (long)v[i].size() > cap) return -2;
    std::memcpy(out + o, v[i].data(), v[i].size());
    o += (long)v[i].size();
  }
  if (off) off[v.size()] = (uint64_t)o;
  return o;
}
}  // namespace

extern "C" {

// real reorder_compress_quality_id on dir/{quality_1,quality_2,id_1,id_2,read_order.bin}; qvz_flag = false
int ref_q_write(const char *dir, uint32_t num_reads, int paired_end, uint32_t num_reads_per_block, int num_thr,
                int preserve_quality, int preserve_id, int paired_id_match) {
  spring::compression_params cp;
  memset(&cp, 0, sizeof(cp));
  cp.num_reads = num_reads;
  cp.paired_end = paired_end != 0;
  cp.num_reads_per_block = (int)num_reads_per_block;
  cp.num_thr = num_thr;
  cp.preserve_quality = preserve_quality != 0;
  cp.preserve_id = preserve_id != 0;
  cp.paired_id_match = paired_id_match != 0;
  cp.qvz_flag = false;
  try {
    spring::reorder_compress_quality_id(dir, cp);
  } catch (std::exception &) { return -1; }
  return 0;
}

// real BSC_str_array_decompress: one quality block, `count` lines of the given lengths -> the lines back to back
long ref_q_read_quality(const char *path, uint32_t count, const uint32_t *lens, char *out, long cap) {
  if (count == 0) return 0;
  std::vector<std::string> v(count);
  std::vector<uint32_t> l(lens, lens + count);
  try {
    spring::bsc::BSC_str_array_decompress(path, v.data(), count, l.data());
  } catch (std::exception &) { return -1; }
  return pack(v, out, cap, nullptr);
}

// real decompress_id_block: one id block of `count` ids -> ids back to back + offsets[count + 1]
long ref_q_read_ids(const char *path, uint32_t count, char *out, long cap, uint64_t *off) {
  std::vector<std::string> v(count);
  try {
    spring::decompress_id_block(path, v.data(), count);
  } catch (std::exception &) { return -1; }
  return pack(v, out, cap, off);
}

void ref_q_illumina_table(char *t128) { spring::generate_illumina_binning_table(t128); }

void ref_q_binary_table(char *t128, unsigned thr, unsigned high, unsigned low) {
  spring::generate_binary_binning_table(t128, thr, high, low);
}

// real quantize_quality over `count` lines, in place
void ref_q_quantize(char *buf, const uint64_t *off, uint32_t count, const char *table128) {
  std::vector<std::string> v(count);
  for (uint32_t i = 0; i < count; i++) v[i].assign(buf + off[i], off[i + 1] - off[i]);
  std::vector<char> t(table128, table128 + 128);
  spring::quantize_quality(v.data(), count, t.data());
  for (uint32_t i = 0; i < count; i++) std::memcpy(buf + off[i], v[i].data(), v[i].size());
}

int ref_q_find_id_pattern(const char *a, size_t la, const char *b, size_t lb) {
  return spring::find_id_pattern(std::string(a, la), std::string(b, lb));
}

int ref_q_check_id_pattern(const char *a, size_t la, const char *b, size_t lb, int code) {
  try {
    return spring::check_id_pattern(std::string(a, la), std::string(b, lb), (uint8_t)code) ? 1 : 0;
  } catch (std::exception &) { return -1; }
}

// real modify_id, in place (the length never changes)
void ref_q_modify_id(char *id, size_t len, int code) {
  std::string s(id, len);
  spring::modify_id(s, (uint8_t)code);
  std::memcpy(id, s.data(), len);
}

}  // extern "C"
