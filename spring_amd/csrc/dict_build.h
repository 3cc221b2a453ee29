// spring_amd/csrc/dict_build.h -- the dictionary build's one-pass kernels (dict_build.hip): the unpack pass that also
// emits the dictionary keys, and the writer that produces the hash-addressed bucket table front to back.
#ifndef SPRING_DICT_BUILD_H_
#define SPRING_DICT_BUILD_H_

#include "reorder_device.h"

namespace sr {

// ---- keys in the unpack pass (pools of one read length, fixed-size records).  As launch_unpack's wide path, and for
// every read i also keys{0,1}[i] = mix64(window of dictionary {0,1}), vals{0,1}[i] = i: what k_keys2 would make of the
// limbs.  Returns false (nothing launched) where the wide path does not apply: the caller unpacks as before.
bool launch_unpack_keys(hipStream_t st, const uint8_t *dna, uint32_t n, int L, int W, int S, uint32_t rec_fixed,
                        uint64_t *reads, uint16_t *lens, uint32_t *bad_len, int dstart0, int dend0, int dstart1, int dend1,
                        uint64_t *keys0, uint32_t *vals0, uint64_t *keys1, uint32_t *vals1);

// ---- the table in one pass (hash-addressed tables).  h0 / h1: the sorted unique hashes of the two dictionaries.
constexpr int TAB_WRITE_LG = 10;  // buckets per workgroup of the writer: 2^10 = a 32 KB image in LDS
inline int tab_write_lg(int bshift) { return 64 - bshift < TAB_WRITE_LG ? 64 - bshift : TAB_WRITE_LG; }
inline uint32_t tab_write_blocks(int bshift) { return (uint32_t)(1ull << (64 - bshift - tab_write_lg(bshift))); }
// part: 2 * (tab_write_blocks + 1) words -- where each workgroup's keys start in h0, then in h1
void launch_tab_partition(hipStream_t st, const uint64_t *h0, uint32_t nk0, const uint64_t *h1, uint32_t nk1, int bshift,
                          uint32_t *part);
// every bucket of the table (no memset before it), every pair's record, the deep-bin lists.  The pairs past the fourth
// of a bucket, as the index of the key in its dictionary, + nk0 for those of dictionary 1: the first TAB_OVF_SLOTS of a
// workgroup in ovf_blk[workgroup * TAB_OVF_SLOTS ...], their number in ovf_cnt[workgroup]; any further ones in the list
// ovf (ovf[0] = count, must be zero; entries from ovf + 1, room for nk0 + nk1)
constexpr uint32_t TAB_OVF_SLOTS = 8;
void launch_tab_write(hipStream_t st, const uint64_t *h0, uint32_t nk0, const uint64_t *h1, uint32_t nk1,
                      const uint32_t *part, DictBuild d0, DictBuild d1, uint4 *fpt, int bshift, uint32_t *ovf,
                      uint32_t *ovf_blk, uint32_t *ovf_cnt);
// the overflow pairs claim the next free slot after their home bucket: those of ovf_blk, then the novf listed in ovf
void launch_tab_overflow_blocks(hipStream_t st, const uint64_t *h0, uint32_t nk0, const uint64_t *h1, DictBuild d0,
                                DictBuild d1, uint32_t *fpt, int bshift, const uint32_t *ovf_blk, const uint32_t *ovf_cnt);
void launch_tab_overflow_pairs(hipStream_t st, const uint64_t *h0, uint32_t nk0, const uint64_t *h1, DictBuild d0,
                               DictBuild d1, uint32_t *fpt, int bshift, const uint32_t *ovf, uint32_t novf);

// ---- the strand-symmetric presence table (strand_filter.h): 2^lgb buckets of four 32-bit slots at pres.  Every unique
// key of both dictionaries (h0 / h1: their sorted unique hashes, windows of wl bases) is entered under its canonical
// form; drops: PRES_DROP_CTRS zeroed counters whose sum is the number of keys that met a full bucket.
//   launch_pres_insert  the table zeroed by the caller (skip_self_canonical = false), or written by launch_pres_write
//                       earlier on the same stream (true: only the keys filed under their reverse complement are entered)
//   launch_pres_write   writes EVERY bucket of the table, no memset before it, with the keys that are their own canonical
//                       form in place (they come in bucket order).  part: 2 * (pres_write_blocks(lgb) + 1) words of scratch
constexpr uint32_t PRES_DROP_CTRS = 1024;
constexpr int PRES_WRITE_LG = 10;  // buckets per workgroup of the writer: 2^10 = a 16 KB image in LDS
inline int pres_write_lg(int lgb) { return lgb < PRES_WRITE_LG ? lgb : PRES_WRITE_LG; }
inline uint32_t pres_write_blocks(int lgb) { return 1u << (lgb - pres_write_lg(lgb)); }
void launch_pres_insert(hipStream_t st, const uint64_t *h0, uint32_t nk0, const uint64_t *h1, uint32_t nk1, int wl, uint32_t *pres,
                        int lgb, uint32_t *drops, bool skip_self_canonical);
void launch_pres_write(hipStream_t st, const uint64_t *h0, uint32_t nk0, const uint64_t *h1, uint32_t nk1, int wl, uint4 *pres,
                       int lgb, uint32_t *part, uint32_t *drops);

}  // namespace sr

#endif
