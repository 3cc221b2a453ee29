// spring_amd/csrc/dict_build.hip
//
// The dictionary build's one-pass kernels (gfx950 / CDNA4, wave64):
//   k_unpack_fixed_keys  the wide unpack of fixed-size records that also emits both dictionaries' (hash, id) pairs from
//                        the records it holds in LDS -- no second pass over the limbs (k_keys2)
//   k_tab_partition      where the keys of every block of 1 024 buckets start in the two sorted unique-hash arrays
//   k_tab_write          one workgroup per block of buckets builds the block's image in LDS and stores it in full
//                        lines -- no memset of the table, no merged list of the two dictionaries (merge_by_hash)
//   k_tab_overflow_blocks / _pairs  the pairs past the fourth of a bucket claim a free slot further on (CAS), as before
//   k_pres_write         the strand-symmetric presence table (strand_filter.h), the keys that are their own canonical
//                        form: they arrive in bucket order, so the table is written front to back like the main one
//   k_pres_insert        ... and the keys filed under their reverse complement: one claim-or-OR per key, anywhere
// The table they produce answers every lookup as the one k_tab_insert builds (reorder_kernels.hip): same tags, same
// payloads, the same pairs in the home buckets.
#include <hip/hip_runtime.h>

#include "dict_build.h"
#include "strand_filter.h"

namespace sr {

// ---- the table's hash, fingerprint and bucket rules: the same as in reorder_kernels.hip (tab_find reads what this writes)
__device__ __forceinline__ uint64_t db_mix64(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}
__device__ __forceinline__ uint64_t db_unmix64(uint64_t x) {
  x ^= x >> 33; x *= 0x9cb4b2f8129337dbull; x ^= x >> 33; x *= 0x4f74430c22a54005ull; x ^= x >> 33;
  return x;
}
__device__ __forceinline__ uint32_t db_fp30_of(uint64_t h) {
  const uint32_t f = (uint32_t)h & 0x3fffffffu;
  return f == 0u ? 1u : f == 0x3fffffffu ? 0x3ffffffeu : f;
}

// ------------------------------------------------ unpack + keys
// k_unpack_fixed (reorder_kernels.hip) with one more step: once the block's records are in LDS, thread t < nr cuts the
// two dictionary windows of read r0 + t out of the same limbs the block stores -- limb() is the one function both go
// through, so a key is exactly what read_window would cut from the stored limbs -- and writes mix64(window) and the id.
__global__ __launch_bounds__(256) void k_unpack_fixed_keys(const uint8_t *__restrict__ dna, uint32_t n, int L, int W, int lgS,
                                                           uint32_t rec, uint64_t *__restrict__ reads,
                                                           uint16_t *__restrict__ lens, uint32_t *__restrict__ bad_len,
                                                           int dstart0, int klen0, int dstart1, int klen1,
                                                           uint64_t *__restrict__ keys0, uint32_t *__restrict__ vals0,
                                                           uint64_t *__restrict__ keys1, uint32_t *__restrict__ vals1) {
  extern __shared__ uint4 s_unpack[];
  const uint32_t r0 = blockIdx.x * (uint32_t)UNPACK_READS;
  const uint32_t nr = min((uint32_t)UNPACK_READS, n - r0);
  const uint8_t *g = dna + (uint64_t)r0 * rec;
  const uint32_t sh = (uint32_t)((uintptr_t)g & 15u);
  const uint4 *ga = reinterpret_cast<const uint4 *>(g - sh);
  const uint32_t nchunk = (sh + nr * rec + 15u) >> 4;
  for (uint32_t k = threadIdx.x; k < nchunk; k += 256) s_unpack[k] = ga[k];
  __syncthreads();
  const uint8_t *sb = reinterpret_cast<const uint8_t *>(s_unpack);
  const uint32_t *sw = reinterpret_cast<const uint32_t *>(s_unpack);
  const bool chk = bad_len != nullptr;
  const uint32_t S = 1u << lgS;
  auto len_of = [&](uint32_t r) -> uint32_t {
    const uint32_t p = sh + r * rec;
    return (uint32_t)sb[p] | ((uint32_t)sb[p + 1] << 8);
  };
  auto limb = [&](uint32_t m) -> uint64_t {
    const uint32_t r = m >> lgS, j = m & (S - 1u);
    if ((int)j >= W) return 0;
    uint32_t len = len_of(r);
    if (chk && len != (uint32_t)L) len = (uint32_t)L;  // (stay inside the record; the result is discarded)
    const uint32_t nb = min((len + 3u) / 4u, rec - 2u), pos = 8u * j;
    if (pos >= nb) return 0;
    const uint32_t p = sh + r * rec + 2u + pos, k = p >> 2, s8 = (p & 3u) * 8u;
    uint64_t v = (uint64_t)sw[k] | ((uint64_t)sw[k + 1] << 32);
    if (s8) v = (v >> s8) | ((uint64_t)sw[k + 2] << (64u - s8));
    if (nb - pos < 8u) v &= (1ull << (8u * (nb - pos))) - 1ull;
    return v;
  };
  for (uint32_t t = threadIdx.x; 2u * t < nr; t += 256) {
    const uint32_t r = 2u * t;
    uint32_t l0 = len_of(r), l1 = r + 1 < nr ? len_of(r + 1) : (uint32_t)L;
    if (chk && (l0 != (uint32_t)L || l1 != (uint32_t)L)) {
      *bad_len = 1u;
      l0 = l1 = (uint32_t)L;
    }
    if (r + 1 < nr) *reinterpret_cast<uint32_t *>(lens + r0 + r) = l0 | (l1 << 16);
    else lens[r0 + r] = (uint16_t)l0;
  }
  const uint32_t nl = nr << lgS;
  uint64_t *out = reads + ((uint64_t)r0 << lgS);
  for (uint32_t q = threadIdx.x; 2u * q < nl; q += 256) {
    const uint32_t m = 2u * q;
    const uint64_t v0 = limb(m);
    if (m + 1 < nl) *reinterpret_cast<ulonglong2 *>(out + m) = make_ulonglong2(v0, limb(m + 1));
    else out[m] = v0;
  }
  // the dictionary windows ((read & mask) >> 2 * start, bitset_util.h:94-95): read_window over the limbs above
  auto window = [&](uint32_t r, int dstart, int klen2) -> uint64_t {
    const uint32_t bitpos = 2u * (uint32_t)dstart, li = bitpos >> 6, off = bitpos & 63u;
    uint64_t v = limb((r << lgS) + li) >> off;
    if (off && li + 1u < S) v |= limb((r << lgS) + li + 1u) << (64u - off);
    if (klen2 < 64) v &= (1ull << klen2) - 1ull;
    return v;
  };
  for (uint32_t r = threadIdx.x; r < nr; r += 256) {
    const uint32_t i = r0 + r;
    keys0[i] = db_mix64(window(r, dstart0, 2 * klen0));
    vals0[i] = i;
    keys1[i] = db_mix64(window(r, dstart1, 2 * klen1));
    vals1[i] = i;
  }
}

bool launch_unpack_keys(hipStream_t st, const uint8_t *dna, uint32_t n, int L, int W, int S, uint32_t rec_fixed,
                        uint64_t *reads, uint16_t *lens, uint32_t *bad_len, int dstart0, int dend0, int dstart1, int dend1,
                        uint64_t *keys0, uint32_t *vals0, uint64_t *keys1, uint32_t *vals1) {
  if (!n || ((uintptr_t)reads & 15u) || ((uintptr_t)lens & 3u)) return false;
  if (dstart0 < 0 || dstart1 < 0 || dend0 >= L || dend1 >= L || 2 * dend0 / 64 >= S || 2 * dend1 / 64 >= S) return false;
  int lgS = 0;
  while ((1 << lgS) < S) lgS++;
  const size_t lds = ((size_t)UNPACK_READS * rec_fixed + 15 + 12 + 15) / 16 * 16;
  hipLaunchKernelGGL(k_unpack_fixed_keys, dim3((n + UNPACK_READS - 1) / UNPACK_READS), dim3(256), lds, st, dna, n, L, W, lgS,
                     rec_fixed, reads, lens, bad_len, dstart0, dend0 - dstart0 + 1, dstart1, dend1 - dstart1 + 1, keys0, vals0,
                     keys1, vals1);
  return true;
}

// ------------------------------------------------ the table in one pass
// Both unique-hash arrays are sorted, and the home bucket is the top bits of the hash: the keys of buckets
// [j << lg, (j + 1) << lg) are one interval of each array.  One thread per boundary and array finds where it starts.
__global__ void k_tab_partition(const uint64_t *__restrict__ h0, uint32_t nk0, const uint64_t *__restrict__ h1, uint32_t nk1,
                                int bshift, int lg, uint32_t nblk, uint32_t *__restrict__ part) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2ull * ((uint64_t)nblk + 1)) return;
  const uint32_t l = t > nblk ? 1u : 0u, j = (uint32_t)(t - (l ? (uint64_t)nblk + 1 : 0));
  const uint64_t *__restrict__ h = l ? h1 : h0;
  const uint32_t nk = l ? nk1 : nk0;
  uint32_t lo = 0, hi = nk;
  if (j == nblk) {
    lo = nk;
  } else if (j != 0u) {  // (block 0 starts at key 0; a table of one bucket has bshift = 64 and no other block)
    const uint64_t bound = ((uint64_t)j << lg) << bshift;  // the smallest hash of bucket j << lg
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (h[mid] < bound) lo = mid + 1; else hi = mid;
    }
  }
  part[t] = lo;
}

// One workgroup per block of 2^lg buckets.  The slot a pair gets in its home bucket is its rank among the bucket's
// pairs in the merged order (by hash, dictionary 0 first on equal hashes) -- what k_tab_insert<false> counts by looking
// back in the merged list.  Here: the pair's predecessors of its own dictionary (looking back at most four entries of
// its own array) plus those of the other dictionary (first[][] says where the bucket's keys of the other array begin;
// at most four are read from there).  The block's hashes are staged in LDS, the first TAB_WRITE_TILE of either
// dictionary -- at most 0.8 pairs per bucket: about 410 a dictionary -- so that none of this waits for memory; a block
// with more keys than that (many keys in few buckets) finds a pair's place in the other array by binary search and
// reads the keys past the tile from the arrays themselves, and the
// loop strides over the block's keys however many there are.  Ranks 0..3 are distinct per bucket, so every image word
// has one writer.  Every pair writes its bin record.
// Pairs of rank >= 4 (about two a block at load 0.2): the first TAB_OVF_SLOTS of a block go to the block's own slots of
// ovf_blk, counted in LDS, and the count to ovf_cnt[block] -- chunked append slots, not one same-address atomic on memory
// per pair.  Only a block with more of them appends the rest to the list ovf with an atomic.
constexpr uint32_t TAB_WRITE_TILE = 512, TAB_WRITE_THREADS = 512;
__global__ __launch_bounds__(TAB_WRITE_THREADS) void k_tab_write(const uint64_t *__restrict__ h0, uint32_t nk0,
                                                                 const uint64_t *__restrict__ h1, uint32_t nk1,
                                                                 const uint32_t *__restrict__ part, uint32_t nblk,
                                                                 DictBuild d0, DictBuild d1, uint4 *__restrict__ fpt,
                                                                 int bshift, int lg, uint32_t *__restrict__ ovf,
                                                                 uint32_t *__restrict__ ovf_blk, uint32_t *__restrict__ ovf_cnt) {
  __shared__ uint4 img[2u << TAB_WRITE_LG];
  __shared__ uint64_t tile[2][TAB_WRITE_TILE];
  __shared__ uint16_t first[2][1u << TAB_WRITE_LG];  // per bucket of the block and dictionary: 1 + place of its first staged key
  __shared__ uint32_t s_novf;
  const uint32_t nbk = 1u << lg, bmask = nbk - 1u, blk = blockIdx.x;
  for (uint32_t k = threadIdx.x; k < 2u * nbk; k += TAB_WRITE_THREADS) img[k] = make_uint4(0u, 0u, 0u, 0u);
  for (uint32_t k = threadIdx.x; k < nbk / 2u + 1u; k += TAB_WRITE_THREADS) {  // (two entries a word; nbk >= 8)
    if (2u * k < nbk) { reinterpret_cast<uint32_t *>(first[0])[k] = 0u; reinterpret_cast<uint32_t *>(first[1])[k] = 0u; }
  }
  if (threadIdx.x == 0) s_novf = 0u;
  const uint32_t a0 = part[blk], a1 = part[(uint64_t)nblk + 1 + blk];
  const uint32_t c0 = part[blk + 1] - a0, c1 = part[(uint64_t)nblk + 2 + blk] - a1;
  const uint32_t ntot = c0 + c1;
  // pair t of the block: dictionary l = t >= c0, place k = t - l * c0 among the block's keys of l, index a_l + k in l
  auto bin_of = [&](uint32_t t, uint32_t &st, uint32_t &cn, uint32_t &pay) {  // the pair's bin; payload: a lone read's id, or the index
    const bool l = t >= c0;
    const uint32_t i = l ? a1 + (t - c0) : a0 + t;
    st = (l ? d1.ustart : d0.ustart)[i]; cn = (l ? d1.ucount : d0.ucount)[i];
    pay = cn == 1u ? (l ? d1.ids : d0.ids)[st] : i;
  };
  // the first two pairs of this thread (a block holds about 750): their loads are on their way while the tiles arrive
  uint32_t st0 = 0, cn0 = 0, pay0 = 0, st1 = 0, cn1 = 0, pay1 = 0;
  if (threadIdx.x < ntot) bin_of(threadIdx.x, st0, cn0, pay0);
  if (threadIdx.x + TAB_WRITE_THREADS < ntot) bin_of(threadIdx.x + TAB_WRITE_THREADS, st1, cn1, pay1);
  __syncthreads();  // (first[][] is zero before anyone marks a bucket)
  for (uint32_t k = threadIdx.x; k < min(c0, TAB_WRITE_TILE); k += TAB_WRITE_THREADS) {
    const uint64_t x = h0[a0 + k];
    tile[0][k] = x;
    if (k == 0u || (h0[a0 + k - 1u] >> bshift) != (x >> bshift)) first[0][(uint32_t)(x >> bshift) & bmask] = (uint16_t)(k + 1u);
  }
  for (uint32_t k = threadIdx.x; k < min(c1, TAB_WRITE_TILE); k += TAB_WRITE_THREADS) {
    const uint64_t x = h1[a1 + k];
    tile[1][k] = x;
    if (k == 0u || (h1[a1 + k - 1u] >> bshift) != (x >> bshift)) first[1][(uint32_t)(x >> bshift) & bmask] = (uint16_t)(k + 1u);
  }
  const bool staged = c0 <= TAB_WRITE_TILE && c1 <= TAB_WRITE_TILE;  // every key of the block is in LDS: first[][] is complete
  __syncthreads();
  if (ntot) {  // (the same for the whole workgroup)
    uint32_t *imgw = reinterpret_cast<uint32_t *>(img);
    auto H = [&](bool l, uint32_t k) -> uint64_t {  // hash k of the block's keys of dictionary l
      if (k < TAB_WRITE_TILE) return l ? tile[1][k] : tile[0][k];
      return l ? h1[a1 + k] : h0[a0 + k];
    };
    auto place = [&](uint32_t t, uint32_t st, uint32_t cn, uint32_t pay) {
      const bool l = t >= c0;
      const uint32_t k = l ? t - c0 : t, i = (l ? a1 : a0) + k;
      const uint64_t hh = H(l, k), b = hh >> bshift;
      uint32_t rank = 0;
      while (rank < 4u && k > rank && (H(l, k - 1u - rank) >> bshift) == b) rank++;
      if (rank < 4u && staged) {  // the other dictionary's keys of this bucket, from its first: those that come before this one
        const uint32_t f = l ? first[0][(uint32_t)b & bmask] : first[1][(uint32_t)b & bmask], co = l ? c0 : c1;
        if (f) {
          for (uint32_t o = f - 1u; rank < 4u && o < co; o++) {
            const uint64_t x = l ? tile[0][o] : tile[1][o];
            if ((x >> bshift) != b || (l ? x > hh : x >= hh)) break;
            rank++;
          }
        }
      } else if (rank < 4u) {
        uint32_t lo = 0, hi = l ? c0 : c1;  // the other dictionary's keys that come before this one in the merged order
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          const uint64_t x = H(!l, mid);
          if (l ? x <= hh : x < hh) lo = mid + 1u; else hi = mid;
        }
        while (rank < 4u && lo > 0u && (H(!l, lo - 1u) >> bshift) == b) { rank++; lo--; }
      }
      uint32_t *nd = l ? d1.ndeep : d0.ndeep;
      if (cn >= DEEP_BIN) (l ? d1.deep : d0.deep)[atomicAdd(nd, 1u)] = i;  // bins worth trimming (k_trim_bins)
      if (cn >= BIG_BIN) atomicAdd(nd + 1, cn);
      if (cn >= MID_BIN) atomicAdd(nd + 2, cn);
      (l ? d1.urec : d0.urec)[i] = make_ulonglong2(db_unmix64(hh), (uint64_t)st | ((uint64_t)cn << 32));
      if (rank >= 4u) {
        const uint32_t g = l ? nk0 + i : i, slot = atomicAdd(&s_novf, 1u);
        if (slot < TAB_OVF_SLOTS) ovf_blk[(uint64_t)blk * TAB_OVF_SLOTS + slot] = g;
        else ovf[1u + atomicAdd(ovf, 1u)] = g;
      } else {
        const uint32_t bl = (uint32_t)b & bmask;
        imgw[bl * 8u + rank] = (db_fp30_of(hh) << 2) | ((uint32_t)l << 1) | (cn == 1u ? 1u : 0u);
        imgw[bl * 8u + 4u + rank] = pay;
      }
    };
    if (threadIdx.x < ntot) place(threadIdx.x, st0, cn0, pay0);
    if (threadIdx.x + TAB_WRITE_THREADS < ntot) place(threadIdx.x + TAB_WRITE_THREADS, st1, cn1, pay1);
    for (uint32_t t = threadIdx.x + 2u * TAB_WRITE_THREADS; t < ntot; t += TAB_WRITE_THREADS) {
      bin_of(t, st0, cn0, pay0);
      place(t, st0, cn0, pay0);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) ovf_cnt[blk] = min(s_novf, TAB_OVF_SLOTS);
  uint4 *__restrict__ out = fpt + (((uint64_t)blk << lg) << 1);
  for (uint32_t k = threadIdx.x; k < 2u * nbk; k += TAB_WRITE_THREADS) out[k] = img[k];
}

// pair g of the overflow lists (index in its dictionary, + nk0 for dictionary 1) claims the next free slot after its home bucket
__device__ __forceinline__ void tab_overflow_insert(uint32_t g, const uint64_t *__restrict__ h0, uint32_t nk0,
                                                    const uint64_t *__restrict__ h1, const DictBuild &d0, const DictBuild &d1,
                                                    uint32_t *fpt, int bshift) {
  const uint32_t l = g >= nk0 ? 1u : 0u, u = l ? g - nk0 : g;
  const uint64_t h = (l ? h1 : h0)[u];
  const DictBuild &d = l ? d1 : d0;
  const uint32_t st = d.ustart[u], cn = d.ucount[u];
  const bool single = cn == 1u;
  const uint32_t tag = (db_fp30_of(h) << 2) | (l << 1) | (single ? 1u : 0u);
  const uint32_t pay = single ? d.ids[st] : u;
  const uint64_t bmask = (1ull << (64 - bshift)) - 1;
  uint64_t b = ((h >> bshift) + 1) & bmask;  // the home bucket is full by construction
  for (;;) {
    uint32_t *bk = fpt + b * 8;
    for (int sl = 0; sl < 4; sl++) {
      if (atomicCAS(bk + sl, 0u, tag) == 0u) {
        bk[4 + sl] = pay;
        return;
      }
    }
    b = (b + 1) & bmask;
  }
}
// one thread per slot of ovf_blk
__global__ void k_tab_overflow_blocks(const uint64_t *__restrict__ h0, uint32_t nk0, const uint64_t *__restrict__ h1,
                                      DictBuild d0, DictBuild d1, uint32_t *fpt, int bshift, uint32_t nblk,
                                      const uint32_t *__restrict__ ovf_blk, const uint32_t *__restrict__ ovf_cnt) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t blk = t / TAB_OVF_SLOTS;
  if (blk >= nblk || (uint32_t)(t % TAB_OVF_SLOTS) >= ovf_cnt[blk]) return;
  tab_overflow_insert(ovf_blk[t], h0, nk0, h1, d0, d1, fpt, bshift);
}
// one thread per entry of the list ovf
__global__ void k_tab_overflow_pairs(const uint64_t *__restrict__ h0, uint32_t nk0, const uint64_t *__restrict__ h1,
                                     DictBuild d0, DictBuild d1, uint32_t *fpt, int bshift, const uint32_t *__restrict__ ovf) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ovf[0]) return;
  tab_overflow_insert(ovf[1u + t], h0, nk0, h1, d0, d1, fpt, bshift);
}

void launch_tab_partition(hipStream_t st, const uint64_t *h0, uint32_t nk0, const uint64_t *h1, uint32_t nk1, int bshift,
                          uint32_t *part) {
  const uint32_t nblk = tab_write_blocks(bshift);
  const uint64_t nt = 2ull * ((uint64_t)nblk + 1);
  hipLaunchKernelGGL(k_tab_partition, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, h0, nk0, h1, nk1, bshift,
                     tab_write_lg(bshift), nblk, part);
}
void launch_tab_write(hipStream_t st, const uint64_t *h0, uint32_t nk0, const uint64_t *h1, uint32_t nk1,
                      const uint32_t *part, DictBuild d0, DictBuild d1, uint4 *fpt, int bshift, uint32_t *ovf,
                      uint32_t *ovf_blk, uint32_t *ovf_cnt) {
  const uint32_t nblk = tab_write_blocks(bshift);
  hipLaunchKernelGGL(k_tab_write, dim3(nblk), dim3(TAB_WRITE_THREADS), 0, st, h0, nk0, h1, nk1, part, nblk, d0, d1, fpt, bshift,
                     tab_write_lg(bshift), ovf, ovf_blk, ovf_cnt);
}
void launch_tab_overflow_blocks(hipStream_t st, const uint64_t *h0, uint32_t nk0, const uint64_t *h1, DictBuild d0,
                                DictBuild d1, uint32_t *fpt, int bshift, const uint32_t *ovf_blk, const uint32_t *ovf_cnt) {
  const uint32_t nblk = tab_write_blocks(bshift);
  const uint64_t nt = (uint64_t)nblk * TAB_OVF_SLOTS;
  hipLaunchKernelGGL(k_tab_overflow_blocks, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, h0, nk0, h1, d0, d1, fpt, bshift,
                     nblk, ovf_blk, ovf_cnt);
}
void launch_tab_overflow_pairs(hipStream_t st, const uint64_t *h0, uint32_t nk0, const uint64_t *h1, DictBuild d0,
                               DictBuild d1, uint32_t *fpt, int bshift, const uint32_t *ovf, uint32_t novf) {
  if (!novf) return;
  hipLaunchKernelGGL(k_tab_overflow_pairs, dim3((novf + 255) / 256), dim3(256), 0, st, h0, nk0, h1, d0, d1, fpt, bshift, ovf);
}

// ------------------------------------------------ the strand-symmetric presence table (strand_filter.h)
// One thread per unique key of either dictionary (h = mix64(key): the sorted unique-hash arrays the main table is built
// from, so every key of the main table is covered).  The slot of canon(key) is claimed with one CAS that already carries
// the key's flag; a thread that finds the fingerprint there ORs its flag in.  Keys that meet a full bucket are counted per
// workgroup in LDS and added to one of PRES_DROP_CTRS counters: no same-address atomic per dropped key.
//
// k_pres_write: the keys that are their own canonical form, K <= rc(K) -- half of the others and every palindrome.  Such
// a key is filed under mix64(canon(K)) = mix64(K), the very hash its array is sorted by, so the keys of the buckets
// [j << lg, (j + 1) << lg) are one interval of each array (k_tab_partition with the shift 64 - lgb).  One workgroup per
// block of 2^lg buckets: it zeroes the block's image in LDS, enters its keys there by k_pres_insert's rule -- slots 0..3
// in order, claim an empty one with a CAS that carries the flags, or OR them into the slot that has the fingerprint,
// else count a drop -- and stores the image in 16-byte pieces.  Every bucket of the table is written, by the workgroups
// without keys too: nothing zeroes the table before this kernel.  The loop strides over however many keys the block has
// (a capped table: all of them in a few buckets).  The keys with rc(K) < K are read and passed over: k_pres_insert's.
constexpr uint32_t PRES_WRITE_THREADS = 256;
__global__ __launch_bounds__(PRES_WRITE_THREADS) void k_pres_write(const uint64_t *__restrict__ h0, const uint64_t *__restrict__ h1,
                                                                   const uint32_t *__restrict__ part, uint32_t nblk, int wl,
                                                                   uint4 *__restrict__ pres, int lgb, int lg,
                                                                   uint32_t *__restrict__ drops) {
  __shared__ uint4 img[1u << PRES_WRITE_LG];
  __shared__ uint32_t s_drop;
  const uint32_t nbk = 1u << lg, bmask = nbk - 1u, blk = blockIdx.x;
  for (uint32_t k = threadIdx.x; k < nbk; k += PRES_WRITE_THREADS) img[k] = make_uint4(0u, 0u, 0u, 0u);
  if (threadIdx.x == 0) s_drop = 0u;
  const uint32_t a0 = part[blk], a1 = part[(uint64_t)nblk + 1 + blk];
  const uint32_t c0 = part[blk + 1] - a0, c1 = part[(uint64_t)nblk + 2 + blk] - a1;
  const uint32_t ntot = c0 + c1;
  __syncthreads();
  uint32_t *imgw = reinterpret_cast<uint32_t *>(img);
  for (uint32_t t = threadIdx.x; t < ntot; t += PRES_WRITE_THREADS) {
    const int l = t >= c0 ? 1 : 0;
    const uint64_t h = l ? h1[a1 + (t - c0)] : h0[a0 + t];
    uint32_t flags;
    const uint64_t cw = sf::canon_and_flags(db_unmix64(h), wl, l, flags);
    if (!(flags & (1u << l))) continue;  // rc(K) < K
    const uint64_t hc = sf::mix64(cw);   // (= h: the key is its canonical form)
    const uint32_t fp = sf::fp_of(hc), word = (fp << 4) | flags;
    uint32_t *bk = imgw + 4u * (sf::bucket_of(hc, lgb) & bmask);
    bool placed = false;
    for (int sl = 0; sl < 4 && !placed; sl++) {
      const uint32_t old = atomicCAS(bk + sl, 0u, word);
      if (old == 0u) placed = true;
      else if ((old >> 4) == fp) {
        if ((old & word & 15u) != (word & 15u)) atomicOr(bk + sl, word & 15u);
        placed = true;
      }
    }
    if (!placed) atomicAdd(&s_drop, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_drop) atomicAdd(drops + (blk & (PRES_DROP_CTRS - 1u)), s_drop);
  uint4 *__restrict__ out = pres + ((uint64_t)blk << lg);
  for (uint32_t k = threadIdx.x; k < nbk; k += PRES_WRITE_THREADS) out[k] = img[k];
}
// skip_self: the keys that are their own canonical form (a palindrome is) are in the table already (k_pres_write, a
// kernel boundary earlier): their threads leave before they touch it.
__global__ __launch_bounds__(256) void k_pres_insert(const uint64_t *__restrict__ h0, uint32_t nk0, const uint64_t *__restrict__ h1,
                                                     uint32_t nk1, int wl, uint32_t *__restrict__ pres, int lgb,
                                                     uint32_t *__restrict__ drops, int skip_self) {
  __shared__ uint32_t s_drop;
  if (threadIdx.x == 0) s_drop = 0u;
  __syncthreads();
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool mine = t < (uint64_t)nk0 + nk1;
  if (mine) {
    const int l = t >= nk0 ? 1 : 0;
    const uint64_t key = db_unmix64(l ? h1[t - nk0] : h0[t]);
    uint32_t flags;
    const uint64_t cw = sf::canon_and_flags(key, wl, l, flags);
    if (skip_self && (flags & (1u << l))) mine = false;  // (bit l: key <= rc(key))
    const uint64_t hc = sf::mix64(cw);
    const uint32_t fp = sf::fp_of(hc), word = (fp << 4) | flags;
    uint32_t *bk = pres + 4ull * sf::bucket_of(hc, lgb);
    bool placed = !mine;
    for (int sl = 0; sl < 4 && !placed; sl++) {
      uint32_t old = __hip_atomic_load(bk + sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old == 0u) old = atomicCAS(bk + sl, 0u, word);
      if (old == 0u) placed = true;
      else if ((old >> 4) == fp) {
        if ((old & word & 15u) != (word & 15u)) atomicOr(bk + sl, word & 15u);
        placed = true;
      }
    }
    if (!placed) atomicAdd(&s_drop, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_drop) atomicAdd(drops + (blockIdx.x & (PRES_DROP_CTRS - 1u)), s_drop);
}
void launch_pres_insert(hipStream_t st, const uint64_t *h0, uint32_t nk0, const uint64_t *h1, uint32_t nk1, int wl, uint32_t *pres,
                        int lgb, uint32_t *drops, bool skip_self_canonical) {
  const uint64_t nt = (uint64_t)nk0 + nk1;
  if (!nt) return;
  hipLaunchKernelGGL(k_pres_insert, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, h0, nk0, h1, nk1, wl, pres, lgb, drops,
                     skip_self_canonical ? 1 : 0);
}
void launch_pres_write(hipStream_t st, const uint64_t *h0, uint32_t nk0, const uint64_t *h1, uint32_t nk1, int wl, uint4 *pres,
                       int lgb, uint32_t *part, uint32_t *drops) {
  const int lg = pres_write_lg(lgb);
  const uint32_t nblk = pres_write_blocks(lgb);
  const uint64_t nt = 2ull * ((uint64_t)nblk + 1);
  hipLaunchKernelGGL(k_tab_partition, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, h0, nk0, h1, nk1, 64 - lgb, lg, nblk, part);
  hipLaunchKernelGGL(k_pres_write, dim3(nblk), dim3(PRES_WRITE_THREADS), 0, st, h0, h1, part, nblk, wl, pres, lgb, lg, drops);
}

}  // namespace sr
