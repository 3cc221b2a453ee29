// spring_amd/csrc/copy_words.h -- what the destination-driven copies share: a lane owns one
// 16-byte word of the output, finds the piece that covers the word's first byte (last_le; block_piece where the pieces
// that meet a block of 4 KiB are looked up in LDS), gathers the source bytes of every piece that overlaps the word
// (fetch) and issues one store (put16).  The walk over a word's pieces is the kernel's own: it knows the format.
// Host- and device-callable, so that a host program runs the code the kernels run (tests/test_copy_words_cpu.py); only
// the block lookup at the end is device code.
#ifndef SPRING_COPY_WORDS_H_
#define SPRING_COPY_WORDS_H_

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define CW_HD __host__ __device__ __forceinline__
#else
#define CW_HD inline
#endif

namespace sr {

typedef unsigned __int128 u128;

// ------------------------------------------------------------------ the search
// The largest i in [0, n) with key(i) <= x, given key(0) <= x and key non-decreasing.  Equal neighbours are empty pieces:
// the last of a run of them is the answer, so the piece found is the one that holds x.  I is the index type (the
// arithmetic stays in it); the loop ends after at most as many steps as I has bits.
template <class I, class X, class Key>
CW_HD I last_le(I n, X x, Key key) {
  I lo = 0, hi = n - 1;
  for (int it = 0; it < (int)(8 * sizeof(I)) && lo < hi; it++) {
    const I mid = lo + (hi - lo + 1) / 2;
    if (key(mid) <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// an array as the key
template <class T>
struct ArrayKey {
  const T *a;
  template <class I> CW_HD T operator()(I i) const { return a[i]; }
};
template <class I, class X, class T>
CW_HD I last_le(I n, X x, T *a) { return last_le(n, x, ArrayKey<T>{a}); }

// ------------------------------------------------------------------ the gather
// The aligned word t[a0, a0 + 16) of a source of which t[0, limit) exists; t is 16-byte aligned, a0 % 16 == 0.  Of the
// source's last word only the bytes that exist are read; the others are zero.
CW_HD u128 ld16(const uint8_t *__restrict__ t, uint64_t a0, uint64_t limit) {
  if (a0 + 16 <= limit) {
#if defined(__HIP_DEVICE_COMPILE__)
    const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(t + a0);
    return ((u128)v.y << 64) | v.x;
#else
    u128 v;
    memcpy(&v, t + a0, 16);
    return v;
#endif
  }
  u128 v = 0;
  for (uint32_t i = 0; i < 16 && a0 + i < limit; i++) v |= (u128)t[a0 + i] << (8 * i);
  return v;
}
// the c (1..16) bytes from t + a on, in the low bytes of the result, zero above them; a + c <= limit
CW_HD u128 fetch(const uint8_t *__restrict__ t, uint64_t a, uint32_t c, uint64_t limit) {
  const uint64_t a0 = a & ~15ull;
  const uint32_t sh = (uint32_t)(a & 15);
  u128 v = ld16(t, a0, limit) >> (8 * sh);
  if (sh + c > 16) v |= ld16(t, a0 + 16, limit) << (128 - 8 * sh);   // sh > 0 here
  if (c < 16) v &= ((u128)1 << (8 * c)) - 1;
  return v;
}

// ------------------------------------------------------------------ the store
// out[p, p + nb) = the low nb (1..16) bytes of acc; p % 16 == 0 and out 16-byte aligned.  A whole word is one store, the
// last, partial word of an output goes byte by byte.
CW_HD void put16(uint8_t *out, uint64_t p, uint32_t nb, u128 acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (nb == 16) {
    *reinterpret_cast<uint4 *>(out + p) =
        make_uint4((uint32_t)acc, (uint32_t)(acc >> 32), (uint32_t)(acc >> 64), (uint32_t)(acc >> 96));
    return;
  }
#endif
  for (uint32_t i = 0; i < nb; i++) out[p + i] = (uint8_t)(acc >> (8 * i));
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------ the pieces of a copy block
// A workgroup of 256 lanes writes COPY_BLOCK_BYTES of output.  key(i), i in [0, n], is the offset of piece i in the
// output (key(n) = its size); bs[b] is the piece that holds the first byte of block b.
constexpr int COPY_BLOCK_BYTES = 4096;    // 256 lanes x 16 bytes
constexpr int COPY_LDS_OFFSETS = 1024;    // offsets of a block's pieces held in LDS (more: searched in memory)

// bs[b] = the piece that holds output byte b * COPY_BLOCK_BYTES, bs[nblk] = n
template <class Key>
__global__ void k_block_pieces(Key key, uint64_t n, uint64_t nblk, uint32_t *__restrict__ bs) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b > nblk) return;
  bs[b] = (uint32_t)(b < nblk ? last_le(n + 1, b * COPY_BLOCK_BYTES, key) : n);
}

// The piece that covers byte p of this workgroup's block.  The offsets of the pieces that meet the block go to soff
// (COPY_LDS_OFFSETS entries of LDS), where every lane searches; a block that more pieces meet is searched in memory.
// Contains a __syncthreads(): all 256 lanes call it, in front of any exit.  A lane behind the output's last word passes
// live = false: it helps to fill soff and does not search.
template <class Key>
__device__ __forceinline__ uint64_t block_piece(const Key &key, const uint32_t *__restrict__ bs, uint64_t p, bool live,
                                                uint64_t *soff) {
  const uint64_t s_lo = bs[blockIdx.x], s_hi = bs[blockIdx.x + 1];
  const uint64_t cnt = s_hi - s_lo + 1;
  const bool in_lds = cnt <= COPY_LDS_OFFSETS;
  if (in_lds)
    for (uint32_t t = threadIdx.x; t < cnt; t += 256) soff[t] = key(s_lo + t);
  __syncthreads();
  if (!live) return s_lo;
  if (in_lds) return s_lo + last_le((uint32_t)cnt, p, soff);
  return s_lo + last_le(cnt, p, [&](uint64_t i) { return key(s_lo + i); });
}
#endif

}  // namespace sr
#endif
