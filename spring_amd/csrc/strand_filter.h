// spring_amd/csrc/strand_filter.h -- the strand-symmetric presence table: the arithmetic its build
// (dict_build.hip: k_pres_insert), its lookups (reorder_round_mc.h: sweep_ka) and the host-side checker share.  Plain
// C++ on 64-bit words: usable from device and host code.
//
// A window W of wl bases (2 bits a base, base 0 in bits 0-1, as in the read limbs) and its reverse complement rc(W) are
// the same window of a consensus seen from its two strands.  The table has one slot per CANONICAL window canon(W) =
// min(W, rc(W)) that is a key of either dictionary on either strand:
//   2^lgb buckets of four 32-bit slots (16 bytes; four buckets a 64-byte line), bucket = top lgb bits of mix64(canon);
//   slot word = fingerprint (bits 4..31, never zero) | flags (bits 0..3); 0 = empty;
//   flag bit l     : canon is a key of dictionary l          (l = 0, 1)
//   flag bit 2 + l : rc(canon) is a key of dictionary l
//   a palindrome (W == rc(W)) sets both bits of its dictionary: the two strands' answers are the same.
// Insert: claim the first empty slot of the bucket (slots fill in order) or take the slot that already carries the
// fingerprint, and OR the flag in; a key whose bucket is full without its fingerprint is DROPPED (and counted).
//
// Lookup contract -- the exactness argument.  A lookup may conclude "absent" for a (strand, dictionary) question only
// when the bucket is NOT full and either no slot carries the fingerprint or the slot that does has that flag clear.
//   * A key is dropped only from a full bucket, and a bucket that is full stays full (slots are never released): a
//     bucket seen not full holds every key that ever asked for it.
//   * Two keys with the same fingerprint in one bucket share a slot and OR their flags: a collision can only turn an
//     "absent" into "maybe present", never the other way.
//   * A full bucket without the fingerprint answers nothing ("unknown").
// So a proven absence is exact, and everything else falls through to the main table, which decides as before.
#ifndef SPRING_STRAND_FILTER_H_
#define SPRING_STRAND_FILTER_H_

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SF_FN __host__ __device__ inline
#else
#define SF_FN inline
#endif

namespace sf {

SF_FN uint64_t mix64(uint64_t x) {  // the main table's hash (reorder_kernels.hip)
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}
SF_FN uint64_t brev64(uint64_t x) {
  x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
  x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
  x = ((x >> 4) & 0x0f0f0f0f0f0f0f0full) | ((x & 0x0f0f0f0f0f0f0f0full) << 4);
  x = ((x >> 8) & 0x00ff00ff00ff00ffull) | ((x & 0x00ff00ff00ff00ffull) << 8);
  x = ((x >> 16) & 0x0000ffff0000ffffull) | ((x & 0x0000ffff0000ffffull) << 16);
  return (x >> 32) | (x << 32);
}
// reverse complement of a window of wl bases (1 <= wl <= 32); the complement of code c is 3 - c (A0 G1 C2 T3)
SF_FN uint64_t rc_window(uint64_t w, int wl) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint64_t x = __builtin_bitreverse64(w);
#else
  uint64_t x = brev64(w);
#endif
  x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);  // bases reversed, bits of a base in order
  return ~x >> (64 - 2 * wl);
}
// Limb j (bases [32 j, 32 j + 32)) of the reverse complement of the first R bases of a consensus, 32 j < R (the four-chain
// round kernel rebuilds a chain's reverse consensus with it instead of keeping a copy): it is made of the 64 consensus bits
// from bit rc_limb_bitpos(R, j) on -- bits in front of base 0 read as zero -- and holds nv = R - 32 j bases (the top limb:
// fewer than 32, the rest zero).
SF_FN int rc_limb_bitpos(int R, int j) { return 2 * (R - 32 - 32 * j); }
SF_FN uint64_t rc_limb(uint64_t w, int nv) {
  return rc_window(w, 32) & (nv >= 32 ? ~0ull : ((1ull << (2 * nv)) - 1));
}
SF_FN uint64_t canon(uint64_t w, int wl, bool &swapped) {
  const uint64_t r = rc_window(w, wl);
  swapped = r < w;
  return swapped ? r : w;
}
SF_FN uint32_t bucket_of(uint64_t h, int lgb) { return lgb ? (uint32_t)(h >> (64 - lgb)) : 0u; }
SF_FN uint32_t fp_of(uint64_t h) {  // 28 bits, never zero: a claimed slot is never 0
  const uint32_t f = (uint32_t)h & 0x0fffffffu;
  return f ? f : 1u;
}
// canon(W), and what a key W of dictionary l adds to the slot of canon(W) -- its own strand's bit, both strands' for a
// palindrome -- from one reverse complement (the insert pass: once per key)
SF_FN uint64_t canon_and_flags(uint64_t w, int wl, int l, uint32_t &flags) {
  const uint64_t r = rc_window(w, wl);
  flags = (w <= r ? 1u << l : 0u) | (r <= w ? 4u << l : 0u);
  return r < w ? r : w;
}
SF_FN uint32_t flags_of_key(uint64_t w, int wl, int l) {
  uint32_t f;
  (void)canon_and_flags(w, wl, l, f);
  return f;
}
// The questions a bucket's four slot words settle for the window with fingerprint fp, in the CANONICAL frame: bit l =
// "canon is absent from dictionary l", bit 2 + l = "rc(canon) is absent from dictionary l".  0: nothing is proven.
SF_FN uint32_t absent_of(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, uint32_t fp) {
  const uint32_t f0 = (s0 >> 4) == fp ? s0 : 0u, f1 = (s1 >> 4) == fp ? s1 : 0u, f2 = (s2 >> 4) == fp ? s2 : 0u,
                 f3 = (s3 >> 4) == fp ? s3 : 0u;
  const uint32_t hit = f0 | f1 | f2 | f3;  // (an insert never makes a second slot of one fingerprint; OR is the safe reading)
  return s3 != 0u ? 0u : ~hit & 15u;       // slots fill in order: the bucket is full exactly when its last slot is taken
}
// from the canonical frame to the window's own: bit l = "W absent from l", bit 2 + l = "rc(W) absent from l"
SF_FN uint32_t to_window_frame(uint32_t a, bool swapped) { return swapped ? ((a >> 2) | (a << 2)) & 15u : a; }

}  // namespace sf

#endif
