// spring_amd/csrc/gzip_codes.h -- the parts of the deflate coder (gzip.hip) that are plain
// sequential code: the length / distance / extra-bit tables of RFC 1951 section 3.2.5 as formulas, the length-limited
// prefix code of a histogram, the run-length form of the code lengths, the dynamic block header, CRC-32 arithmetic.
// Everything is __host__ __device__, so a CPU build reaches the same code the kernels run.  Internal to the library.
#ifndef SPRING_GZIP_CODES_H_
#define SPRING_GZIP_CODES_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define GZ_HD __host__ __device__ inline
#else
#define GZ_HD inline
#endif

namespace gz {

constexpr int NUM_LL = 286, NUM_D = 30, NUM_CL = 19, EOB = 256;
constexpr int MAX_BITS = 15, MAX_CL_BITS = 7;
constexpr int MIN_MATCH = 4;          // what the 4-byte hash finds (RFC 1951 allows 3)
constexpr int MAX_MATCH = 258, MAX_DIST = 32768;
constexpr int MAX_CL_SEQ = NUM_LL + NUM_D;
constexpr uint32_t TOK_MATCH = 0x80000000u;   // token: a literal byte, or TOK_MATCH | (len - 3) << 16 | (dist - 1)

GZ_HD int log2_floor(uint32_t v) { return 31 - __builtin_clz(v); }   // v > 0

// ---- RFC 1951 3.2.5: symbol, number of extra bits and extra value of a match length 3 .. 258
GZ_HD int len_symbol(int len, int *ebits, int *evalue) {
  const int l = len - 3;
  if (l < 8) { *ebits = 0; *evalue = 0; return 257 + l; }
  if (len == 258) { *ebits = 0; *evalue = 0; return 285; }
  const int e = log2_floor((uint32_t)l) - 2;
  *ebits = e;
  *evalue = l & ((1 << e) - 1);
  return 257 + 4 * (e + 1) + ((l >> e) & 3);
}
GZ_HD int len_ebits(int sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
// ... and of a distance 1 .. 32768
GZ_HD int dist_symbol(int dist, int *ebits, int *evalue) {
  const int d = dist - 1;
  if (d < 4) { *ebits = 0; *evalue = 0; return d; }
  const int e = log2_floor((uint32_t)d) - 1;
  *ebits = e;
  *evalue = d & ((1 << e) - 1);
  return 2 * e + 2 + ((d >> e) & 1);
}
GZ_HD int dist_ebits(int sym) { return sym < 4 ? 0 : (sym - 2) >> 1; }

GZ_HD uint32_t bit_reverse(uint32_t v, int n) {   // the low n bits of v, reversed
  uint32_t r = 0;
  for (int i = 0; i < n; i++) r |= ((v >> i) & 1u) << (n - 1 - i);
  return r;
}

// ---- a length-limited prefix code
// Lengths of a minimum-redundancy code over frequencies sorted in ascending order, in place (Moffat and Katajainen,
// "In-place calculation of minimum-redundancy codes", 1995): A[i] in: frequency, out: code length.  n >= 2.
GZ_HD void minimum_redundancy(uint32_t *A, int n) {
  A[0] += A[1];
  int root = 0, leaf = 2, next;
  for (next = 1; next < n - 1; next++) {
    if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; }
    else A[next] = A[leaf++];
    if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; }
    else A[next] += A[leaf++];
  }
  A[n - 2] = 0;
  for (next = n - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
  int avbl = 1, used = 0, dpth = 0;
  root = n - 2;
  next = n - 1;
  while (avbl > 0) {
    while (root >= 0 && (int)A[root] == dpth) { used++; root--; }
    while (avbl > used) { A[next--] = (uint32_t)dpth; avbl--; }
    avbl = 2 * used;
    dpth++;
    used = 0;
  }
}

struct CodeWork {
  uint32_t key[NUM_LL];      // freq << 9 | symbol of the used symbols, then sorted
  uint32_t A[NUM_LL];
  uint32_t count[64];        // codes per length (an unlimited code over 286 symbols of <= 2^17 occurrences is < 64 deep)
};

// len[s] (0 = unused) of a prefix code over freq[0 .. n) with no length above maxbits: complete when two or more symbols
// are used, never over-subscribed.  One used symbol gets length 1; none leaves all lengths 0.  Ties are broken by the
// symbol value, so the code is a function of the histogram.  freq[s] < 2^23 (a chunk holds at most 65536 tokens).
// Returns the number of used symbols.
GZ_HD int limited_lengths(const uint32_t *freq, int n, int maxbits, uint8_t *len, CodeWork *w) {
  int used = 0;
  for (int s = 0; s < n; s++) {
    len[s] = 0;
    if (freq[s]) w->key[used++] = freq[s] << 9 | (uint32_t)s;
  }
  if (used == 0) return 0;
  if (used == 1) { len[w->key[0] & 511] = 1; return 1; }
  for (int i = 1; i < used; i++) {   // insertion sort: at most 286 keys, nearly all of them small
    const uint32_t k = w->key[i];
    int j = i - 1;
    while (j >= 0 && w->key[j] > k) { w->key[j + 1] = w->key[j]; j--; }
    w->key[j + 1] = k;
  }
  for (int i = 0; i < used; i++) w->A[i] = w->key[i] >> 9;
  minimum_redundancy(w->A, used);
  for (int i = 0; i < 64; i++) w->count[i] = 0;
  for (int i = 0; i < used; i++) w->count[w->A[i] < 63 ? w->A[i] : 63]++;
  // the limit: everything deeper than maxbits moves up to maxbits, then the Kraft sum is paid back from the deepest
  // shorter codes (one code one level down frees half of its share)
  for (int i = maxbits + 1; i < 64; i++) { w->count[maxbits] += w->count[i]; w->count[i] = 0; }
  uint32_t total = 0;
  for (int i = maxbits; i >= 1; i--) total += w->count[i] << (maxbits - i);
  for (int guard = 0; guard < (1 << MAX_BITS) && total != (1u << maxbits); guard++) {
    w->count[maxbits]--;
    for (int i = maxbits - 1; i >= 1; i--)
      if (w->count[i]) { w->count[i]--; w->count[i + 1] += 2; break; }
    total--;
  }
  // rarest symbols get the longest codes
  int j = used;
  for (int i = 1; i <= maxbits; i++)
    for (uint32_t l = w->count[i]; l > 0; l--) len[w->key[--j] & 511] = (uint8_t)i;
  return used;
}

// canonical codes of RFC 1951 3.2.2, stored bit-reversed (deflate packs prefix codes from their most significant bit)
GZ_HD void canonical_codes(const uint8_t *len, int n, int maxbits, uint16_t *code, CodeWork *w) {
  uint32_t *count = w->count, *next = w->count + MAX_BITS + 2;   // work arrays outside the registers
  for (int i = 0; i <= maxbits; i++) count[i] = 0;
  for (int s = 0; s < n; s++) count[len[s]]++;
  count[0] = 0;
  uint32_t c = 0;
  for (int b = 1; b <= maxbits; b++) { c = (c + count[b - 1]) << 1; next[b] = c; }
  for (int s = 0; s < n; s++) code[s] = len[s] ? (uint16_t)bit_reverse(next[len[s]]++, len[s]) : 0;
}

// ---- bits, least significant first, to bytes
struct BitSink {
  uint8_t *out;
  uint64_t acc = 0;
  int nb = 0;
  uint64_t total = 0;   // bits put so far
};
GZ_HD void put_bits(BitSink *b, uint32_t v, int n) {   // n <= 32
  b->acc |= (uint64_t)v << b->nb;
  b->nb += n;
  b->total += (uint64_t)n;
  while (b->nb >= 8) { *b->out++ = (uint8_t)b->acc; b->acc >>= 8; b->nb -= 8; }
}

struct ChunkCode {
  uint8_t ll_len[NUM_LL], d_len[NUM_D];
  uint16_t ll_code[NUM_LL], d_code[NUM_D];
};
struct HeaderWork {
  CodeWork cw;
  uint8_t seq_sym[MAX_CL_SEQ], seq_extra[MAX_CL_SEQ];
  uint32_t cl_freq[NUM_CL];
  uint8_t cl_len[NUM_CL];
  uint16_t cl_code[NUM_CL];
};

// The codes of one chunk from its histograms (ll_freq[EOB] included), and the dynamic block header (BFINAL = 0,
// BTYPE = 10, HLIT, HDIST, HCLEN, the code-length code, the run-length coded lengths) into sink; bits that do not fill
// a byte stay in sink->acc.  *body_bits = the bits all symbols and their extra bits will take.
GZ_HD void build_chunk_code(const uint32_t *ll_freq, const uint32_t *d_freq, ChunkCode *cc, HeaderWork *w, BitSink *sink,
                            uint64_t *body_bits) {
  limited_lengths(ll_freq, NUM_LL, MAX_BITS, cc->ll_len, &w->cw);
  // no distance used: one code of zero bits; one used: one code of one bit (RFC 1951 3.2.7)
  limited_lengths(d_freq, NUM_D, MAX_BITS, cc->d_len, &w->cw);
  canonical_codes(cc->ll_len, NUM_LL, MAX_BITS, cc->ll_code, &w->cw);
  canonical_codes(cc->d_len, NUM_D, MAX_BITS, cc->d_code, &w->cw);
  uint64_t bits = 0;
  for (int s = 0; s < NUM_LL; s++) bits += (uint64_t)ll_freq[s] * (uint32_t)(cc->ll_len[s] + (s > 256 ? len_ebits(s) : 0));
  for (int s = 0; s < NUM_D; s++) bits += (uint64_t)d_freq[s] * (uint32_t)(cc->d_len[s] + dist_ebits(s));
  *body_bits = bits;
  int hlit = NUM_LL, hdist = NUM_D;
  while (hlit > 257 && cc->ll_len[hlit - 1] == 0) hlit--;
  while (hdist > 1 && cc->d_len[hdist - 1] == 0) hdist--;
  // the lengths of both codes as one sequence, run-length coded with 16 / 17 / 18
  const int n = hlit + hdist;
  int m = 0;
  for (int s = 0; s < NUM_CL; s++) w->cl_freq[s] = 0;
  for (int i = 0; i < n;) {
    const int v = i < hlit ? cc->ll_len[i] : cc->d_len[i - hlit];
    int run = 1;
    while (i + run < n && (i + run < hlit ? cc->ll_len[i + run] : cc->d_len[i + run - hlit]) == v) run++;
    i += run;
    if (v == 0) {
      while (run > 0) {
        if (run >= 11) { const int r = run < 138 ? run : 138; w->seq_sym[m] = 18; w->seq_extra[m++] = (uint8_t)(r - 11); run -= r; }
        else if (run >= 3) { w->seq_sym[m] = 17; w->seq_extra[m++] = (uint8_t)(run - 3); run = 0; }
        else { w->seq_sym[m] = 0; w->seq_extra[m++] = 0; run--; }
      }
    } else {
      w->seq_sym[m] = (uint8_t)v; w->seq_extra[m++] = 0; run--;
      while (run > 0) {
        if (run >= 3) { const int r = run < 6 ? run : 6; w->seq_sym[m] = 16; w->seq_extra[m++] = (uint8_t)(r - 3); run -= r; }
        else { w->seq_sym[m] = (uint8_t)v; w->seq_extra[m++] = 0; run--; }
      }
    }
  }
  for (int i = 0; i < m; i++) w->cl_freq[w->seq_sym[i]]++;
  if (limited_lengths(w->cl_freq, NUM_CL, MAX_CL_BITS, w->cl_len, &w->cw) == 1) {
    // the code-length code must be complete: a second code of one bit beside the only one in use
    w->cl_len[w->cl_len[0] ? 1 : 0] = 1;
  }
  canonical_codes(w->cl_len, NUM_CL, MAX_CL_BITS, w->cl_code, &w->cw);
  const uint8_t order[NUM_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  int hclen = NUM_CL;
  while (hclen > 4 && w->cl_len[order[hclen - 1]] == 0) hclen--;
  put_bits(sink, 0, 1);
  put_bits(sink, 2, 2);
  put_bits(sink, (uint32_t)(hlit - 257), 5);
  put_bits(sink, (uint32_t)(hdist - 1), 5);
  put_bits(sink, (uint32_t)(hclen - 4), 4);
  for (int i = 0; i < hclen; i++) put_bits(sink, w->cl_len[order[i]], 3);
  for (int i = 0; i < m; i++) {
    const int s = w->seq_sym[i];
    put_bits(sink, w->cl_code[s], w->cl_len[s]);
    if (s == 16) put_bits(sink, w->seq_extra[i], 2);
    else if (s == 17) put_bits(sink, w->seq_extra[i], 3);
    else if (s == 18) put_bits(sink, w->seq_extra[i], 7);
  }
}

// ---- CRC-32 (the polynomial of RFC 1952, bit-reflected: bit 31 is x^0)
constexpr uint32_t CRC_POLY = 0xedb88320u;
GZ_HD uint32_t crc_table_entry(uint32_t i) {
  for (int k = 0; k < 8; k++) i = (i & 1) ? (i >> 1) ^ CRC_POLY : i >> 1;
  return i;
}
GZ_HD uint32_t gf_mul(uint32_t a, uint32_t b) {   // a * b mod P
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1) ? (b >> 1) ^ CRC_POLY : b >> 1;
  }
  return p;
}
GZ_HD uint32_t gf_x_pow(uint64_t n) {   // x^n mod P
  uint32_t r = 0x80000000u, b = 0x40000000u;
  for (int i = 0; i < 64 && n; i++, n >>= 1) {
    if (n & 1) r = gf_mul(r, b);
    b = gf_mul(b, b);
  }
  return r;
}
// crc(A || B) from crc(A), crc(B) and x^(8 |B|)
GZ_HD uint32_t crc_join(uint32_t crc_a, uint32_t crc_b, uint32_t x_pow_8lenb) { return gf_mul(crc_a, x_pow_8lenb) ^ crc_b; }

}  // namespace gz
#endif
