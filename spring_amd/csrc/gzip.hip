// spring_amd/csrc/gzip.hip -- gzip members compressed on the device (include/spring_gzip.h): the
// gzip_flag branch of write_fastq_block (reference src/util.cpp:70-110) for the text the assembler left in HBM.
//
//   member cuts  ->  chunk table  ->  match + parse (one wavefront per chunk, hash table in LDS)  ->  histograms, length-
//   limited codes and the block header (one wavefront per chunk, gzip_codes.h)  ->  emit (token bit lengths, scan, bits
//   through LDS into the chunk's slot)  ->  CRC-32 per chunk  ->  scan of the chunk sizes  ->  the copy of headers,
//   chunks and trailers to their final place, one 16-byte word per lane (copy_words.h).
//
// Every loop on the device has a static bound; a wrong table entry ends in a wrong byte.
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "copy_words.h"
#include "fastq_out_internal.h"
#include "gzip_codes.h"
#include "reorder_device.h"
#include "reorder_internal.h"
#include "spring_gzip.h"
#include "stage_host.h"

using namespace sr;

namespace {

constexpr uint32_t DEFAULT_CHUNK = 32768;
constexpr int HASH_BITS = 14;                  // 16384 slots of 16 bits: 32 KiB of LDS per workgroup
constexpr int INTRA = 16;                      // candidates looked for among the lanes below, this far
constexpr uint32_t STORED_MAX = 65535;
constexpr uint32_t F_FIRST = 1, F_LAST = 2, F_STORED = 4;
constexpr uint64_t BATCH_TOKEN_BYTES = 1ull << 30;   // token scratch of one batch of chunks
constexpr int EMIT_T = 256;
constexpr int STAGE_WORDS = EMIT_T * 48 / 32 + 4;

__host__ __device__ inline uint32_t stored_size(uint32_t len) { return len + 5 * ((len + STORED_MAX - 1) / STORED_MAX); }

// per chunk
struct Chunks {
  uint64_t *start;     // first byte in the source
  uint32_t *len;
  uint32_t *member;
  uint32_t *flags;     // F_*
  uint32_t *payload;   // bytes of its deflate blocks
  uint32_t *crc;
  uint32_t *ntok, *hdr_bits, *carry;
  uint8_t *slots;      // the coded form of chunk c is built at slots + slot_off[c] (16-byte aligned, as large as its
  uint64_t *slot_off;  // stored form: a chunk is only coded when that is smaller)
};

// ------------------------------------------------------------------ cuts and the chunk table
// member m of a fastq_out text = records [m * R, min((m + 1) * R, n))
__global__ void k_member_cuts(const uint64_t *__restrict__ rec_off, uint64_t n, uint64_t R, uint64_t M,
                              uint64_t *__restrict__ moff) {
  const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m > M) return;
  const uint64_t r = m * R;
  moff[m] = rec_off[r < n ? r : n];
}
__host__ __device__ inline uint32_t slot_size(uint32_t len) { return (stored_size(len) + 16 + 15) & ~15u; }
__global__ void k_chunk_count(const uint64_t *__restrict__ moff, uint64_t M, uint32_t chunk, uint32_t *__restrict__ cnt) {
  const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m > M) return;
  cnt[m] = m < M ? (uint32_t)((moff[m + 1] - moff[m] + chunk - 1) / chunk) : 0;
}
// one entry per chunk; every chunk starts out stored
__global__ void k_chunk_table(const uint64_t *__restrict__ moff, const uint64_t *__restrict__ cfirst, uint64_t M,
                              uint64_t NC, uint32_t chunk, Chunks C) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= NC) return;
  const uint64_t lo = last_le(M, c, cfirst);   // the last member whose first chunk is <= c
  const uint64_t k = c - cfirst[lo], s = moff[lo] + k * chunk, e = min(s + chunk, moff[lo + 1]);
  C.start[c] = s;
  C.len[c] = (uint32_t)(e - s);
  C.member[c] = (uint32_t)lo;
  C.flags[c] = (k == 0 ? F_FIRST : 0) | (e == moff[lo + 1] ? F_LAST : 0) | F_STORED;
  C.payload[c] = stored_size((uint32_t)(e - s));
}
__global__ void k_slot_sizes(Chunks C, uint64_t NC, uint32_t *__restrict__ sz) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c > NC) return;
  sz[c] = c < NC ? slot_size(C.len[c]) : 0;
}

// ------------------------------------------------------------------ match + parse
// four bytes from t + a on; t is 4-byte aligned and at least 7 bytes exist behind a
__device__ __forceinline__ uint32_t ld32u(const uint8_t *__restrict__ t, uint64_t a) {
  const uint32_t *w = reinterpret_cast<const uint32_t *>(t + (a & ~3ull));
  const uint64_t v = (uint64_t)w[1] << 32 | w[0];
  return (uint32_t)(v >> (8 * (uint32_t)(a & 3)));
}
__device__ __forceinline__ uint32_t hash4(uint32_t v) { return (v * 0x9E3779B1u) >> (32 - HASH_BITS); }

// tab[h] = rel for the lanes that ask; of lanes that meet in a slot the highest rel stays, whatever order the stores of
// a wavefront land in: a lane that reads back less than it wrote writes again.  rel only grows from call to call.
__device__ __forceinline__ void insert_max(uint16_t *tab, bool want, uint32_t h, uint32_t rel) {
  bool pend = want;
  for (int it = 0; it < 64; it++) {
    if (pend) tab[h] = (uint16_t)rel;
    __syncthreads();
    if (pend) pend = tab[h] < rel;
    __syncthreads();
    if (__ballot(pend) == 0) break;
  }
}

// One wavefront per chunk.  Positions are kept as rel = p - (chunk start - window) in 16 bits.  The table is primed with
// the window before the chunk (never before the member's start); then 64 positions at a time: every lane looks up the
// latest earlier position with its four bytes (among the lanes below, else in the table), extends the match up to 258
// bytes and the chunk's end, the window's positions enter the table, and the wavefront walks its 64 lengths greedily.
// A position whose four bytes would reach past the chunk's end neither looks up nor enters: the tokens depend on the
// bytes of the member up to the chunk's end and on nothing else.
__global__ __launch_bounds__(64) void k_match(const uint8_t *__restrict__ t, const uint64_t *__restrict__ moff, Chunks C,
                                              uint64_t first, uint32_t chunk_bytes, uint32_t window,
                                              uint32_t *__restrict__ tokens) {
  __shared__ uint16_t tab[1 << HASH_BITS];
  const uint32_t lane = threadIdx.x;
  const uint64_t c = first + blockIdx.x;
  const uint64_t cs = C.start[c], ce = cs + C.len[c], ms = moff[C.member[c]];
  const int64_t base = (int64_t)cs - (int64_t)window;
  const uint64_t lo = base > (int64_t)ms ? (uint64_t)base : ms;
  uint32_t *tok = tokens + (uint64_t)blockIdx.x * chunk_bytes;
  for (uint32_t i = lane; i < (1u << HASH_BITS) / 2; i += 64) reinterpret_cast<uint32_t *>(tab)[i] = 0;
  __syncthreads();
  for (uint32_t k = 0; k < 32768 / 64; k++) {   // the window
    const uint64_t p = lo + (uint64_t)k * 64 + lane;
    if (lo + (uint64_t)k * 64 >= cs) break;
    const bool valid = p < cs && p + 4 <= ce;
    const uint32_t v = valid ? ld32u(t, p) : 0;
    insert_max(tab, valid, hash4(v), (uint32_t)((int64_t)p - base));
  }
  uint64_t cur = cs;
  uint32_t nt = 0;
  for (uint32_t iter = 0; iter < 65536 && cur < ce; iter++) {
    const uint64_t p = cur + lane;
    const bool valid = p + 4 <= ce;
    const uint32_t v = p < ce ? ld32u(t, p) : 0;
    const uint32_t h = hash4(v);
    const uint64_t vm = __ballot(valid);
    uint32_t len = 0, dist = 0;
    for (int d = 1; d <= INTRA; d++) {   // the nearest lane below with the same four bytes
      const uint32_t vj = __shfl_up(v, d);
      if (!dist && valid && lane >= (uint32_t)d && ((vm >> (lane - d)) & 1) && vj == v) dist = (uint32_t)d;
    }
    if (valid && !dist) {
      const int64_t q = base + (int64_t)tab[h];
      if (q >= (int64_t)lo && q < (int64_t)p && p - (uint64_t)q <= (uint64_t)gz::MAX_DIST && ld32u(t, (uint64_t)q) == v)
        dist = (uint32_t)(p - (uint64_t)q);
    }
    if (dist) {
      const uint64_t q = p - dist;
      const uint32_t maxlen = (uint32_t)min((uint64_t)gz::MAX_MATCH, ce - p);
      len = 4;
      for (int k = 0; k < 64 && len < maxlen; k++) {
        const uint32_t x = ld32u(t, p + len) ^ ld32u(t, q + len);
        if (x) { len += (uint32_t)__builtin_ctz(x) >> 3; break; }
        len += 4;
      }
      len = min(len, maxlen);
    }
    __syncthreads();   // every lane has read its slot
    insert_max(tab, valid, h, (uint32_t)((int64_t)p - base));
    const uint64_t mask = __ballot(len >= (uint32_t)gz::MIN_MATCH);
    const uint32_t wend = (uint32_t)min((uint64_t)64, ce - cur);
    uint32_t pos = 0;
    for (int it = 0; it < 64 && pos < wend; it++) {
      const uint64_t m = mask >> pos;
      uint32_t nlit = m ? (uint32_t)__builtin_ctzll(m) : 64u;
      nlit = min(nlit, wend - pos);
      if (lane >= pos && lane < pos + nlit) tok[nt + lane - pos] = v & 0xffu;
      nt += nlit;
      pos += nlit;
      if (pos < wend) {   // a match starts at lane pos
        const uint32_t L = __shfl(len, (int)pos), D = __shfl(dist, (int)pos);
        if (lane == pos) tok[nt] = gz::TOK_MATCH | (L - 3) << 16 | (D - 1);
        nt++;
        pos += L;
      }
    }
    cur += pos;
  }
  if (lane == 0) C.ntok[c] = nt;
}

// ------------------------------------------------------------------ codes and the block header
__device__ __forceinline__ void token_symbols(uint32_t tk, int *ls, int *leb, int *lev, int *ds, int *deb, int *dev) {
  *ls = gz::len_symbol((int)((tk >> 16) & 0xff) + 3, leb, lev);
  *ds = gz::dist_symbol((int)(tk & 0x7fff) + 1, deb, dev);
}

// One wavefront per chunk: histograms of its tokens, then lane 0 builds the two codes and the header (gzip_codes.h).  A
// chunk whose coded form is not smaller than its stored form stays stored.
__global__ __launch_bounds__(64) void k_codes(Chunks C, uint64_t first, uint32_t chunk_bytes,
                                              const uint32_t *__restrict__ tokens, gz::ChunkCode *__restrict__ codes) {
  __shared__ uint32_t ll_freq[gz::NUM_LL], d_freq[gz::NUM_D];
  __shared__ __align__(16) gz::ChunkCode cc;
  __shared__ gz::HeaderWork hw;
  __shared__ __align__(16) uint32_t hbuf[160];   // the header: at most 4498 bits
  __shared__ uint32_t s_bits, s_coded;
  const uint32_t lane = threadIdx.x;
  const uint64_t c = first + blockIdx.x;
  const uint32_t *tok = tokens + (uint64_t)blockIdx.x * chunk_bytes;
  const uint32_t nt = C.ntok[c];
  for (uint32_t i = lane; i < gz::NUM_LL; i += 64) ll_freq[i] = 0;
  if (lane < gz::NUM_D) d_freq[lane] = 0;
  for (uint32_t i = lane; i < 160; i += 64) hbuf[i] = 0;
  __syncthreads();
  for (uint32_t i = lane; i < nt; i += 64) {
    const uint32_t tk = tok[i];
    if (tk & gz::TOK_MATCH) {
      int ls, leb, lev, ds, deb, dev;
      token_symbols(tk, &ls, &leb, &lev, &ds, &deb, &dev);
      atomicAdd(&ll_freq[ls], 1u);
      atomicAdd(&d_freq[ds], 1u);
    } else {
      atomicAdd(&ll_freq[tk & 0xff], 1u);
    }
  }
  __syncthreads();
  if (lane == 0) {
    ll_freq[gz::EOB] = 1;
    gz::BitSink bs;
    bs.out = reinterpret_cast<uint8_t *>(hbuf);
    uint64_t body = 0;
    gz::build_chunk_code(ll_freq, d_freq, &cc, &hw, &bs, &body);
    if (bs.nb) *bs.out = (uint8_t)bs.acc;   // the bits that do not fill a byte
    // header, tokens, end of block, the 3 header bits of the empty stored block, padding, its LEN and NLEN
    const uint64_t coded = (bs.total + body + 3 + 7) / 8 + 4;
    s_bits = (uint32_t)bs.total;
    s_coded = coded < (uint64_t)stored_size(C.len[c]) ? (uint32_t)coded : 0;
  }
  __syncthreads();
  if (s_coded == 0) return;   // stays stored
  uint32_t *slot = reinterpret_cast<uint32_t *>(C.slots + C.slot_off[c]);
  const uint32_t full = s_bits / 32;
  for (uint32_t i = lane; i < full; i += 64) slot[i] = hbuf[i];
  uint32_t *dst = reinterpret_cast<uint32_t *>(codes + blockIdx.x);
  const uint32_t *src = reinterpret_cast<const uint32_t *>(&cc);
  for (uint32_t i = lane; i < sizeof(gz::ChunkCode) / 4; i += 64) dst[i] = src[i];
  if (lane == 0) {
    C.hdr_bits[c] = s_bits;
    C.carry[c] = hbuf[full];
    C.payload[c] = s_coded;
    C.flags[c] &= ~F_STORED;
  }
}

// ------------------------------------------------------------------ emit
// One workgroup per coded chunk.  256 tokens at a time: code and extra bits of a token (at most 48), an exclusive scan
// of the bit counts, the bits OR-ed into an LDS stage at their offsets, the stage's full words stored to the slot.
__global__ __launch_bounds__(EMIT_T) void k_emit(Chunks C, uint64_t first, uint32_t chunk_bytes,
                                                 const uint32_t *__restrict__ tokens, const gz::ChunkCode *__restrict__ codes) {
  __shared__ __align__(16) gz::ChunkCode cc;
  __shared__ uint32_t stage[STAGE_WORDS];
  __shared__ uint32_t wsum[EMIT_T / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t c = first + blockIdx.x;
  if (C.flags[c] & F_STORED) return;
  const uint32_t *tok = tokens + (uint64_t)blockIdx.x * chunk_bytes;
  const uint32_t nt = C.ntok[c];
  {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(codes + blockIdx.x);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&cc);
    for (uint32_t i = tid; i < sizeof(gz::ChunkCode) / 4; i += EMIT_T) dst[i] = src[i];
  }
  for (uint32_t i = tid; i < STAGE_WORDS; i += EMIT_T) stage[i] = 0;
  __syncthreads();
  uint32_t *slot = reinterpret_cast<uint32_t *>(C.slots + C.slot_off[c]);
  uint64_t pos = C.hdr_bits[c];   // bits of the chunk's stream so far; the words below pos / 32 are in the slot
  if (tid == 0) stage[0] = C.carry[c];
  __syncthreads();
  for (uint32_t t0 = 0; t0 < nt; t0 += EMIT_T) {   // at most chunk_bytes / 256 turns
    uint64_t bits = 0;
    uint32_t nb = 0;
    if (t0 + tid < nt) {
      const uint32_t tk = tok[t0 + tid];
      if (tk & gz::TOK_MATCH) {
        int ls, leb, lev, ds, deb, dev;
        token_symbols(tk, &ls, &leb, &lev, &ds, &deb, &dev);
        bits = cc.ll_code[ls]; nb = cc.ll_len[ls];
        bits |= (uint64_t)lev << nb; nb += leb;
        bits |= (uint64_t)cc.d_code[ds] << nb; nb += cc.d_len[ds];
        bits |= (uint64_t)dev << nb; nb += deb;
      } else {
        bits = cc.ll_code[tk & 0xff]; nb = cc.ll_len[tk & 0xff];
      }
    }
    uint32_t incl = nb;   // inclusive scan in the wavefront, then across the four of them
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(incl, d);
      if (lane >= (uint32_t)d) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, sum = 0;
    for (uint32_t w = 0; w < EMIT_T / 64; w++) { if (w < wave) before += wsum[w]; sum += wsum[w]; }
    const uint32_t r = (uint32_t)(pos & 31);
    const uint32_t off = r + before + incl - nb;
    if (nb) {
      const uint32_t w = off >> 5, sh = off & 31;
      const uint64_t a = bits << sh;
      atomicOr(&stage[w], (uint32_t)a);
      if (sh + nb > 32) atomicOr(&stage[w + 1], (uint32_t)(a >> 32));
      if (sh + nb > 64) atomicOr(&stage[w + 2], (uint32_t)(bits >> (64 - sh)));
    }
    __syncthreads();
    const uint32_t full = (r + sum) >> 5;
    const uint64_t w0 = pos >> 5;
    for (uint32_t i = tid; i < full; i += EMIT_T) slot[w0 + i] = stage[i];
    __syncthreads();
    const uint32_t rem = stage[full];
    __syncthreads();
    for (uint32_t i = tid; i <= full; i += EMIT_T) stage[i] = 0;
    __syncthreads();
    if (tid == 0) stage[0] = rem;
    __syncthreads();
    pos += sum;
  }
  if (tid == 0) {   // end of block; an empty stored block (BFINAL on the member's last chunk) ends the chunk on a byte
    uint64_t acc = stage[0];
    uint32_t n = (uint32_t)(pos & 31);
    acc |= (uint64_t)cc.ll_code[gz::EOB] << n; n += cc.ll_len[gz::EOB];
    acc |= (uint64_t)((C.flags[c] & F_LAST) ? 1 : 0) << n; n += 3;
    n = (n + 7) & ~7u;
    uint8_t *o = reinterpret_cast<uint8_t *>(slot) + (pos >> 5) * 4;
    uint32_t k = 0;
    for (; k < n / 8; k++) o[k] = (uint8_t)(acc >> (8 * k));
    o[k] = 0; o[k + 1] = 0; o[k + 2] = 0xff; o[k + 3] = 0xff;
  }
}

// ------------------------------------------------------------------ CRC-32
// One workgroup per chunk.  The chunk is cut into 256 slices of equal length that end at the chunk's end (the first
// ones are short or empty: zero bytes in front of a message do not change a remainder); every lane runs the table over
// its slice, the one that holds the first byte from the preset 0xffffffff, and the states are joined pairwise:
// state(A || B) = state(A) * x^(8 |B|) + state(B)  (mod P).
__global__ __launch_bounds__(256) void k_crc(const uint8_t *__restrict__ t, Chunks C, uint64_t NC) {
  __shared__ uint32_t tab[256], st[256];
  const uint32_t tid = threadIdx.x;
  const uint64_t c = blockIdx.x;
  if (c >= NC) return;
  tab[tid] = gz::crc_table_entry(tid);
  const uint64_t cs = C.start[c];
  const uint32_t len = C.len[c], s = (len + 255) / 256, pad = 256 * s - len;
  const uint32_t v0 = tid * s, v1 = v0 + s;   // with the padding in front
  const uint32_t a = v0 > pad ? v0 - pad : 0, b = v1 > pad ? v1 - pad : 0;
  __syncthreads();
  uint32_t crc = (a == 0 && b > 0) ? 0xffffffffu : 0;
  uint32_t i = a;
  for (int k = 0; k < 15 && i < b && ((cs + i) & 15); k++, i++) crc = tab[(crc ^ t[cs + i]) & 0xff] ^ (crc >> 8);
  for (int k = 0; k < 16 && i + 16 <= b; k++, i += 16) {   // the slice's aligned 16-byte words: at most 256 bytes a slice
    const uint4 w = *reinterpret_cast<const uint4 *>(t + cs + i);
    const uint32_t x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      crc ^= x[j];
#pragma unroll
      for (int r = 0; r < 4; r++) crc = tab[crc & 0xff] ^ (crc >> 8);
    }
  }
  for (int k = 0; k < 15 && i < b; k++, i++) crc = tab[(crc ^ t[cs + i]) & 0xff] ^ (crc >> 8);
  st[tid] = crc;
  uint32_t xp = gz::gf_x_pow(8ull * s);
  for (uint32_t stride = 1; stride < 256; stride <<= 1) {
    __syncthreads();
    if ((tid & (2 * stride - 1)) == 0) st[tid] = gz::gf_mul(st[tid], xp) ^ st[tid + stride];
    xp = gz::gf_mul(xp, xp);
  }
  if (tid == 0) C.crc[c] = st[0] ^ 0xffffffffu;
}

// ------------------------------------------------------------------ compaction
__global__ void k_seg_sizes(Chunks C, uint64_t NC, uint32_t *__restrict__ seg) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c > NC) return;
  seg[c] = c < NC ? C.payload[c] + ((C.flags[c] & F_FIRST) ? 10 : 0) + ((C.flags[c] & F_LAST) ? 8 : 0) : 0;
}

struct CompactArg {
  const uint8_t *t;            // the source, t[0, limit) exists
  uint64_t limit;
  Chunks C;
  const uint64_t *out_off;     // NC + 1: where the segment of a chunk (member header, blocks, member trailer) starts
  const uint32_t *m_crc, *m_isize;
  uint64_t NC, total;
  uint8_t *out;
};

// A lane owns one 16-byte word of the output, finds the chunk that covers its first byte and walks the pieces that
// overlap the word: the member header before a member's first chunk, the chunk's blocks (from its slot, or stored:
// 5 bytes of block header and up to 65535 bytes of the source, at most twice), the trailer behind its last chunk.
__global__ __launch_bounds__(256) void k_compact(CompactArg A) {
  const uint64_t p = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16;
  if (p >= A.total) return;
  const uint64_t end = min(p + 16, A.total);
  uint64_t c = last_le(A.NC, p, A.out_off), q = p;
  u128 acc = 0;
  for (int guard = 0; guard < 16 && q < end; guard++) {   // a segment is at least 6 bytes
    const uint64_t so = A.out_off[c];
    const uint32_t flags = A.C.flags[c], payload = A.C.payload[c], len = A.C.len[c];
    const uint32_t hdr = (flags & F_FIRST) ? 10 : 0, size = hdr + payload + ((flags & F_LAST) ? 8 : 0);
    uint32_t k = (uint32_t)(q - so);
    for (int g2 = 0; g2 < 16 && q < end && k < size; g2++) {
      const uint32_t left = (uint32_t)(end - q);
      uint32_t n = 1;
      u128 v = 0;
      if (k < hdr) {                       // 1f 8b 08 00, mtime 0, XFL 0, OS 255
        v = k == 0 ? 0x1f : k == 1 ? 0x8b : k == 2 ? 8 : k == 9 ? 0xff : 0;
      } else if (k < hdr + payload) {
        const uint32_t j = k - hdr;
        if (!(flags & F_STORED)) {
          n = min(payload - j, left);
          v = fetch(A.C.slots, A.C.slot_off[c] + j, n, ~0ull);
        } else {
          const uint32_t b = j / (STORED_MAX + 5), r = j % (STORED_MAX + 5);
          const uint32_t bl = min(STORED_MAX, len - b * STORED_MAX);
          if (r < 5) {
            const uint32_t fin = ((flags & F_LAST) && b * STORED_MAX + bl == len) ? 1 : 0;
            v = r == 0 ? fin : r == 1 ? (bl & 0xff) : r == 2 ? (bl >> 8) : r == 3 ? (~bl & 0xff) : ((~bl >> 8) & 0xff);
          } else {
            n = min(bl - (r - 5), left);
            v = fetch(A.t, A.C.start[c] + (uint64_t)b * STORED_MAX + (r - 5), n, A.limit);
          }
        }
      } else {                             // CRC-32, ISIZE
        const uint32_t x = k - hdr - payload, m = A.C.member[c];
        v = ((x < 4 ? A.m_crc[m] : A.m_isize[m]) >> (8 * (x & 3))) & 0xff;
      }
      acc |= v << (8 * (uint32_t)(q - p));
      q += n;
      k += n;
    }
    c++;
  }
  put16(A.out, p, (uint32_t)(end - p), acc);
}

// ------------------------------------------------------------------ host side

}  // namespace

struct spring_gzip_ctx {
  int dev = 0;
  hipStream_t st = nullptr;
  uint32_t chunk_bytes = DEFAULT_CHUNK;
  uint64_t token_bytes = BATCH_TOKEN_BYTES;
  bool have = false;
  spring_gzip_info info;
  DBuf out, out_off, cfirst;   // the members; per chunk and per member where they start
};

namespace {

void drop_result(spring_gzip_ctx *ctx) {
  ctx->have = false;
  ctx->out.release();
  ctx->out_off.release();
  ctx->cfirst.release();
  memset(&ctx->info, 0, sizeof(ctx->info));
}

// t[0, nbytes) on the device (16-byte aligned, limit bytes exist, 8 readable bytes behind nbytes); the cuts are either
// d_rec_off with member_records (a fastq_out text) or h_moff (host, M + 1 offsets).
int compress(spring_gzip_ctx *ctx, const uint8_t *t, uint64_t nbytes, const uint64_t *d_rec_off, uint64_t n_rec,
             uint64_t member_records, const uint64_t *h_moff, uint64_t M, int32_t mode, spring_gzip_info *info_out) {
  const int dev = ctx->dev;
  hipStream_t st = ctx->st;
  const uint32_t chunk = ctx->chunk_bytes, window = std::min<uint32_t>(32768, 65536 - chunk);
  spring_gzip_info I;
  memset(&I, 0, sizeof(I));
  I.chunk_bytes = chunk;
  I.bytes_in = nbytes;
  if (nbytes == 0) {   // no members at all
    ctx->info = I;
    ctx->have = true;
    if (info_out) *info_out = I;
    return 0;
  }
  Events ev;
  for (auto &e : ev.e) HIPCHK(hipEventCreate(&e));
  DBuf moff, cnt, tmp, b_start, b_len, b_member, b_flags, b_payload, b_crc, b_ntok, b_hbits, b_carry, slots, tokens, codes,
      seg, m_crc, m_isize, b_slotoff;
  SyncOnExit sync_on_exit{st};
  HIPCHK(hipEventRecord(ev.e[0], st));
  // ---- cuts, chunk table
  DALLOC(moff, (M + 1) * 8);
  if (d_rec_off)
    hipLaunchKernelGGL(k_member_cuts, grid(M + 1), dim3(256), 0, st, d_rec_off, n_rec, member_records, M, moff.as<uint64_t>());
  else
    HIPCHK(hipMemcpyAsync(moff.p, h_moff, (M + 1) * 8, hipMemcpyHostToDevice, st));
  DALLOC(cnt, (M + 1) * 4);
  DALLOC(ctx->cfirst, (M + 1) * 8);
  hipLaunchKernelGGL(k_chunk_count, grid(M + 1), dim3(256), 0, st, moff.as<uint64_t>(), M, chunk, cnt.as<uint32_t>());
  size_t tb = 0;
  HIPCHK(sr::excl_scan_u32_to_u64(st, nullptr, tb, nullptr, nullptr, M + 1));
  DALLOC(tmp, tb + 16);
  HIPCHK(sr::excl_scan_u32_to_u64(st, tmp.p, tb, cnt.as<uint32_t>(), ctx->cfirst.as<uint64_t>(), M + 1));
  uint64_t NC = 0;
  HIPCHK(rd(st, &NC, ctx->cfirst.as<uint64_t>() + M, 8));
  if (NC == 0 || NC > nbytes) return fail(SPRING_REORDER_E_ARG, "the member cuts do not cover the %llu bytes", (unsigned long long)nbytes);
  Chunks C;
  DALLOC(b_start, NC * 8); DALLOC(b_len, NC * 4); DALLOC(b_member, NC * 4); DALLOC(b_flags, NC * 4);
  DALLOC(b_payload, NC * 4); DALLOC(b_crc, NC * 4); DALLOC(b_ntok, NC * 4); DALLOC(b_hbits, NC * 4); DALLOC(b_carry, NC * 4);
  C.start = b_start.as<uint64_t>(); C.len = b_len.as<uint32_t>(); C.member = b_member.as<uint32_t>();
  C.flags = b_flags.as<uint32_t>(); C.payload = b_payload.as<uint32_t>(); C.crc = b_crc.as<uint32_t>();
  C.ntok = b_ntok.as<uint32_t>(); C.hdr_bits = b_hbits.as<uint32_t>(); C.carry = b_carry.as<uint32_t>();
  C.slots = nullptr;
  C.slot_off = nullptr;
  hipLaunchKernelGGL(k_chunk_table, grid(NC), dim3(256), 0, st, moff.as<uint64_t>(), ctx->cfirst.as<uint64_t>(), M, NC, chunk, C);
  HIPCHK(hipEventRecord(ev.e[1], st));
  // ---- match + parse, codes, emit: in batches that share one token buffer
  float ms_match = 0, ms_codes = 0, ms_emit = 0;
  if (mode == SPRING_GZIP_DEFLATE) {
    // a slot per chunk, sized by the chunk (a member of one record must not cost a slot of chunk_bytes)
    DALLOC(seg, (NC + 1) * 4);
    DALLOC(b_slotoff, (NC + 1) * 8);
    C.slot_off = b_slotoff.as<uint64_t>();
    hipLaunchKernelGGL(k_slot_sizes, grid(NC + 1), dim3(256), 0, st, C, NC, seg.as<uint32_t>());
    size_t tbs = 0;
    HIPCHK(sr::excl_scan_u32_to_u64(st, nullptr, tbs, nullptr, nullptr, NC + 1));
    if (tbs > tb) { HIPCHK(hipStreamSynchronize(st)); DALLOC(tmp, tbs + 16); tb = tbs; }
    HIPCHK(sr::excl_scan_u32_to_u64(st, tmp.p, tbs, seg.as<uint32_t>(), C.slot_off, NC + 1));
    DALLOC(slots, nbytes + NC * 48 + 32);   // the sum of the slot sizes is at most this
    C.slots = slots.as<uint8_t>();
    const uint64_t batch = std::min<uint64_t>(NC, std::max<uint64_t>(1, ctx->token_bytes / ((uint64_t)chunk * 4)));
    DALLOC(tokens, batch * chunk * 4);
    DALLOC(codes, batch * sizeof(gz::ChunkCode));
    Events bev;
    for (int k = 0; k < 4; k++) HIPCHK(hipEventCreate(&bev.e[k]));
    for (uint64_t first = 0; first < NC; first += batch) {
      const unsigned nb = (unsigned)std::min<uint64_t>(batch, NC - first);
      HIPCHK(hipEventRecord(bev.e[0], st));
      hipLaunchKernelGGL(k_match, dim3(nb), dim3(64), 0, st, t, moff.as<uint64_t>(), C, first, chunk, window, tokens.as<uint32_t>());
      HIPCHK(hipEventRecord(bev.e[1], st));
      hipLaunchKernelGGL(k_codes, dim3(nb), dim3(64), 0, st, C, first, chunk, tokens.as<uint32_t>(), codes.as<gz::ChunkCode>());
      HIPCHK(hipEventRecord(bev.e[2], st));
      hipLaunchKernelGGL(k_emit, dim3(nb), dim3(EMIT_T), 0, st, C, first, chunk, tokens.as<uint32_t>(), codes.as<gz::ChunkCode>());
      HIPCHK(hipEventRecord(bev.e[3], st));
      HIPCHK(hipStreamSynchronize(st));
      float a = 0, b = 0, c = 0;
      HIPCHK(hipEventElapsedTime(&a, bev.e[0], bev.e[1]));
      HIPCHK(hipEventElapsedTime(&b, bev.e[1], bev.e[2]));
      HIPCHK(hipEventElapsedTime(&c, bev.e[2], bev.e[3]));
      ms_match += a; ms_codes += b; ms_emit += c;
      I.num_batches++;
    }
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(ev.e[2], st));
  // ---- CRC-32 of every chunk; joined per member on the host (one multiplication per chunk)
  hipLaunchKernelGGL(k_crc, dim3((unsigned)NC), dim3(256), 0, st, t, C, NC);
  HIPCHK(hipEventRecord(ev.e[3], st));
  std::vector<uint32_t> h_crc(NC), h_len(NC), h_flags(NC), hm_crc(M), hm_isize(M);
  HIPCHK(hipMemcpyAsync(h_crc.data(), C.crc, NC * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(h_len.data(), C.len, NC * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(rd(st, h_flags.data(), C.flags, NC * 4));
  {
    const uint32_t xp_chunk = gz::gf_x_pow(8ull * chunk);
    uint64_t m = 0, isize = 0;
    uint32_t crc = 0;
    for (uint64_t c = 0; c < NC; c++) {
      if (h_flags[c] & F_FIRST) { crc = h_crc[c]; isize = h_len[c]; }
      else { crc = gz::crc_join(crc, h_crc[c], h_len[c] == chunk ? xp_chunk : gz::gf_x_pow(8ull * h_len[c])); isize += h_len[c]; }
      if (h_flags[c] & F_STORED) I.chunks_stored++;
      if (h_flags[c] & F_LAST) {
        if (m >= M) return fail(SPRING_REORDER_E_HIP, "the chunk table holds more members than the cuts");
        hm_crc[m] = crc; hm_isize[m] = (uint32_t)isize; m++;
      }
    }
    if (m != M) return fail(SPRING_REORDER_E_HIP, "the chunk table holds %llu members, the cuts %llu", (unsigned long long)m, (unsigned long long)M);
  }
  DALLOC(m_crc, M * 4); DALLOC(m_isize, M * 4);
  HIPCHK(hipMemcpyAsync(m_crc.p, hm_crc.data(), M * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(m_isize.p, hm_isize.data(), M * 4, hipMemcpyHostToDevice, st));
  // ---- sizes, scan, the copy
  HIPCHK(hipEventRecord(ev.e[4], st));
  if (!seg.p) DALLOC(seg, (NC + 1) * 4);
  DALLOC(ctx->out_off, (NC + 1) * 8);
  hipLaunchKernelGGL(k_seg_sizes, grid(NC + 1), dim3(256), 0, st, C, NC, seg.as<uint32_t>());
  size_t tb2 = 0;
  HIPCHK(sr::excl_scan_u32_to_u64(st, nullptr, tb2, nullptr, nullptr, NC + 1));
  if (tb2 > tb) { HIPCHK(hipStreamSynchronize(st)); DALLOC(tmp, tb2 + 16); }
  HIPCHK(sr::excl_scan_u32_to_u64(st, tmp.p, tb2, seg.as<uint32_t>(), ctx->out_off.as<uint64_t>(), NC + 1));
  uint64_t total = 0;
  HIPCHK(rd(st, &total, ctx->out_off.as<uint64_t>() + NC, 8));
  DALLOC(ctx->out, total + 16);
  CompactArg A;
  A.t = t; A.limit = nbytes; A.C = C; A.out_off = ctx->out_off.as<uint64_t>();
  A.m_crc = m_crc.as<uint32_t>(); A.m_isize = m_isize.as<uint32_t>(); A.NC = NC; A.total = total;
  A.out = ctx->out.as<uint8_t>();
  hipLaunchKernelGGL(k_compact, grid(total, 4096), dim3(256), 0, st, A);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev.e[5], st));
  HIPCHK(hipStreamSynchronize(st));
  float ms[3] = {0, 0, 0}, all = 0;
  HIPCHK(hipEventElapsedTime(&ms[0], ev.e[0], ev.e[1]));
  HIPCHK(hipEventElapsedTime(&ms[1], ev.e[2], ev.e[3]));
  HIPCHK(hipEventElapsedTime(&ms[2], ev.e[4], ev.e[5]));
  HIPCHK(hipEventElapsedTime(&all, ev.e[0], ev.e[5]));
  I.num_members = M;
  I.num_chunks = NC;
  I.bytes_out = total;
  I.ms_device = all;
  I.ms_pass[0] = ms[0]; I.ms_pass[1] = ms_match; I.ms_pass[2] = ms_codes; I.ms_pass[3] = ms_emit; I.ms_pass[4] = ms[1];
  I.ms_pass[5] = ms[2];
  ctx->info = I;
  ctx->have = true;
  if (info_out) *info_out = I;
  return 0;
}

}  // namespace

extern "C" {

int spring_gzip_create(int device, spring_gzip_ctx **out) {
  if (!out) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  const int r = stage_device(&device, "the gzip stage");
  if (r) return r;
  spring_gzip_ctx *c = new spring_gzip_ctx();
  c->dev = device;
  memset(&c->info, 0, sizeof(c->info));
  *out = c;
  return 0;
}

void spring_gzip_destroy(spring_gzip_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->dev);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  drop_result(ctx);
  if (ctx->st) (void)hipStreamDestroy(ctx->st);
  delete ctx;
}

int spring_gzip_set_chunk_bytes(spring_gzip_ctx *ctx, uint32_t chunk_bytes) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (chunk_bytes < 4096 || chunk_bytes > 65536 || chunk_bytes % 4096)
    return fail(SPRING_REORDER_E_ARG, "chunk_bytes must be a multiple of 4096 in 4096 .. 65536 (got %u)", chunk_bytes);
  ctx->chunk_bytes = chunk_bytes;
  return 0;
}

int spring_gzip_set_token_bytes(spring_gzip_ctx *ctx, uint64_t bytes) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  ctx->token_bytes = bytes ? bytes : BATCH_TOKEN_BYTES;
  return 0;
}

int spring_gzip_from_fastq_out(spring_gzip_ctx *ctx, spring_fastq_out_ctx *text, uint64_t member_records, int32_t mode,
                               spring_gzip_info *info) {
  if (!ctx || !text) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  (void)hipSetDevice(ctx->dev);
  drop_result(ctx);
  if (mode != SPRING_GZIP_STORED && mode != SPRING_GZIP_DEFLATE) return fail(SPRING_REORDER_E_ARG, "bad mode %d", mode);
  sr::FastqOutView V;
  int r = sr::fastq_out_view(text, &V);
  if (r) return r;
  if (V.dev != ctx->dev) return fail(SPRING_REORDER_E_ARG, "assembler and gzip contexts live on different devices");
  const uint64_t n = V.info.num_units;
  const uint64_t M = n == 0 ? 0 : member_records == 0 ? 1 : (n + member_records - 1) / member_records;
  if (M > 0xffffffffull) return fail(SPRING_REORDER_E_ARG, "too many members");
  if ((r = stream_begin(ctx->dev, &ctx->st))) return r;
  r = compress(ctx, V.text, V.info.bytes, V.rec_off, n, member_records == 0 ? n : member_records, nullptr, M, mode, info);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  if (r) drop_result(ctx);
  return r;
}

int spring_gzip_from_host(spring_gzip_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const uint64_t *member_off,
                          uint64_t num_members, int32_t mode, spring_gzip_info *info) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  (void)hipSetDevice(ctx->dev);
  drop_result(ctx);
  if (mode != SPRING_GZIP_STORED && mode != SPRING_GZIP_DEFLATE) return fail(SPRING_REORDER_E_ARG, "bad mode %d", mode);
  if (nbytes && !bytes) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  const uint64_t one[2] = {0, nbytes};
  if (!member_off) { member_off = one; num_members = nbytes ? 1 : 0; }
  if (num_members > 0xffffffffull) return fail(SPRING_REORDER_E_ARG, "too many members");
  if (member_off[0] != 0 || member_off[num_members] != nbytes)
    return fail(SPRING_REORDER_E_ARG, "the member cuts do not start at 0 and end at the %llu bytes", (unsigned long long)nbytes);
  for (uint64_t m = 0; m < num_members; m++)
    if (member_off[m + 1] <= member_off[m]) return fail(SPRING_REORDER_E_ARG, "the member cuts do not increase strictly");
  int r = stream_begin(ctx->dev, &ctx->st);
  if (r) return r;
  const int dev = ctx->dev;
  DBuf up;
  DALLOC(up, nbytes + 32);
  if (nbytes) HIPCHK(hipMemcpyAsync(up.p, bytes, nbytes, hipMemcpyHostToDevice, ctx->st));
  r = compress(ctx, up.as<uint8_t>(), nbytes, nullptr, 0, 0, member_off, num_members, mode, info);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  if (r) drop_result(ctx);
  return r;
}

int spring_gzip_get_info(spring_gzip_ctx *ctx, spring_gzip_info *info) {
  if (!ctx || !info) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing compressed yet");
  *info = ctx->info;
  return 0;
}

int spring_gzip_download(spring_gzip_ctx *ctx, uint8_t *gz_out, uint64_t *member_off) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing compressed yet");
  HIPCHK(hipSetDevice(ctx->dev));
  const uint64_t M = ctx->info.num_members, NC = ctx->info.num_chunks;
  if (gz_out && ctx->info.bytes_out) HIPCHK(rd(ctx->st, gz_out, ctx->out.p, ctx->info.bytes_out));
  if (member_off) {
    member_off[0] = 0;
    if (M) {   // member m starts where its first chunk's segment starts
      std::vector<uint64_t> cf(M + 1), oo(NC + 1);
      HIPCHK(hipMemcpyAsync(cf.data(), ctx->cfirst.p, (M + 1) * 8, hipMemcpyDeviceToHost, ctx->st));
      HIPCHK(rd(ctx->st, oo.data(), ctx->out_off.p, (NC + 1) * 8));
      for (uint64_t m = 0; m <= M; m++) member_off[m] = oo[cf[m]];
    }
  }
  return 0;
}

int spring_gzip_write(spring_gzip_ctx *ctx, const char *path, int32_t append, spring_gzip_info *info) {
  if (!ctx || !path) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing compressed yet");
  const auto t0 = std::chrono::steady_clock::now();
  const int fd = open(path, O_WRONLY | O_CREAT | (append ? O_APPEND : O_TRUNC), 0644);
  if (fd < 0) return fail(SPRING_REORDER_E_IO, "cannot open %s for writing: %s", path, strerror(errno));
  // A ring of two pinned chunks: chunk i + 1 is on its way from the device while chunk i goes to the file.
  struct Ring {
    void *pin[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    int fd;
    ~Ring() {
      for (int k = 0; k < 2; k++) { if (ev[k]) (void)hipEventDestroy(ev[k]); if (pin[k]) sr::pinned_put(pin[k]); }
      if (fd >= 0) close(fd);
    }
  } R;
  R.fd = fd;
  HIPCHK(hipSetDevice(ctx->dev));
  const uint64_t total = ctx->info.bytes_out, nchunk = (total + sr::PIN_CHUNK - 1) / sr::PIN_CHUNK;
  if (nchunk) { const int r = stream_begin(ctx->dev, &ctx->st); if (r) return r; }
  for (int k = 0; k < 2 && (uint64_t)k < nchunk; k++) {
    if (!(R.pin[k] = sr::pinned_get())) return fail(SPRING_REORDER_E_HIP, "cannot pin a staging chunk for the members");
    HIPCHK(hipEventCreateWithFlags(&R.ev[k], hipEventDisableTiming));
  }
  auto chunk_len = [&](uint64_t i) { return (size_t)std::min<uint64_t>(sr::PIN_CHUNK, total - i * sr::PIN_CHUNK); };
  auto issue = [&](uint64_t i) -> hipError_t {
    hipError_t e = hipMemcpyAsync(R.pin[i & 1], ctx->out.as<uint8_t>() + i * sr::PIN_CHUNK, chunk_len(i),
                                  hipMemcpyDeviceToHost, ctx->st);
    return e != hipSuccess ? e : hipEventRecord(R.ev[i & 1], ctx->st);
  };
  if (nchunk) HIPCHK(issue(0));
  for (uint64_t i = 0; i < nchunk; i++) {
    HIPCHK(hipEventSynchronize(R.ev[i & 1]));
    if (i + 1 < nchunk) HIPCHK(issue(i + 1));   // into the other chunk: written out one turn ago
    const uint8_t *p = (const uint8_t *)R.pin[i & 1];
    size_t left = chunk_len(i);
    while (left) {
      const ssize_t w = write(fd, p, left);
      if (w < 0 && errno == EINTR) continue;
      if (w <= 0) {
        const int e = errno;
        (void)hipStreamSynchronize(ctx->st);
        return fail(SPRING_REORDER_E_IO, "write failed for %s: %s", path, strerror(e));
      }
      p += w;
      left -= (size_t)w;
    }
  }
  R.fd = -1;
  if (close(fd) != 0) return fail(SPRING_REORDER_E_IO, "close failed for %s: %s", path, strerror(errno));
  ctx->info.ms_file = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (info) *info = ctx->info;
  return 0;
}

}  // extern "C"
