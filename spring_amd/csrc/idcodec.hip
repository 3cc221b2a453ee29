// spring_amd/csrc/idcodec.hip -- SPRING's id codec for the id blocks of a run in HBM (include/spring_idcodec.h;
// DESIGN.md section 17): the bytes compress_id_block (reference src/util.cpp:113-126, src/id_compression/) writes to
// id_N.<block>.
//
//   line offsets (scan of length + 1)  ->  k_tokens<Count>: one lane per line counts its symbols, applies the refusals
//   and reports its token count  ->  scan: symbol offsets  ->  k_tokens<Write>: the symbol words  ->  k_block_off: the
//   symbol offset of every block  ->  k_code: one wavefront per block, sub-batch by sub-batch: models in global memory,
//   output into a per-block buffer sized from the block's symbol count  ->  k_gather: the blocks back to back.
//
// The token symbols of a line depend on that line and on the line before it in the block only: the token boundaries of
// an id are a function of the id alone, so a lane re-derives the previous id's token starts while it walks its own.
// Every loop on the device is bounded by data checked before it: a line's length (at most 1 023), a block's symbol
// count, 26 renormalisation steps per symbol, the pending-bit count (at most the steps taken so far).
#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include <hip/hip_runtime.h>

#include "fastq_out_internal.h"
#include "reorder_device.h"
#include "reorder_internal.h"
#include "spring_idcodec.h"
#include "stage_host.h"

using namespace sr;

namespace {

constexpr uint32_t MAX_ID = SPRING_IDCODEC_MAX_ID, MAX_RUN = SPRING_IDCODEC_MAX_RUN;
constexpr uint32_t NUM_LIMIT = 1u << 28;   // a number stops taking digits once its value reaches this
enum : uint32_t { T_ALPHA = 0, T_DIGIT = 1, T_CHAR = 2, T_MATCH = 3, T_ZEROS = 4, T_DELTA = 5, T_END = 6 };
enum : uint32_t { K_TYPE = 0, K_ALEN = 1, K_ABYTE = 2, K_CHAR = 3, K_DELTA = 4, K_ZEROS = 5, K_INT = 6 };
// refusals, in the low bits of the word the tokenizer reports (the line above them: the first line wins)
enum : uint32_t { E_LONG = 1, E_BYTE = 2, E_LETTERS = 3, E_ZEROS = 4, E_NEWLINE = 5 };

// The models of one token number (one context), in 32-bit words: [0, 10) the counts of the token type, [16, 26) the
// sums n of the ten models (type, the five byte-wide kinds 1 .. 5, the four bytes of a number), then nine tables of 256
// counts: kinds 1 .. 5, then the four bytes of a number.  2 336 words = 9 344 bytes.
constexpr uint32_t CTX_N = 16, CTX_TABLES = 32, CTX_WORDS = CTX_TABLES + 9 * 256;
constexpr uint32_t RESCALE = 1u << 20, STEP = 10;
constexpr uint32_t WORD_BITS = 26, HALF = 1u << (WORD_BITS - 1), LOW_MASK = HALF - 1;
// Output bound.  A model's n is below 2^20 when a symbol is coded (it is halved as soon as it reaches that), a count is
// at least 1 and the interval is wider than 2^24 after a renormalisation (neither of its conditions holds), so a coded
// symbol leaves an interval of at least floor((2^24 + 1) / (2^20 - 1)) = 16.  Every renormalisation step doubles the
// interval and none is taken once it is wider than 2^25: at most 22 steps a symbol.  Every step puts out one bit, at
// once or as a pending bit; the end adds 26 bits and pads to a byte, always writing the byte in progress.
constexpr uint32_t MAX_STEPS = 22, RENORM_BOUND = 26;
inline uint64_t block_capacity(uint64_t symbols) {
  const uint64_t bytes = (MAX_STEPS * symbols + WORD_BITS) / 8 + 1;
  return ((bytes + 7) & ~7ull) + 8;   // whole 4-byte stores stay inside it
}

// ------------------------------------------------------------------ tokenizer
__device__ __forceinline__ bool is_letter(uint32_t b) { return (b | 32u) - 'a' < 26u; }
__device__ __forceinline__ bool is_digit(uint32_t b) { return b - '0' < 10u; }

// where the token that starts at s[c] ends (c < n)
__device__ __forceinline__ uint32_t token_end(const uint8_t *s, uint32_t n, uint32_t c, uint32_t *value) {
  const uint32_t b = s[c];
  uint32_t e = c + 1;
  if (is_letter(b)) {
    while (e < n && is_letter(s[e])) e++;
  } else if (b == '0') {
    while (e < n && s[e] == '0') e++;
  } else if (is_digit(b)) {
    uint32_t v = b - '0';
    while (e < n && v < NUM_LIMIT && is_digit(s[e])) v = v * 10 + (s[e++] - '0');
    *value = v;
  }
  return e;
}

struct Count {
  uint32_t n = 0;
  __device__ __forceinline__ void put(uint32_t, uint32_t, uint32_t) { n++; }
};
struct Write {
  uint32_t *w;
  __device__ __forceinline__ void put(uint32_t kind, uint32_t ctx, uint32_t value) { *w++ = value | (kind << 8) | (ctx << 11); }
};

// The symbols of cur[0 .. n) after prev[0 .. plen), both at most MAX_ID bytes.  Returns the token count; *err receives
// a run that is too long.
template <class Sink>
__device__ uint32_t tokenize(const uint8_t *cur, uint32_t n, const uint8_t *prev, uint32_t plen, Sink &S, uint32_t *err) {
  auto pb = [&](uint32_t i) -> uint32_t { return i < plen ? prev[i] : 0u; };
  uint32_t c = 0, t = 0, pp = 0;   // pp: where token t of prev starts, plen once prev has no more tokens
  while (c < n) {
    const uint32_t p = pp < plen ? pp : 0;
    const uint32_t b = cur[c];
    uint32_t v = 0;
    const uint32_t e = token_end(cur, n, c, &v), len = e - c;
    bool same = true;   // the token's bytes equal prev's from p on
    if (is_letter(b)) {
      if (len > MAX_RUN) *err = E_LETTERS;
      for (uint32_t k = 0; k < len && same; k++) same = cur[c + k] == pb(p + k);
      if (same && !is_letter(pb(p + len))) {
        S.put(K_TYPE, t, T_MATCH);
      } else {
        S.put(K_TYPE, t, T_ALPHA);
        S.put(K_ALEN, t, len & 0xff);
        for (uint32_t k = 0; k < len; k++) S.put(K_ABYTE, t, cur[c + k]);
      }
    } else if (b == '0') {
      if (len > MAX_RUN) *err = E_ZEROS;
      for (uint32_t k = 0; k < len && same; k++) same = pb(p + k) == '0';
      if (same && pb(p + len) != '0') {
        S.put(K_TYPE, t, T_MATCH);
      } else {
        S.put(K_TYPE, t, T_ZEROS);
        S.put(K_ZEROS, t, len & 0xff);
      }
    } else if (is_digit(b)) {
      bool is_num = true;
      uint32_t pv = 0;
      if (plen) {
        is_num = is_digit(pb(p)) && pb(p) != '0';
        if (is_num) {
          pv = pb(p) - '0';
          for (uint32_t k = 1; pv < NUM_LIMIT && is_digit(pb(p + k)); k++) pv = pv * 10 + (pb(p + k) - '0');
        }
      }
      for (uint32_t k = 0; k < len && same; k++) same = cur[c + k] == pb(p + k);
      const int32_t d = (int32_t)(v - pv);
      if (is_num && same && !is_digit(pb(p + len))) {
        S.put(K_TYPE, t, T_MATCH);
      } else if (is_num && d > 0 && d < 256) {
        S.put(K_TYPE, t, T_DELTA);
        S.put(K_DELTA, t, (uint32_t)d);
      } else {
        S.put(K_TYPE, t, T_DIGIT);
        for (uint32_t k = 0; k < 4; k++) S.put(K_INT, 4 * t + k, (v >> (8 * k)) & 0xff);
      }
    } else if (b == pb(p)) {
      S.put(K_TYPE, t, T_MATCH);
    } else {
      S.put(K_TYPE, t, T_CHAR);
      S.put(K_CHAR, t, b);
    }
    if (pp < plen) {
      uint32_t unused;
      pp = token_end(prev, plen, pp, &unused);
    }
    c = e;
    t++;
  }
  S.put(K_TYPE, t, T_END);
  return t;
}

struct Lines {
  const uint8_t *t;      // the lines back to back, each with its '\n'
  const uint64_t *off;   // n + 1 line starts
  uint64_t n;
  uint32_t B;            // lines per block: line i has a previous line unless i % B == 0
};

// Pass 1 (Sink = Count): cnt[i] = the symbols of line i; stat[0] = the largest token count; *err = the first refused
// line and why.  Pass 2 (Sink = Write): the symbol words of line i from sym[sym_off[i]] on; runs only after pass 1 found
// nothing to refuse, so every length it meets is at most MAX_ID.
template <class Sink>
__global__ __launch_bounds__(256) void k_tokens(Lines L, uint32_t *__restrict__ cnt, uint32_t *__restrict__ stat,
                                                unsigned long long *__restrict__ err, uint32_t *__restrict__ sym,
                                                const uint64_t *__restrict__ sym_off) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  uint32_t ntok = 0;
  if (i < L.n) {
    const uint64_t a = L.off[i], z = L.off[i + 1];
    const uint32_t n = (uint32_t)min(z - a - 1, (uint64_t)MAX_ID + 1);
    const uint8_t *cur = L.t + a;
    uint32_t plen = 0;
    const uint8_t *prev = cur;
    if (i % L.B) {
      const uint64_t pa = L.off[i - 1];
      plen = (uint32_t)min(a - pa - 1, (uint64_t)MAX_ID + 1);
      prev = L.t + pa;
    }
    uint32_t e = 0;
    if (n > MAX_ID) e = E_LONG;
    else if (cur[n] != '\n') e = E_NEWLINE;
    else
      for (uint32_t k = 0; k < n; k++)
        if (cur[k] == 0 || cur[k] >= 128) e = E_BYTE;
    Sink S;
    if constexpr (std::is_same<Sink, Write>::value) S.w = sym + sym_off[i];
    if (!e && plen <= MAX_ID) ntok = tokenize(cur, n, prev, plen, S, &e);   // a previous line that is too long is refused by its own lane
    if constexpr (std::is_same<Sink, Count>::value) {
      cnt[i] = S.n;
      if (e) atomicMin(err, (unsigned long long)((i << 3) | e));
    }
  }
  if constexpr (std::is_same<Sink, Count>::value) {
    uint32_t mx = ntok;
    for (int o = 32; o; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&stat[0], mx);
  }
}

// len1[i] = len[i] + 1 (the '\n') for i < n, 0 at n: the input of the line-offset scan
__global__ __launch_bounds__(256) void k_len1(const uint32_t *__restrict__ len, uint64_t n, uint32_t *__restrict__ len1) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  if (i <= n) len1[i] = i < n ? len[i] + 1 : 0;
}

// blk[b] = sym_off[min(b * B, n)], b <= nb
__global__ __launch_bounds__(256) void k_block_off(const uint64_t *__restrict__ sym_off, uint64_t n, uint64_t B, uint64_t nb,
                                                   uint64_t *__restrict__ blk) {
  const uint64_t b = blockIdx.x * 256ull + threadIdx.x;
  if (b <= nb) blk[b] = sym_off[min(b * B, n)];
}

// ------------------------------------------------------------------ coder
struct Coder {
  const uint32_t *sym;
  const uint64_t *sym_off;   // per block + 1
  const uint64_t *cap_off;   // per block + 1: its buffer in out
  uint8_t *out;
  uint64_t *out_len;         // per block: the bytes written
  uint32_t *tables;          // count * nctx * CTX_WORDS words
  uint32_t *flag;            // set when a block met a word outside the tables or the end of its buffer
  uint32_t first, count;     // the sub-batch
  uint32_t nctx;             // contexts per block
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// The bits of a block, most significant first, in whole 4-byte stores by lane 0; the state is the same in every lane.
struct BitOut {
  uint8_t *dst;
  uint64_t cap, pos = 0;
  uint64_t acc = 0;
  uint32_t nacc = 0;   // bits of acc not stored yet: below 32 between calls
  bool overrun = false;
  __device__ __forceinline__ void put(uint32_t v, uint32_t k) {   // 1 <= k <= 32
    acc = (acc << k) | v;
    nacc += k;
    if (nacc >= 32) {
      const uint32_t w = (uint32_t)(acc >> (nacc - 32));
      if (pos + 4 <= cap) {
        if (threadIdx.x == 0) *reinterpret_cast<uint32_t *>(dst + pos) = __builtin_bswap32(w);
      } else {
        overrun = true;
      }
      pos += 4;
      nacc -= 32;
    }
  }
  __device__ __forceinline__ void run(uint32_t bit, uint64_t count) {
    while (count) {
      const uint32_t k = count < 32 ? (uint32_t)count : 32u;
      put(bit ? (uint32_t)((1ull << k) - 1) : 0u, k);
      count -= k;
    }
  }
  // pads the byte in progress with zeros and always writes it; returns the bytes of the block
  __device__ __forceinline__ uint64_t finish() {
    const uint32_t tail = (uint32_t)(acc << (32 - nacc)), nb = nacc / 8 + 1;
    for (uint32_t k = 0; k < nb; k++) {
      if (pos + k < cap) {
        if (threadIdx.x == 0) dst[pos + k] = (uint8_t)(tail >> (24 - 8 * k));
      } else {
        overrun = true;
      }
    }
    return pos + nb;
  }
};

__global__ __launch_bounds__(64) void k_code(Coder G) {
  const uint32_t lane = threadIdx.x;
  const uint32_t b = G.first + blockIdx.x;
  uint32_t *T = G.tables + (uint64_t)blockIdx.x * G.nctx * CTX_WORDS;
  {   // all counts 1; n = the alphabet: 10 for the type, 256 for the other nine models
    const uint32_t quads = G.nctx * (CTX_WORDS / 4);
    for (uint32_t q = lane; q < quads; q += 64) {
      const uint32_t w = (q % (CTX_WORDS / 4)) * 4;
      uint4 v = make_uint4(1, 1, 1, 1);
      if (w == CTX_N) v = make_uint4(10, 256, 256, 256);
      else if (w == CTX_N + 4) v = make_uint4(256, 256, 256, 256);
      else if (w == CTX_N + 8) v = make_uint4(256, 256, 1, 1);
      reinterpret_cast<uint4 *>(T)[q] = v;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  const uint64_t s0 = G.sym_off[b], s1 = G.sym_off[b + 1];
  uint32_t l = 0, u = (1u << WORD_BITS) - 1;
  uint64_t pending = 0;
  BitOut O;
  O.dst = G.out + G.cap_off[b];
  O.cap = G.cap_off[b + 1] - G.cap_off[b];
  bool bad = false;
  for (uint64_t base = s0; base < s1 && !bad; base += 64) {
    const uint32_t mine = base + lane < s1 ? G.sym[base + lane] : 0u;
    const uint32_t here = s1 - base < 64 ? (uint32_t)(s1 - base) : 64u;
    for (uint32_t j = 0; j < here; j++) {
      const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)j);
      const uint32_t x = w & 0xff, kind = (w >> 8) & 7, ctx = (w >> 11) & 0xfff;
      const uint32_t t = kind == K_INT ? ctx >> 2 : ctx;
      if (t >= G.nctx || kind > K_INT || (kind == K_TYPE && x >= 10)) { bad = true; break; }
      uint32_t *C = T + t * CTX_WORDS;
      uint32_t *np = C + CTX_N + (kind == K_INT ? 6 + (ctx & 3) : kind);
      uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)*np);
      uint32_t cum, cx, n2;
      if (kind == K_TYPE) {
        uint32_t c = lane < 10 ? C[lane] : 0u;
        cum = wave_sum(lane < x ? c : 0u);
        cx = (uint32_t)__builtin_amdgcn_readlane((int)c, (int)x);
        n2 = n + STEP;
        if (lane == x) c += STEP;
        if (n2 >= RESCALE) {
          c = lane < 10 ? (c >> 1) + 1 : 0u;
          if (lane < 10) C[lane] = c;
          n2 = wave_sum(c);
        } else if (lane == x) {
          C[lane] = c;
        }
      } else {
        uint32_t *M = C + CTX_TABLES + (kind == K_INT ? 5 + (ctx & 3) : kind - 1) * 256;
        uint4 c = reinterpret_cast<const uint4 *>(M)[lane];
        const uint32_t i0 = 4 * lane;
        cum = wave_sum((i0 < x ? c.x : 0u) + (i0 + 1 < x ? c.y : 0u) + (i0 + 2 < x ? c.z : 0u) + (i0 + 3 < x ? c.w : 0u));
        const uint32_t e = x & 3, sel = e == 0 ? c.x : e == 1 ? c.y : e == 2 ? c.z : c.w;
        cx = (uint32_t)__builtin_amdgcn_readlane((int)sel, (int)(x >> 2));
        n2 = n + STEP;
        if (lane == (x >> 2)) {
          if (e == 0) c.x += STEP; else if (e == 1) c.y += STEP; else if (e == 2) c.z += STEP; else c.w += STEP;
        }
        if (n2 >= RESCALE) {
          c.x = (c.x >> 1) + 1; c.y = (c.y >> 1) + 1; c.z = (c.z >> 1) + 1; c.w = (c.w >> 1) + 1;
          reinterpret_cast<uint4 *>(M)[lane] = c;
          n2 = wave_sum(c.x + c.y + c.z + c.w);
        } else if (lane == (x >> 2)) {
          M[x] = cx + STEP;
        }
      }
      if (lane == 0) *np = n2;
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // the next symbol's loads come behind these stores
      // ---- the interval: exact 64-bit arithmetic
      const uint64_t range = (uint64_t)u - l + 1;
      u = l + (uint32_t)(range * (cum + cx) / n) - 1;
      l = l + (uint32_t)(range * cum / n);
      for (uint32_t step = 0; step < RENORM_BOUND; step++) {
        const uint32_t ml = l >> (WORD_BITS - 1), mu = u >> (WORD_BITS - 1);
        if (ml == mu) {   // top bits equal: that bit, then the pending opposite bits
          O.put(ml, 1);
          O.run(ml ^ 1, pending);
          pending = 0;
          l = (l & LOW_MASK) << 1;
          u = ((u & LOW_MASK) << 1) + 1;
        } else if ((l >> (WORD_BITS - 2)) == 1 && (u >> (WORD_BITS - 2)) == 2) {   // 01... and 10...: the middle expansion
          pending++;
          u = (((u << 1) & LOW_MASK) | HALF) + 1;
          l = (l << 1) & LOW_MASK;
        } else {
          break;
        }
      }
    }
  }
  const uint32_t ml = l >> (WORD_BITS - 1);
  O.put(ml, 1);
  O.run(ml ^ 1, pending);
  O.put(l & LOW_MASK, WORD_BITS - 1);
  const uint64_t bytes = O.finish();
  if (lane == 0) {
    G.out_len[b] = bytes;
    if (bad || O.overrun) atomicOr(G.flag, bad ? 1u : 2u);
  }
}

// block b of the capacity buffers -> its place in the result; blockIdx.y strides over the block's bytes
__global__ __launch_bounds__(256) void k_gather(const uint8_t *__restrict__ src, const uint64_t *__restrict__ cap_off,
                                                const uint64_t *__restrict__ out_off, uint8_t *__restrict__ dst) {
  const uint64_t b = blockIdx.x;
  const uint64_t n = out_off[b + 1] - out_off[b];
  const uint8_t *s = src + cap_off[b];
  uint8_t *d = dst + out_off[b];
  for (uint64_t i = blockIdx.y * 256ull + threadIdx.x; i < n; i += 256ull * gridDim.y) d[i] = s[i];
}

}  // namespace

struct spring_idcodec_ctx {
  int dev = 0;
  hipStream_t st = nullptr;
  uint64_t workspace_bytes = 0;   // 0: from the free HBM
  bool have = false;
  spring_idcodec_info info;
  DBuf out, sym;
  std::vector<uint64_t> out_off, sym_off;   // num_blocks + 1 each
};

namespace {

void drop_result(spring_idcodec_ctx *ctx) {
  ctx->have = false;
  ctx->out.release();
  ctx->sym.release();
  ctx->out_off.clear();
  ctx->sym_off.clear();
  memset(&ctx->info, 0, sizeof(ctx->info));
}

uint64_t workspace_need(uint64_t blocks, uint64_t max_tokens) { return blocks * (max_tokens + 1) * CTX_WORDS * 4; }

int refuse(uint64_t line, uint32_t why) {
  const unsigned long long i = (unsigned long long)line;
  switch (why) {
    case E_LONG: return fail(SPRING_REORDER_E_ARG, "id %llu is longer than %u bytes", i, MAX_ID);
    case E_BYTE: return fail(SPRING_REORDER_E_ARG, "id %llu holds a byte 0 or >= 128", i);
    case E_LETTERS: return fail(SPRING_REORDER_E_ARG, "id %llu holds a run of more than %u letters", i, MAX_RUN);
    case E_ZEROS: return fail(SPRING_REORDER_E_ARG, "id %llu holds a run of more than %u zeros", i, MAX_RUN);
    default: return fail(SPRING_REORDER_E_ARG, "id %llu does not end in a newline", i);
  }
}

// d_lines: nbytes bytes on the device, n lines with their '\n'; d_len: their n (+ 1 readable) lengths without it.
int run(spring_idcodec_ctx *ctx, const uint8_t *d_lines, uint64_t nbytes, const uint32_t *d_len, uint64_t n, uint32_t B,
        spring_idcodec_info *info_out) {
  const int dev = ctx->dev;
  hipStream_t st = ctx->st;
  if (n >= (1ull << 39)) return fail(SPRING_REORDER_E_ARG, "too many lines");
  spring_idcodec_info I;
  memset(&I, 0, sizeof(I));
  I.num_lines = n;
  const uint64_t nb = (n + B - 1) / B;
  I.num_blocks = nb;
  if (nb >= 0x7fffffffull) return fail(SPRING_REORDER_E_ARG, "too many blocks");
  ctx->out_off.assign(nb + 1, 0);
  ctx->sym_off.assign(nb + 1, 0);
  if (n == 0) {
    ctx->info = I;
    ctx->have = true;
    if (info_out) *info_out = I;
    return 0;
  }
  Events ev;
  HIPCHK(hipEventCreate(&ev.a)); HIPCHK(hipEventCreate(&ev.b));
  DBuf len1, loff, cnt, soff, tmp, stat, d_blk, d_cap, d_len_out, d_out_off, tables, flag, cap_buf;
  SyncOnExit sync_on_exit{st};
  float ms = 0;
  // ---- tokens, pass 1
  size_t tb = 0;
  HIPCHK(sr::excl_scan_u32_to_u64(st, nullptr, tb, nullptr, nullptr, n + 1));
  DALLOC(tmp, tb + 16);
  DALLOC(len1, (n + 1) * 4); DALLOC(loff, (n + 1) * 8); DALLOC(cnt, (n + 1) * 4); DALLOC(soff, (n + 1) * 8);
  DALLOC(stat, 16);   // [0] the largest token count; bytes 8 .. 15 the first refusal
  const unsigned long long stat0[2] = {0, ~0ull};
  HIPCHK(hipMemcpyAsync(stat.p, stat0, 16, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(cnt.p, 0, (n + 1) * 4, st));
  HIPCHK(hipEventRecord(ev.a, st));
  hipLaunchKernelGGL(k_len1, grid(n + 1), dim3(256), 0, st, d_len, n, len1.as<uint32_t>());
  size_t t2 = tb;
  HIPCHK(sr::excl_scan_u32_to_u64(st, tmp.p, t2, len1.as<uint32_t>(), loff.as<uint64_t>(), n + 1));
  HIPCHK(hipEventRecord(ev.b, st));
  uint64_t total = 0;
  HIPCHK(rd(st, &total, loff.as<uint64_t>() + n, 8));
  if (total != nbytes)   // the kernels below read nothing outside [0, nbytes)
    return fail(SPRING_REORDER_E_ARG, "the line lengths take %llu bytes, the lines hold %llu", (unsigned long long)total,
                (unsigned long long)nbytes);
  HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
  I.ms_tokens += ms;
  Lines L;
  L.t = d_lines; L.off = loff.as<uint64_t>(); L.n = n; L.B = B;
  unsigned long long *d_err = stat.as<unsigned long long>() + 1;
  HIPCHK(hipEventRecord(ev.a, st));
  hipLaunchKernelGGL(k_tokens<Count>, grid(n), dim3(256), 0, st, L, cnt.as<uint32_t>(), stat.as<uint32_t>(), d_err,
                     (uint32_t *)nullptr, (const uint64_t *)nullptr);
  t2 = tb;
  HIPCHK(sr::excl_scan_u32_to_u64(st, tmp.p, t2, cnt.as<uint32_t>(), soff.as<uint64_t>(), n + 1));
  DALLOC(d_blk, (nb + 1) * 8);
  hipLaunchKernelGGL(k_block_off, grid(nb + 1), dim3(256), 0, st, soff.as<uint64_t>(), n, (uint64_t)B, nb, d_blk.as<uint64_t>());
  HIPCHK(hipEventRecord(ev.b, st));
  HIPCHK(hipGetLastError());
  unsigned long long hstat[2] = {0, 0};
  HIPCHK(rd(st, hstat, stat.p, 16));
  if (hstat[1] != ~0ull) return refuse(hstat[1] >> 3, (uint32_t)(hstat[1] & 7));
  HIPCHK(rd(st, ctx->sym_off.data(), d_blk.p, (nb + 1) * 8));
  HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
  I.ms_tokens += ms;
  I.max_tokens = (uint32_t)hstat[0];
  I.num_symbols = ctx->sym_off[nb];
  if (I.max_tokens > MAX_ID) return fail(SPRING_REORDER_E_HIP, "the tokenizer reports %llu tokens in an id", (unsigned long long)I.max_tokens);
  // ---- tokens, pass 2
  DALLOC(ctx->sym, I.num_symbols * 4);
  HIPCHK(hipEventRecord(ev.a, st));
  hipLaunchKernelGGL(k_tokens<Write>, grid(n), dim3(256), 0, st, L, (uint32_t *)nullptr, (uint32_t *)nullptr,
                     (unsigned long long *)nullptr, ctx->sym.as<uint32_t>(), soff.as<uint64_t>());
  HIPCHK(hipEventRecord(ev.b, st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
  I.ms_tokens += ms;
  len1.release(); loff.release(); cnt.release(); soff.release(); tmp.release();
  // ---- the coder's buffers: a block's capacity from its symbol count, the model tables from the budget
  std::vector<uint64_t> cap(nb + 1, 0);
  for (uint64_t b = 0; b < nb; b++) cap[b + 1] = cap[b] + block_capacity(ctx->sym_off[b + 1] - ctx->sym_off[b]);
  DALLOC(cap_buf, cap[nb]);
  DALLOC(d_cap, (nb + 1) * 8); DALLOC(d_len_out, nb * 8); DALLOC(d_out_off, (nb + 1) * 8); DALLOC(flag, 4);
  HIPCHK(hipMemcpyAsync(d_cap.p, cap.data(), (nb + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(flag.p, 0, 4, st));
  const uint64_t per_block = workspace_need(1, I.max_tokens);
  uint64_t budget = 0;
  if (int r = workspace_budget(ctx->workspace_bytes, 0, &budget)) return r;
  const uint64_t per_sub = std::min<uint64_t>(nb, budget / per_block);
  if (per_sub == 0)
    return fail(SPRING_REORDER_E_ARG, "the models of one block (%llu tokens an id) need %llu bytes of workspace, the budget is %llu",
                (unsigned long long)I.max_tokens, (unsigned long long)per_block, (unsigned long long)budget);
  DALLOC(tables, per_sub * per_block);
  Coder G;
  G.sym = ctx->sym.as<uint32_t>(); G.sym_off = d_blk.as<uint64_t>(); G.cap_off = d_cap.as<uint64_t>();
  G.out = cap_buf.as<uint8_t>(); G.out_len = d_len_out.as<uint64_t>(); G.tables = tables.as<uint32_t>();
  G.flag = flag.as<uint32_t>(); G.nctx = (uint32_t)I.max_tokens + 1;
  HIPCHK(hipEventRecord(ev.a, st));
  for (uint64_t first = 0; first < nb; first += per_sub) {
    G.first = (uint32_t)first;
    G.count = (uint32_t)std::min<uint64_t>(per_sub, nb - first);
    hipLaunchKernelGGL(k_code, dim3(G.count), dim3(64), 0, st, G);
    I.sub_batches++;
  }
  HIPCHK(hipEventRecord(ev.b, st));
  HIPCHK(hipGetLastError());
  std::vector<uint64_t> out_len(nb);
  uint32_t hflag = 0;
  HIPCHK(rd(st, out_len.data(), d_len_out.p, nb * 8));
  HIPCHK(rd(st, &hflag, flag.p, 4));
  HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
  I.ms_coder += ms;
  if (hflag) return fail(SPRING_REORDER_E_HIP, "the coder left its tables or a block's buffer (flag %u)", hflag);
  for (uint64_t b = 0; b < nb; b++) {
    if (out_len[b] > cap[b + 1] - cap[b]) return fail(SPRING_REORDER_E_HIP, "block %llu reports more bytes than its buffer holds", (unsigned long long)b);
    ctx->out_off[b + 1] = ctx->out_off[b] + out_len[b];
  }
  I.bytes = ctx->out_off[nb];
  DALLOC(ctx->out, I.bytes);
  HIPCHK(hipMemcpyAsync(d_out_off.p, ctx->out_off.data(), (nb + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(ev.a, st));
  hipLaunchKernelGGL(k_gather, dim3((unsigned)nb, 8), dim3(256), 0, st, cap_buf.as<uint8_t>(), d_cap.as<uint64_t>(),
                     d_out_off.as<uint64_t>(), ctx->out.as<uint8_t>());
  HIPCHK(hipEventRecord(ev.b, st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
  I.ms_coder += ms;
  ctx->info = I;
  ctx->have = true;
  if (info_out) *info_out = I;
  return 0;
}

}  // namespace

extern "C" {

int spring_idcodec_create(int device, spring_idcodec_ctx **out) {
  if (!out) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  const int r = stage_device(&device, "the id codec stage");
  if (r) return r;
  spring_idcodec_ctx *c = new spring_idcodec_ctx();
  c->dev = device;
  memset(&c->info, 0, sizeof(c->info));
  *out = c;
  return 0;
}

void spring_idcodec_destroy(spring_idcodec_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->dev);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  drop_result(ctx);
  if (ctx->st) (void)hipStreamDestroy(ctx->st);
  delete ctx;
}

int spring_idcodec_set_workspace_bytes(spring_idcodec_ctx *ctx, uint64_t workspace_bytes) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  ctx->workspace_bytes = workspace_bytes;
  return 0;
}

uint64_t spring_idcodec_workspace_need(uint64_t blocks, uint64_t max_tokens) { return workspace_need(blocks, max_tokens); }

int spring_idcodec_from_qualid(spring_idcodec_ctx *ctx, spring_qualid_ctx *q, spring_idcodec_info *info) {
  if (!ctx || !q) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  (void)hipSetDevice(ctx->dev);
  drop_result(ctx);
  sr::QualIdView V;
  int r = sr::qualid_view(q, &V);
  if (r) return r;
  if (!V.have[SPRING_QUALID_ID]) return fail(SPRING_REORDER_E_STATE, "the quality / id context holds no id result");
  if (V.dev != ctx->dev) return fail(SPRING_REORDER_E_ARG, "quality / id and id codec contexts live on different devices");
  if (V.num_reads_per_block == 0) return fail(SPRING_REORDER_E_ARG, "num_reads_per_block must be positive");
  if ((r = stream_begin(ctx->dev, &ctx->st))) return r;
  r = run(ctx, V.bytes[SPRING_QUALID_ID], V.info.bytes[SPRING_QUALID_ID], V.len[SPRING_QUALID_ID], V.info.num_units,
          V.num_reads_per_block, info);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  if (r) drop_result(ctx);
  return r;
}

int spring_idcodec_from_host(spring_idcodec_ctx *ctx, const uint8_t *lines, uint64_t nbytes, uint64_t num_lines,
                             uint32_t num_reads_per_block, spring_idcodec_info *info) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  (void)hipSetDevice(ctx->dev);
  drop_result(ctx);
  if (nbytes && !lines) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (num_reads_per_block == 0) return fail(SPRING_REORDER_E_ARG, "num_reads_per_block must be positive");
  if (nbytes && lines[nbytes - 1] != '\n') return fail(SPRING_REORDER_E_ARG, "the last id does not end in a newline");
  std::vector<uint32_t> len;
  len.reserve(std::min(num_lines, nbytes) + 1);
  for (uint64_t a = 0; a < nbytes;) {
    const uint8_t *e = (const uint8_t *)memchr(lines + a, '\n', nbytes - a);   // found: the last byte is one
    const uint64_t n = (uint64_t)(e - (lines + a));
    if (len.size() >= num_lines) return fail(SPRING_REORDER_E_ARG, "the ids hold more than num_lines = %llu lines", (unsigned long long)num_lines);
    if (n > MAX_ID) return refuse(len.size(), E_LONG);
    len.push_back((uint32_t)n);
    a += n + 1;
  }
  if (len.size() != num_lines)
    return fail(SPRING_REORDER_E_ARG, "the ids hold %llu lines, num_lines is %llu", (unsigned long long)len.size(), (unsigned long long)num_lines);
  len.push_back(0);
  int r = stream_begin(ctx->dev, &ctx->st);
  if (r) return r;
  const int dev = ctx->dev;
  DBuf up, d_len;
  DALLOC(up, nbytes + 16);
  DALLOC(d_len, len.size() * 4);
  if (nbytes) HIPCHK(hipMemcpyAsync(up.p, lines, nbytes, hipMemcpyHostToDevice, ctx->st));
  HIPCHK(hipMemcpyAsync(d_len.p, len.data(), len.size() * 4, hipMemcpyHostToDevice, ctx->st));
  r = run(ctx, up.as<uint8_t>(), nbytes, d_len.as<uint32_t>(), num_lines, num_reads_per_block, info);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  if (r) drop_result(ctx);
  return r;
}

int spring_idcodec_download(spring_idcodec_ctx *ctx, uint8_t *bytes, uint64_t *block_off) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "no id blocks compressed yet");
  HIPCHK(hipSetDevice(ctx->dev));
  if (block_off) memcpy(block_off, ctx->out_off.data(), (ctx->info.num_blocks + 1) * 8);
  if (bytes && ctx->info.bytes) HIPCHK(rd(ctx->st, bytes, ctx->out.p, ctx->info.bytes));
  return 0;
}

int spring_idcodec_symbols(spring_idcodec_ctx *ctx, uint32_t *words, uint64_t *block_off) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "no id blocks compressed yet");
  HIPCHK(hipSetDevice(ctx->dev));
  if (block_off) memcpy(block_off, ctx->sym_off.data(), (ctx->info.num_blocks + 1) * 8);
  if (words && ctx->info.num_symbols) HIPCHK(rd(ctx->st, words, ctx->sym.p, ctx->info.num_symbols * 4));
  return 0;
}

int spring_idcodec_get_info(spring_idcodec_ctx *ctx, spring_idcodec_info *info) {
  if (!ctx || !info) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "no id blocks compressed yet");
  *info = ctx->info;
  return 0;
}

}  // extern "C"
