// spring_amd/csrc/unbwt.hip -- libbsc's bsc_bwt_decode for a batch of transformed segments in HBM
// (include/spring_unbwt.h): list ranking over the LF mapping, one sub-batch of whole segments at
// a time.
//
//   words (segment | byte | the byte's row)  ->  stable radix sort by segment | byte, the row riding along: the place
//   of a byte inside its segment is its rank among the equal bytes plus the count of the smaller ones  ->  LF scatter:
//   row r receives (LF[r] << 8) | byte  ->  every head walks LF to the next head: (next head, steps)  ->  pointer
//   doubling over the heads alone: distance of every head to its segment's primary row  ->  one flag per segment: row 0
//   is n steps away (read by the host; a shorter path is refused here)  ->  every head on the path walks its sublist
//   again and stores its bytes backwards from its distance.
//
// Rows are numbered through the sub-batch: segment s (relative to the sub-batch) owns rows off[s] + s .. off[s + 1] + s,
// one more than it has bytes.  The head rule and the round bound are in unbwt_plan.h.  Every loop on the device has a
// static bound: a walk takes at most its segment's length in steps.
#include <algorithm>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "bwt_internal.h"
#include "copy_words.h"
#include "reorder_internal.h"
#include "spring_unbwt.h"
#include "stage_host.h"
#include "unbwt_plan.h"

using namespace sr;

namespace {

constexpr uint64_t SORT_FIXED_BYTES = 8ull << 20;   // the sort's tables that do not grow with the input
constexpr int NPASS = SPRING_UNBWT_PASSES;

// A sub-batch: segments [first, first + count) of the batch; byte p of it is byte off[first] + p of the batch.
struct Sub {
  const uint64_t *src;    // per segment of the batch: the device address of its first byte
  const uint64_t *off;    // per segment + 1: its offset in the batch
  const int32_t *prim;    // per segment: its primary index
  uint32_t first, count;
  uint64_t base;          // off[first]
  uint32_t m;             // bytes
  uint32_t rows;          // m + count
  uint32_t hreg;          // regular heads: one per block of 2^log_k rows
  int log_k;
};

// What a lane knows of a segment (s relative to G.first).
struct Seg {
  uint32_t so;     // its first byte in the sub-batch
  uint32_t n;      // its bytes
  uint32_t row0;   // its row 0: so + s
  uint32_t prow;   // its primary row
};
__device__ __forceinline__ Seg seg_at(const Sub &G, uint32_t s) {
  Seg g;
  const uint64_t a = G.off[G.first + s], b = G.off[G.first + s + 1];
  g.so = (uint32_t)(a - G.base);
  g.n = (uint32_t)(b - a);
  g.row0 = g.so + s;
  g.prow = g.row0 + (uint32_t)G.prim[G.first + s];
  return g;
}

// the segment that holds byte p < G.m: the last one that starts at or before p, which skips the empty ones
__device__ __forceinline__ uint32_t seg_of_byte(const Sub &G, uint32_t p) {
  return last_le(G.count, p, [&](uint32_t i) { return G.off[G.first + i] - G.base; });
}
// the segment that owns row r < G.rows: every segment has at least one row, so the row starts strictly increase
__device__ __forceinline__ uint32_t seg_of_row(const Sub &G, uint32_t r) {
  return last_le(G.count, r, [&](uint32_t i) { return G.off[G.first + i] - G.base + i; });
}

// ------------------------------------------------------------------ rows and keys
// Word of a byte: segment | byte in the upper half, which the sort goes by; the byte's row (the primary row is skipped)
// in the lower half, which rides along.
__device__ __forceinline__ uint64_t key_word(uint32_t s, uint32_t c, const Seg &g, uint32_t q) {
  const uint32_t row = g.row0 + q;
  return ((uint64_t)((s << 8) | c) << 32) | (row < g.prow ? row : row + 1);
}

// Eight consecutive bytes per lane: one search for the segment.  Where all eight lie in one segment and at least eight
// bytes from both of its ends, they come from the two aligned 8-byte words around them (both inside the segment) and
// leave as four 16-byte stores; elsewhere byte by byte, never past a segment's end.
__global__ __launch_bounds__(256) void k_keys(Sub G, uint64_t *__restrict__ key) {
  const uint64_t p0 = 8ull * (blockIdx.x * 256ull + threadIdx.x);
  if (p0 >= G.m) return;
  uint32_t s = seg_of_byte(G, (uint32_t)p0);
  Seg g = seg_at(G, s);
  const uint32_t q0 = (uint32_t)p0 - g.so;
  if (q0 >= 8 && (uint64_t)q0 + 16 <= g.n) {
    const uint64_t addr = G.src[G.first + s] + q0;
    const uint64_t *w = reinterpret_cast<const uint64_t *>(addr & ~7ull);
    const uint32_t sh = 8 * (uint32_t)(addr & 7);
    uint64_t v = w[0] >> sh;
    if (sh) v |= w[1] << (64 - sh);
    ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(key + p0);   // p0 is a multiple of eight: 64-byte aligned
    for (uint32_t e = 0; e < 8; e += 2) {
      ulonglong2 o;
      o.x = key_word(s, (uint32_t)(v >> (8 * e)) & 0xff, g, q0 + e);
      o.y = key_word(s, (uint32_t)(v >> (8 * e + 8)) & 0xff, g, q0 + e + 1);
      dst[e / 2] = o;
    }
    return;
  }
  for (uint32_t e = 0; e < 8; e++) {
    const uint64_t p = p0 + e;
    if (p >= G.m) return;
    if (p - g.so >= g.n) {   // behind this segment's end: the next one that has bytes
      s = seg_of_byte(G, (uint32_t)p);
      g = seg_at(G, s);
    }
    const uint32_t q = (uint32_t)p - g.so;
    key[p] = key_word(s, reinterpret_cast<const uint8_t *>(G.src[G.first + s])[q], g, q);
  }
}

// ------------------------------------------------------------------ LF scatter
// The sorted entry at place t belongs to segment s and is the (t - so)-th byte of it in sorted order: LF of its row is
// row (t - so) + 1 of the segment, which is row t + s + 1 of the sub-batch.  The primary rows receive nothing and are
// never read.
__global__ __launch_bounds__(256) void k_scatter(Sub G, const uint64_t *__restrict__ key, uint64_t *__restrict__ lf) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= G.m) return;
  const uint64_t k = key[t];
  const uint32_t s = (uint32_t)(k >> 40);
  lf[(uint32_t)k] = ((uint64_t)(t + s + 1) << 8) | ((k >> 32) & 0xff);
}

// ------------------------------------------------------------------ sublists
// Head slots: h < hreg is the regular head of block h of rows; hreg + 2 s is row 0 of segment s and hreg + 2 s + 1 its
// primary row, the terminal.  A regular head that falls on a row 0, on a primary row or behind the last row is dead.
struct Head {
  uint32_t s, row;
  bool live, terminal;
};
__device__ __forceinline__ Head head_at(const Sub &G, uint32_t h, Seg *g) {
  Head H;
  H.terminal = false;
  if (h < G.hreg) {
    H.row = unbwt::head_row(h, G.log_k);
    if (H.row >= G.rows) { H.s = 0; H.live = false; *g = seg_at(G, 0); return H; }
    H.s = seg_of_row(G, H.row);
    *g = seg_at(G, H.s);
    H.live = H.row != g->row0 && H.row != g->prow;
  } else {
    const uint32_t e = h - G.hreg;
    H.s = e >> 1;
    *g = seg_at(G, H.s);
    H.terminal = e & 1;
    H.row = H.terminal ? g->prow : g->row0;
    H.live = !H.terminal;
  }
  return H;
}

// rank word of a head: next head slot (high half) | steps to it (low half)
__device__ __forceinline__ uint64_t rank_word(uint32_t next, uint32_t dist) { return ((uint64_t)next << 32) | dist; }

// One head per lane: walk LF to the next head.  stat[0] receives the longest walk.
__global__ __launch_bounds__(256) void k_walk(Sub G, const uint64_t *__restrict__ lf, uint64_t *__restrict__ rank,
                                              uint32_t *__restrict__ stat) {
  const uint32_t h = blockIdx.x * 256u + threadIdx.x;
  const uint32_t H = G.hreg + 2 * G.count;
  uint32_t steps = 0;
  if (h < H) {
    Seg g;
    const Head hd = head_at(G, h, &g);
    uint32_t next = h;   // dead heads, terminals and walks that meet no head point at themselves, distance 0
    if (hd.live) {
      const uint32_t term = G.hreg + 2 * hd.s + 1;
      if (hd.row == g.prow) {   // row 0 of an empty segment is its primary row
        next = term;
      } else {
        uint32_t x = hd.row, k = 0;
        for (uint32_t i = 0; i < g.n; i++) {
          const uint32_t nx = (uint32_t)(lf[x] >> 8);
          k++;
          if (nx == g.prow) { next = term; steps = k; break; }
          if (unbwt::is_regular_head(nx, G.log_k)) { next = nx >> G.log_k; steps = k; break; }
          x = nx;
        }
      }
    }
    rank[h] = rank_word(next, steps);
  }
  uint32_t mx = steps;
  for (int o = 32; o; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
  if ((threadIdx.x & 63) == 0 && mx) atomicMax(&stat[0], mx);
}

// One round of pointer doubling, from one array into the other.  Distances saturate: on a cycle they would grow without
// end.
__global__ __launch_bounds__(256) void k_rank(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, uint32_t H) {
  const uint32_t h = blockIdx.x * 256u + threadIdx.x;
  if (h >= H) return;
  const uint64_t e = in[h];
  const uint32_t nx = (uint32_t)(e >> 32);
  const uint64_t f = nx < H ? in[nx] : rank_word(h, 0);
  const uint64_t d = (e & 0xffffffffu) + (f & 0xffffffffu);
  out[h] = rank_word((uint32_t)(f >> 32), d > unbwt::DIST_CLAMP ? unbwt::DIST_CLAMP : (uint32_t)d);
}

// One segment per lane: row 0 must be exactly n steps from the primary row.  stat[1] receives the first segment (of the
// batch) that fails.
__global__ __launch_bounds__(256) void k_check(Sub G, const uint64_t *__restrict__ rank, uint32_t *__restrict__ stat) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= G.count) return;
  const uint32_t n = (uint32_t)(G.off[G.first + s + 1] - G.off[G.first + s]);
  const uint64_t e = rank[G.hreg + 2 * s];
  if (e != rank_word(G.hreg + 2 * s + 1, n)) atomicMin(&stat[1], G.first + s);
}

// ------------------------------------------------------------------ write
// Every head on the path walks its sublist again.  The byte of a row d steps from the primary row is T[d - 1].  The
// bytes of a sublist are consecutive, downwards: they are gathered into aligned 4-byte words and stored whole where the
// sublist covers the word, byte by byte at its two ends.
__device__ __forceinline__ void flush(uint8_t *word_addr, uint32_t acc, uint32_t have) {
  if (have == 15u) {
    *reinterpret_cast<uint32_t *>(word_addr) = acc;
  } else {
    for (uint32_t e = 0; e < 4; e++)
      if (have >> e & 1) word_addr[e] = (uint8_t)(acc >> (8 * e));
  }
}

__global__ __launch_bounds__(256) void k_write(Sub G, const uint64_t *__restrict__ lf, const uint64_t *__restrict__ rank,
                                               uint8_t *__restrict__ out) {
  const uint32_t h = blockIdx.x * 256u + threadIdx.x;
  if (h >= G.hreg + 2 * G.count) return;
  Seg g;
  const Head hd = head_at(G, h, &g);
  if (!hd.live) return;
  const uint64_t e = rank[h];
  const uint32_t d = (uint32_t)e;
  if ((uint32_t)(e >> 32) != G.hreg + 2 * hd.s + 1 || d == 0 || d > g.n) return;   // not on the path
  uint8_t *T = out + G.base + g.so;   // the segment's n bytes; nothing below is stored outside T[0 .. n)
  uint32_t pos = d - 1, x = hd.row, acc = 0, have = 0;
  for (uint32_t i = 0; i < g.n; i++) {
    const uint64_t w = lf[x];
    const uint64_t a = reinterpret_cast<uint64_t>(T + pos);
    const uint32_t lane = (uint32_t)(a & 3);
    acc |= (uint32_t)(w & 0xff) << (8 * lane);
    have |= 1u << lane;
    const uint32_t nx = (uint32_t)(w >> 8);
    const bool last = pos == 0 || nx == g.prow || unbwt::is_regular_head(nx, G.log_k);
    if (lane == 0 || last) {
      flush(reinterpret_cast<uint8_t *>(a & ~3ull), acc, have);
      acc = 0;
      have = 0;
    }
    if (last) break;
    pos--;
    x = nx;
  }
}

// The sort: 64-bit words, stable over the bits [32, end_bit); the lower half rides along, so no value array moves.  A
// bit range that does not start at bit 0 stays off rocPRIM's merge-sort path, as in sr::sort_pairs (reorder_kernels.hip,
// where the reason is written down): merge-sort limit 0 = block sort up to one block, one-sweep beyond.
hipError_t sort_words(hipStream_t st, void *tmp, size_t &tmp_bytes, const uint64_t *in, uint64_t *out, size_t n,
                      unsigned end_bit) {
  return rocprim::radix_sort_keys<rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 0>>(
      tmp, tmp_bytes, in, out, n, 32u, end_bit, st);
}

}  // namespace

struct spring_unbwt_ctx {
  int dev = 0;
  hipStream_t st = nullptr;
  uint64_t workspace_bytes = 0;   // 0: from the free HBM
  int log_k = unbwt::LOG_K_DEFAULT;
  bool have = false;
  spring_unbwt_info info;
  std::vector<uint64_t> off;      // num_segments + 1
  DBuf out;
};

namespace {

void drop_result(spring_unbwt_ctx *ctx) {
  ctx->have = false;
  ctx->out.release();
  ctx->off.clear();
  memset(&ctx->info, 0, sizeof(ctx->info));
}

struct Work {   // the arrays of a sub-batch, sized for the largest one
  DBuf key, key2, rankA, rankB, tmp, stat;
  size_t tmp_bytes = 0;
};

// One sub-batch.  *bad receives the first segment whose path is short (0xffffffff: none); then nothing was written.
int invert_sub(spring_unbwt_ctx *ctx, const Sub &G, uint64_t longest, Work &W, spring_unbwt_info &I, uint32_t *bad,
               double *ms) {
  hipStream_t st = ctx->st;
  *bad = 0xffffffffu;
  Events ev;
  for (int k = 0; k < 8; k++) HIPCHK(hipEventCreate(&ev.e[k]));
  const uint32_t H = G.hreg + 2 * G.count;
  const int rounds = unbwt::rank_rounds(unbwt::max_heads_of_segment(longest, G.log_k));
  uint64_t *lf = W.key.as<uint64_t>();   // the unsorted keys are done with once the sort has run
  uint64_t *ra = W.rankA.as<uint64_t>(), *rb = W.rankB.as<uint64_t>();
  const uint32_t stat0[2] = {0, 0xffffffffu};
  HIPCHK(hipMemcpyAsync(W.stat.p, stat0, 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(ev.e[0], st));
  if (G.m) hipLaunchKernelGGL(k_keys, grid(G.m, 2048), dim3(256), 0, st, G, W.key.as<uint64_t>());
  HIPCHK(hipEventRecord(ev.e[1], st));
  if (G.m) {
    const unsigned bits = (unsigned)(32 + bwt::bits_for(G.count) + 8);
    size_t tb = 0;
    HIPCHK(sort_words(st, nullptr, tb, nullptr, nullptr, G.m, bits));
    if (tb > W.tmp_bytes) return fail(SPRING_REORDER_E_HIP, "the sort asks for %zu bytes of temporary storage, %zu are planned", tb, W.tmp_bytes);
    HIPCHK(sort_words(st, W.tmp.p, tb, W.key.as<uint64_t>(), W.key2.as<uint64_t>(), G.m, bits));
  }
  HIPCHK(hipEventRecord(ev.e[2], st));
  if (G.m) hipLaunchKernelGGL(k_scatter, grid(G.m), dim3(256), 0, st, G, W.key2.as<uint64_t>(), lf);
  HIPCHK(hipEventRecord(ev.e[3], st));
  hipLaunchKernelGGL(k_walk, grid(H), dim3(256), 0, st, G, lf, ra, W.stat.as<uint32_t>());
  HIPCHK(hipEventRecord(ev.e[4], st));
  for (int r = 0; r < rounds; r++) {
    hipLaunchKernelGGL(k_rank, grid(H), dim3(256), 0, st, ra, rb, H);
    std::swap(ra, rb);
  }
  hipLaunchKernelGGL(k_check, grid(G.count), dim3(256), 0, st, G, ra, W.stat.as<uint32_t>());
  HIPCHK(hipEventRecord(ev.e[5], st));
  HIPCHK(hipGetLastError());
  uint32_t stat[2] = {0, 0};
  HIPCHK(rd(st, stat, W.stat.p, 8));
  I.max_walk = std::max<uint64_t>(I.max_walk, stat[0]);
  I.rank_rounds = std::max<uint64_t>(I.rank_rounds, (uint64_t)rounds);
  I.heads += H;
  *bad = stat[1];
  HIPCHK(hipEventRecord(ev.e[6], st));
  if (*bad == 0xffffffffu)
    hipLaunchKernelGGL(k_write, grid(H), dim3(256), 0, st, G, lf, ra, ctx->out.as<uint8_t>());
  HIPCHK(hipEventRecord(ev.e[7], st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  for (int k = 0; k < NPASS; k++) {
    float x = 0;
    HIPCHK(hipEventElapsedTime(&x, ev.e[k < 5 ? k : 6], ev.e[k < 5 ? k + 1 : 7]));
    ms[k] += x;
  }
  return 0;
}

// src[s]: device address of segment s; d_prim: the primary indexes on the device, prim: the same on the host;
// ctx->off holds the S + 1 offsets.  Plans, inverts, leaves the result in ctx.
int invert(spring_unbwt_ctx *ctx, const std::vector<uint64_t> &src, const int32_t *d_prim, const int32_t *prim,
           spring_unbwt_info *info_out) {
  const int dev = ctx->dev;
  hipStream_t st = ctx->st;
  const std::vector<uint64_t> &off = ctx->off;
  const uint64_t S = src.size(), nbytes = off[S];
  spring_unbwt_info I;
  memset(&I, 0, sizeof(I));
  I.num_segments = S;
  I.bytes = nbytes;
  I.head_spacing = 1ull << ctx->log_k;
  for (uint64_t s = 0; s < S; s++) I.max_segment = std::max(I.max_segment, off[s + 1] - off[s]);
  if (I.max_segment > unbwt::MAX_SEGMENT)
    return fail(SPRING_REORDER_E_ARG, "a segment of %llu bytes: more than 1 GiB", (unsigned long long)I.max_segment);
  if (S >= 0x7fffffffull) return fail(SPRING_REORDER_E_ARG, "too many segments");
  for (uint64_t s = 0; s < S; s++) {
    const uint64_t n = off[s + 1] - off[s];
    if (n ? (prim[s] < 1 || (uint64_t)prim[s] > n) : prim[s] != 0)
      return fail(SPRING_REORDER_E_ARG, "segment %llu of %llu bytes: primary index %d out of range", (unsigned long long)s,
                  (unsigned long long)n, (int)prim[s]);
  }
  // ---- the result's own buffer, then the budget from what is left
  DALLOC(ctx->out, nbytes + 16);
  DBuf d_off, d_src;
  DALLOC(d_off, (S + 1) * 8);
  DALLOC(d_src, S * 8);
  uint64_t budget = 0;
  if (int r = workspace_budget(ctx->workspace_bytes, SORT_FIXED_BYTES << 2, &budget)) return r;
  I.workspace_bytes = budget;
  std::vector<uint64_t> first(S + 2);
  const int64_t nsub = unbwt::plan_sub_batches(off.data(), S, budget, first.data());
  if (nsub < 0) {
    const uint64_t s = (uint64_t)(-1 - nsub);
    return fail(SPRING_REORDER_E_ARG, "segment %llu of %llu bytes needs %llu bytes of workspace, the budget is %llu",
                (unsigned long long)s, (unsigned long long)(off[s + 1] - off[s]),
                (unsigned long long)unbwt::workspace_need(off[s + 1] - off[s], 1), (unsigned long long)budget);
  }
  I.sub_batches = (uint64_t)nsub;
  if (S == 0) {
    ctx->info = I;
    ctx->have = true;
    if (info_out) *info_out = I;
    return 0;
  }
  HIPCHK(hipMemcpyAsync(d_off.p, off.data(), (S + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_src.p, src.data(), S * 8, hipMemcpyHostToDevice, st));
  uint64_t mmax = 0, rmax = 0, hmax = 0;
  for (int64_t b = 0; b < nsub; b++) {
    const uint64_t m = off[first[b + 1]] - off[first[b]], k = first[b + 1] - first[b];
    mmax = std::max(mmax, m);
    rmax = std::max(rmax, m + k);
    hmax = std::max(hmax, unbwt::regular_heads(m + k, ctx->log_k) + 2 * k);
  }
  Work W;
  SyncOnExit sync_on_exit{st};
  if (mmax) {
    size_t tb = 0;
    HIPCHK(sort_words(st, nullptr, tb, nullptr, nullptr, mmax, 64));
    if (tb > mmax * unbwt::SORT_TMP_PER_POS + SORT_FIXED_BYTES)
      return fail(SPRING_REORDER_E_HIP, "the sort asks for %zu bytes of temporary storage for %llu entries", tb, (unsigned long long)mmax);
    W.tmp_bytes = std::max<size_t>(tb, mmax * 8 + (1u << 20));   // smaller sub-batches sort fewer entries and fewer bits
    DALLOC(W.tmp, W.tmp_bytes + 16);
    DALLOC(W.key2, mmax * 8);
  }
  DALLOC(W.key, rmax * 8);   // the keys, then the LF word of every row
  DALLOC(W.rankA, hmax * 8); DALLOC(W.rankB, hmax * 8);
  DALLOC(W.stat, 16);
  double ms[NPASS] = {0, 0, 0, 0, 0, 0};
  for (int64_t b = 0; b < nsub; b++) {
    Sub G;
    G.src = d_src.as<uint64_t>();
    G.off = d_off.as<uint64_t>();
    G.prim = d_prim;
    G.first = (uint32_t)first[b];
    G.count = (uint32_t)(first[b + 1] - first[b]);
    G.base = off[first[b]];
    G.m = (uint32_t)(off[first[b + 1]] - off[first[b]]);
    G.rows = G.m + G.count;
    G.log_k = ctx->log_k;
    G.hreg = (uint32_t)unbwt::regular_heads(G.rows, G.log_k);
    uint64_t longest = 0;
    for (uint64_t s = first[b]; s < first[b + 1]; s++) longest = std::max(longest, off[s + 1] - off[s]);
    uint32_t bad = 0;
    const int r = invert_sub(ctx, G, longest, W, I, &bad, ms);
    if (r) return r;
    if (bad != 0xffffffffu)
      return fail(SPRING_REORDER_E_ARG, "segment %u: its %llu bytes with primary index %d are not the transform of any text "
                  "(the path from row 0 reaches the primary row in fewer steps)", bad,
                  (unsigned long long)(off[bad + 1] - off[bad]), (int)prim[bad]);
  }
  for (int k = 0; k < NPASS; k++) { I.ms_pass[k] = ms[k]; I.ms_device += ms[k]; }
  ctx->info = I;
  ctx->have = true;
  if (info_out) *info_out = I;
  return 0;
}

}  // namespace

extern "C" {

int spring_unbwt_create(int device, spring_unbwt_ctx **out) {
  if (!out) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  const int r = stage_device(&device, "the inverse block-sort stage");
  if (r) return r;
  spring_unbwt_ctx *c = new spring_unbwt_ctx();
  c->dev = device;
  memset(&c->info, 0, sizeof(c->info));
  *out = c;
  return 0;
}

void spring_unbwt_destroy(spring_unbwt_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->dev);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  drop_result(ctx);
  if (ctx->st) (void)hipStreamDestroy(ctx->st);
  delete ctx;
}

int spring_unbwt_set_workspace_bytes(spring_unbwt_ctx *ctx, uint64_t workspace_bytes) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  ctx->workspace_bytes = workspace_bytes;
  return 0;
}

uint64_t spring_unbwt_workspace_need(uint64_t bytes, uint64_t segments) { return unbwt::workspace_need(bytes, segments); }

int spring_unbwt_set_head_spacing(spring_unbwt_ctx *ctx, uint32_t head_spacing) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (head_spacing == 0) { ctx->log_k = unbwt::LOG_K_DEFAULT; return 0; }
  for (int b = unbwt::LOG_K_MIN; b <= unbwt::LOG_K_MAX; b++)
    if (head_spacing == (1u << b)) { ctx->log_k = b; return 0; }
  return fail(SPRING_REORDER_E_ARG, "head_spacing must be a power of two in 16 .. 1024, or 0 (got %u)", head_spacing);
}

int spring_unbwt_from_host(spring_unbwt_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const uint64_t *seg_off,
                           const int32_t *primary, uint64_t num_segments, spring_unbwt_info *info) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  (void)hipSetDevice(ctx->dev);
  drop_result(ctx);
  if (nbytes && !bytes) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  const uint64_t one[2] = {0, nbytes};
  if (!seg_off) { seg_off = one; num_segments = 1; }
  if (num_segments >= 0x7fffffffull) return fail(SPRING_REORDER_E_ARG, "too many segments");
  if (num_segments && !primary) return fail(SPRING_REORDER_E_ARG, "NULL primary indexes");
  if (seg_off[0] != 0 || seg_off[num_segments] != nbytes)
    return fail(SPRING_REORDER_E_ARG, "the segment offsets do not start at 0 and end at the %llu bytes", (unsigned long long)nbytes);
  for (uint64_t s = 0; s < num_segments; s++)
    if (seg_off[s + 1] < seg_off[s]) return fail(SPRING_REORDER_E_ARG, "the segment offsets decrease");
  int r = stream_begin(ctx->dev, &ctx->st);
  if (r) return r;
  const int dev = ctx->dev;
  DBuf up, d_prim;
  DALLOC(up, nbytes + 32);
  DALLOC(d_prim, num_segments * 4);
  if (nbytes) HIPCHK(hipMemcpyAsync(up.p, bytes, nbytes, hipMemcpyHostToDevice, ctx->st));
  if (num_segments) HIPCHK(hipMemcpyAsync(d_prim.p, primary, num_segments * 4, hipMemcpyHostToDevice, ctx->st));
  ctx->off.assign(seg_off, seg_off + num_segments + 1);
  std::vector<uint64_t> src(num_segments);
  for (uint64_t s = 0; s < num_segments; s++) src[s] = reinterpret_cast<uint64_t>(up.as<uint8_t>() + seg_off[s]);
  r = invert(ctx, src, d_prim.as<int32_t>(), primary, info);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  if (r) drop_result(ctx);
  return r;
}

int spring_unbwt_from_bwt(spring_unbwt_ctx *ctx, spring_bwt_ctx *bwt_ctx, spring_unbwt_info *info) {
  if (!ctx || !bwt_ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  (void)hipSetDevice(ctx->dev);
  drop_result(ctx);
  sr::BwtView V;
  int r = sr::bwt_view(bwt_ctx, &V);
  if (r) return r;
  if (V.dev != ctx->dev) return fail(SPRING_REORDER_E_ARG, "block-sort and inverse contexts live on different devices");
  if ((r = stream_begin(ctx->dev, &ctx->st))) return r;
  const uint64_t S = V.num_segments;
  std::vector<int32_t> prim(S ? S : 1);
  if (S) HIPCHK(rd(ctx->st, prim.data(), V.primary, S * 4));
  ctx->off.assign(V.off, V.off + S + 1);
  std::vector<uint64_t> src(S);
  for (uint64_t s = 0; s < S; s++) src[s] = reinterpret_cast<uint64_t>(V.bwt + V.off[s]);
  r = invert(ctx, src, V.primary, prim.data(), info);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  if (r) drop_result(ctx);
  return r;
}

int spring_unbwt_from_unqlfc(spring_unbwt_ctx *ctx, spring_unqlfc_ctx *unqlfc_ctx, const int32_t *primary, spring_unbwt_info *info) {
  if (!ctx || !unqlfc_ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  (void)hipSetDevice(ctx->dev);
  drop_result(ctx);
  sr::UnqlfcView V;
  int r = sr::unqlfc_view(unqlfc_ctx, &V);
  if (r) return r;
  if (V.dev != ctx->dev) return fail(SPRING_REORDER_E_ARG, "QLFC decoder and inverse contexts live on different devices");
  const uint64_t S = V.num_segments;
  if (S && !primary) return fail(SPRING_REORDER_E_ARG, "NULL primary indexes");
  if ((r = stream_begin(ctx->dev, &ctx->st))) return r;
  const int dev = ctx->dev;
  DBuf d_prim;
  DALLOC(d_prim, S * 4);
  if (S) HIPCHK(hipMemcpyAsync(d_prim.p, primary, S * 4, hipMemcpyHostToDevice, ctx->st));
  ctx->off.assign(V.off, V.off + S + 1);
  std::vector<uint64_t> src(S);
  for (uint64_t s = 0; s < S; s++) src[s] = reinterpret_cast<uint64_t>(V.out + V.off[s]);
  r = invert(ctx, src, d_prim.as<int32_t>(), primary, info);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  if (r) drop_result(ctx);
  return r;
}

int spring_unbwt_get_info(spring_unbwt_ctx *ctx, spring_unbwt_info *info) {
  if (!ctx || !info) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing inverted yet");
  *info = ctx->info;
  return 0;
}

int spring_unbwt_download(spring_unbwt_ctx *ctx, uint8_t *text, uint64_t *seg_off) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing inverted yet");
  HIPCHK(hipSetDevice(ctx->dev));
  if (seg_off) memcpy(seg_off, ctx->off.data(), (ctx->info.num_segments + 1) * 8);
  if (text && ctx->info.bytes) HIPCHK(rd(ctx->st, text, ctx->out.p, ctx->info.bytes));
  return 0;
}

int spring_unbwt_decode_inplace(spring_unbwt_ctx *ctx, uint8_t *T, int32_t n, int32_t index, uint8_t num_indexes,
                                const int32_t *indexes) {
  (void)num_indexes;
  (void)indexes;
  if (!ctx || n < 0 || (n && !T)) return fail(SPRING_REORDER_E_ARG, "bad argument");
  const int r = spring_unbwt_from_host(ctx, T, (uint64_t)n, nullptr, &index, 0, nullptr);
  if (r) return r;
  return spring_unbwt_download(ctx, T, nullptr);
}

}  // extern "C"
