// spring_amd/csrc/bwt.hip -- libbsc's bsc_bwt_encode for a batch of byte segments in HBM (include/spring_bwt.h;
// DESIGN.md section 15): suffix sorting by prefix doubling, one sub-batch of whole segments at a time.
//
//   first keys (segment | next bytes big-endian | bytes valid)  ->  radix sort  ->  group heads, max-scan to ranks,
//   rank[sa[j]] = first slot of j's group  ->  compaction of the positions whose group is not yet a single suffix  ->
//   keys (rank[i], rank[i + h] + 1 or 0 past the segment's end) of those only  ->  sort, re-rank inside their slots,
//   compact, h doubles ... until the host reads a count of zero  ->  gather T[sa[j] - 1] around the primary index, the
//   sampled ranks.
//
// A group occupies consecutive slots and its rank is its first slot, so a re-sorted group falls back into its own
// slots and the ranks of every other position stay what they are (Larsson & Sadakane).  Every loop on the device has a
// static bound; the round loop on the host carries bwt::max_rounds.
//
// With run-aware keys on (spring_bwt_set_run_keys) the first key also carries, for a position inside a run of one byte,
// on which side of the run's byte the byte behind the run lies and how long the rest of the run is, and the doubling
// rounds of such a position look behind its run (hop) instead of into it.
#include <algorithm>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "bwt_internal.h"
#include "bwt_plan.h"
#include "copy_words.h"
#include "fastq_out_internal.h"
#include "reorder_device.h"
#include "reorder_internal.h"
#include "spring_bwt.h"
#include "stage_host.h"
#include "streams_internal.h"

using namespace sr;

namespace {

constexpr uint64_t DEFAULT_BLOCK_BYTES = 25ull * 1024 * 1024;   // bsc.cpp:80
constexpr uint64_t QUALID_BLOCK_BYTES = 64ull * 1024 * 1024;    // "-b64", what BSC_str_array_compress passes
constexpr uint64_t SORT_FIXED_BYTES = 8ull << 20;               // the sort's tables that do not grow with the input

// A sub-batch: segments [first, first + count) of the batch; position p of it is byte off[first] + p of the batch.
struct Sub {
  const uint64_t *src;   // per segment of the batch: the device address of its first byte
  const uint64_t *off;   // per segment + 1: its offset in the batch
  uint32_t first, count;
  uint64_t base;         // off[first]
  uint32_t m;            // positions
};

// the segment (relative to G.first) that holds position p < G.m: the last one that starts at or before p, which skips
// the empty ones
__device__ __forceinline__ uint32_t seg_of(const Sub &G, uint32_t p) {
  return last_le(G.count, p, [&](uint32_t i) { return G.off[G.first + i] - G.base; });
}

// ------------------------------------------------------------------ first keys
// The next eight bytes at a (byte i of its segment, rem bytes left), the first one on top; only the first `valid` (at
// most 7) of them count, and behind the segment's end they are zero.  Away from the segment's ends the bytes come from
// the two aligned 8-byte words around the position (both inside the segment); within 16 bytes of an end, byte by byte
// and never past it.
__device__ __forceinline__ uint64_t next_bytes(const uint8_t *a, uint64_t i, uint64_t rem, uint32_t valid) {
  uint64_t be = 0;
  if (i >= 8 && rem >= 16) {
    const uint64_t addr = reinterpret_cast<uint64_t>(a);
    const uint64_t *w = reinterpret_cast<const uint64_t *>(addr & ~7ull);
    const uint32_t sh = 8 * (uint32_t)(addr & 7);
    uint64_t v = w[0] >> sh;
    if (sh) v |= w[1] << (64 - sh);
    be = __builtin_bswap64(v);
  } else {
    for (uint32_t k = 0; k < 7; k++)
      if (k < valid) be |= (uint64_t)a[k] << (56 - 8 * k);
  }
  return be;
}

// One position per lane.
__global__ __launch_bounds__(256) void k_first_keys(Sub G, bwt::KeyLayout K, uint64_t *__restrict__ key,
                                                    uint32_t *__restrict__ val, uint32_t *__restrict__ uslot) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= G.m) return;
  const uint32_t s = seg_of(G, p);
  const uint64_t so = G.off[G.first + s] - G.base, len = G.off[G.first + s + 1] - G.off[G.first + s];
  const uint64_t i = p - so, rem = len - i;
  const uint8_t *a = reinterpret_cast<const uint8_t *>(G.src[G.first + s]) + i;
  const uint32_t valid = rem < (uint64_t)K.key_bytes ? (uint32_t)rem : (uint32_t)K.key_bytes;
  const uint64_t be = next_bytes(a, i, rem, valid);
  const uint64_t bytes = be >> (64 - 8 * K.key_bytes);
  key[p] = ((uint64_t)s << (8 * K.key_bytes + bwt::VALID_BITS)) | (bytes << bwt::VALID_BITS) | valid;
  val[p] = p;
  uslot[p] = p;
}

// ------------------------------------------------------------------ run-aware first keys
// Run ends, mirrored so that a forward inclusive max-scan serves: flag[m - 1 - p] = m - 1 - p where p is the last
// position of its run of equal bytes or of its segment, else 0 (the neutral element; slot 0 is position m - 1, which
// ends its segment).  After the scan, word m - 1 - p holds m - 1 - e for the first such e >= p.
__global__ __launch_bounds__(256) void k_run_ends(Sub G, uint32_t *__restrict__ flag) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= G.m) return;
  const uint32_t s = seg_of(G, p);
  const uint64_t so = G.off[G.first + s] - G.base, len = G.off[G.first + s + 1] - G.off[G.first + s];
  const uint64_t i = p - so;
  const uint8_t *a = reinterpret_cast<const uint8_t *>(G.src[G.first + s]) + i;
  const bool last = i + 1 == len || a[1] != a[0];
  const uint32_t j = G.m - 1 - p;
  flag[j] = last ? j : 0;
}

// The first key of k_first_keys with two more fields below `valid`: side (1 bit) and mag (run_bits), both zero unless
// the next key_bytes bytes exist and are equal -- position p lies in a run of its byte c with L >= key_bytes bytes left
// inside the segment.  d = the byte behind the run:  the run ends the segment, or d < c: side 0, mag = min(L, cap);
// d > c: side 1, mag = cap - min(L, cap).  hop[p] = L where key_bytes <= L < cap (the positions that tie with p have
// the same c, side and L, so what tells them apart starts L bytes on), else 0.  rend: the scan over k_run_ends.
__global__ __launch_bounds__(256) void k_first_keys_runs(Sub G, bwt::RunKeyLayout K, uint32_t cap,
                                                         const uint32_t *__restrict__ rend, uint64_t *__restrict__ key,
                                                         uint32_t *__restrict__ val, uint32_t *__restrict__ uslot,
                                                         uint32_t *__restrict__ hop, uint32_t *__restrict__ run_count) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= G.m) return;
  const uint32_t s = seg_of(G, p);
  const uint64_t so = G.off[G.first + s] - G.base, len = G.off[G.first + s + 1] - G.off[G.first + s];
  const uint64_t i = p - so, rem = len - i;
  const uint8_t *a = reinterpret_cast<const uint8_t *>(G.src[G.first + s]) + i;
  const uint32_t valid = rem < (uint64_t)K.key_bytes ? (uint32_t)rem : (uint32_t)K.key_bytes;
  const uint64_t be = next_bytes(a, i, rem, valid);
  const uint64_t bytes = be >> (64 - 8 * K.key_bytes);
  const uint32_t e = G.m - 1 - rend[G.m - 1 - p];   // p <= e < so + len
  const uint32_t L = e - p + 1;
  uint32_t side = 0, mag = 0, hp = 0;
  const bool run = L >= (uint32_t)K.key_bytes;
  if (run) {
    const uint32_t c = (uint32_t)(be >> 56);
    if ((uint64_t)L < rem) side = a[L] > c ? 1u : 0u;   // a[L] is the byte behind the run, inside the segment
    const uint32_t lc = L < cap ? L : cap;
    mag = side ? cap - lc : lc;
    hp = L < cap ? L : 0;
  }
  const int low = bwt::SIDE_BITS + K.run_bits;
  key[p] = ((uint64_t)s << (8 * K.key_bytes + bwt::VALID_BITS + low)) | (bytes << (bwt::VALID_BITS + low)) |
           ((uint64_t)valid << low) | ((uint64_t)side << K.run_bits) | mag;
  val[p] = p;
  uslot[p] = p;
  hop[p] = hp;
  const uint64_t runs = __ballot(run);   // lane 0 of a wavefront is live whenever one of its lanes is
  if ((threadIdx.x & 63u) == 0 && runs) atomicAdd(run_count, (uint32_t)__popcll(runs));
}

// ------------------------------------------------------------------ a doubling round
// key of an unresolved position i: (rank[i], rank[i + h] + 1), or 0 for the second half when i + h is past the end of
// i's segment -- the shorter suffix sorts first.  RUNS: i + max(h, hop[i]) in the place of i + h.
template <bool RUNS>
__global__ __launch_bounds__(256) void k_round_keys(Sub G, uint32_t h, int lb, const uint32_t *__restrict__ rank,
                                                    const uint32_t *__restrict__ upos, uint32_t cnt,
                                                    uint64_t *__restrict__ key, const uint32_t *__restrict__ hop) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= cnt) return;
  const uint32_t p = upos[t];
  const uint32_t s = seg_of(G, p);
  const uint64_t end = G.off[G.first + s + 1] - G.base;
  if (RUNS) {
    const uint32_t hp = hop[p];
    if (hp > h) h = hp;
  }
  const uint64_t q = (uint64_t)p + h;
  const uint64_t nx = q < end ? (uint64_t)rank[q] + 1 : 0;
  key[t] = ((uint64_t)rank[p] << lb) | nx;
}

// head[t] = t where a group starts in the sorted list, else 0; an inclusive max-scan makes it "my group's first entry"
__global__ __launch_bounds__(256) void k_heads(const uint64_t *__restrict__ key, uint32_t cnt, uint32_t *__restrict__ flag) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= cnt) return;
  flag[t] = (t > 0 && key[t] != key[t - 1]) ? t : 0;
}

// The sorted entries go back into the slots of the list, in order: entry t into slot uslot[t].  Its rank is the slot of
// its group's first entry.  u[t] = 1 when the group holds more than this entry.
__global__ __launch_bounds__(256) void k_rerank(const uint32_t *__restrict__ head, const uint32_t *__restrict__ uslot,
                                                const uint32_t *__restrict__ pos, uint32_t cnt, uint32_t *__restrict__ rank,
                                                uint32_t *__restrict__ sa, uint32_t *__restrict__ u) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= cnt) return;
  const uint32_t hd = head[t], p = pos[t];
  rank[p] = uslot[hd];
  sa[uslot[t]] = p;
  const bool single = hd == t && (t + 1 == cnt || head[t + 1] == t + 1);
  u[t] = single ? 0 : 1;
}

// the unresolved entries move to the front of the list, their slots with them; the last lane leaves their count
__global__ __launch_bounds__(256) void k_compact(const uint32_t *__restrict__ u, const uint32_t *__restrict__ idx,
                                                 const uint32_t *__restrict__ uslot, const uint32_t *__restrict__ pos,
                                                 uint32_t cnt, uint32_t *__restrict__ uslot_out,
                                                 uint32_t *__restrict__ upos_out, uint32_t *__restrict__ counter) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= cnt) return;
  const uint32_t f = u[t], k = idx[t];
  if (f) { uslot_out[k] = uslot[t]; upos_out[k] = pos[t]; }
  if (t == cnt - 1) *counter = k + f;
}

// ------------------------------------------------------------------ gather
// A lane owns one aligned 4-byte word of the batch's output.  Byte q of a segment of n bytes whose suffix 0 has rank r0:
// q = 0 is T[n - 1]; q >= 1 is T[i - 1] for the suffix i of rank q - 1 (q - 1 < r0) or q (beyond r0): suffix 0 has no
// byte in front of it and is left out.
__global__ __launch_bounds__(256) void k_gather(Sub G, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ rank,
                                                uint8_t *__restrict__ out) {
  const uint64_t w0 = (G.base & ~3ull) + 4ull * (blockIdx.x * 256ull + threadIdx.x);
  const uint64_t lim = G.base + G.m;
  if (w0 >= lim) return;
  uint32_t word = 0, have = 0;
  for (uint32_t e = 0; e < 4; e++) {
    const uint64_t g = w0 + e;
    if (g < G.base || g >= lim) continue;
    const uint32_t p = (uint32_t)(g - G.base);
    const uint32_t s = seg_of(G, p);
    const uint32_t so = (uint32_t)(G.off[G.first + s] - G.base);
    const uint32_t n = (uint32_t)(G.off[G.first + s + 1] - G.off[G.first + s]);
    const uint8_t *T = reinterpret_cast<const uint8_t *>(G.src[G.first + s]);
    const uint32_t q = p - so;
    uint32_t b;
    if (q == 0) {
      b = T[n - 1];
    } else {
      const uint32_t r0 = rank[so] - so;
      const uint32_t r = (q - 1 < r0) ? q - 1 : q;
      const uint32_t i = sa[so + r] - so;   // never suffix 0: r != r0
      b = T[i - 1];
    }
    word |= b << (8 * e);
    have |= 1u << e;
  }
  if (have == 15u) {
    *reinterpret_cast<uint32_t *>(out + w0) = word;
  } else {   // the first or last word of the sub-batch
    for (uint32_t e = 0; e < 4; e++)
      if (have >> e & 1) out[w0 + e] = (uint8_t)(word >> (8 * e));
  }
}

// one workgroup per segment: primary index and the sampled ranks (bwt_plan.h)
__global__ __launch_bounds__(256) void k_indexes(Sub G, const uint32_t *__restrict__ rank, int32_t *__restrict__ primary,
                                                 int32_t *__restrict__ nidx, int32_t *__restrict__ indexes) {
  const uint32_t s = blockIdx.x, k = threadIdx.x;
  if (s >= G.count) return;
  const uint64_t gs = (uint64_t)G.first + s;
  const uint32_t so = (uint32_t)(G.off[gs] - G.base), n = (uint32_t)(G.off[gs + 1] - G.off[gs]);
  const uint32_t step = bwt::index_step(n), ni = bwt::num_indexes(n);
  indexes[gs * SPRING_BWT_MAX_INDEXES + k] = k < ni ? (int32_t)(rank[so + (k + 1) * step] - so) : 0;
  if (k == 0) {
    primary[gs] = n ? (int32_t)(rank[so] - so + 1) : 0;
    nidx[gs] = (int32_t)ni;
  }
}

}  // namespace

struct spring_bwt_ctx {
  int dev = 0;
  hipStream_t st = nullptr;
  uint64_t block_bytes = DEFAULT_BLOCK_BYTES;
  uint64_t workspace_bytes = 0;   // 0: from the free HBM
  bool run_keys = false;
  uint32_t cap_bits = 0;          // 0: the layout's own run_bits
  bool have = false;
  spring_bwt_info info;
  std::vector<uint64_t> off;      // num_segments + 1
  std::vector<int32_t> seg_stream;
  std::vector<uint32_t> seg_block, seg_cut;
  std::vector<uint64_t> round_entries;   // per sort round: the entries sorted, summed over the sub-batches
  DBuf out, primary, nidx, indexes;
};

namespace {

void drop_result(spring_bwt_ctx *ctx) {
  ctx->have = false;
  ctx->out.release();
  ctx->primary.release();
  ctx->nidx.release();
  ctx->indexes.release();
  ctx->off.clear();
  ctx->seg_stream.clear();
  ctx->seg_block.clear();
  ctx->seg_cut.clear();
  ctx->round_entries.clear();
  memset(&ctx->info, 0, sizeof(ctx->info));
}

struct Work {   // the arrays of a sub-batch, sized for the largest one
  DBuf key, key2, posA, posB, uslot, uslot2, rank, sa, f, h, hop, tmp, counter;   // hop: with run keys only
  size_t tmp_bytes = 0;
};

// temp storage the sort and the two scans need for n entries
int tmp_need(hipStream_t st, uint64_t n, size_t *out) {
  size_t a = 0, b = 0, c = 0;
  HIPCHK(sr::sort_pairs(st, nullptr, a, nullptr, nullptr, nullptr, nullptr, n, 64));
  HIPCHK(rocprim::inclusive_scan(nullptr, b, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n,
                                 rocprim::maximum<uint32_t>(), st));
  HIPCHK(sr::excl_scan_u32(st, nullptr, c, nullptr, nullptr, n));
  *out = std::max(a, std::max(b, c));
  return 0;
}

// One sub-batch: suffix order of its positions, then the output bytes and the index tables of its segments.
int sort_sub(spring_bwt_ctx *ctx, const Sub &G, uint64_t longest, Work &W, uint64_t *rounds_out, uint64_t *runs_out,
             double *ms) {
  hipStream_t st = ctx->st;
  const uint32_t m = G.m;
  const bool runs = ctx->run_keys;
  *rounds_out = 0;
  *runs_out = 0;
  Events ev;
  for (int k = 0; k < 6; k++) HIPCHK(hipEventCreate(&ev.e[k]));
  uint32_t *uslot = W.uslot.as<uint32_t>(), *uslot2 = W.uslot2.as<uint32_t>();
  if (m) {
    const bwt::KeyLayout K = bwt::key_layout(G.count);
    const bwt::RunKeyLayout RK = bwt::run_key_layout(G.count);
    const uint32_t cap = (1u << (ctx->cap_bits ? (int)ctx->cap_bits : RK.run_bits)) - 1;   // cap_bits <= run_bits: transform()
    const int lb = bwt::bits_for((uint64_t)m + 1);
    const int max_rounds = bwt::max_rounds(longest);
    uint32_t cnt = m;
    uint64_t h = (uint64_t)(runs ? RK.key_bytes : K.key_bytes);
    unsigned bits = (unsigned)(runs ? RK.total_bits : K.total_bits);
    if (runs) HIPCHK(hipMemsetAsync(W.counter.as<uint32_t>() + 1, 0, 4, st));
    for (int round = 0; round < max_rounds && cnt > 0; round++) {
      HIPCHK(hipEventRecord(ev.e[0], st));
      const uint32_t hh = (uint32_t)std::min<uint64_t>(h, 0x80000000ull);
      if (round == 0 && runs) {   // the two scan words are free before the first sort
        hipLaunchKernelGGL(k_run_ends, grid(m), dim3(256), 0, st, G, W.f.as<uint32_t>());
        size_t sb = W.tmp_bytes;
        HIPCHK(rocprim::inclusive_scan(W.tmp.p, sb, W.f.as<uint32_t>(), W.h.as<uint32_t>(), (size_t)m,
                                       rocprim::maximum<uint32_t>(), st));
        hipLaunchKernelGGL(k_first_keys_runs, grid(m), dim3(256), 0, st, G, RK, cap, W.h.as<uint32_t>(), W.key.as<uint64_t>(),
                           W.posA.as<uint32_t>(), uslot, W.hop.as<uint32_t>(), W.counter.as<uint32_t>() + 1);
      } else if (round == 0) {
        hipLaunchKernelGGL(k_first_keys, grid(m), dim3(256), 0, st, G, K, W.key.as<uint64_t>(), W.posA.as<uint32_t>(), uslot);
      } else if (runs) {
        hipLaunchKernelGGL(k_round_keys<true>, grid(cnt), dim3(256), 0, st, G, hh, lb, W.rank.as<uint32_t>(),
                           W.posA.as<uint32_t>(), cnt, W.key.as<uint64_t>(), W.hop.as<uint32_t>());
      } else {
        hipLaunchKernelGGL(k_round_keys<false>, grid(cnt), dim3(256), 0, st, G, hh, lb, W.rank.as<uint32_t>(),
                           W.posA.as<uint32_t>(), cnt, W.key.as<uint64_t>(), (const uint32_t *)nullptr);
      }
      HIPCHK(hipEventRecord(ev.e[1], st));
      size_t tb = 0;
      HIPCHK(sr::sort_pairs(st, nullptr, tb, nullptr, nullptr, nullptr, nullptr, cnt, bits));
      if (tb > W.tmp_bytes) return fail(SPRING_REORDER_E_HIP, "the sort asks for %zu bytes of temporary storage, %zu are planned", tb, W.tmp_bytes);
      HIPCHK(sr::sort_pairs(st, W.tmp.p, tb, W.key.as<uint64_t>(), W.key2.as<uint64_t>(), W.posA.as<uint32_t>(),
                            W.posB.as<uint32_t>(), cnt, bits));
      HIPCHK(hipEventRecord(ev.e[2], st));
      hipLaunchKernelGGL(k_heads, grid(cnt), dim3(256), 0, st, W.key2.as<uint64_t>(), cnt, W.f.as<uint32_t>());
      tb = W.tmp_bytes;
      HIPCHK(rocprim::inclusive_scan(W.tmp.p, tb, W.f.as<uint32_t>(), W.h.as<uint32_t>(), (size_t)cnt,
                                     rocprim::maximum<uint32_t>(), st));
      hipLaunchKernelGGL(k_rerank, grid(cnt), dim3(256), 0, st, W.h.as<uint32_t>(), uslot, W.posB.as<uint32_t>(), cnt,
                         W.rank.as<uint32_t>(), W.sa.as<uint32_t>(), W.f.as<uint32_t>());
      HIPCHK(hipEventRecord(ev.e[3], st));
      tb = W.tmp_bytes;
      HIPCHK(sr::excl_scan_u32(st, W.tmp.p, tb, W.f.as<uint32_t>(), W.h.as<uint32_t>(), cnt));
      hipLaunchKernelGGL(k_compact, grid(cnt), dim3(256), 0, st, W.f.as<uint32_t>(), W.h.as<uint32_t>(), uslot,
                         W.posB.as<uint32_t>(), cnt, uslot2, W.posA.as<uint32_t>(), W.counter.as<uint32_t>());
      HIPCHK(hipEventRecord(ev.e[4], st));
      HIPCHK(hipGetLastError());
      uint32_t left = 0;
      HIPCHK(rd(st, &left, W.counter.p, 4));
      for (int k = 0; k < 4; k++) {
        float x = 0;
        HIPCHK(hipEventElapsedTime(&x, ev.e[k], ev.e[k + 1]));
        ms[k] += x;
      }
      if (left > cnt) return fail(SPRING_REORDER_E_HIP, "the unresolved positions grew from %u to %u", cnt, left);
      if (ctx->round_entries.size() <= (size_t)round) ctx->round_entries.resize((size_t)round + 1, 0);
      ctx->round_entries[(size_t)round] += cnt;
      cnt = left;
      std::swap(uslot, uslot2);
      if (round > 0) h *= 2;
      bits = (unsigned)(2 * lb);
      (*rounds_out)++;
    }
    if (cnt) return fail(SPRING_REORDER_E_HIP, "%u suffixes unresolved after %d rounds", cnt, max_rounds);
    if (runs) {
      uint32_t n_runs = 0;
      HIPCHK(rd(st, &n_runs, W.counter.as<uint32_t>() + 1, 4));
      *runs_out = n_runs;
    }
  }
  HIPCHK(hipEventRecord(ev.e[0], st));
  if (m) hipLaunchKernelGGL(k_gather, grid((uint64_t)m + 3 + 3, 1024), dim3(256), 0, st, G, W.sa.as<uint32_t>(),
                            W.rank.as<uint32_t>(), ctx->out.as<uint8_t>());
  hipLaunchKernelGGL(k_indexes, dim3(G.count), dim3(256), 0, st, G, W.rank.as<uint32_t>(), ctx->primary.as<int32_t>(),
                     ctx->nidx.as<int32_t>(), ctx->indexes.as<int32_t>());
  HIPCHK(hipEventRecord(ev.e[1], st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  float x = 0;
  HIPCHK(hipEventElapsedTime(&x, ev.e[0], ev.e[1]));
  ms[4] += x;
  return 0;
}

// src[s]: device address of segment s; ctx->off holds the S + 1 offsets.  Plans, sorts, leaves the result in ctx.
int transform(spring_bwt_ctx *ctx, const std::vector<uint64_t> &src, spring_bwt_info *info_out) {
  const int dev = ctx->dev;
  hipStream_t st = ctx->st;
  const std::vector<uint64_t> &off = ctx->off;
  const uint64_t S = src.size(), nbytes = off[S];
  spring_bwt_info I;
  memset(&I, 0, sizeof(I));
  I.num_segments = S;
  I.bytes = nbytes;
  for (uint64_t s = 0; s < S; s++) I.max_segment = std::max(I.max_segment, off[s + 1] - off[s]);
  if (I.max_segment > bwt::MAX_SEGMENT)
    return fail(SPRING_REORDER_E_ARG, "a segment of %llu bytes: more than 1 GiB", (unsigned long long)I.max_segment);
  if (S >= 0x7fffffffull) return fail(SPRING_REORDER_E_ARG, "too many segments");
  // ---- the result's own buffers, then the budget from what is left
  DALLOC(ctx->out, nbytes + 16);
  DALLOC(ctx->primary, S * 4);
  DALLOC(ctx->nidx, S * 4);
  DALLOC(ctx->indexes, S * SPRING_BWT_MAX_INDEXES * 4);
  DBuf d_off, d_src;
  DALLOC(d_off, (S + 1) * 8);
  DALLOC(d_src, S * 8);
  uint64_t budget = 0;
  if (int r = workspace_budget(ctx->workspace_bytes, SORT_FIXED_BYTES << 2, &budget)) return r;
  I.workspace_bytes = budget;
  std::vector<uint64_t> first(S + 2);
  const bool runs = ctx->run_keys;
  const int64_t nsub = bwt::plan_sub_batches(off.data(), S, budget, first.data(), runs);
  if (nsub < 0) {
    const uint64_t s = (uint64_t)(-1 - nsub);
    return fail(SPRING_REORDER_E_ARG, "segment %llu of %llu bytes needs %llu bytes of workspace, the budget is %llu",
                (unsigned long long)s, (unsigned long long)(off[s + 1] - off[s]),
                (unsigned long long)bwt::workspace_need(off[s + 1] - off[s], 1, runs), (unsigned long long)budget);
  }
  I.sub_batches = (uint64_t)nsub;
  if (runs && ctx->cap_bits)
    for (int64_t b = 0; b < nsub; b++) {
      const int own = bwt::run_key_layout(first[b + 1] - first[b]).run_bits;
      if ((int)ctx->cap_bits > own)
        return fail(SPRING_REORDER_E_ARG, "cap_bits %u, but the run-key layout of a sub-batch of %llu segments has %d bits",
                    ctx->cap_bits, (unsigned long long)(first[b + 1] - first[b]), own);
    }
  if (S == 0) {
    ctx->info = I;
    ctx->have = true;
    if (info_out) *info_out = I;
    return 0;
  }
  HIPCHK(hipMemcpyAsync(d_off.p, off.data(), (S + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_src.p, src.data(), S * 8, hipMemcpyHostToDevice, st));
  uint64_t mmax = 0;
  for (int64_t b = 0; b < nsub; b++) mmax = std::max(mmax, off[first[b + 1]] - off[first[b]]);
  Work W;
  SyncOnExit sync_on_exit{st};
  if (mmax) {
    size_t tb = 0;
    const int r = tmp_need(st, mmax, &tb);
    if (r) return r;
    if (tb > mmax * 24 + SORT_FIXED_BYTES)
      return fail(SPRING_REORDER_E_HIP, "the sort asks for %zu bytes of temporary storage for %llu entries", tb, (unsigned long long)mmax);
    W.tmp_bytes = std::max<size_t>(tb, mmax * 16 + (1u << 20));   // later rounds sort fewer entries and fewer bits
    DALLOC(W.tmp, W.tmp_bytes + 16);
    DALLOC(W.key, mmax * 8); DALLOC(W.key2, mmax * 8);
    DALLOC(W.posA, mmax * 4); DALLOC(W.posB, mmax * 4);
    DALLOC(W.uslot, mmax * 4); DALLOC(W.uslot2, mmax * 4);
    DALLOC(W.rank, mmax * 4); DALLOC(W.sa, mmax * 4);
    DALLOC(W.f, mmax * 4); DALLOC(W.h, mmax * 4);
    if (runs) DALLOC(W.hop, mmax * 4);
  }
  DALLOC(W.counter, 16);
  double ms[5] = {0, 0, 0, 0, 0};
  for (int64_t b = 0; b < nsub; b++) {
    Sub G;
    G.src = d_src.as<uint64_t>();
    G.off = d_off.as<uint64_t>();
    G.first = (uint32_t)first[b];
    G.count = (uint32_t)(first[b + 1] - first[b]);
    G.base = off[first[b]];
    G.m = (uint32_t)(off[first[b + 1]] - off[first[b]]);
    uint64_t longest = 0, rounds = 0, run_positions = 0;
    for (uint64_t s = first[b]; s < first[b + 1]; s++) longest = std::max(longest, off[s + 1] - off[s]);
    const int r = sort_sub(ctx, G, longest, W, &rounds, &run_positions, ms);
    if (r) return r;
    I.run_positions += run_positions;
    I.rounds = std::max(I.rounds, rounds);
    I.rounds_total += rounds;
  }
  for (int k = 0; k < 5; k++) { I.ms_pass[k] = ms[k]; I.ms_device += ms[k]; }
  ctx->info = I;
  ctx->have = true;
  if (info_out) *info_out = I;
  return 0;
}

}  // namespace

extern "C" {

int spring_bwt_create(int device, spring_bwt_ctx **out) {
  if (!out) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  const int r = stage_device(&device, "the block-sort stage");
  if (r) return r;
  spring_bwt_ctx *c = new spring_bwt_ctx();
  c->dev = device;
  memset(&c->info, 0, sizeof(c->info));
  *out = c;
  return 0;
}

void spring_bwt_destroy(spring_bwt_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->dev);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  drop_result(ctx);
  if (ctx->st) (void)hipStreamDestroy(ctx->st);
  delete ctx;
}

int spring_bwt_set_block_bytes(spring_bwt_ctx *ctx, uint64_t block_bytes) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (block_bytes < 1 || block_bytes > bwt::MAX_SEGMENT)
    return fail(SPRING_REORDER_E_ARG, "block_bytes must be in 1 .. 2^30 (got %llu)", (unsigned long long)block_bytes);
  ctx->block_bytes = block_bytes;
  return 0;
}

int spring_bwt_set_workspace_bytes(spring_bwt_ctx *ctx, uint64_t workspace_bytes) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  ctx->workspace_bytes = workspace_bytes;
  return 0;
}

uint64_t spring_bwt_workspace_need(uint64_t bytes, uint64_t segments) { return bwt::workspace_need(bytes, segments); }

int spring_bwt_set_run_keys(spring_bwt_ctx *ctx, int32_t on, uint32_t cap_bits) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (cap_bits == 1 || cap_bits > (uint32_t)bwt::MAX_RUN_BITS)
    return fail(SPRING_REORDER_E_ARG, "cap_bits must be 0 or in 2 .. %d (got %u)", bwt::MAX_RUN_BITS, cap_bits);
  ctx->run_keys = on != 0;
  ctx->cap_bits = cap_bits;
  return 0;
}

int spring_bwt_from_host(spring_bwt_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const uint64_t *seg_off,
                         uint64_t num_segments, spring_bwt_info *info) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  (void)hipSetDevice(ctx->dev);
  drop_result(ctx);
  if (nbytes && !bytes) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  const uint64_t one[2] = {0, nbytes};
  if (!seg_off) { seg_off = one; num_segments = 1; }
  if (num_segments >= 0x7fffffffull) return fail(SPRING_REORDER_E_ARG, "too many segments");
  if (seg_off[0] != 0 || seg_off[num_segments] != nbytes)
    return fail(SPRING_REORDER_E_ARG, "the segment offsets do not start at 0 and end at the %llu bytes", (unsigned long long)nbytes);
  for (uint64_t s = 0; s < num_segments; s++)
    if (seg_off[s + 1] < seg_off[s]) return fail(SPRING_REORDER_E_ARG, "the segment offsets decrease");
  int r = stream_begin(ctx->dev, &ctx->st);
  if (r) return r;
  const int dev = ctx->dev;
  DBuf up;
  DALLOC(up, nbytes + 32);
  if (nbytes) HIPCHK(hipMemcpyAsync(up.p, bytes, nbytes, hipMemcpyHostToDevice, ctx->st));
  ctx->off.assign(seg_off, seg_off + num_segments + 1);
  std::vector<uint64_t> src(num_segments);
  ctx->seg_stream.assign(num_segments, -1);
  ctx->seg_block.resize(num_segments);
  ctx->seg_cut.assign(num_segments, 0);
  for (uint64_t s = 0; s < num_segments; s++) {
    src[s] = reinterpret_cast<uint64_t>(up.as<uint8_t>() + seg_off[s]);
    ctx->seg_block[s] = (uint32_t)s;
  }
  r = transform(ctx, src, info);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  if (r) drop_result(ctx);
  return r;
}

int spring_bwt_from_streams(spring_bwt_ctx *ctx, spring_streams_ctx *streams, uint32_t stream_mask, spring_bwt_info *info) {
  if (!ctx || !streams) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  (void)hipSetDevice(ctx->dev);
  drop_result(ctx);
  sr::StreamsView V;
  int r = sr::streams_view(streams, &V);
  if (r) return r;
  if (V.dev != ctx->dev) return fail(SPRING_REORDER_E_ARG, "streams and block-sort contexts live on different devices");
  const uint64_t nb = V.info.num_blocks, B = ctx->block_bytes;
  std::vector<uint64_t> src;
  ctx->off.assign(1, 0);
  for (int s = 0; s < SPRING_STREAMS_NUM; s++) {
    if (!(stream_mask >> s & 1)) continue;
    const uint64_t *tab = V.table + (uint64_t)s * (nb + 1);
    for (uint64_t b = 0; b < nb; b++) {
      if (tab[b + 1] < tab[b] || tab[b + 1] > V.info.bytes[s]) return fail(SPRING_REORDER_E_STATE, "the streams context's block table is damaged");
      for (uint64_t lo = tab[b], c = 0; lo < tab[b + 1]; lo += B, c++) {
        const uint64_t len = std::min(B, tab[b + 1] - lo);
        src.push_back(reinterpret_cast<uint64_t>(V.bytes[s] + lo));
        ctx->off.push_back(ctx->off.back() + len);
        ctx->seg_stream.push_back(s);
        ctx->seg_block.push_back((uint32_t)b);
        ctx->seg_cut.push_back((uint32_t)c);
      }
    }
  }
  if ((r = stream_begin(ctx->dev, &ctx->st))) { drop_result(ctx); return r; }
  r = transform(ctx, src, info);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  if (r) drop_result(ctx);
  return r;
}

int spring_bwt_from_qualid(spring_bwt_ctx *ctx, spring_qualid_ctx *q, int32_t kind, uint64_t block_bytes,
                           spring_bwt_info *info) {
  if (!ctx || !q) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  (void)hipSetDevice(ctx->dev);
  drop_result(ctx);
  if (kind != SPRING_QUALID_QUALITY && kind != SPRING_QUALID_ID)
    return fail(SPRING_REORDER_E_ARG, "kind must be SPRING_QUALID_QUALITY or SPRING_QUALID_ID (got %d)", kind);
  if (block_bytes > bwt::MAX_SEGMENT)
    return fail(SPRING_REORDER_E_ARG, "block_bytes must be 0 or in 1 .. 2^30 (got %llu)", (unsigned long long)block_bytes);
  sr::QualIdView V;
  int r = sr::qualid_view(q, &V);
  if (r) return r;
  if (!V.have[kind]) return fail(SPRING_REORDER_E_STATE, "the quality / id context holds no %s blocks", kind ? "id" : "quality");
  if (V.dev != ctx->dev) return fail(SPRING_REORDER_E_ARG, "quality / id and block-sort contexts live on different devices");
  const uint64_t nb = V.info.num_blocks, B = block_bytes ? block_bytes : QUALID_BLOCK_BYTES;
  const uint64_t *tab = V.table[kind];
  std::vector<uint64_t> src;
  ctx->off.assign(1, 0);
  for (uint64_t b = 0; b < nb; b++) {
    if (tab[b + 1] < tab[b] || tab[b + 1] > V.info.bytes[kind])
      return fail(SPRING_REORDER_E_STATE, "the quality / id context's block table is damaged");
    for (uint64_t lo = tab[b], c = 0; lo < tab[b + 1]; lo += B, c++) {
      const uint64_t len = std::min(B, tab[b + 1] - lo);
      src.push_back(reinterpret_cast<uint64_t>(V.bytes[kind] + lo));
      ctx->off.push_back(ctx->off.back() + len);
      ctx->seg_stream.push_back(kind == SPRING_QUALID_QUALITY ? SPRING_BWT_SRC_QUALITY : SPRING_BWT_SRC_ID);
      ctx->seg_block.push_back((uint32_t)b);
      ctx->seg_cut.push_back((uint32_t)c);
    }
  }
  if ((r = stream_begin(ctx->dev, &ctx->st))) { drop_result(ctx); return r; }
  r = transform(ctx, src, info);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  if (r) drop_result(ctx);
  return r;
}

int spring_bwt_get_info(spring_bwt_ctx *ctx, spring_bwt_info *info) {
  if (!ctx || !info) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing transformed yet");
  *info = ctx->info;
  return 0;
}

int spring_bwt_download(spring_bwt_ctx *ctx, uint8_t *out, uint64_t *seg_off, int32_t *primary, int32_t *num_indexes,
                        int32_t *indexes) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing transformed yet");
  HIPCHK(hipSetDevice(ctx->dev));
  const uint64_t S = ctx->info.num_segments;
  if (seg_off) memcpy(seg_off, ctx->off.data(), (S + 1) * 8);
  if (out && ctx->info.bytes) HIPCHK(rd(ctx->st, out, ctx->out.p, ctx->info.bytes));
  if (primary && S) HIPCHK(rd(ctx->st, primary, ctx->primary.p, S * 4));
  if (num_indexes && S) HIPCHK(rd(ctx->st, num_indexes, ctx->nidx.p, S * 4));
  if (indexes && S) HIPCHK(rd(ctx->st, indexes, ctx->indexes.p, S * SPRING_BWT_MAX_INDEXES * 4));
  return 0;
}

int spring_bwt_segments(spring_bwt_ctx *ctx, int32_t *stream, uint32_t *block, uint32_t *cut) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing transformed yet");
  const uint64_t S = ctx->info.num_segments;
  if (stream && S) memcpy(stream, ctx->seg_stream.data(), S * 4);
  if (block && S) memcpy(block, ctx->seg_block.data(), S * 4);
  if (cut && S) memcpy(cut, ctx->seg_cut.data(), S * 4);
  return 0;
}

int spring_bwt_round_entries(spring_bwt_ctx *ctx, uint64_t *entries, uint64_t max_entries) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing transformed yet");
  for (uint64_t k = 0; entries && k < max_entries; k++) entries[k] = k < ctx->round_entries.size() ? ctx->round_entries[k] : 0;
  return 0;
}

int spring_bwt_encode_inplace(spring_bwt_ctx *ctx, uint8_t *T, int32_t n, uint8_t *num_indexes, int32_t *indexes) {
  if (!ctx || n < 0 || (n && !T)) return fail(SPRING_REORDER_E_ARG, "bad argument");
  if (num_indexes) *num_indexes = 0;
  const int r = spring_bwt_from_host(ctx, T, (uint64_t)n, nullptr, 0, nullptr);
  if (r) return r;
  int32_t primary = 0, ni = 0;
  std::vector<int32_t> idx(SPRING_BWT_MAX_INDEXES);
  const int r2 = spring_bwt_download(ctx, T, nullptr, &primary, &ni, idx.data());
  if (r2) return r2;
  if (num_indexes) *num_indexes = (uint8_t)ni;
  if (indexes) memcpy(indexes, idx.data(), (size_t)ni * 4);
  return primary;
}

}  // extern "C"

namespace sr {
int bwt_view(spring_bwt_ctx *ctx, BwtView *v) {
  if (!ctx || !v) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing transformed yet");
  *v = BwtView{ctx->dev, ctx->info.num_segments, ctx->info.bytes, ctx->out.as<uint8_t>(), ctx->primary.as<int32_t>(),
               ctx->off.data(), ctx->nidx.as<int32_t>(), ctx->indexes.as<int32_t>(), ctx->seg_stream.data(),
               ctx->seg_block.data(), ctx->seg_cut.data()};
  return 0;
}
int bwt_device(spring_bwt_ctx *ctx) { return ctx->dev; }
}  // namespace sr
