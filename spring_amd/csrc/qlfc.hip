// spring_amd/csrc/qlfc.hip -- libbsc's bsc_coder_compress (LIBBSC_CODER_QLFC_STATIC, fast mode) for a batch of byte
// segments in HBM (include/spring_qlfc.h), one sub-batch of whole segments at a time.
//
// The static coder's binary decisions, their order and the three predictors each one reads are a function of the input
// alone, and every predictor ("slot") is a recurrence over its own decisions.  So:
//
//   1  chunk cuts, run heads (scan), per run its byte and start; ranks from a tile-wise next-occurrence table
//   2  contexts: one wavefront per chunk walks its runs (integers only: histories, avgRank, sliding contexts) and
//      leaves per run the two state-table indexes, the escape flag and the number of its events;  events: one lane per
//      run looks the states up and writes (bit, three slots)
//   3  slots: stable radix sort of the (chunk, slot) keys, then one lane per slot walks its list and writes the value
//      in front of every update back to the event
//   4  probabilities: one lane per event, the weighted sum
//   5  range coder: one wavefront per chunk over its (bit, probability) stream, 64 events loaded at a time
//   6  assembly: the host settles CheckEOB, raw chunks and sizes from two integers per chunk; one copy kernel
//
// Every loop on the device is bounded by a count known before it starts; no kernel waits for another lane's result.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include <hip/hip_runtime.h>

#include "bwt_internal.h"
#include "copy_words.h"
#include "qlfc_plan.h"
#include "reorder_device.h"
#include "reorder_internal.h"
#include "spring_qlfc.h"
#include "stage_host.h"

using namespace sr;

static_assert(qlfc::EVENT_NEED == SPRING_QLFC_EVENT_BYTES, "spring_qlfc.h and qlfc_plan.h disagree");
static_assert(qlfc::MAX_SEGMENT == SPRING_QLFC_MAX_SEGMENT, "spring_qlfc.h and qlfc_plan.h disagree");

namespace {

using qlfc::INF;
using qlfc::TILE;

// qlfc_params.h, in the order of qlfc::Family and qlfc::Kind
#define QLFC_ROW_(f, k, th0, ar0, th1, ar1) {th0, ar0, th1, ar1},
#define QLFC_MIX_(f, a, b, c) {a, b, c},
#define QLFC_NONE_(...)
__constant__ int c_rows[QLFC_FAMILIES * QLFC_KINDS][4] = {QLFC_PARAM_TABLE(QLFC_ROW_, QLFC_NONE_)};
__constant__ int c_mix[QLFC_FAMILIES][QLFC_KINDS] = {QLFC_PARAM_TABLE(QLFC_NONE_, QLFC_MIX_)};

// A sub-batch: segments [first, first + count) of the batch; position p of it is byte off[first] + p of the batch.
struct Sub {
  const uint64_t *src;      // per segment of the batch: the device address of its first byte
  const uint64_t *off;      // per segment + 1: its offset in the batch
  const uint32_t *cfirst;   // per segment of the sub-batch + 1: its first chunk
  uint32_t first, count;
  uint64_t base;            // off[first]
  uint32_t m;               // positions
  uint32_t C;               // chunks
};

struct Chunks {
  uint32_t *seg;     // C: the segment (relative to Sub.first)
  uint32_t *start;   // C + 1: first position; start[C] = m
  uint32_t *run;     // C + 1: first run; run[C] = R
};

__device__ __forceinline__ const uint8_t *byte_at(const Sub &G, const Chunks &K, uint32_t c, uint32_t p) {
  const uint32_t s = K.seg[c];
  return reinterpret_cast<const uint8_t *>(G.src[G.first + s]) + (p - (uint32_t)(G.off[G.first + s] - G.base));
}

// ------------------------------------------------------------------ 1: cuts, runs, ranks
// bsc_coder_split_blocks: one block per segment.
__global__ __launch_bounds__(1024) void k_cuts(Sub G, Chunks K) {
  __shared__ uint32_t sh[1024];
  __shared__ uint32_t total;
  const uint32_t s = blockIdx.x, t = threadIdx.x;
  if (s == 0 && t == 0) K.start[G.C] = G.m;
  const uint32_t so = (uint32_t)(G.off[G.first + s] - G.base);
  const uint32_t n = (uint32_t)(G.off[G.first + s + 1] - G.off[G.first + s]);
  const uint32_t c0 = G.cfirst[s], k = G.cfirst[s + 1] - c0;
  if (k == 0) return;
  if (t < k) K.seg[c0 + t] = s;
  if (k == 1) {
    if (t == 0) K.start[c0] = so;
    return;
  }
  const uint8_t *a = reinterpret_cast<const uint8_t *>(G.src[G.first + s]);
  const uint32_t ns = (n - 1 + 31) / 32;   // the samples: positions 1 + 32 j < n
  const uint32_t per = (ns + 1023) / 1024;
  const uint32_t lo = min(ns, t * per), hi = min(ns, lo + per);
  uint32_t cnt = 0;
  for (uint32_t j = lo; j < hi; j++) cnt += a[1 + 32 * j] != a[32 * j];
  sh[t] = cnt;
  __syncthreads();
  if (t == 0) {
    uint32_t acc = 0;
    for (uint32_t i = 0; i < 1024; i++) { const uint32_t v = sh[i]; sh[i] = acc; acc += v; }
    total = acc;
  }
  __syncthreads();
  if (total > k) {
    const uint32_t every = total / k;
    uint32_t seen = sh[t];
    if (t == 0) K.start[c0] = so;
    for (uint32_t j = lo; j < hi; j++)
      if (a[1 + 32 * j] != a[32 * j]) {
        seen++;
        const uint32_t id = seen / every;
        if (seen % every == 0 && id < k) K.start[c0 + id] = so + 1 + 32 * j;
      }
  } else if (t < k) {
    K.start[c0 + t] = so + (n / k) * t;
  }
}

// One position per lane: is it the first of a run of its chunk?
__global__ __launch_bounds__(256) void k_heads(Sub G, Chunks K, uint32_t *__restrict__ flag) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= G.m) return;
  const uint32_t c = last_le(G.C, p, K.start);
  bool head = p == K.start[c];
  if (!head) {
    const uint8_t *a = byte_at(G, K, c, p);
    head = a[0] != a[-1];
  }
  flag[p] = head;
}

// ridx: the exclusive scan of flag.  counter[0] = R.
__global__ __launch_bounds__(256) void k_runs(Sub G, Chunks K, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ ridx,
                                              uint32_t *__restrict__ rpos, uint8_t *__restrict__ rsym, uint32_t *__restrict__ counter) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= G.m) return;
  if (p == G.m - 1) {
    const uint32_t R = ridx[p] + flag[p];
    rpos[R] = G.m;
    K.run[G.C] = R;
    counter[0] = R;
  }
  if (!flag[p]) return;
  const uint32_t r = ridx[p], c = last_le(G.C, p, K.start);
  rpos[r] = p;
  rsym[r] = *byte_at(G, K, c, p);
  if (p == K.start[c]) K.run[c] = r;
}

// first[t * 256 + s]: the first run of tile t with byte s, or INF.
__global__ __launch_bounds__(256) void k_tile_first(const uint8_t *__restrict__ rsym, uint32_t R, uint32_t *__restrict__ first) {
  __shared__ uint32_t tab[256];
  tab[threadIdx.x] = INF;
  __syncthreads();
  const uint32_t r = blockIdx.x * TILE + threadIdx.x;
  if (r < R) atomicMin(&tab[rsym[r]], r);
  __syncthreads();
  first[blockIdx.x * TILE + threadIdx.x] = tab[threadIdx.x];
}

// In place: next[t * 256 + s] = the first run behind tile t with byte s, or INF.  One block, lane s walks the tiles.
__global__ __launch_bounds__(256) void k_tile_next(uint32_t *__restrict__ tab, uint32_t tiles) {
  uint32_t cur = INF;
  for (uint32_t t = tiles; t-- > 0;) {
    const uint32_t f = tab[t * TILE + threadIdx.x];
    tab[t * TILE + threadIdx.x] = cur;
    if (f != INF) cur = f;
  }
}

// One wavefront per tile of 256 runs, walking it backwards.  Lane l keeps, for the bytes l, 64 + l, 128 + l, 192 + l,
// the next run of its chunk with that byte (nx).  The rank of a run is the number of bytes whose next run comes before
// the next run of the run's own byte: the distinct bytes in between, or all bytes behind it when its byte does not
// come again (qlfc.cpp:52-109 read backwards).  The last run of a chunk gets 1 (:97).  At the first run of a chunk nx
// is the first occurrence of every byte: their order is the symbol table's.
__global__ __launch_bounds__(64) void k_ranks(Chunks K, uint32_t C, const uint8_t *__restrict__ rsym, uint32_t R,
                                              const uint32_t *__restrict__ next, uint8_t *__restrict__ rrank,
                                              uint8_t *__restrict__ order, uint32_t *__restrict__ nsym) {
  const uint32_t t = blockIdx.x, l = threadIdx.x;
  uint32_t nx[4], sym[4], chunk[4];
  const uint32_t rl = min(R, (t + 1) * TILE) - 1;   // the tile's last run
  const uint32_t cl = last_le(C, rl, K.run), end = K.run[cl + 1];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t v = next[t * TILE + k * 64 + l];
    nx[k] = v < end ? v : INF;
    const uint32_t r = t * TILE + k * 64 + l;
    sym[k] = r < R ? rsym[r] : 0;
    chunk[k] = r < R ? last_le(C, r, K.run) : 0;
  }
#pragma unroll
  for (int k = 3; k >= 0; k--) {
    for (int i = 63; i >= 0; i--) {
      const uint32_t r = t * TILE + k * 64 + i;
      if (r >= R) continue;   // uniform
      const uint32_t c = __shfl(sym[k], i), ch = __shfl(chunk[k], i);
      const bool last = r + 1 == K.run[ch + 1];
      uint32_t rank = 1;
      if (last) {
        nx[0] = nx[1] = nx[2] = nx[3] = INF;
      } else {
        const uint32_t mine = (c >> 6) == 0 ? nx[0] : (c >> 6) == 1 ? nx[1] : (c >> 6) == 2 ? nx[2] : nx[3];
        const uint32_t nc = __shfl(mine, c & 63);
        rank = __popcll(__ballot(nx[0] < nc)) + __popcll(__ballot(nx[1] < nc)) + __popcll(__ballot(nx[2] < nc)) +
               __popcll(__ballot(nx[3] < nc));
      }
      if (l == (c & 63)) {
        if ((c >> 6) == 0) nx[0] = r; else if ((c >> 6) == 1) nx[1] = r; else if ((c >> 6) == 2) nx[2] = r; else nx[3] = r;
      }
      if (l == 0) rrank[r] = (uint8_t)rank;
      if (r == K.run[ch]) {   // the chunk's first run: the symbol table's order
        uint32_t before[4] = {0, 0, 0, 0};
#pragma unroll
        for (int kk = 0; kk < 4; kk++)
          for (int j = 0; j < 64; j++) {
            const uint32_t v = __shfl(nx[kk], j);
#pragma unroll
            for (int q = 0; q < 4; q++) before[q] += v < nx[q];
          }
#pragma unroll
        for (int q = 0; q < 4; q++)
          if (nx[q] != INF) order[(size_t)ch * 256 + before[q]] = (uint8_t)(q * 64 + l);
        const uint32_t ns = __popcll(__ballot(nx[0] != INF)) + __popcll(__ballot(nx[1] != INF)) +
                            __popcll(__ballot(nx[2] != INF)) + __popcll(__ballot(nx[3] != INF));
        if (l == 0) nsym[ch] = ns;
      }
    }
  }
}

// ------------------------------------------------------------------ 2: contexts and events
// One wavefront per chunk walks its runs: the recurrences of qlfc.cpp:543-748 that carry no probability.  The lanes load
// 64 runs at a time; every lane then steps through them on the same values (v_readlane), so the walk itself waits for no
// memory but the two history bytes in LDS, and lane i keeps what belongs to run i.  The walk leaves the two table indexes
// of a run, not the states: the look-up feeds nothing back, so it is k_events' (one lane per run).
__device__ __forceinline__ uint32_t lane_value(uint32_t v, uint32_t lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}

__global__ __launch_bounds__(64) void k_contexts(Chunks K, const uint8_t *__restrict__ rsym, const uint8_t *__restrict__ rrank,
                                                 const uint32_t *__restrict__ rpos, const uint32_t *__restrict__ nsym,
                                                 uint16_t *__restrict__ irank, uint16_t *__restrict__ irun, uint8_t *__restrict__ resc,
                                                 uint32_t *__restrict__ evoff, uint64_t *__restrict__ cevn) {
  __shared__ uint8_t hist[2][256];   // rankHistory, runHistory
  const uint32_t c = blockIdx.x, l = threadIdx.x;
  for (uint32_t i = l; i < 256; i += 64) hist[0][i] = hist[1][i] = 0;
  __syncthreads();
  const int maxrank = qlfc::max_rank(nsym[c]);
  uint32_t ctx0 = 0, ctx4 = 0, ctxrun = 0, avg = 0;
  uint64_t ev = 0;
  const uint32_t r1 = K.run[c + 1];
  for (uint32_t base = K.run[c]; base < r1; base += 64) {
    const uint32_t r = base + l;
    uint32_t sym_l = 0, rank_l = 1, run_l = 1;
    if (r < r1) { sym_l = rsym[r]; rank_l = rrank[r]; run_l = rpos[r + 1] - rpos[r]; }
    const uint32_t cnt = min(64u, r1 - base);
    uint32_t my_irank = 0, my_irun = 0, my_esc = 0, my_ev = 0;
    for (uint32_t i = 0; i < cnt; i++) {
      const uint32_t sym = lane_value(sym_l, i), rank = lane_value(rank_l, i), run = lane_value(run_l, i);
      const bool esc = avg >= 32;
      const uint32_t rk = rank - 1, hr = hist[0][sym], hu = hist[1][sym];
      const uint32_t ir = ctxrun << 11 | ctx4 << 3 | hr;
      const uint32_t iu = ctx0 << 10 | ctxrun << 6 | min(rk, 7u) << 3 | min(hu, 7u);
      hist[0][sym] = (uint8_t)qlfc::log2i(rank);   // every lane writes the same byte (rank 1 gives 0 on either path)
      hist[1][sym] = (uint8_t)(run == 1 ? (hu + 2) >> 2 : (hu + 3 * (uint32_t)qlfc::log2i(run) + 3) >> 2);
      if (i == l) { my_irank = ir; my_irun = iu; my_esc = esc; my_ev = (uint32_t)ev; }
      avg = (avg * 124 + rank * 4) >> 7;
      ev += qlfc::rank_events(rank, esc, maxrank) + qlfc::run_events(run);
      ctx0 = (ctx0 << 1 | (rk == 0)) & 7;
      ctx4 = (ctx4 << 2 | min(rk, 3u)) & 0xff;
      ctxrun = (ctxrun << 1 | (run < 3)) & 0xf;
    }
    if (r < r1) {
      irank[r] = (uint16_t)my_irank;
      irun[r] = (uint16_t)my_irun;
      resc[r] = (uint8_t)my_esc;
      evoff[r] = my_ev;
    }
  }
  if (l == 0) cevn[c] = ev;
}

struct EventOut {
  uint64_t *key;    // 3 E: chunk << 24 | slot
  uint32_t *val;    // 3 E: its own index
  uint8_t *bit;     // E: bit | family << 1
};

__device__ __forceinline__ void put(const EventOut &V, uint32_t &e, uint32_t chunk, int family, uint32_t bit, uint32_t sym,
                                    uint32_t state, uint32_t hi, uint32_t lo) {
  const uint64_t top = (uint64_t)chunk << qlfc::SLOT_BITS;
  V.key[3 * (size_t)e + 0] = top | qlfc::slot(family, qlfc::CHAR, sym, hi, lo);
  V.key[3 * (size_t)e + 1] = top | qlfc::slot(family, qlfc::STATE, state, hi, lo);
  V.key[3 * (size_t)e + 2] = top | qlfc::slot(family, qlfc::STATIC, 0, hi, lo);
  V.val[3 * (size_t)e + 0] = 3 * e + 0;
  V.val[3 * (size_t)e + 1] = 3 * e + 1;
  V.val[3 * (size_t)e + 2] = 3 * e + 2;
  V.bit[e] = (uint8_t)(bit | family << 1);
  e++;
}

// One lane per run: its decisions in the coder's order (qlfc.cpp:551-744).  cev: the first event of every chunk.
__global__ __launch_bounds__(256) void k_events(Chunks K, uint32_t C, uint32_t R, const uint8_t *__restrict__ rsym,
                                                const uint8_t *__restrict__ rrank, const uint32_t *__restrict__ rpos,
                                                const uint32_t *__restrict__ nsym, const uint16_t *__restrict__ irank,
                                                const uint16_t *__restrict__ irun, const uint8_t *__restrict__ rank_tab,
                                                const uint8_t *__restrict__ run_tab, const uint8_t *__restrict__ resc,
                                                const uint32_t *__restrict__ evoff, const uint32_t *__restrict__ cev, EventOut V,
                                                uint32_t *__restrict__ lastev) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= R) return;
  const uint32_t ch = last_le(C, r, K.run);
  const int maxrank = qlfc::max_rank(nsym[ch]);
  const uint32_t sym = rsym[r], rank = rrank[r], run = rpos[r + 1] - rpos[r];
  uint32_t e = cev[ch] + evoff[r];
  if (r + 1 == K.run[ch + 1]) lastev[ch] = e;
  uint32_t st = rank_tab[irank[r]];
  if (resc[r]) {
    uint32_t ctx = 1;
    for (int b = maxrank; b >= 0; b--) {
      const uint32_t bit = rank >> b & 1;
      put(V, e, ch, qlfc::RANK_ESC, bit, sym, st, 0, ctx);
      ctx += ctx + bit;
    }
  } else if (rank == 1) {
    put(V, e, ch, qlfc::RANK_TOP, 0, sym, st, 0, 0);
  } else {
    put(V, e, ch, qlfc::RANK_TOP, 1, sym, st, 0, 0);
    const int x = qlfc::log2i(rank);
    for (int j = 0; j < x - 1; j++) put(V, e, ch, qlfc::RANK_EXP, 1, sym, st, 0, j);
    if (x < maxrank) put(V, e, ch, qlfc::RANK_EXP, 0, sym, st, 0, x - 1);
    uint32_t ctx = 1;
    for (int b = x - 1; b >= 0; b--) {
      const uint32_t bit = rank >> b & 1;
      put(V, e, ch, qlfc::RANK_MAN, bit, sym, st, x, ctx);
      ctx += ctx + bit;
    }
  }
  st = run_tab[irun[r]];
  if (run == 1) {
    put(V, e, ch, qlfc::RUN_TOP, 0, sym, st, 0, 0);
  } else {
    put(V, e, ch, qlfc::RUN_TOP, 1, sym, st, 0, 0);
    const int x = qlfc::log2i(run);
    for (int j = 0; j < x - 1; j++) put(V, e, ch, qlfc::RUN_EXP, 1, sym, st, 0, j);
    put(V, e, ch, qlfc::RUN_EXP, 0, sym, st, 0, x - 1);
    uint32_t ctx = 1;
    for (int b = x - 1; b >= 0; b--) {
      const uint32_t bit = run >> b & 1;
      put(V, e, ch, qlfc::RUN_MAN, bit, sym, st, x, ctx);
      ctx = x <= 5 ? ctx + ctx + bit : ctx + 1;   // above exponent 5 the context is the bit's position (:733, :741)
    }
  }
}

// ------------------------------------------------------------------ 3: slots
// Sorted by (chunk, slot), stable: one lane per list, from its head on.  pval[v]: the slot's value in front of the
// update of entry v (predictor.h:45-53 through a short).
__global__ __launch_bounds__(256) void k_chains(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                const uint8_t *__restrict__ ebit, uint32_t n3, int16_t *__restrict__ pval) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n3) return;
  const uint64_t k0 = key[j];
  if (j && key[j - 1] == k0) return;
  const int cls = (int)(k0 >> qlfc::CLASS_SHIFT) & 31;
  const int th0 = c_rows[cls][0], ar0 = c_rows[cls][1], th1 = c_rows[cls][2], ar1 = c_rows[cls][3];
  int p = 2048;
  for (uint32_t i = j; i < n3 && key[i] == k0; i++) {
    const uint32_t v = val[i];
    pval[v] = (int16_t)p;
    if (ebit[v / 3] & 1) p = (int16_t)(p - (((p - th1) * ar1) >> 12));
    else p = (int16_t)(p + (((4096 - th0 - p) * ar0) >> 12));
  }
}

// ------------------------------------------------------------------ 4: probabilities
__global__ __launch_bounds__(256) void k_probs(const uint8_t *__restrict__ ebit, const int16_t *__restrict__ pval, uint32_t E,
                                               int32_t *__restrict__ prob) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= E) return;
  const int f = ebit[e] >> 1;
  prob[e] = (pval[3 * (size_t)e] * c_mix[f][0] + pval[3 * (size_t)e + 1] * c_mix[f][1] + pval[3 * (size_t)e + 2] * c_mix[f][2]) >> 5;
}

// ------------------------------------------------------------------ 5: range coder
// rangecoder.h:73-129.  Writes stop at cap (the position goes on counting): a chunk that runs past it has failed.
struct Coder {
  uint64_t low = 0;
  uint32_t range = 0xffffffffu, ffnum = 0, cache = 0, pos = 0, cap;
  uint8_t *out;
  bool writer;
  __device__ __forceinline__ void emit(uint32_t s) {
    if (writer && pos + 2 <= cap) *reinterpret_cast<uint16_t *>(out + pos) = (uint16_t)s;
    pos += 2;
  }
  __device__ __forceinline__ void shift_low() {
    const uint32_t low32 = (uint32_t)low, carry = (uint32_t)(low >> 32);
    if (low32 < 0xffff0000u || carry) {
      emit(cache + carry);
      for (uint32_t k = ffnum; k > 0; k--) emit(carry - 1);
      ffnum = 0;
      cache = low32 >> 16;
    } else {
      ffnum++;
    }
    low = (uint64_t)(uint32_t)(low32 << 16);
  }
  __device__ __forceinline__ void code(uint32_t bit, int32_t p) {
    const uint32_t r = (range >> 12) * (uint32_t)p;
    if (bit) { low += r; range -= r; } else { range = r; }
    if (range < 0x10000u) { range <<= 16; shift_low(); }
  }
};

__device__ __forceinline__ bool any_in(const uint64_t *m, uint32_t lo, uint32_t len) {
  if (len == 128) return (m[lo >> 6] | m[(lo >> 6) + 1]) != 0;
  if (len == 64) return m[lo >> 6] != 0;
  return ((m[lo >> 6] >> (lo & 63)) & ((1ull << len) - 1)) != 0;
}

// One wavefront per chunk: the chunk's size, the symbol table (qlfc.cpp:476-510: a bit is coded only where both of its
// values are still possible among the bytes not yet listed and the one listed last), the events, three shifts.  As in
// k_contexts the lanes load 64 events at a time and every lane runs the coder on the same values; lane 0 writes.
// poslast: the bytes written at the start of the last run, what CheckEOB sees last.
__global__ __launch_bounds__(64) void k_coder(Chunks K, const uint8_t *__restrict__ order, const uint32_t *__restrict__ nsym,
                                              const uint32_t *__restrict__ cev, const uint32_t *__restrict__ lastev,
                                              const uint8_t *__restrict__ ebit, const int32_t *__restrict__ prob,
                                              uint8_t *__restrict__ pay, const uint64_t *__restrict__ payoff,
                                              uint32_t *__restrict__ clen, uint32_t *__restrict__ poslast) {
  const uint32_t c = blockIdx.x, l = threadIdx.x;
  const uint32_t n = K.start[c + 1] - K.start[c];
  Coder co;
  co.writer = l == 0;
  co.out = pay + payoff[c];
  co.cap = n + qlfc::PAY_SLACK - 8;
  for (int b = 31; b >= 0; b--) co.code(n >> b & 1, 2048);
  uint64_t avail[4] = {~0ull, ~0ull, ~0ull, ~0ull};
  const uint32_t ns = nsym[c], listed = ns < 256 ? ns + 1 : 256;   // the last symbol again ends a shorter table
  uint32_t prev = 256;
  for (uint32_t i = 0; i < listed; i++) {
    const uint32_t cur = order[(size_t)c * 256 + (i < ns ? i : ns - 1)];
    if (prev < 256) avail[prev >> 6] |= 1ull << (prev & 63);   // the byte listed last counts as possible once more
    for (int b = 7; b >= 0; b--) {
      const uint32_t lo = cur >> (b + 1) << (b + 1), half = 1u << b;
      if (any_in(avail, lo, half) && any_in(avail, lo + half, half)) co.code(cur >> b & 1, 2048);
    }
    if (prev < 256) avail[prev >> 6] &= ~(1ull << (prev & 63));
    avail[cur >> 6] &= ~(1ull << (cur & 63));
    prev = cur;
  }
  const uint32_t e1 = cev[c + 1], el = lastev[c];
  uint32_t pl = 0;
  for (uint32_t base = cev[c]; base < e1; base += 64) {
    const uint32_t e = base + l;
    uint32_t bit_l = 0, prob_l = 0;
    if (e < e1) { bit_l = ebit[e] & 1; prob_l = (uint32_t)prob[e]; }
    const uint32_t cnt = min(64u, e1 - base);
    for (uint32_t i = 0; i < cnt; i++) {
      if (base + i == el) pl = co.pos;
      co.code(lane_value(bit_l, i), (int32_t)lane_value(prob_l, i));
    }
  }
  co.shift_low();
  co.shift_low();
  co.shift_low();
  if (l == 0) {
    clen[c] = co.pos;
    poslast[c] = pl;
  }
}

// ------------------------------------------------------------------ 6: assembly
struct Piece {
  uint64_t src;   // device address
  uint64_t dst;   // offset in the sub-batch's output
  uint64_t len;
};
__global__ __launch_bounds__(256) void k_assemble(const Piece *__restrict__ pieces, uint8_t *__restrict__ out) {
  const Piece P = pieces[blockIdx.x];
  const uint8_t *s = reinterpret_cast<const uint8_t *>(P.src);
  for (uint64_t i = threadIdx.x; i < P.len; i += 256) out[P.dst + i] = s[i];
}

}  // namespace

struct spring_qlfc_ctx {
  int dev = 0;
  hipStream_t st = nullptr;
  uint64_t workspace_bytes = 0;   // 0: from the free HBM
  bool have_tables = false, have = false;
  DBuf rank_tab, run_tab;
  spring_qlfc_info info;
  std::vector<uint64_t> coded_off;   // num_segments + 1
  std::vector<uint64_t> in_off;      // num_segments + 1: the segments as they came in
  std::vector<int32_t> status;
  std::vector<std::unique_ptr<DBuf>> out;   // per sub-batch: its coded bytes
  std::vector<uint64_t> out_bytes;
  bool have_view = false;            // the device copies a QlfcView hands out
  DBuf v_src, v_off, v_status;
};

namespace {

void drop_result(spring_qlfc_ctx *ctx) {
  ctx->have = false;
  ctx->out.clear();
  ctx->out_bytes.clear();
  ctx->coded_off.clear();
  ctx->in_off.clear();
  ctx->status.clear();
  ctx->have_view = false;
  ctx->v_src.release();
  ctx->v_off.release();
  ctx->v_status.release();
  memset(&ctx->info, 0, sizeof(ctx->info));
}

// One sub-batch, segments [first, first + count).  *fit = false: its events do not fit the budget (nothing is kept).
int code_sub(spring_qlfc_ctx *ctx, const uint64_t *off, const uint64_t *d_src, const uint64_t *d_off, const uint64_t *h_src,
             uint64_t first, uint64_t count, uint64_t budget, bool *fit, uint64_t *events_need) {
  const int dev = ctx->dev;
  hipStream_t st = ctx->st;
  spring_qlfc_info &I = ctx->info;
  *fit = true;
  // ---- chunks
  std::vector<uint32_t> cfirst(count + 1, 0);
  for (uint64_t s = 0; s < count; s++) {
    const uint64_t n = off[first + s + 1] - off[first + s];
    cfirst[s + 1] = cfirst[s] + (n ? qlfc::num_chunks(n) : 0);
  }
  const uint32_t C = cfirst[count];
  const uint32_t m = (uint32_t)(off[first + count] - off[first]);
  std::vector<uint64_t> seg_bytes(count, 0);
  std::vector<int32_t> seg_status(count, 1);
  auto keep = [&](DBuf *out, uint64_t bytes) {
    for (uint64_t s = 0; s < count; s++) {
      ctx->coded_off.push_back(ctx->coded_off.back() + seg_bytes[s]);
      ctx->status.push_back(seg_status[s]);
      I.not_compressible += seg_status[s] != 0;
    }
    ctx->out.emplace_back(out);
    ctx->out_bytes.push_back(bytes);
    I.bytes_out += bytes;
    I.sub_batches++;
  };
  if (C == 0) {   // only empty segments
    keep(new DBuf(), 0);
    return 0;
  }
  Laps T{st};
  DBuf d_cfirst, cseg, cstart, crun, flag, ridx, rpos, rsym, rrank, irank, irun, resc, evoff, tiles, order, nsym, cevn, cev,
      lastev, counter, tmp, pay, payoff, clen, poslast;
  SyncOnExit sync_on_exit{st};
  DALLOC(d_cfirst, (count + 1) * 4);
  DALLOC(cseg, (size_t)C * 4); DALLOC(cstart, ((size_t)C + 1) * 4); DALLOC(crun, ((size_t)C + 1) * 4);
  DALLOC(flag, (size_t)m * 4); DALLOC(ridx, (size_t)m * 4);
  DALLOC(rpos, ((size_t)m + 1) * 4); DALLOC(rsym, m); DALLOC(rrank, m);
  DALLOC(irank, (size_t)m * 2); DALLOC(irun, (size_t)m * 2); DALLOC(resc, m); DALLOC(evoff, (size_t)m * 4);
  DALLOC(order, (size_t)C * 256); DALLOC(nsym, (size_t)C * 4); DALLOC(cevn, (size_t)C * 8); DALLOC(cev, ((size_t)C + 1) * 4);
  DALLOC(lastev, (size_t)C * 4); DALLOC(counter, 16); DALLOC(clen, (size_t)C * 4); DALLOC(poslast, (size_t)C * 4);
  DALLOC(payoff, (size_t)C * 8);
  size_t scan_bytes = 0;
  HIPCHK(sr::excl_scan_u32(st, nullptr, scan_bytes, nullptr, nullptr, m));
  DALLOC(tmp, scan_bytes + 16);
  HIPCHK(hipMemcpyAsync(d_cfirst.p, cfirst.data(), (count + 1) * 4, hipMemcpyHostToDevice, st));
  Sub G{d_src, d_off, d_cfirst.as<uint32_t>(), (uint32_t)first, (uint32_t)count, off[first], m, C};
  Chunks K{cseg.as<uint32_t>(), cstart.as<uint32_t>(), crun.as<uint32_t>()};
  // ---- 1: cuts, runs, ranks
  HIPCHK(T.begin(0));
  hipLaunchKernelGGL(k_cuts, dim3((unsigned)count), dim3(1024), 0, st, G, K);
  hipLaunchKernelGGL(k_heads, grid(m), dim3(256), 0, st, G, K, flag.as<uint32_t>());
  HIPCHK(sr::excl_scan_u32(st, tmp.p, scan_bytes, flag.as<uint32_t>(), ridx.as<uint32_t>(), m));
  hipLaunchKernelGGL(k_runs, grid(m), dim3(256), 0, st, G, K, flag.as<uint32_t>(), ridx.as<uint32_t>(), rpos.as<uint32_t>(),
                     rsym.as<uint8_t>(), counter.as<uint32_t>());
  HIPCHK(hipGetLastError());
  uint32_t R = 0;
  HIPCHK(rd(st, &R, counter.p, 4));
  if (R == 0 || R > m) return fail(SPRING_REORDER_E_STATE, "the run scan gave %u runs for %u bytes", R, m);
  const uint32_t ntiles = (R + TILE - 1) / TILE;
  DALLOC(tiles, (size_t)ntiles * TILE * 4);
  hipLaunchKernelGGL(k_tile_first, dim3(ntiles), dim3(256), 0, st, rsym.as<uint8_t>(), R, tiles.as<uint32_t>());
  hipLaunchKernelGGL(k_tile_next, dim3(1), dim3(256), 0, st, tiles.as<uint32_t>(), ntiles);
  hipLaunchKernelGGL(k_ranks, dim3(ntiles), dim3(64), 0, st, K, C, rsym.as<uint8_t>(), R, tiles.as<uint32_t>(), rrank.as<uint8_t>(),
                     order.as<uint8_t>(), nsym.as<uint32_t>());
  HIPCHK(T.end());
  // ---- 2: contexts, then the events once their number is known
  HIPCHK(T.begin(1));
  hipLaunchKernelGGL(k_contexts, dim3(C), dim3(64), 0, st, K, rsym.as<uint8_t>(), rrank.as<uint8_t>(), rpos.as<uint32_t>(),
                     nsym.as<uint32_t>(), irank.as<uint16_t>(), irun.as<uint16_t>(), resc.as<uint8_t>(), evoff.as<uint32_t>(),
                     cevn.as<uint64_t>());
  HIPCHK(T.end());
  HIPCHK(hipGetLastError());
  std::vector<uint64_t> h_cevn(C);
  std::vector<uint32_t> h_cstart(C + 1), h_cev(C + 1, 0);
  HIPCHK(rd(st, h_cevn.data(), cevn.p, (size_t)C * 8));
  HIPCHK(rd(st, h_cstart.data(), cstart.p, ((size_t)C + 1) * 4));
  uint64_t E = 0;
  for (uint32_t c = 0; c < C; c++) E += h_cevn[c];
  size_t sort_bytes = 0;
  HIPCHK(sr::sort_pairs(st, nullptr, sort_bytes, nullptr, nullptr, nullptr, nullptr, 3 * E, 64));
  const uint64_t need = qlfc::workspace_need(m, count) + E * qlfc::EVENT_NEED;
  *events_need = need;
  if (3 * E >= 0xffffff00ull || need > budget) {
    *fit = false;
    return 0;
  }
  if (sort_bytes > E * (qlfc::EVENT_NEED - qlfc::EVENT_ARRAYS) + qlfc::FIXED_NEED)
    return fail(SPRING_REORDER_E_HIP, "the sort asks for %zu bytes of temporary storage for %llu entries", sort_bytes, (unsigned long long)(3 * E));
  for (uint32_t c = 0; c < C; c++) h_cev[c + 1] = h_cev[c] + (uint32_t)h_cevn[c];
  HIPCHK(hipMemcpyAsync(cev.p, h_cev.data(), ((size_t)C + 1) * 4, hipMemcpyHostToDevice, st));
  std::vector<uint64_t> h_payoff(C);
  for (uint32_t c = 0; c < C; c++) h_payoff[c] = (((uint64_t)h_cstart[c] + 1) & ~1ull) + (uint64_t)qlfc::PAY_SLACK * c;
  HIPCHK(hipMemcpyAsync(payoff.p, h_payoff.data(), (size_t)C * 8, hipMemcpyHostToDevice, st));
  DALLOC(pay, (size_t)m + (size_t)qlfc::PAY_SLACK * (C + 1));
  DBuf key, key2, val, val2, ebit, pval, prob, sort_tmp;
  DALLOC(key, 3 * E * 8); DALLOC(key2, 3 * E * 8); DALLOC(val, 3 * E * 4); DALLOC(val2, 3 * E * 4);
  DALLOC(ebit, E); DALLOC(pval, 3 * E * 2); DALLOC(prob, E * 4); DALLOC(sort_tmp, sort_bytes + 16);
  EventOut V{key.as<uint64_t>(), val.as<uint32_t>(), ebit.as<uint8_t>()};
  HIPCHK(T.begin(1));
  hipLaunchKernelGGL(k_events, grid(R), dim3(256), 0, st, K, C, R, rsym.as<uint8_t>(), rrank.as<uint8_t>(), rpos.as<uint32_t>(),
                     nsym.as<uint32_t>(), irank.as<uint16_t>(), irun.as<uint16_t>(), ctx->rank_tab.as<uint8_t>(), ctx->run_tab.as<uint8_t>(),
                     resc.as<uint8_t>(), evoff.as<uint32_t>(),
                     cev.as<uint32_t>(), V, lastev.as<uint32_t>());
  HIPCHK(T.end());
  // ---- 3: slots
  HIPCHK(T.begin(2));
  int cbits = 1;
  while ((1ull << cbits) < C) cbits++;
  size_t sb = sort_bytes;
  HIPCHK(sr::sort_pairs(st, sort_tmp.p, sb, key.as<uint64_t>(), key2.as<uint64_t>(), val.as<uint32_t>(), val2.as<uint32_t>(), 3 * E,
                        (unsigned)(qlfc::SLOT_BITS + cbits)));
  hipLaunchKernelGGL(k_chains, grid(3 * E), dim3(256), 0, st, key2.as<uint64_t>(), val2.as<uint32_t>(), ebit.as<uint8_t>(),
                     (uint32_t)(3 * E), pval.as<int16_t>());
  HIPCHK(T.end());
  // ---- 4: probabilities
  HIPCHK(T.begin(3));
  hipLaunchKernelGGL(k_probs, grid(E), dim3(256), 0, st, ebit.as<uint8_t>(), pval.as<int16_t>(), (uint32_t)E, prob.as<int32_t>());
  HIPCHK(T.end());
  // ---- 5: range coder
  HIPCHK(T.begin(4));
  hipLaunchKernelGGL(k_coder, dim3(C), dim3(64), 0, st, K, order.as<uint8_t>(), nsym.as<uint32_t>(), cev.as<uint32_t>(),
                     lastev.as<uint32_t>(), ebit.as<uint8_t>(), prob.as<int32_t>(), pay.as<uint8_t>(), payoff.as<uint64_t>(),
                     clen.as<uint32_t>(), poslast.as<uint32_t>());
  HIPCHK(T.end());
  HIPCHK(hipGetLastError());
  std::vector<uint32_t> h_clen(C), h_poslast(C);
  HIPCHK(rd(st, h_clen.data(), clen.p, (size_t)C * 4));
  HIPCHK(rd(st, h_poslast.data(), poslast.p, (size_t)C * 4));
  // ---- 6: CheckEOB, raw chunks, sizes (coder.cpp:110-149), then one copy kernel
  std::vector<Piece> pieces;
  std::vector<uint8_t> heads;
  std::vector<size_t> head_piece;   // pieces whose src is an offset into heads until that is uploaded
  uint64_t total = 0, raw = 0;
  for (uint64_t s = 0; s < count; s++) {
    const int64_t n = (int64_t)(off[first + s + 1] - off[first + s]);
    const uint32_t c0 = cfirst[s], k = cfirst[s + 1] - c0;
    if (k == 0) continue;
    const uint64_t so = off[first + s] - off[first];
    const size_t piece0 = pieces.size(), head0 = heads.size();
    const uint64_t raw0 = raw;
    auto coded_ok = [&](uint32_t c, int64_t output_size) {
      return (int64_t)h_poslast[c] < output_size - 16 && h_clen[c] <= (h_cstart[c + 1] - h_cstart[c]) + qlfc::PAY_SLACK - 8;
    };
    bool ok = true;
    int64_t ptr;
    if (k == 1) {
      ok = coded_ok(c0, n - 1);
      heads.push_back(1);
      ptr = 1;
      if (ok) {
        pieces.push_back(Piece{(uint64_t)(uintptr_t)(pay.as<uint8_t>() + h_payoff[c0]), total + 1, h_clen[c0]});
        ptr += h_clen[c0];
      }
    } else {
      heads.resize(head0 + 1 + 8 * k);
      heads[head0] = (uint8_t)k;
      ptr = 1 + 8 * (int64_t)k;
      for (uint32_t j = 0; j < k && ok; j++) {
        const uint32_t c = c0 + j;
        const int64_t in_size = h_cstart[c + 1] - h_cstart[c];
        int32_t res;
        if (coded_ok(c, std::min<int64_t>(in_size, n - ptr))) {
          res = (int32_t)h_clen[c];
          pieces.push_back(Piece{(uint64_t)(uintptr_t)(pay.as<uint8_t>() + h_payoff[c]), total + (uint64_t)ptr, h_clen[c]});
        } else if (ptr + in_size >= n) {
          ok = false;
          break;
        } else {
          res = (int32_t)in_size;
          raw++;
          pieces.push_back(Piece{h_src[first + s] + (h_cstart[c] - so), total + (uint64_t)ptr, (uint64_t)in_size});
        }
        const int32_t sizes[2] = {(int32_t)in_size, res};
        memcpy(&heads[head0 + 1 + 8 * j], sizes, 8);
        ptr += res;
      }
    }
    if (!ok) {
      pieces.resize(piece0);
      heads.resize(head0);
      raw = raw0;
      continue;
    }
    head_piece.push_back(pieces.size());
    pieces.push_back(Piece{(uint64_t)head0, total, heads.size() - head0});
    seg_status[s] = 0;
    seg_bytes[s] = (uint64_t)ptr;
    total += (uint64_t)ptr;
  }
  std::unique_ptr<DBuf> out(new DBuf());
  HIPCHK(out->alloc(dev, total + 16));
  if (!pieces.empty()) {
    DBuf d_heads, d_pieces;
    DALLOC(d_heads, heads.size() + 16);
    DALLOC(d_pieces, pieces.size() * sizeof(Piece));
    for (size_t i : head_piece) pieces[i].src += (uint64_t)(uintptr_t)d_heads.p;
    HIPCHK(hipMemcpyAsync(d_heads.p, heads.data(), heads.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_pieces.p, pieces.data(), pieces.size() * sizeof(Piece), hipMemcpyHostToDevice, st));
    HIPCHK(T.begin(5));
    hipLaunchKernelGGL(k_assemble, dim3((unsigned)pieces.size()), dim3(256), 0, st, d_pieces.as<Piece>(), out->as<uint8_t>());
    HIPCHK(T.end());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));   // heads and pieces are read until here
  }
  HIPCHK(hipStreamSynchronize(st));
  if (int r = T.collect(I.ms_pass, &I.ms_device)) return r;
  I.chunks += C;
  I.runs += R;
  I.events += E;
  I.chunks_raw += raw;
  keep(out.release(), total);
  return 0;
}

// The batch: S segments of at most 1 GiB (from_host checks it, the block-sort stage holds nothing longer) at the device
// addresses src, offsets off.
int code_batch(spring_qlfc_ctx *ctx, const std::vector<uint64_t> &off, const std::vector<uint64_t> &src, spring_qlfc_info *info_out) {
  const int dev = ctx->dev;
  hipStream_t st = ctx->st;
  const uint64_t S = src.size();
  spring_qlfc_info &I = ctx->info;
  memset(&I, 0, sizeof(I));
  I.num_segments = S;
  I.bytes_in = off[S];
  if (S >= 0x7fffffffull) return fail(SPRING_REORDER_E_ARG, "too many segments");
  DBuf d_off, d_src;
  DALLOC(d_off, (S + 1) * 8);
  DALLOC(d_src, S * 8);
  uint64_t budget = 0;
  if (int r = workspace_budget(ctx->workspace_bytes, 0, &budget)) return r;
  I.workspace_bytes = budget;
  SyncOnExit sync_on_exit{st};
  HIPCHK(hipMemcpyAsync(d_off.p, off.data(), (S + 1) * 8, hipMemcpyHostToDevice, st));
  if (S) HIPCHK(hipMemcpyAsync(d_src.p, src.data(), S * 8, hipMemcpyHostToDevice, st));
  ctx->coded_off.assign(1, 0);
  ctx->in_off = off;
  for (uint64_t first = 0; first < S;) {
    uint64_t count = qlfc::take_segments(off.data(), S, first, budget);
    if (count == 0)
      return fail(SPRING_REORDER_E_ARG, "segment %llu of %llu bytes needs %llu bytes of workspace, the budget is %llu",
                  (unsigned long long)first, (unsigned long long)(off[first + 1] - off[first]),
                  (unsigned long long)qlfc::workspace_need(off[first + 1] - off[first], 1), (unsigned long long)budget);
    for (;;) {   // a sub-batch whose events do not fit is halved: at most log2(count) times
      bool fit = true;
      uint64_t need = 0;
      const int r = code_sub(ctx, off.data(), d_src.as<uint64_t>(), d_off.as<uint64_t>(), src.data(), first, count, budget, &fit, &need);
      if (r) return r;
      if (fit) break;
      if (count == 1)
        return fail(SPRING_REORDER_E_ARG, "segment %llu of %llu bytes needs %llu bytes of workspace with its events, the budget is %llu",
                    (unsigned long long)first, (unsigned long long)(off[first + 1] - off[first]), (unsigned long long)need,
                    (unsigned long long)budget);
      count = (count + 1) / 2;
    }
    first += count;
  }
  ctx->have = true;
  if (info_out) *info_out = I;
  return 0;
}

int begin(spring_qlfc_ctx *ctx) {
  (void)hipSetDevice(ctx->dev);
  drop_result(ctx);
  if (!ctx->have_tables) return fail(SPRING_REORDER_E_STATE, "spring_qlfc_set_state_tables has not been called");
  return 0;
}

int finish(spring_qlfc_ctx *ctx, int r) {
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  if (r) drop_result(ctx);
  return r;
}

}  // namespace

extern "C" {

int spring_qlfc_create(int device, spring_qlfc_ctx **out) {
  if (!out) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  const int r = stage_device(&device, "the QLFC stage");
  if (r) return r;
  spring_qlfc_ctx *c = new spring_qlfc_ctx();
  c->dev = device;
  memset(&c->info, 0, sizeof(c->info));
  *out = c;
  return 0;
}

void spring_qlfc_destroy(spring_qlfc_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->dev);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  drop_result(ctx);
  ctx->rank_tab.release();
  ctx->run_tab.release();
  if (ctx->st) (void)hipStreamDestroy(ctx->st);
  delete ctx;
}

int spring_qlfc_set_state_tables(spring_qlfc_ctx *ctx, const uint8_t *rank_table, const uint8_t *run_table) {
  if (!ctx || !rank_table || !run_table) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  int r = stream_begin(ctx->dev, &ctx->st);
  if (r) return r;
  const int dev = ctx->dev;
  ctx->have_tables = false;
  DALLOC(ctx->rank_tab, SPRING_QLFC_RANK_TABLE);
  DALLOC(ctx->run_tab, SPRING_QLFC_RUN_TABLE);
  HIPCHK(hipMemcpyAsync(ctx->rank_tab.p, rank_table, SPRING_QLFC_RANK_TABLE, hipMemcpyHostToDevice, ctx->st));
  HIPCHK(hipMemcpyAsync(ctx->run_tab.p, run_table, SPRING_QLFC_RUN_TABLE, hipMemcpyHostToDevice, ctx->st));
  HIPCHK(hipStreamSynchronize(ctx->st));
  ctx->have_tables = true;
  return 0;
}

int spring_qlfc_set_workspace_bytes(spring_qlfc_ctx *ctx, uint64_t workspace_bytes) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  ctx->workspace_bytes = workspace_bytes;
  return 0;
}

uint64_t spring_qlfc_workspace_need(uint64_t bytes, uint64_t segments) { return qlfc::workspace_need(bytes, segments); }

int spring_qlfc_from_host(spring_qlfc_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const uint64_t *seg_off,
                          uint64_t num_segments, spring_qlfc_info *info) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  int r = begin(ctx);
  if (r) return r;
  if (nbytes && !bytes) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  const uint64_t one[2] = {0, nbytes};
  if (!seg_off) { seg_off = one; num_segments = 1; }
  if (num_segments >= 0x7fffffffull) return fail(SPRING_REORDER_E_ARG, "too many segments");
  if (seg_off[0] != 0 || seg_off[num_segments] != nbytes)
    return fail(SPRING_REORDER_E_ARG, "the segment offsets do not start at 0 and end at the %llu bytes", (unsigned long long)nbytes);
  for (uint64_t s = 0; s < num_segments; s++)
    if (seg_off[s + 1] < seg_off[s]) return fail(SPRING_REORDER_E_ARG, "the segment offsets decrease");
  for (uint64_t s = 0; s < num_segments; s++)   // before anything is uploaded
    if (seg_off[s + 1] - seg_off[s] > qlfc::MAX_SEGMENT)
      return fail(SPRING_REORDER_E_ARG, "a segment of %llu bytes: more than 1 GiB", (unsigned long long)(seg_off[s + 1] - seg_off[s]));
  if ((r = stream_begin(ctx->dev, &ctx->st))) return r;
  const int dev = ctx->dev;
  DBuf up;
  DALLOC(up, nbytes + 32);
  if (nbytes) HIPCHK(hipMemcpyAsync(up.p, bytes, nbytes, hipMemcpyHostToDevice, ctx->st));
  std::vector<uint64_t> off(seg_off, seg_off + num_segments + 1), src(num_segments);
  for (uint64_t s = 0; s < num_segments; s++) src[s] = reinterpret_cast<uint64_t>(up.as<uint8_t>() + seg_off[s]);
  return finish(ctx, code_batch(ctx, off, src, info));
}

int spring_qlfc_from_bwt(spring_qlfc_ctx *ctx, spring_bwt_ctx *bwt, spring_qlfc_info *info) {
  if (!ctx || !bwt) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  int r = begin(ctx);
  if (r) return r;
  sr::BwtView V;
  if ((r = sr::bwt_view(bwt, &V))) return r;
  if (V.dev != ctx->dev) return fail(SPRING_REORDER_E_ARG, "block-sort and QLFC contexts live on different devices");
  if ((r = stream_begin(ctx->dev, &ctx->st))) return r;
  std::vector<uint64_t> off(V.off, V.off + V.num_segments + 1), src(V.num_segments);
  for (uint64_t s = 0; s < V.num_segments; s++) src[s] = reinterpret_cast<uint64_t>(V.bwt + V.off[s]);
  return finish(ctx, code_batch(ctx, off, src, info));
}

int spring_qlfc_get_info(spring_qlfc_ctx *ctx, spring_qlfc_info *info) {
  if (!ctx || !info) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing coded yet");
  *info = ctx->info;
  return 0;
}

int spring_qlfc_download(spring_qlfc_ctx *ctx, uint8_t *coded, uint64_t *coded_off, int32_t *status) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing coded yet");
  HIPCHK(hipSetDevice(ctx->dev));
  const uint64_t S = ctx->info.num_segments;
  if (coded_off) memcpy(coded_off, ctx->coded_off.data(), (S + 1) * 8);
  if (status && S) memcpy(status, ctx->status.data(), S * 4);
  uint64_t at = 0;
  for (size_t b = 0; coded && b < ctx->out.size(); b++) {
    if (ctx->out_bytes[b]) HIPCHK(rd(ctx->st, coded + at, ctx->out[b]->p, ctx->out_bytes[b]));
    at += ctx->out_bytes[b];
  }
  return 0;
}

int spring_qlfc_compress(spring_qlfc_ctx *ctx, const uint8_t *in, uint8_t *out, int32_t n) {
  if (!ctx || n < 0 || (n && (!in || !out))) return fail(SPRING_REORDER_E_ARG, "bad argument");
  const int r = spring_qlfc_from_host(ctx, in, (uint64_t)n, nullptr, 0, nullptr);
  if (r) return r;
  if (ctx->status[0] != 0) return SPRING_QLFC_NOT_COMPRESSIBLE;
  if (ctx->info.bytes_out > (uint64_t)n) return fail(SPRING_REORDER_E_STATE, "%llu coded bytes for %d", (unsigned long long)ctx->info.bytes_out, n);
  const int r2 = spring_qlfc_download(ctx, out, nullptr, nullptr);
  return r2 ? r2 : (int)ctx->info.bytes_out;
}

}  // extern "C"

namespace sr {
int qlfc_view(spring_qlfc_ctx *ctx, QlfcView *v) {
  if (!ctx || !v) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing coded yet");
  const uint64_t S = ctx->info.num_segments;
  if (!ctx->have_view) {
    const int r = stream_begin(ctx->dev, &ctx->st);
    if (r) return r;
    const int dev = ctx->dev;
    std::vector<uint64_t> src(S + 1, 0);
    uint64_t start = 0;   // the coded bytes in front of sub-batch b
    for (uint64_t s = 0, b = 0; s < S; s++) {
      while (b + 1 < ctx->out.size() && ctx->coded_off[s] >= start + ctx->out_bytes[b]) start += ctx->out_bytes[b++];
      if (!ctx->out.empty()) src[s] = reinterpret_cast<uint64_t>(ctx->out[b]->as<uint8_t>()) + (ctx->coded_off[s] - start);
    }
    DALLOC(ctx->v_src, (S + 1) * 8);
    DALLOC(ctx->v_off, (S + 1) * 8);
    DALLOC(ctx->v_status, S * 4);
    HIPCHK(hipMemcpyAsync(ctx->v_src.p, src.data(), (S + 1) * 8, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipMemcpyAsync(ctx->v_off.p, ctx->coded_off.data(), (S + 1) * 8, hipMemcpyHostToDevice, ctx->st));
    if (S) HIPCHK(hipMemcpyAsync(ctx->v_status.p, ctx->status.data(), S * 4, hipMemcpyHostToDevice, ctx->st));
    HIPCHK(hipStreamSynchronize(ctx->st));   // src is the host's until here
    ctx->have_view = true;
  }
  *v = QlfcView{ctx->dev, S, ctx->info.bytes_out, ctx->coded_off.data(), ctx->status.data(), ctx->v_src.as<uint64_t>(),
                ctx->v_off.as<uint64_t>(), ctx->v_status.as<int32_t>(), ctx->in_off.data()};
  return 0;
}
int qlfc_device(spring_qlfc_ctx *ctx, bool *have_tables) {
  if (have_tables) *have_tables = ctx->have_tables;
  return ctx->dev;
}
}  // namespace sr
