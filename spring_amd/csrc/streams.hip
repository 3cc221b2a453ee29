// spring_amd/csrc/streams.hip -- the per-block read streams on the GPU (include/spring_streams.h).
//
// What reorder_compress_streams (reference src/reorder_compress_streams.cpp:31-441) writes before its BSC calls,
// re-designed as data-parallel passes over HBM-resident arrays:
//   index      noise line ends: flag + scan + compaction over read_noise.txt; unaligned record offsets: scan of
//              2 + (len + 1) / 2 over the unaligned reads' lengths, each record header checked against it
//   scatter    record k -> slot order[k] (paired_end || preserve_order) or k, as SoA arrays (length, aligned,
//              orientation, position or record offset, noise count); a hit count per slot refuses a non-permutation
//   prev       prevpos of a unit = position of the last aligned read 1 before it in its block: one max-scan of
//              "unit index + 1 if read 1 is aligned" over all units, cut at the block start
//   size       one thread per unit: the bytes it adds to each variable-size stream (:245-360), flag histogram
//   scan       one exclusive scan per stream -> every unit's write offset; the offsets at multiples of
//              num_reads_per_block are the block table (all blocks of a stream lie back to back in one buffer)
//   write      fixed-width fields one thread per unit; noise lines, noise positions and unaligned reads in record
//              order with a lane group per read, so a wave reads and writes contiguous runs
// Only the scatter and the record -> unit offset lookups are random accesses.  No CPU fallback.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "encoder_internal.h"
#include "reorder_device.h"
#include "reorder_internal.h"
#include "spring_streams.h"
#include "stage_host.h"
#include "streams_internal.h"

using namespace sr;

namespace {

// variable-size streams: per-unit size array + scan each
constexpr int NV = 7;
enum { V_POS, V_NOISE, V_NP, V_REV, V_UN, V_PP, V_RP };
__host__ __device__ inline int var_stream(int v) {
  switch (v) {
    case V_POS: return SPRING_STREAMS_POS;
    case V_NOISE: return SPRING_STREAMS_NOISE;
    case V_NP: return SPRING_STREAMS_NOISEPOS;
    case V_REV: return SPRING_STREAMS_REV;
    case V_UN: return SPRING_STREAMS_UNALIGNED;
    case V_PP: return SPRING_STREAMS_POS_PAIR;
    default: return SPRING_STREAMS_REV_PAIR;
  }
}

// error bits of the device checks
constexpr uint32_t ERR_PERM = 1, ERR_UNREC = 2, ERR_CODE = 4;

// ------------------------------------------------------------------ index
__global__ void k_nl_flag(const char *__restrict__ noise, uint64_t nb, uint32_t *__restrict__ f) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= nb) f[i] = (i < nb && noise[i] == '\n') ? 1u : 0u;
}
__global__ void k_nl_pos(const char *__restrict__ noise, uint64_t nb, const uint32_t *__restrict__ idx, uint64_t na,
                         uint64_t *__restrict__ nl_end) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb && noise[i] == '\n' && idx[i] < na) nl_end[idx[i]] = i;
}
__global__ void k_un_size(const uint16_t *__restrict__ ulen, uint64_t nu, uint32_t *__restrict__ sz) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j <= nu) sz[j] = j < nu ? 2u + (ulen[j] + 1u) / 2u : 0u;
}
// the u16 header of every write_dnaN_in_bits record equals its read_lengths.bin entry (roff[nu] == bytes is checked
// on the host first, so every record lies inside the image)
__global__ void k_un_check(const uint8_t *__restrict__ un, const uint64_t *__restrict__ roff,
                           const uint16_t *__restrict__ ulen, uint64_t nu, uint32_t *__restrict__ err) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nu) return;
  const uint8_t *p = un + roff[j];
  if ((uint32_t)(p[0] | (p[1] << 8)) != ulen[j]) atomicOr(err, ERR_UNREC);
}

// ------------------------------------------------------------------ scatter (reorder_compress_streams.cpp:112-171)
struct Soa {
  uint16_t *len;
  uint8_t *al, *rc;
  uint64_t *pos;    // aligned: position; unaligned: byte offset of its record in read_unaligned.txt
  uint32_t *ncnt;   // noise characters of an aligned read
};
__global__ void k_scatter(uint64_t N, uint64_t na, const uint32_t *__restrict__ order, uint32_t *__restrict__ hits,
                          const uint64_t *__restrict__ pos, const char *__restrict__ rc, const uint16_t *__restrict__ rlen,
                          const uint64_t *__restrict__ nl_end, const uint64_t *__restrict__ roff, Soa S,
                          uint32_t *__restrict__ err) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= N) return;
  uint64_t s = k;
  if (order) {
    s = order[k];
    if (s >= N) { atomicOr(err, ERR_PERM); return; }
    if (atomicAdd(&hits[s], 1u) != 0u) { atomicOr(err, ERR_PERM); return; }  // N entries, none repeated: a permutation
  }
  S.len[s] = rlen[k];
  if (k < na) {
    const uint64_t start = k ? nl_end[k - 1] + 1 : 0;
    S.al[s] = 1;
    S.rc[s] = (uint8_t)rc[k];
    S.pos[s] = pos[k];
    S.ncnt[s] = (uint32_t)(nl_end[k] - start);
  } else {
    S.al[s] = 0;
    S.rc[s] = 0;
    S.pos[s] = roff[k - na];
    S.ncnt[s] = 0;
  }
}
__global__ void k_check_perm(const uint32_t *__restrict__ order, uint64_t N, uint32_t *__restrict__ hits,
                             uint32_t *__restrict__ err) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= N) return;
  const uint32_t s = order[k];
  if (s >= N || atomicAdd(&hits[s], 1u) != 0u) atomicOr(err, ERR_PERM);
}

// ------------------------------------------------------------------ per-unit decisions (:245-360)
struct Par {
  uint64_t N, U, B, half;
  bool pe, po;
};
__global__ void k_last_key(const uint8_t *__restrict__ al, uint64_t U, uint32_t *__restrict__ key) {
  const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u < U) key[u] = al[u] ? (uint32_t)(u + 1) : 0u;
}
// paired-end flag of a unit (:286-298); single-end: 0 aligned, 2 not
__device__ __forceinline__ int unit_flag(const Soa &S, const Par &P, uint64_t u) {
  const bool a1 = S.al[u];
  if (!P.pe) return a1 ? 0 : 2;
  const uint64_t v = P.half + u;
  const bool a2 = S.al[v];
  if (a1 && a2) {
    const int64_t d = (int64_t)S.pos[v] - (int64_t)S.pos[u];
    return (d < 32767 && d > -32767) ? 0 : 1;
  }
  if (!a1 && !a2) return 2;
  return a1 ? 3 : 4;
}
// bytes read 1 of unit u adds to read_pos.bin; *absolute / *escape say how
__device__ __forceinline__ uint32_t pos1_bytes(const Soa &S, const Par &P, const uint32_t *__restrict__ last, uint64_t u,
                                               uint64_t *prevpos, bool *absolute) {
  if (P.po) { *absolute = true; return 8; }
  const uint64_t b0 = u - u % P.B;
  if (u == b0) { *absolute = true; return 8; }
  const uint32_t p = last[u - 1];   // 1 + index of the last aligned read 1 in [0, u), 0 if none
  *prevpos = (p > b0) ? S.pos[p - 1] : 0ull;
  *absolute = false;
  return (S.pos[u] - *prevpos < 65535ull) ? 2u : 10u;
}
__global__ __launch_bounds__(256) void k_sizes(Soa S, Par P, const uint32_t *__restrict__ last, uint32_t *__restrict__ sz,
                                               unsigned long long *__restrict__ stats /* flag[5], escapes */) {
  __shared__ unsigned int cnt[6];
  if (threadIdx.x < 6) cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t U1 = P.U + 1;
  if (u < P.U) {
    const int f = unit_flag(S, P, u);
    uint32_t s_pos = 0, s_noise = 0, s_np = 0, s_rev = 0, s_un = 0, s_pp = 0, s_rp = 0;
    if (f == 0 || f == 1 || f == 3) {  // read 1 aligned
      uint64_t prev = 0;
      bool ab = false;
      s_pos += pos1_bytes(S, P, last, u, &prev, &ab);
      if (s_pos == 10) atomicAdd(&cnt[5], 1u);
      s_noise += S.ncnt[u] + 1;
      s_np += 2 * S.ncnt[u];
      s_rev += 1;
    } else {
      s_un += S.len[u];
    }
    if (P.pe) {
      const uint64_t v = P.half + u;
      if (f == 0) { s_pp += 2; s_rp += 1; }
      if (f == 0 || f == 1 || f == 4) {
        s_noise += S.ncnt[v] + 1;
        s_np += 2 * S.ncnt[v];
        if (f != 0) { s_pos += 8; s_rev += 1; }
      } else {
        s_un += S.len[v];
      }
    }
    sz[V_POS * U1 + u] = s_pos; sz[V_NOISE * U1 + u] = s_noise; sz[V_NP * U1 + u] = s_np; sz[V_REV * U1 + u] = s_rev;
    sz[V_UN * U1 + u] = s_un;
    if (P.pe) { sz[V_PP * U1 + u] = s_pp; sz[V_RP * U1 + u] = s_rp; }
    atomicAdd(&cnt[f], 1u);
  } else if (u == P.U) {
    for (int v = 0; v < NV; v++) sz[v * U1 + u] = 0;
  }
  __syncthreads();
  if (threadIdx.x < 6 && cnt[threadIdx.x]) atomicAdd(&stats[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

// block table: tab[s * (nb + 1) + b] = offset of unit min(b * B, U) in stream s
__global__ void k_table(const uint64_t *__restrict__ off, Par P, uint64_t nb, uint64_t *__restrict__ tab) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)SPRING_STREAMS_NUM * (nb + 1)) return;
  const int s = (int)(i / (nb + 1));
  const uint64_t b = i % (nb + 1);
  const uint64_t u = b * P.B < P.U ? b * P.B : P.U;
  uint64_t o = 0;
  if (s == SPRING_STREAMS_FLAG) o = u;
  else if (s == SPRING_STREAMS_LENGTHS) o = u * (P.pe ? 4 : 2);
  else {
    for (int v = 0; v < NV; v++)
      if (var_stream(v) == s) o = (P.pe || v < V_PP) ? off[v * (P.U + 1) + u] : 0;
  }
  tab[i] = o;
}

// ------------------------------------------------------------------ write
struct Out {
  uint8_t *p[SPRING_STREAMS_NUM];
};
__device__ __forceinline__ void st_u64(uint8_t *p, uint64_t v) {  // read_pos.bin entries sit at any even offset
  for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i));
}
__device__ __forceinline__ void st_u16(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)v;
  p[1] = (uint8_t)(v >> 8);
}
// flag, lengths, positions, orientations, pair fields: one thread per unit
__global__ __launch_bounds__(256) void k_write_fixed(Soa S, Par P, const uint32_t *__restrict__ last,
                                                     const uint64_t *__restrict__ off, Out O) {
  const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= P.U) return;
  const uint64_t U1 = P.U + 1;
  const int f = unit_flag(S, P, u);
  O.p[SPRING_STREAMS_FLAG][u] = (uint8_t)('0' + f);
  uint64_t opos = off[V_POS * U1 + u], orev = off[V_REV * U1 + u];
  const uint64_t v = P.half + u;
  if (P.pe) {
    st_u16(O.p[SPRING_STREAMS_LENGTHS] + 4 * u, S.len[u]);
    st_u16(O.p[SPRING_STREAMS_LENGTHS] + 4 * u + 2, S.len[v]);
    if (f == 0) {
      st_u16(O.p[SPRING_STREAMS_POS_PAIR] + off[V_PP * U1 + u], (uint32_t)(uint16_t)(int16_t)((int64_t)S.pos[v] - (int64_t)S.pos[u]));
      O.p[SPRING_STREAMS_REV_PAIR][off[V_RP * U1 + u]] = S.rc[u] != S.rc[v] ? '0' : '1';
    }
  } else {
    st_u16(O.p[SPRING_STREAMS_LENGTHS] + 2 * u, S.len[u]);
  }
  if (f == 0 || f == 1 || f == 3) {
    uint64_t prev = 0;
    bool ab = false;
    const uint32_t nbytes = pos1_bytes(S, P, last, u, &prev, &ab);
    uint8_t *q = O.p[SPRING_STREAMS_POS] + opos;
    if (ab) st_u64(q, S.pos[u]);
    else if (nbytes == 2) st_u16(q, (uint32_t)(S.pos[u] - prev));
    else { st_u16(q, 65535u); st_u64(q + 2, S.pos[u]); }
    opos += nbytes;
    O.p[SPRING_STREAMS_REV][orev++] = S.rc[u];
  }
  if (P.pe && (f == 1 || f == 4)) {
    st_u64(O.p[SPRING_STREAMS_POS] + opos, S.pos[v]);
    O.p[SPRING_STREAMS_REV][orev] = S.rc[v];
  }
}

// unit of the read in slot s and whether it is read 2
__device__ __forceinline__ uint64_t unit_of(const Par &P, uint64_t s, bool *second) {
  *second = P.pe && s >= P.half;
  return *second ? s - P.half : s;
}

// noise line (+ '\n') and noise positions of aligned record k: G lanes per record
template <int G>
__global__ __launch_bounds__(256) void k_write_noise(Par P, uint64_t na, const uint32_t *__restrict__ order, Soa S,
                                                     const char *__restrict__ noise, const uint16_t *__restrict__ noisepos,
                                                     const uint64_t *__restrict__ nl_end, const uint64_t *__restrict__ off,
                                                     Out O) {
  const uint64_t k = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  const int lane = threadIdx.x % G;
  if (k >= na) return;
  bool second;
  const uint64_t u = unit_of(P, order ? order[k] : k, &second);
  const uint64_t U1 = P.U + 1;
  uint64_t on = off[V_NOISE * U1 + u], onp = off[V_NP * U1 + u];
  if (second && S.al[u]) { on += S.ncnt[u] + 1; onp += 2 * (uint64_t)S.ncnt[u]; }
  const uint64_t start = k ? nl_end[k - 1] + 1 : 0, cnt = nl_end[k] - start;
  uint8_t *dn = O.p[SPRING_STREAMS_NOISE] + on;
  for (uint64_t j = lane; j <= cnt; j += G) dn[j] = (uint8_t)noise[start + j];   // the line's own '\n' included
  uint16_t *dp = (uint16_t *)(O.p[SPRING_STREAMS_NOISEPOS] + onp);              // every entry is 2 bytes: aligned
  const uint16_t *sp = noisepos + (start - k);
  for (uint64_t j = lane; j < cnt; j += G) dp[j] = sp[j];
}

// unaligned record j = k - na: its bases as characters (read_dnaN_from_bits, util.cpp:350-374), G lanes per record
template <int G>
__global__ __launch_bounds__(256) void k_write_unaligned(Par P, uint64_t na, const uint32_t *__restrict__ order, Soa S,
                                                         const uint8_t *__restrict__ un, const uint64_t *__restrict__ roff,
                                                         const uint64_t *__restrict__ off, Out O, uint32_t *__restrict__ err) {
  const uint64_t j = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  const int lane = threadIdx.x % G;
  if (j >= P.N - na) return;
  const uint64_t k = na + j;
  bool second;
  const uint64_t u = unit_of(P, order ? order[k] : k, &second);
  uint64_t o = off[V_UN * (P.U + 1) + u];
  if (second && !S.al[u]) o += S.len[u];
  const uint8_t *rec = un + roff[j];
  const uint32_t len = rec[0] | (rec[1] << 8);
  uint8_t *d = O.p[SPRING_STREAMS_UNALIGNED] + o;
  bool bad = false;
  for (uint32_t c = lane; c < len; c += G) {
    const uint32_t code = (rec[2 + c / 2] >> (4 * (c & 1))) & 15u;
    bad |= code > 4;
    d[c] = (uint8_t)("AGCTN"[code > 4 ? 4 : code]);
  }
  if (bad) atomicOr(err, ERR_CODE);
}

// ------------------------------------------------------------------ host side
struct In {   // device arrays
  const uint64_t *pos;
  const char *rc, *noise;
  const uint16_t *noisepos, *rlen;
  const uint32_t *order;   // null: record k -> slot k
  const uint8_t *un;
  uint64_t na, noise_bytes, n_noisepos, un_bytes;
};

}  // namespace

struct spring_streams_ctx {
  int dev = 0;
  hipStream_t st = nullptr;
  bool have = false;
  spring_streams_info info;
  DBuf out[SPRING_STREAMS_NUM];
  std::vector<uint64_t> table;   // SPRING_STREAMS_NUM x (num_blocks + 1)
  uint32_t num_reads = 0, num_reads_per_block = 0;   // parameters of the last run (streams_view)
  bool pe = false, po = false;
};

namespace {

int check_params(uint64_t n_total, uint32_t N, int pe, uint32_t B) {
  if (n_total != N) return fail(SPRING_REORDER_E_ARG, "the encoder holds %llu reads, num_reads is %u",
                                (unsigned long long)n_total, N);
  if (pe && (N & 1)) return fail(SPRING_REORDER_E_ARG, "paired-end data needs an even num_reads (got %u)", N);
  if (B == 0) return fail(SPRING_REORDER_E_ARG, "num_reads_per_block must be > 0");
  return 0;
}

int run_core(spring_streams_ctx *ctx, const In &I, uint32_t N, bool pe, bool po, uint32_t B, spring_streams_info *info_out) {
  const int dev = ctx->dev;
  hipStream_t st = ctx->st;
  ctx->have = false;
  spring_streams_info &R = ctx->info;
  memset(&R, 0, sizeof(R));
  const uint64_t na = I.na, nu = (uint64_t)N - na;
  if (I.noise_bytes >= 0xFFFFFFF0ull) return fail(SPRING_REORDER_E_ARG, "read_noise.txt larger than 4 GB");
  if (na > N) return fail(SPRING_REORDER_E_ARG, "%llu aligned reads but num_reads is %u", (unsigned long long)na, N);
  if (I.noise_bytes < na || I.noise_bytes - na != I.n_noisepos)
    return fail(SPRING_REORDER_E_ARG, "read_noise.txt holds %llu bytes for %llu reads, read_noisepos.bin %llu entries",
                (unsigned long long)I.noise_bytes, (unsigned long long)na, (unsigned long long)I.n_noisepos);
  Par P;
  P.N = N; P.pe = pe; P.po = po; P.B = B; P.half = pe ? N / 2 : 0;
  P.U = pe ? N / 2 : N;
  const uint64_t U = P.U, U1 = U + 1, nb = (U + B - 1) / B;
  hipEvent_t ev[2];
  for (auto &e : ev) HIPCHK(hipEventCreate(&e));
  struct EvGuard { hipEvent_t *e; ~EvGuard() { (void)hipEventDestroy(e[0]); (void)hipEventDestroy(e[1]); } } evg{ev};
  HIPCHK(hipEventRecord(ev[0], st));

  DBuf d_err, flag, idx, nl_end, usz, roff, tmp, hits;
  DALLOC(d_err, 4);
  HIPCHK(hipMemsetAsync(d_err.p, 0, 4, st));
  uint32_t *err = d_err.as<uint32_t>();
  // ---- index: noise line ends
  DALLOC(flag, (I.noise_bytes + 1) * 4);
  DALLOC(idx, (I.noise_bytes + 1) * 4);
  DALLOC(nl_end, na * 8);
  size_t tb = 0, tb2 = 0;
  HIPCHK(sr::excl_scan_u32(st, nullptr, tb, flag.as<uint32_t>(), idx.as<uint32_t>(), I.noise_bytes + 1));
  HIPCHK(sr::excl_scan_u32_to_u64(st, nullptr, tb2, flag.as<uint32_t>(), roff.as<uint64_t>(), nu + 1));
  tb = std::max(tb, tb2);
  HIPCHK(sr::excl_scan_u32_to_u64(st, nullptr, tb2, flag.as<uint32_t>(), roff.as<uint64_t>(), U1));
  tb = std::max(tb, tb2);
  HIPCHK(rocprim::inclusive_scan(nullptr, tb2, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)(U ? U : 1),
                                 rocprim::maximum<uint32_t>(), st));
  tb = std::max(tb, tb2);
  DALLOC(tmp, tb);
  hipLaunchKernelGGL(k_nl_flag, grid(I.noise_bytes + 1), dim3(256), 0, st, I.noise, I.noise_bytes, flag.as<uint32_t>());
  HIPCHK(sr::excl_scan_u32(st, tmp.p, tb2 = tb, flag.as<uint32_t>(), idx.as<uint32_t>(), I.noise_bytes + 1));
  if (na) hipLaunchKernelGGL(k_nl_pos, grid(I.noise_bytes), dim3(256), 0, st, I.noise, I.noise_bytes, idx.as<uint32_t>(),
                             na, nl_end.as<uint64_t>());
  // ---- index: unaligned records
  DALLOC(usz, (nu + 1) * 4);
  DALLOC(roff, (nu + 1) * 8);
  hipLaunchKernelGGL(k_un_size, grid(nu + 1), dim3(256), 0, st, I.rlen + na, nu, usz.as<uint32_t>());
  HIPCHK(sr::excl_scan_u32_to_u64(st, tmp.p, tb2 = tb, usz.as<uint32_t>(), roff.as<uint64_t>(), nu + 1));
  uint32_t nlines = 0;
  uint64_t last_nl = 0, rec_total = 0;
  HIPCHK(rd(st, &nlines, idx.as<uint32_t>() + I.noise_bytes, 4));
  HIPCHK(rd(st, &rec_total, roff.as<uint64_t>() + nu, 8));
  if (nlines != na) return fail(SPRING_REORDER_E_ARG, "read_noise.txt holds %u lines for %llu aligned reads", nlines,
                                (unsigned long long)na);
  if (na) {
    HIPCHK(rd(st, &last_nl, nl_end.as<uint64_t>() + na - 1, 8));
    if (last_nl != I.noise_bytes - 1) return fail(SPRING_REORDER_E_ARG, "read_noise.txt does not end with a newline");
  }
  if (rec_total != I.un_bytes)
    return fail(SPRING_REORDER_E_ARG, "read_unaligned.txt holds %llu bytes, read_lengths.bin implies %llu",
                (unsigned long long)I.un_bytes, (unsigned long long)rec_total);
  flag.release();
  idx.release();
  if (nu) hipLaunchKernelGGL(k_un_check, grid(nu), dim3(256), 0, st, I.un, roff.as<uint64_t>(), I.rlen + na, nu, err);
  // ---- scatter to slots
  DBuf s_len, s_al, s_rc, s_pos, s_ncnt;
  DALLOC(s_len, (uint64_t)N * 2); DALLOC(s_al, N); DALLOC(s_rc, N); DALLOC(s_pos, (uint64_t)N * 8);
  DALLOC(s_ncnt, (uint64_t)N * 4);
  Soa S{s_len.as<uint16_t>(), s_al.as<uint8_t>(), s_rc.as<uint8_t>(), s_pos.as<uint64_t>(), s_ncnt.as<uint32_t>()};
  if (I.order) {
    DALLOC(hits, (uint64_t)N * 4);
    HIPCHK(hipMemsetAsync(hits.p, 0, (uint64_t)N * 4, st));
  }
  if (N) hipLaunchKernelGGL(k_scatter, grid(N), dim3(256), 0, st, (uint64_t)N, na, I.order, hits.as<uint32_t>(), I.pos,
                            I.rc, I.rlen, nl_end.as<uint64_t>(), roff.as<uint64_t>(), S, err);
  uint32_t herr = 0;
  HIPCHK(rd(st, &herr, err, 4));
  if (herr & ERR_PERM) return fail(SPRING_REORDER_E_ARG, "read_order.bin is not a permutation of [0, %u)", N);
  if (herr & ERR_UNREC) return fail(SPRING_REORDER_E_ARG, "a read_unaligned.txt record does not match read_lengths.bin");
  hits.release();
  usz.release();

  // ---- prev aligned read 1, sizes, scans
  DBuf key, last, sz, off, stats;
  DALLOC(key, U * 4); DALLOC(last, U * 4);
  DALLOC(sz, NV * U1 * 4); DALLOC(off, NV * U1 * 8); DALLOC(stats, 6 * 8);
  HIPCHK(hipMemsetAsync(stats.p, 0, 6 * 8, st));
  HIPCHK(hipMemsetAsync(sz.p, 0, NV * U1 * 4, st));
  if (!po && U) {
    hipLaunchKernelGGL(k_last_key, grid(U), dim3(256), 0, st, S.al, U, key.as<uint32_t>());
    HIPCHK(rocprim::inclusive_scan(tmp.p, tb2 = tb, key.as<uint32_t>(), last.as<uint32_t>(), (size_t)U,
                                   rocprim::maximum<uint32_t>(), st));
  }
  hipLaunchKernelGGL(k_sizes, grid(U1), dim3(256), 0, st, S, P, last.as<uint32_t>(), sz.as<uint32_t>(),
                     stats.as<unsigned long long>());
  const int nv = pe ? NV : V_PP;
  for (int v = 0; v < nv; v++)
    HIPCHK(sr::excl_scan_u32_to_u64(st, tmp.p, tb2 = tb, sz.as<uint32_t>() + v * U1, off.as<uint64_t>() + v * U1, U1));
  key.release();
  sz.release();
  std::vector<uint64_t> tot(NV, 0), st6(6);
  for (int v = 0; v < nv; v++) HIPCHK(rd(st, &tot[v], off.as<uint64_t>() + v * U1 + U, 8));
  HIPCHK(rd(st, st6.data(), stats.p, 6 * 8));
  // ---- outputs
  R.num_units = U;
  R.num_blocks = nb;
  R.n_aligned = na;
  R.bytes[SPRING_STREAMS_FLAG] = U;
  R.bytes[SPRING_STREAMS_LENGTHS] = U * (pe ? 4 : 2);
  for (int v = 0; v < nv; v++) R.bytes[var_stream(v)] = tot[v];
  for (int f = 0; f < 5; f++) R.flag_count[f] = st6[f];
  R.pos_escapes = st6[5];
  Out O;
  for (int s = 0; s < SPRING_STREAMS_NUM; s++) {
    DALLOC(ctx->out[s], R.bytes[s]);
    O.p[s] = ctx->out[s].as<uint8_t>();
  }
  DBuf tab;
  DALLOC(tab, SPRING_STREAMS_NUM * (nb + 1) * 8);
  hipLaunchKernelGGL(k_table, grid(SPRING_STREAMS_NUM * (nb + 1)), dim3(256), 0, st, off.as<uint64_t>(), P, nb,
                     tab.as<uint64_t>());
  if (U) hipLaunchKernelGGL(k_write_fixed, grid(U), dim3(256), 0, st, S, P, last.as<uint32_t>(), off.as<uint64_t>(), O);
  constexpr int GN = 8, GU = 32;
  if (na) hipLaunchKernelGGL(k_write_noise<GN>, grid(na * GN), dim3(256), 0, st, P, na, I.order, S, I.noise, I.noisepos,
                             nl_end.as<uint64_t>(), off.as<uint64_t>(), O);
  if (nu) hipLaunchKernelGGL(k_write_unaligned<GU>, grid(nu * GU), dim3(256), 0, st, P, na, I.order, S, I.un,
                             roff.as<uint64_t>(), off.as<uint64_t>(), O, err);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev[1], st));
  ctx->table.assign(SPRING_STREAMS_NUM * (nb + 1), 0);
  HIPCHK(rd(st, ctx->table.data(), tab.p, ctx->table.size() * 8));
  HIPCHK(rd(st, &herr, err, 4));
  if (herr & ERR_CODE) return fail(SPRING_REORDER_E_ARG, "read_unaligned.txt holds a base code other than A G C T N");
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
  R.ms_device = ms;
  ctx->num_reads = N;
  ctx->num_reads_per_block = B;
  ctx->pe = pe;
  ctx->po = po;
  ctx->have = true;
  if (info_out) *info_out = R;
  return 0;
}

}  // namespace

extern "C" {

int spring_streams_create(int device, spring_streams_ctx **out) {
  if (!out) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  const int r = stage_device(&device, "the streams stage");
  if (r) return r;
  spring_streams_ctx *c = new spring_streams_ctx();
  c->dev = device;
  memset(&c->info, 0, sizeof(c->info));
  *out = c;
  return 0;
}

void spring_streams_destroy(spring_streams_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->dev);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  for (auto &b : ctx->out) b.release();
  if (ctx->st) (void)hipStreamDestroy(ctx->st);
  delete ctx;
}

int spring_streams_from_encoder(spring_streams_ctx *ctx, spring_encoder_ctx *enc, uint32_t num_reads, int32_t paired_end,
                                int32_t preserve_order, uint32_t num_reads_per_block, int32_t apply_pe_encode,
                                spring_streams_info *info) {
  if (!ctx || !enc) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  sr::EncoderView V;
  int r = sr::encoder_view(enc, &V);
  if (r) return r;
  if (V.dev != ctx->dev) return fail(SPRING_REORDER_E_ARG, "encoder and streams contexts live on different devices");
  if ((r = check_params(V.info.n_total, num_reads, paired_end, num_reads_per_block))) return r;
  if (apply_pe_encode && (!paired_end || preserve_order))
    return fail(SPRING_REORDER_E_ARG, "apply_pe_encode is for paired-end data without preserve_order");
  if ((r = stream_begin(ctx->dev, &ctx->st))) return r;
  ctx->have = false;
  const int dev = ctx->dev;
  In I;
  I.pos = V.pos; I.rc = V.rc; I.noise = V.noise; I.noisepos = V.noisepos; I.rlen = V.rlen; I.un = V.unaligned;
  I.order = (paired_end || preserve_order) ? V.order : nullptr;
  I.na = V.info.n_aligned; I.noise_bytes = V.info.noise_bytes; I.n_noisepos = V.info.n_noisepos;
  I.un_bytes = V.info.unaligned_bytes;
  DBuf pe_order;
  if (apply_pe_encode && num_reads) {
    // pe_encode inverts the order: it must be a permutation before it runs
    DBuf hits, d_err;
    DALLOC(hits, (uint64_t)num_reads * 4); DALLOC(d_err, 4); DALLOC(pe_order, (uint64_t)num_reads * 4);
    HIPCHK(hipMemsetAsync(hits.p, 0, (uint64_t)num_reads * 4, ctx->st));
    HIPCHK(hipMemsetAsync(d_err.p, 0, 4, ctx->st));
    hipLaunchKernelGGL(k_check_perm, grid(num_reads), dim3(256), 0, ctx->st, V.order, (uint64_t)num_reads,
                       hits.as<uint32_t>(), d_err.as<uint32_t>());
    uint32_t herr = 0;
    HIPCHK(rd(ctx->st, &herr, d_err.p, 4));
    if (herr) return fail(SPRING_REORDER_E_ARG, "read_order.bin is not a permutation of [0, %u)", num_reads);
    if ((r = sr::pe_encode_device(ctx->st, V.order, num_reads, pe_order.as<uint32_t>()))) return r;
    I.order = pe_order.as<uint32_t>();
  }
  r = run_core(ctx, I, num_reads, paired_end != 0, preserve_order != 0, num_reads_per_block, info);
  (void)hipStreamSynchronize(ctx->st);
  return r;
}

int spring_streams_from_host(spring_streams_ctx *ctx, const uint64_t *pos, const char *rc, uint64_t n_aligned,
                             const char *noise, uint64_t noise_bytes, const uint16_t *noisepos, uint64_t n_noisepos,
                             const uint32_t *order, const uint16_t *rlen, uint64_t n_total, const uint8_t *unaligned,
                             uint64_t unaligned_bytes, uint32_t num_reads, int32_t paired_end, int32_t preserve_order,
                             uint32_t num_reads_per_block, spring_streams_info *info) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  int r = check_params(n_total, num_reads, paired_end, num_reads_per_block);
  if (r) return r;
  const bool use_order = paired_end || preserve_order;
  if ((n_aligned && (!pos || !rc)) || (noise_bytes && !noise) || (n_noisepos && !noisepos) || (n_total && !rlen) ||
      (unaligned_bytes && !unaligned) || (use_order && n_total && !order))
    return fail(SPRING_REORDER_E_ARG, "NULL stream");
  if ((r = stream_begin(ctx->dev, &ctx->st))) return r;
  ctx->have = false;
  const int dev = ctx->dev;
  hipStream_t st = ctx->st;
  DBuf d_pos, d_rc, d_noise, d_np, d_order, d_rlen, d_un;
  DALLOC(d_pos, n_aligned * 8); DALLOC(d_rc, n_aligned); DALLOC(d_noise, noise_bytes); DALLOC(d_np, n_noisepos * 2);
  DALLOC(d_rlen, n_total * 2); DALLOC(d_un, unaligned_bytes);
  if (use_order) DALLOC(d_order, n_total * 4);
  if (n_aligned) {
    HIPCHK(hipMemcpyAsync(d_pos.p, pos, n_aligned * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_rc.p, rc, n_aligned, hipMemcpyHostToDevice, st));
  }
  if (noise_bytes) HIPCHK(hipMemcpyAsync(d_noise.p, noise, noise_bytes, hipMemcpyHostToDevice, st));
  if (n_noisepos) HIPCHK(hipMemcpyAsync(d_np.p, noisepos, n_noisepos * 2, hipMemcpyHostToDevice, st));
  if (n_total) HIPCHK(hipMemcpyAsync(d_rlen.p, rlen, n_total * 2, hipMemcpyHostToDevice, st));
  if (unaligned_bytes) HIPCHK(hipMemcpyAsync(d_un.p, unaligned, unaligned_bytes, hipMemcpyHostToDevice, st));
  if (use_order && n_total) HIPCHK(hipMemcpyAsync(d_order.p, order, n_total * 4, hipMemcpyHostToDevice, st));
  In I;
  I.pos = d_pos.as<uint64_t>(); I.rc = d_rc.as<char>(); I.noise = d_noise.as<char>(); I.noisepos = d_np.as<uint16_t>();
  I.rlen = d_rlen.as<uint16_t>(); I.un = d_un.as<uint8_t>(); I.order = use_order ? d_order.as<uint32_t>() : nullptr;
  I.na = n_aligned; I.noise_bytes = noise_bytes; I.n_noisepos = n_noisepos; I.un_bytes = unaligned_bytes;
  r = run_core(ctx, I, num_reads, paired_end != 0, preserve_order != 0, num_reads_per_block, info);
  (void)hipStreamSynchronize(st);
  return r;
}

int spring_streams_get_info(spring_streams_ctx *ctx, spring_streams_info *info) {
  if (!ctx || !info) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "no streams computed yet");
  *info = ctx->info;
  return 0;
}

int spring_streams_download(spring_streams_ctx *ctx, int32_t stream_id, uint8_t *bytes, uint64_t *block_off) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "no streams computed yet");
  if (stream_id < 0 || stream_id >= SPRING_STREAMS_NUM) return fail(SPRING_REORDER_E_ARG, "bad stream id %d", stream_id);
  HIPCHK(hipSetDevice(ctx->dev));
  const uint64_t nb1 = ctx->info.num_blocks + 1;
  if (block_off) memcpy(block_off, ctx->table.data() + stream_id * nb1, nb1 * 8);
  if (bytes && ctx->info.bytes[stream_id])
    HIPCHK(rd(ctx->st, bytes, ctx->out[stream_id].p, ctx->info.bytes[stream_id]));
  return 0;
}

}  // extern "C"

namespace sr {
int streams_view(spring_streams_ctx *ctx, StreamsView *v) {
  if (!ctx || !v) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "no streams computed yet");
  v->dev = ctx->dev;
  v->info = ctx->info;
  for (int s = 0; s < SPRING_STREAMS_NUM; s++) v->bytes[s] = ctx->out[s].as<uint8_t>();
  v->table = ctx->table.data();
  v->num_reads = ctx->num_reads;
  v->num_reads_per_block = ctx->num_reads_per_block;
  v->paired_end = ctx->pe;
  v->preserve_order = ctx->po;
  return 0;
}
}  // namespace sr

// ------------------------------------------------------------------ file contract
namespace {

const char *const FILE_NAME[SPRING_STREAMS_NUM] = {"read_flag.txt", "read_pos.bin", "read_noise.txt", "read_noisepos.bin",
                                                   "read_rev.txt", "read_unaligned.txt", "read_lengths.bin",
                                                   "read_pos_pair.bin", "read_rev_pair.txt"};

int slurp(const std::string &path, std::vector<uint8_t> &buf) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return fail(SPRING_REORDER_E_IO, "cannot open %s", path.c_str());
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  if (n < 0) { fclose(f); return fail(SPRING_REORDER_E_IO, "cannot size %s", path.c_str()); }
  buf.resize((size_t)n);
  const size_t got = n ? fread(buf.data(), 1, (size_t)n, f) : 0;
  fclose(f);
  if (got != (size_t)n) return fail(SPRING_REORDER_E_IO, "short read of %s", path.c_str());
  return 0;
}

int spill(const std::string &path, const uint8_t *p, size_t n) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) return fail(SPRING_REORDER_E_IO, "cannot create %s", path.c_str());
  const size_t put = n ? fwrite(p, 1, n, f) : 0;
  const int c = fclose(f);
  if (put != n || c != 0) return fail(SPRING_REORDER_E_IO, "short write of %s", path.c_str());
  return 0;
}

struct CtxGuard {
  spring_streams_ctx *c = nullptr;
  ~CtxGuard() { spring_streams_destroy(c); }
};

}  // namespace

extern "C" int spring_streams_run(const char *temp_dir, uint32_t num_reads, int32_t paired_end, int32_t preserve_order,
                                  uint32_t num_reads_per_block, int32_t device, spring_streams_info *info_out) {
  const auto t0 = std::chrono::steady_clock::now();
  if (!temp_dir) return fail(SPRING_REORDER_E_ARG, "temp_dir is NULL");
  const std::string base(temp_dir);
  const bool use_order = paired_end || preserve_order;
  const std::string f_pos = base + "/read_pos.bin", f_noise = base + "/read_noise.txt",
                    f_np = base + "/read_noisepos.bin", f_rc = base + "/read_rev.txt", f_order = base + "/read_order.bin",
                    f_len = base + "/read_lengths.bin", f_un = base + "/read_unaligned.txt",
                    f_cnt = base + "/read_unaligned.txt.count";
  std::vector<uint8_t> pos, noise, np, rc, order, len, un, cnt;
  int r;
  if ((r = slurp(f_pos, pos)) || (r = slurp(f_noise, noise)) || (r = slurp(f_np, np)) || (r = slurp(f_rc, rc)) ||
      (r = slurp(f_len, len)) || (r = slurp(f_un, un)) || (r = slurp(f_cnt, cnt)))
    return r;
  if (use_order && (r = slurp(f_order, order))) return r;
  const uint64_t na = rc.size(), n_total = len.size() / 2;
  if (pos.size() != na * 8) return fail(SPRING_REORDER_E_ARG, "read_pos.bin holds %zu bytes for %llu aligned reads",
                                        pos.size(), (unsigned long long)na);
  if (len.size() % 2 || np.size() % 2) return fail(SPRING_REORDER_E_ARG, "odd size of a u16 stream");
  if (use_order && order.size() != n_total * 4)
    return fail(SPRING_REORDER_E_ARG, "read_order.bin holds %zu bytes for %llu reads", order.size(),
                (unsigned long long)n_total);
  if (cnt.size() != 8) return fail(SPRING_REORDER_E_ARG, "read_unaligned.txt.count is not one u64");
  uint64_t un_chars = 0, want_chars = 0;
  memcpy(&un_chars, cnt.data(), 8);
  const uint16_t *rl = (const uint16_t *)len.data();
  for (uint64_t k = na; k < n_total; k++) want_chars += rl[k];
  if (un_chars != want_chars)
    return fail(SPRING_REORDER_E_ARG, "read_unaligned.txt.count says %llu bases, read_lengths.bin %llu",
                (unsigned long long)un_chars, (unsigned long long)want_chars);
  CtxGuard g;
  if ((r = spring_streams_create(device, &g.c))) return r;
  spring_streams_info I;
  if ((r = spring_streams_from_host(g.c, (const uint64_t *)pos.data(), (const char *)rc.data(), na,
                                    (const char *)noise.data(), noise.size(), (const uint16_t *)np.data(), np.size() / 2,
                                    use_order ? (const uint32_t *)order.data() : nullptr, rl, n_total, un.data(),
                                    un.size(), num_reads, paired_end, preserve_order, num_reads_per_block, &I)))
    return r;
  std::vector<uint8_t>().swap(pos);
  std::vector<uint8_t>().swap(noise);
  std::vector<uint8_t>().swap(np);
  std::vector<uint8_t>().swap(un);
  // every check has passed: write <stream>.<b>, blocks split over a few threads
  const int ns = paired_end ? SPRING_STREAMS_NUM : SPRING_STREAMS_POS_PAIR;
  const uint64_t nb = I.num_blocks;
  std::vector<std::vector<uint8_t>> data(ns);
  std::vector<std::vector<uint64_t>> tab(ns, std::vector<uint64_t>(nb + 1));
  for (int s = 0; s < ns; s++) {
    data[s].resize(I.bytes[s] ? I.bytes[s] : 1);
    if ((r = spring_streams_download(g.c, s, data[s].data(), tab[s].data()))) return r;
  }
  const unsigned hw = std::thread::hardware_concurrency();
  const int nthr = (int)std::max<uint64_t>(1, std::min<uint64_t>({nb, 8, hw ? hw : 1}));
  std::vector<int> res(nthr, 0);
  std::vector<std::string> msg(nthr);
  auto work = [&](int t) {
    for (uint64_t b = t; b < nb && !res[t]; b += nthr)
      for (int s = 0; s < ns && !res[t]; s++)
        if ((res[t] = spill(base + "/" + FILE_NAME[s] + "." + std::to_string(b), data[s].data() + tab[s][b],
                            tab[s][b + 1] - tab[s][b])))
          msg[t] = spring_reorder_last_error();
  };
  std::vector<std::thread> th;
  try {
    for (int t = 1; t < nthr; t++) th.emplace_back(work, t);
  } catch (const std::system_error &) {
  }
  work(0);
  for (auto &x : th) x.join();
  for (uint64_t t = 1 + th.size(); t < (uint64_t)nthr; t++) work((int)t);  // threads that could not start
  for (int t = 0; t < nthr; t++)
    if (res[t]) return fail(res[t], "%s", msg[t].c_str());
  // inputs go as reorder_compress_streams.cpp:150,:176-182 removes them
  remove(f_cnt.c_str());
  remove(f_noise.c_str());
  remove(f_np.c_str());
  remove(f_rc.c_str());
  remove(f_order.c_str());
  remove(f_len.c_str());
  remove(f_un.c_str());
  remove(f_pos.c_str());
  I.ms_file = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (info_out) *info_out = I;
  return 0;
}
