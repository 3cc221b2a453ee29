// spring_amd/csrc/decode.hip -- the per-block read streams decoded back into reads on the GPU (include/spring_decode.h).
//
// The read part of decompress_short (reference src/decompress.cpp:107-119, :201-321, :615-662), the inverse of
// streams.hip, as data-parallel passes over HBM-resident arrays:
//   units      one thread per unit of the window: flag alphabet, per-unit counts of every variable stream (rev
//              characters, pos-pair entries, rev-pair characters, noise lines, unaligned bytes) and the read lengths;
//              one exclusive scan each.  The scans at every block start must equal the block tables
//   index      noise line ends: flag + scan + compaction over read_noise.txt (line j's noise positions start at
//              index nstart[j] - j of read_noisepos.bin, the identity streams.hip writes by)
//   positions  one wavefront per block, 64 units per step: token offsets by a wave prefix sum of the widths, the
//              escapes found by ballot and the prefix redone until it no longer changes; the previous-position chain
//              is a running value plus a segmented wave prefix.  Each block's bytes must be consumed exactly
//   reads      a lane group per read in slot order: consensus gather (or unaligned copy), noise in line order by the
//              lane that owns the base, reverse complement; the output of a mate is contiguous
// Every check sets a bit of one device error word, read once by the host at the end.  No CPU fallback.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "encoder_internal.h"
#include "fastq_out_internal.h"
#include "reorder_device.h"
#include "reorder_internal.h"
#include "spring_decode.h"
#include "stage_host.h"
#include "streams_internal.h"

using namespace sr;

namespace {

// error bits of the device checks
constexpr uint32_t ERR_FLAG = 1, ERR_TABLE = 2, ERR_POS = 4, ERR_SEQ = 8, ERR_REV = 16, ERR_REVPAIR = 32,
                   ERR_NOISE = 64, ERR_NOISEPOS = 128, ERR_UNALIGNED = 256, ERR_LOOP = 512;
const char *const ERR_TEXT[] = {"a flag outside the alphabet of read_flag.txt",
                                "block tables that do not match the per-unit counts",
                                "read_pos.bin under- or over-consumed in a block",
                                "a read that reaches past the consensus",
                                "read_rev.txt holds a character other than d / r",
                                "read_rev_pair.txt holds a character other than 0 / 1",
                                "read_noise.txt holds a character outside 0..3",
                                "a noise position at or past the read's length",
                                "read_unaligned.txt holds a character other than A C G T N",
                                "the escape iteration of read_pos.bin did not settle"};

// per-unit counts scanned as u32 (totals <= 2 per unit, num_reads < 2^32)
enum { C_REV, C_PP, C_RP, C_LINE, NC };

struct In {   // device images of the window's streams (SPRING_STREAMS_* ids)
  const uint8_t *p[SPRING_STREAMS_NUM];
  uint64_t n[SPRING_STREAMS_NUM];
};
struct Par {
  uint64_t nu, B, seq_len;
  uint32_t nb;
  bool pe, po;
};
struct Scans {   // exclusive scans over the window's units (nu + 1 entries each)
  const uint32_t *c[NC];
  const uint64_t *un;      // unaligned bytes
  const uint64_t *off[2];  // read offsets of mate 0 / 1
};

// flag of unit u; a character outside the alphabet is counted as '2' (both reads unaligned) and refused by k_units
__device__ __forceinline__ int unit_flag(const In &I, const Par &P, uint64_t u, bool *ok) {
  const int f = (int)I.p[SPRING_STREAMS_FLAG][u] - '0';
  *ok = P.pe ? (f >= 0 && f <= 4) : (f == 0 || f == 2);
  return *ok ? f : 2;
}
__device__ __forceinline__ bool al1(int f) { return f != 2 && f != 4; }
__device__ __forceinline__ bool al2(const Par &P, int f) { return P.pe && f != 2 && f != 3; }
__device__ __forceinline__ bool own2(const Par &P, int f) { return P.pe && (f == 1 || f == 4); }
__device__ __forceinline__ uint32_t read_len(const In &I, const Par &P, uint64_t u, int m) {
  const uint8_t *p = I.p[SPRING_STREAMS_LENGTHS] + 2 * (u * (P.pe ? 2 : 1) + m);
  return p[0] | (p[1] << 8);
}

// ------------------------------------------------------------------ units
__global__ __launch_bounds__(256) void k_units(In I, Par P, uint32_t *__restrict__ cnt, uint32_t *__restrict__ un,
                                               uint32_t *__restrict__ len, uint32_t *__restrict__ err) {
  const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t U1 = P.nu + 1;
  if (u > P.nu) return;
  if (u == P.nu) {
    for (int c = 0; c < NC; c++) cnt[c * U1 + u] = 0;
    un[u] = 0;
    len[u] = 0;
    len[U1 + u] = 0;
    return;
  }
  bool ok;
  const int f = unit_flag(I, P, u, &ok);
  if (!ok) atomicOr(err, ERR_FLAG);
  const bool a1 = al1(f), a2 = al2(P, f);
  const uint32_t rl1 = read_len(I, P, u, 0), rl2 = P.pe ? read_len(I, P, u, 1) : 0;
  cnt[C_REV * U1 + u] = (uint32_t)a1 + (uint32_t)own2(P, f);
  cnt[C_PP * U1 + u] = P.pe && f == 0;
  cnt[C_RP * U1 + u] = P.pe && f == 0;
  cnt[C_LINE * U1 + u] = (uint32_t)a1 + (uint32_t)a2;
  un[u] = (a1 ? 0 : rl1) + (P.pe && !a2 ? rl2 : 0);
  len[u] = rl1;
  len[U1 + u] = rl2;
}

// ------------------------------------------------------------------ noise line index
__global__ void k_nl_flag(const uint8_t *__restrict__ noise, uint64_t nb, uint32_t *__restrict__ f) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= nb) f[i] = (i < nb && noise[i] == '\n') ? 1u : 0u;
}
__global__ void k_nl_pos(const uint8_t *__restrict__ noise, uint64_t nb, const uint32_t *__restrict__ idx,
                         uint64_t *__restrict__ nl_end) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb && noise[i] == '\n') nl_end[idx[i]] = i;
}

// ------------------------------------------------------------------ block tables against the unit scans
// tab[s * (nb + 1) + b]: offset of block b of stream s in the window's image; block b starts at unit min(b * B, nu)
__global__ void k_tables(In I, Par P, Scans S, const uint64_t *__restrict__ tab, const uint32_t *__restrict__ nl_idx,
                         uint32_t *__restrict__ err) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nb1 = (uint64_t)P.nb + 1;
  if (b >= nb1) return;
  const uint64_t us = b * P.B < P.nu ? b * P.B : P.nu;
  const uint64_t *t = tab + b;
  bool ok = t[SPRING_STREAMS_REV * nb1] == S.c[C_REV][us] && t[SPRING_STREAMS_UNALIGNED * nb1] == S.un[us];
  if (P.pe)
    ok = ok && t[SPRING_STREAMS_POS_PAIR * nb1] == 2ull * S.c[C_PP][us] && t[SPRING_STREAMS_REV_PAIR * nb1] == S.c[C_RP][us];
  // noise: block b's bytes open with line L = lines before it, at a line start; its noise positions with entry T - L
  const uint64_t T = t[SPRING_STREAMS_NOISE * nb1], L = S.c[C_LINE][us];
  ok = ok && nl_idx[T] == L && (T == 0 || I.p[SPRING_STREAMS_NOISE][T - 1] == '\n') && T >= L &&
       t[SPRING_STREAMS_NOISEPOS * nb1] == 2 * (T - L);
  if (!ok) atomicOr(err, ERR_TABLE);
}

// ------------------------------------------------------------------ positions: one wavefront per block
__device__ __forceinline__ uint32_t wave_incl_u32(uint32_t x, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  return x;
}
__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t x, int d) {
  const uint32_t lo = __shfl_up((uint32_t)x, d, 64), hi = __shfl_up((uint32_t)(x >> 32), d, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_u64(uint64_t x, int l) {
  const uint32_t lo = __shfl((uint32_t)x, l, 64), hi = __shfl((uint32_t)(x >> 32), l, 64);
  return ((uint64_t)hi << 32) | lo;
}
// little-endian value of `w` bytes at p[i] (i + w <= end, checked by the caller; bytes past end read as 0)
__device__ __forceinline__ uint64_t ld_le(const uint8_t *__restrict__ p, uint64_t i, int w, uint64_t end) {
  uint64_t v = 0;
  for (int k = 0; k < w; k++)
    if (i + k < end) v |= (uint64_t)p[i + k] << (8 * k);
  return v;
}

// Token of an aligned read 1: a u64 when preserve_order or it is the block's first aligned read 1
// (first_read_of_block, decompress.cpp:229-247), else a u16 delta, 65535 escaping to a u64.  Read 2 of flags 1 / 4
// appends its own u64.  A step takes 64 * K units, K consecutive ones per lane.  Offsets are the exclusive prefix of
// the widths (lane-local, then across the wave); a token's escape bit is read at its offset, which depends on the
// escapes before it.  Iterating "offsets from the escape bits -> escape bits from the bytes" until no bit changes
// settles: the first token whose offset is wrong moves up by at least one token per round, so the rounds are bounded
// by the tokens whose bit flips (usually one round).  At the fixpoint every offset follows from the true widths of the
// tokens before it.  All loads of a round are independent of each other.
constexpr int KP = 4;
__global__ __launch_bounds__(256) void k_positions(In I, Par P, const uint64_t *__restrict__ tab_pos,
                                                   uint64_t *__restrict__ pos1, uint64_t *__restrict__ pos2,
                                                   unsigned long long *__restrict__ n_esc, uint32_t *__restrict__ err) {
  const uint64_t b = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;   // uniform per wave
  const int lane = threadIdx.x & 63;
  if (b >= P.nb) return;
  const uint64_t us = b * P.B, ue = us + P.B < P.nu ? us + P.B : P.nu;
  const uint8_t *__restrict__ ps = I.p[SPRING_STREAMS_POS];
  const uint8_t *__restrict__ fl = I.p[SPRING_STREAMS_FLAG];
  const uint64_t end = tab_pos[b + 1];
  const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
  uint64_t base = tab_pos[b], prev = 0;
  unsigned long long escapes = 0;
  bool seen = false;
  uint32_t bad = 0;
  uint8_t fnext[KP];
#pragma unroll
  for (int k = 0; k < KP; k++) fnext[k] = us + KP * lane + k < ue ? fl[us + KP * lane + k] : (uint8_t)'2';
  for (uint64_t s0 = us; s0 < ue; s0 += 64 * KP) {
    const uint64_t u0 = s0 + KP * lane;
    bool a1[KP], o2[KP], absolute[KP], delta[KP], esc[KP];
    uint32_t wnom[KP], w[KP];
    uint64_t off[KP], tok[KP], tok2[KP];
    bool any1 = false;
#pragma unroll
    for (int k = 0; k < KP; k++) {
      // this step's flags were loaded one step ahead: their latency hides behind the previous step's bytes
      int f = (int)fnext[k] - '0';
      if (f < 0 || f > 4 || (!P.pe && f != 0 && f != 2)) f = 2;   // refused by k_units
      fnext[k] = u0 + 64 * KP + k < ue ? fl[u0 + 64 * KP + k] : (uint8_t)'2';
      a1[k] = u0 + k < ue && al1(f);
      o2[k] = u0 + k < ue && own2(P, f);
      any1 = any1 || a1[k];
    }
    const unsigned long long m1 = __ballot(any1);
    bool s = seen || (m1 & lt) != 0;
#pragma unroll
    for (int k = 0; k < KP; k++) {
      absolute[k] = a1[k] && (P.po || !s);
      s = s || a1[k];
      delta[k] = a1[k] && !absolute[k];
      wnom[k] = (a1[k] ? (absolute[k] ? 8u : 2u) : 0u) + (o2[k] ? 8u : 0u);
      esc[k] = false;
    }
    seen = seen || m1 != 0;
    uint32_t escbits = 0, lw = 0, incl = 0;
    for (int it = 0;; it++) {
      lw = 0;
#pragma unroll
      for (int k = 0; k < KP; k++) {
        w[k] = wnom[k] + (esc[k] ? 8u : 0u);
        off[k] = lw;
        lw += w[k];
      }
      incl = wave_incl_u32(lw, lane);
      uint32_t eb = 0;
#pragma unroll
      for (int k = 0; k < KP; k++) {
        off[k] += base + incl - lw;
        // the token's bytes at this offset: final once the bits settle (an escape's payload is read below)
        tok[k] = a1[k] ? ld_le(ps, off[k], absolute[k] ? 8 : 2, end) : 0;
        tok2[k] = o2[k] ? ld_le(ps, off[k] + w[k] - 8, 8, end) : 0;
        if (delta[k] && off[k] + 2 <= end && tok[k] == 0xFFFFull) eb |= 1u << k;
      }
      const bool changed = eb != escbits;
      if (!__ballot(changed)) break;
      if (it > 64 * KP) { bad |= ERR_LOOP; break; }
      escbits = eb;
#pragma unroll
      for (int k = 0; k < KP; k++) esc[k] = (eb >> k) & 1u;
    }
    // pos = the last absolute value at or before the token + the deltas since: lane-local inclusive scan, then a
    // segmented scan of the lane totals across the wave
    uint64_t v[KP];
    bool r[KP];
#pragma unroll
    for (int k = 0; k < KP; k++) {
      if (w[k] && off[k] + w[k] > end) bad |= ERR_POS;   // a token runs past the block
      v[k] = tok[k];
      r[k] = absolute[k];
      if (esc[k]) { v[k] = ld_le(ps, off[k] + 2, 8, end); r[k] = true; }
      if (o2[k]) pos2[u0 + k] = tok2[k];
      if (k) { if (!r[k]) { v[k] += v[k - 1]; r[k] = r[k - 1]; } }
    }
    uint64_t tv = v[KP - 1];
    bool tr = r[KP - 1];
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t ov = shfl_up_u64(tv, d);
      const int orst = __shfl_up((int)tr, d, 64);
      if (lane >= d && !tr) { tv += ov; tr = orst != 0; }
    }
    // exclusive: the totals of the lanes before this one, on top of the running value
    const uint64_t xv = shfl_up_u64(tv, 1);
    const bool xr = __shfl_up((int)tr, 1, 64) != 0 && lane > 0;
    const uint64_t before = lane == 0 ? prev : (xr ? xv : prev + xv);
    uint64_t last = 0;
#pragma unroll
    for (int k = 0; k < KP; k++) {
      last = r[k] ? v[k] : before + v[k];
      if (a1[k]) pos1[u0 + k] = last;
    }
    prev = shfl_u64(last, 63);
    base += __shfl(incl, 63, 64);
    escapes += __popc(escbits);
  }
  if (base != end) bad |= ERR_POS;   // trailing bytes (or tokens past the end, flagged above)
  if (escapes) atomicAdd(n_esc, escapes);
  if (bad) atomicOr(err, bad);
}

// ------------------------------------------------------------------ reads: G lanes per read
__device__ __forceinline__ char comp(char c) {
  return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
}
__device__ __forceinline__ char dec_noise(char c, int k) {   // decompress.cpp:664-684
  switch (c) {
    case 'A': return "CGTN"[k];
    case 'C': return "AGTN"[k];
    case 'G': return "TACN"[k];
    case 'T': return "GCAN"[k];
    default: return "AGCT"[k];
  }
}

template <int G>
__global__ __launch_bounds__(256) void k_reads(In I, Par P, Scans S, const uint64_t *__restrict__ pos1,
                                               const uint64_t *__restrict__ pos2, const uint8_t *__restrict__ cons,
                                               const uint64_t *__restrict__ nl_end, uint64_t nlines, char *out0,
                                               char *out1, uint32_t *__restrict__ err) {
  const uint64_t r = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  const int lane = threadIdx.x % G;
  if (r >= (P.pe ? 2 * P.nu : P.nu)) return;
  const int m = r >= P.nu ? 1 : 0;
  const uint64_t u = r - (m ? P.nu : 0);
  bool ok;
  const int f = unit_flag(I, P, u, &ok);
  const bool a1 = al1(f), aligned = m ? al2(P, f) : a1;
  const uint32_t rl = (uint32_t)(S.off[m][u + 1] - S.off[m][u]);
  char *dst = (m ? out1 : out0) + S.off[m][u];
  uint32_t bad = 0;
  if (!aligned) {   // read_unaligned.txt: read 1 of the unit first
    const uint64_t o = S.un[u] + (m && !a1 ? S.off[0][u + 1] - S.off[0][u] : 0);
    if (o + rl > I.n[SPRING_STREAMS_UNALIGNED]) bad |= ERR_TABLE;
    else
      for (uint32_t c = lane; c < rl; c += G) {
        const char ch = (char)I.p[SPRING_STREAMS_UNALIGNED][o + c];
        bad |= (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T' || ch == 'N') ? 0u : ERR_UNALIGNED;
        dst[c] = ch;
      }
    if (bad) atomicOr(err, bad);
    return;
  }
  // position and orientation (decompress.cpp:236-256, :282-297)
  const uint64_t ri = S.c[C_REV][u] + (m && a1 ? 1 : 0);
  const uint8_t *rev = I.p[SPRING_STREAMS_REV];
  uint64_t p = 0;
  char rc = 'd';
  if (m == 0 || own2(P, f)) {
    p = m ? pos2[u] : pos1[u];
    if (ri < I.n[SPRING_STREAMS_REV]) rc = (char)rev[ri];
    else bad |= ERR_TABLE;
  } else {   // flag 0: pos1 + int16, orientation relative to read 1
    const uint64_t k = S.c[C_PP][u], q = S.c[C_RP][u];
    if (2 * k + 2 > I.n[SPRING_STREAMS_POS_PAIR] || q >= I.n[SPRING_STREAMS_REV_PAIR] ||
        S.c[C_REV][u] >= I.n[SPRING_STREAMS_REV]) {
      bad |= ERR_TABLE;
    } else {
      const uint8_t *pp = I.p[SPRING_STREAMS_POS_PAIR] + 2 * k;
      p = pos1[u] + (uint64_t)(int64_t)(int16_t)(uint16_t)(pp[0] | (pp[1] << 8));
      const char rc1 = (char)rev[S.c[C_REV][u]], rel = (char)I.p[SPRING_STREAMS_REV_PAIR][q];
      if (rel != '0' && rel != '1') bad |= ERR_REVPAIR;
      rc = rel == '0' ? (rc1 == 'd' ? 'r' : 'd') : rc1;
      if (rc1 != 'd' && rc1 != 'r') bad |= ERR_REV;
    }
  }
  if (rc != 'd' && rc != 'r') bad |= ERR_REV;
  if (p > P.seq_len || rl > P.seq_len - p) bad |= ERR_SEQ;
  const uint64_t j = S.c[C_LINE][u] + (m && a1 ? 1 : 0);   // noise line of this read
  if (j >= nlines) bad |= ERR_TABLE;
  if (bad) { atomicOr(err, bad); return; }
  const bool rev_c = rc == 'r';
  const uint8_t *src = cons + p;
  const uint32_t alpha = rev_c ? 0x41474354u : 0x54434741u;   // little-endian "TCGA" / "AGCT"
  for (uint32_t c = lane; c < rl; c += G) {
    const uint32_t code = src[rev_c ? rl - 1 - c : c] & 3u;   // SPRING code A0 G1 C2 T3
    dst[c] = (char)(alpha >> (8 * code));                    // "AGCT" or "TCGA" in a register
  }
  // noise in line order; the base at output index o belongs to lane o % G, which wrote it above
  const uint64_t ns = j ? nl_end[j - 1] + 1 : 0, nc = nl_end[j] - ns, npi = ns - j;
  if (2 * (npi + nc) > I.n[SPRING_STREAMS_NOISEPOS]) { atomicOr(err, ERR_TABLE); return; }
  const uint8_t *nz = I.p[SPRING_STREAMS_NOISE] + ns, *np = I.p[SPRING_STREAMS_NOISEPOS] + 2 * npi;
  uint16_t at = 0;
  for (uint64_t k = 0; k < nc; k++) {
    at = (uint16_t)(at + (np[2 * k] | (np[2 * k + 1] << 8)));   // u16 arithmetic, as the reader's
    const int ch = (int)nz[k] - '0';
    if (ch < 0 || ch > 3) { bad |= ERR_NOISE; break; }
    if (at >= rl) { bad |= ERR_NOISEPOS; break; }
    const uint32_t o = rev_c ? rl - 1 - at : at;
    if (o % G == (uint32_t)lane) {
      const char cur = rev_c ? comp(dst[o]) : dst[o];
      const char nw = dec_noise(cur, ch);
      dst[o] = rev_c ? comp(nw) : nw;
    }
  }
  if (bad) atomicOr(err, bad);
}

// ------------------------------------------------------------------ consensus
// packed (A0 C1 G2 T3, 4 bases per byte, first base in the low bits) -> one SPRING code (A0 G1 C2 T3) per base
__global__ void k_unpack_seq(const uint8_t *__restrict__ packed, uint64_t nbytes, uint8_t *__restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nbytes) return;
  const uint32_t v = packed[i];
  uint32_t w = 0;
  for (int k = 0; k < 4; k++) {
    const uint32_t nat = (v >> (2 * k)) & 3u;
    w |= (nat == 1 ? 2u : nat == 2 ? 1u : nat) << (8 * k);
  }
  for (int k = 0; k < 4; k++) out[4 * i + k] = (uint8_t)(w >> (8 * k));
}

}  // namespace

struct spring_decode_ctx {
  int dev = 0;
  hipStream_t st = nullptr;
  DBuf cons;                 // the consensus, SPRING byte codes
  uint64_t seq_len = 0;
  bool have_seq = false;
  bool have = false;         // a decode result
  spring_decode_info info;
  DBuf out[2];               // bases of mate 0 / 1
  DBuf off[2];               // num_units + 1 read offsets of mate 0 / 1
};

namespace {

// the window's geometry and the host-side table checks; -> 0 or E_ARG
int window(uint32_t first_block, uint32_t num_blocks, uint32_t N, bool pe, uint32_t B, uint64_t *nu) {
  if (B == 0) return fail(SPRING_REORDER_E_ARG, "num_reads_per_block must be > 0");
  if (pe && (N & 1)) return fail(SPRING_REORDER_E_ARG, "paired-end data needs an even num_reads (got %u)", N);
  const uint64_t U = pe ? N / 2 : N, total = (U + B - 1) / B;
  if ((uint64_t)first_block + num_blocks > total)
    return fail(SPRING_REORDER_E_ARG, "blocks [%u, %llu) outside the file's %llu blocks", first_block,
                (unsigned long long)first_block + num_blocks, (unsigned long long)total);
  const uint64_t u0 = (uint64_t)first_block * B, u1 = std::min<uint64_t>(((uint64_t)first_block + num_blocks) * B, U);
  *nu = u1 > u0 ? u1 - u0 : 0;
  return 0;
}

int check_tables(const uint64_t *const *tab, const uint64_t *bytes, uint32_t nb, uint64_t nu, bool pe, uint64_t B) {
  const int ns = pe ? SPRING_STREAMS_NUM : SPRING_STREAMS_POS_PAIR;
  for (int s = 0; s < ns; s++) {
    const uint64_t *t = tab[s];
    if (!t) return fail(SPRING_REORDER_E_ARG, "NULL block table of stream %d", s);
    if (t[0] != 0 || t[nb] != bytes[s])
      return fail(SPRING_REORDER_E_ARG, "block table of stream %d does not span its %llu bytes", s,
                  (unsigned long long)bytes[s]);
    for (uint32_t b = 0; b < nb; b++)
      if (t[b + 1] < t[b]) return fail(SPRING_REORDER_E_ARG, "block table of stream %d is not monotone", s);
    if (s == SPRING_STREAMS_FLAG || s == SPRING_STREAMS_LENGTHS) {
      const uint64_t w = s == SPRING_STREAMS_FLAG ? 1 : (pe ? 4 : 2);
      for (uint32_t b = 0; b <= nb; b++)
        if (t[b] != std::min<uint64_t>((uint64_t)b * B, nu) * w)
          return fail(SPRING_REORDER_E_ARG, "block table of stream %d does not match the block sizes", s);
    }
  }
  return 0;
}

// the decode of a window whose streams are on the device (d[s], bytes[s]) with host block tables tab[s]
int decode_core(spring_decode_ctx *ctx, const uint8_t *const *d, const uint64_t *bytes, const uint64_t *const *tab,
                uint32_t first_block, uint32_t nb, uint32_t N, bool pe, bool po, uint32_t B, spring_decode_info *info_out) {
  const int dev = ctx->dev;
  hipStream_t st = ctx->st;
  ctx->have = false;
  for (auto &b : ctx->out) b.release();
  for (auto &b : ctx->off) b.release();
  if (!ctx->have_seq) return fail(SPRING_REORDER_E_STATE, "no consensus loaded (spring_decode_seq_from_*)");
  uint64_t nu = 0;
  int r = window(first_block, nb, N, pe, B, &nu);
  if (r) return r;
  if ((r = check_tables(tab, bytes, nb, nu, pe, B))) return r;
  const uint64_t nbytes_noise = bytes[SPRING_STREAMS_NOISE];
  if (nbytes_noise >= 0xFFFFFFF0ull) return fail(SPRING_REORDER_E_ARG, "read_noise.txt larger than 4 GB");
  spring_decode_info &R = ctx->info;
  memset(&R, 0, sizeof(R));
  R.seq_len = ctx->seq_len;
  R.first_block = first_block;
  R.num_blocks = nb;
  R.num_units = nu;
  In I;
  for (int s = 0; s < SPRING_STREAMS_NUM; s++) {
    const bool used = pe || s < SPRING_STREAMS_POS_PAIR;
    I.p[s] = used ? d[s] : nullptr;
    I.n[s] = used ? bytes[s] : 0;
  }
  Par P;
  P.nu = nu; P.B = B; P.seq_len = ctx->seq_len; P.nb = nb; P.pe = pe; P.po = po;
  const uint64_t U1 = nu + 1, nb1 = (uint64_t)nb + 1;

  hipEvent_t ev[2];
  for (auto &e : ev) HIPCHK(hipEventCreate(&e));
  struct EvGuard { hipEvent_t *e; ~EvGuard() { (void)hipEventDestroy(e[0]); (void)hipEventDestroy(e[1]); } } evg{ev};
  DBuf d_err, d_esc, tabs, cnt, cscan, un, unscan, len, lscan, flag, idx, nl_end, p1, p2, tmp;
  DALLOC(d_err, 4);
  DALLOC(d_esc, 8);
  DALLOC(tabs, SPRING_STREAMS_NUM * nb1 * 8);
  std::vector<uint64_t> htab(SPRING_STREAMS_NUM * nb1, 0);
  for (int s = 0; s < (pe ? SPRING_STREAMS_NUM : SPRING_STREAMS_POS_PAIR); s++)
    memcpy(htab.data() + s * nb1, tab[s], nb1 * 8);
  HIPCHK(hipMemcpyAsync(tabs.p, htab.data(), htab.size() * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(ev[0], st));
  HIPCHK(hipMemsetAsync(d_err.p, 0, 4, st));
  HIPCHK(hipMemsetAsync(d_esc.p, 0, 8, st));
  uint32_t *err = d_err.as<uint32_t>();
  // ---- units + scans
  DALLOC(cnt, NC * U1 * 4); DALLOC(cscan, NC * U1 * 4);
  DALLOC(un, U1 * 4); DALLOC(unscan, U1 * 8);
  DALLOC(len, 2 * U1 * 4); DALLOC(lscan, 2 * U1 * 8);
  DALLOC(flag, (nbytes_noise + 1) * 4); DALLOC(idx, (nbytes_noise + 1) * 4);
  size_t tb = 0, t2 = 0;
  HIPCHK(sr::excl_scan_u32(st, nullptr, t2, nullptr, nullptr, U1)); tb = std::max(tb, t2);
  HIPCHK(sr::excl_scan_u32_to_u64(st, nullptr, t2, nullptr, nullptr, U1)); tb = std::max(tb, t2);
  HIPCHK(sr::excl_scan_u32(st, nullptr, t2, nullptr, nullptr, nbytes_noise + 1)); tb = std::max(tb, t2);
  DALLOC(tmp, tb);
  hipLaunchKernelGGL(k_units, grid(U1), dim3(256), 0, st, I, P, cnt.as<uint32_t>(), un.as<uint32_t>(),
                     len.as<uint32_t>(), err);
  for (int c = 0; c < NC; c++)
    HIPCHK(sr::excl_scan_u32(st, tmp.p, t2 = tb, cnt.as<uint32_t>() + c * U1, cscan.as<uint32_t>() + c * U1, U1));
  HIPCHK(sr::excl_scan_u32_to_u64(st, tmp.p, t2 = tb, un.as<uint32_t>(), unscan.as<uint64_t>(), U1));
  for (int m = 0; m < (pe ? 2 : 1); m++)
    HIPCHK(sr::excl_scan_u32_to_u64(st, tmp.p, t2 = tb, len.as<uint32_t>() + m * U1, lscan.as<uint64_t>() + m * U1, U1));
  // ---- noise line index
  hipLaunchKernelGGL(k_nl_flag, grid(nbytes_noise + 1), dim3(256), 0, st, I.p[SPRING_STREAMS_NOISE], nbytes_noise,
                     flag.as<uint32_t>());
  HIPCHK(sr::excl_scan_u32(st, tmp.p, t2 = tb, flag.as<uint32_t>(), idx.as<uint32_t>(), nbytes_noise + 1));
  uint32_t nlines = 0, lines_tot = 0;
  uint64_t bases[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(&nlines, idx.as<uint32_t>() + nbytes_noise, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&lines_tot, cscan.as<uint32_t>() + C_LINE * U1 + nu, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&bases[0], lscan.as<uint64_t>() + nu, 8, hipMemcpyDeviceToHost, st));
  if (pe) HIPCHK(hipMemcpyAsync(&bases[1], lscan.as<uint64_t>() + U1 + nu, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  DALLOC(nl_end, (uint64_t)nlines * 8);
  if (nlines) hipLaunchKernelGGL(k_nl_pos, grid(nbytes_noise), dim3(256), 0, st, I.p[SPRING_STREAMS_NOISE],
                                 nbytes_noise, idx.as<uint32_t>(), nl_end.as<uint64_t>());
  Scans S;
  for (int c = 0; c < NC; c++) S.c[c] = cscan.as<uint32_t>() + c * U1;
  S.un = unscan.as<uint64_t>();
  S.off[0] = lscan.as<uint64_t>();
  S.off[1] = lscan.as<uint64_t>() + U1;
  hipLaunchKernelGGL(k_tables, grid(nb1), dim3(256), 0, st, I, P, S, tabs.as<uint64_t>(), idx.as<uint32_t>(), err);
  // ---- positions
  DALLOC(p1, nu * 8);
  DALLOC(p2, pe ? nu * 8 : 0);
  if (nb) hipLaunchKernelGGL(k_positions, grid((uint64_t)nb * 64), dim3(256), 0, st, I, P,
                             tabs.as<uint64_t>() + SPRING_STREAMS_POS * nb1, p1.as<uint64_t>(), p2.as<uint64_t>(),
                             d_esc.as<unsigned long long>(), err);
  // ---- reads
  for (int m = 0; m < (pe ? 2 : 1); m++) {
    DALLOC(ctx->out[m], bases[m]);
    DALLOC(ctx->off[m], U1 * 8);
    HIPCHK(hipMemcpyAsync(ctx->off[m].p, S.off[m], U1 * 8, hipMemcpyDeviceToDevice, st));
  }
  constexpr int G = 32;
  const uint64_t nreads = pe ? 2 * nu : nu;
  if (nreads)
    hipLaunchKernelGGL(k_reads<G>, grid(nreads * G), dim3(256), 0, st, I, P, S, p1.as<uint64_t>(), p2.as<uint64_t>(),
                       ctx->cons.as<uint8_t>(), nl_end.as<uint64_t>(), (uint64_t)nlines, ctx->out[0].as<char>(),
                       pe ? ctx->out[1].as<char>() : nullptr, err);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev[1], st));
  uint32_t herr = 0;
  unsigned long long nesc = 0;
  HIPCHK(hipMemcpyAsync(&herr, err, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&nesc, d_esc.p, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (herr || nlines != lines_tot) {
    for (auto &b : ctx->out) b.release();
    for (auto &b : ctx->off) b.release();
    std::string msg;
    for (int k = 0; k < 10; k++)
      if (herr & (1u << k)) msg += std::string(msg.empty() ? "" : "; ") + ERR_TEXT[k];
    if (nlines != lines_tot)
      msg += std::string(msg.empty() ? "" : "; ") + "read_noise.txt holds " + std::to_string(nlines) + " lines for " +
             std::to_string(lines_tot) + " aligned reads";
    return fail(SPRING_REORDER_E_ARG, "refused: %s", msg.c_str());
  }
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
  R.bases[0] = bases[0];
  R.bases[1] = bases[1];
  R.n_aligned = lines_tot;
  R.n_unaligned = nreads - lines_tot;
  R.pos_escapes = nesc;
  R.ms_device = ms;
  ctx->have = true;
  if (info_out) *info_out = R;
  return 0;
}

}  // namespace

extern "C" {

int spring_decode_create(int device, spring_decode_ctx **out) {
  if (!out) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  const int r = stage_device(&device, "the decoder");
  if (r) return r;
  spring_decode_ctx *c = new spring_decode_ctx();
  c->dev = device;
  memset(&c->info, 0, sizeof(c->info));
  *out = c;
  return 0;
}

void spring_decode_destroy(spring_decode_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->dev);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  ctx->cons.release();
  for (auto &b : ctx->out) b.release();
  for (auto &b : ctx->off) b.release();
  if (ctx->st) (void)hipStreamDestroy(ctx->st);
  delete ctx;
}

int spring_decode_seq_from_encoder(spring_decode_ctx *ctx, spring_encoder_ctx *enc) {
  if (!ctx || !enc) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  sr::EncoderView V;
  int r = sr::encoder_view(enc, &V);
  if (r) return r;
  if (V.dev != ctx->dev) return fail(SPRING_REORDER_E_ARG, "encoder and decode contexts live on different devices");
  if ((r = stream_begin(ctx->dev, &ctx->st))) return r;
  ctx->have_seq = false;
  ctx->have = false;
  const int dev = ctx->dev;
  const uint64_t n = V.info.seq_len, b0 = V.num_thr ? V.tid_seq[0] : 0;
  if (V.num_thr && V.tid_seq[V.num_thr] - b0 != n)
    return fail(SPRING_REORDER_E_STATE, "the encoder's tids do not cover its consensus");
  DALLOC(ctx->cons, n + 64);
  if (n) HIPCHK(hipMemcpyAsync(ctx->cons.p, V.refc + b0, n, hipMemcpyDeviceToDevice, ctx->st));
  HIPCHK(hipStreamSynchronize(ctx->st));
  ctx->seq_len = n;
  ctx->have_seq = true;
  return 0;
}

int spring_decode_seq_from_host(spring_decode_ctx *ctx, int32_t num_thr_e, const uint64_t *seq_len_tid,
                                const uint8_t *packed, const char *tail) {
  if (!ctx || num_thr_e < 0 || (num_thr_e && (!seq_len_tid || !tail))) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  uint64_t n = 0, np = 0;
  for (int t = 0; t < num_thr_e; t++) {
    n += seq_len_tid[t];
    np += seq_len_tid[t] / 4;
    for (uint64_t k = 0; k < seq_len_tid[t] % 4; k++) {
      const char c = tail[4 * t + k];
      if (c != 'A' && c != 'C' && c != 'G' && c != 'T')
        return fail(SPRING_REORDER_E_ARG, "read_seq.bin.%d.tail holds a character other than A C G T", t);
    }
  }
  if (np && !packed) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  int r = stream_begin(ctx->dev, &ctx->st);
  if (r) return r;
  ctx->have_seq = false;
  ctx->have = false;
  const int dev = ctx->dev;
  hipStream_t st = ctx->st;
  DBuf d_packed;
  DALLOC(d_packed, np);
  DALLOC(ctx->cons, n + 64);
  if (np) HIPCHK(hipMemcpyAsync(d_packed.p, packed, np, hipMemcpyHostToDevice, st));
  std::vector<uint8_t> tcodes(4 * (size_t)std::max(num_thr_e, 1));
  uint64_t o = 0, po = 0;
  for (int t = 0; t < num_thr_e; t++) {   // tid t: its packed bytes, then its tail (decompress.cpp:107-119, :638-652)
    const uint64_t nb = seq_len_tid[t] / 4, nt = seq_len_tid[t] % 4;
    if (nb) hipLaunchKernelGGL(k_unpack_seq, grid(nb), dim3(256), 0, st, d_packed.as<uint8_t>() + po, nb,
                               ctx->cons.as<uint8_t>() + o);
    for (uint64_t k = 0; k < nt; k++) {
      const char c = tail[4 * t + k];
      tcodes[4 * t + k] = c == 'A' ? 0 : c == 'G' ? 1 : c == 'C' ? 2 : 3;
    }
    if (nt) HIPCHK(hipMemcpyAsync(ctx->cons.as<uint8_t>() + o + 4 * nb, tcodes.data() + 4 * t, nt, hipMemcpyHostToDevice, st));
    o += seq_len_tid[t];
    po += nb;
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  ctx->seq_len = n;
  ctx->have_seq = true;
  return 0;
}

int spring_decode_from_streams(spring_decode_ctx *ctx, spring_streams_ctx *s, spring_decode_info *info) {
  if (!ctx || !s) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  sr::StreamsView V;
  int r = sr::streams_view(s, &V);
  if (r) return r;
  if (V.dev != ctx->dev) return fail(SPRING_REORDER_E_ARG, "streams and decode contexts live on different devices");
  if ((r = stream_begin(ctx->dev, &ctx->st))) return r;
  const uint64_t nb1 = V.info.num_blocks + 1;
  const uint64_t *tab[SPRING_STREAMS_NUM];
  for (int k = 0; k < SPRING_STREAMS_NUM; k++) tab[k] = V.table + k * nb1;
  r = decode_core(ctx, V.bytes, V.info.bytes, tab, 0, (uint32_t)V.info.num_blocks, V.num_reads, V.paired_end,
                  V.preserve_order, V.num_reads_per_block, info);
  (void)hipStreamSynchronize(ctx->st);
  return r;
}

int spring_decode_from_host(spring_decode_ctx *ctx, const uint8_t *const *bytes, const uint64_t *const *block_off,
                            uint32_t first_block, uint32_t num_blocks, uint32_t num_reads, int32_t paired_end,
                            int32_t preserve_order, uint32_t num_reads_per_block, spring_decode_info *info) {
  if (!ctx || !bytes || !block_off) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  const int ns = paired_end ? SPRING_STREAMS_NUM : SPRING_STREAMS_POS_PAIR;
  uint64_t n[SPRING_STREAMS_NUM] = {0};
  for (int s = 0; s < ns; s++) {
    if (!block_off[s]) return fail(SPRING_REORDER_E_ARG, "NULL block table of stream %d", s);
    n[s] = block_off[s][num_blocks];
    if (n[s] && !bytes[s]) return fail(SPRING_REORDER_E_ARG, "NULL stream %d", s);
  }
  int r = stream_begin(ctx->dev, &ctx->st);
  if (r) return r;
  if (!ctx->have_seq) {
    ctx->have = false;
    return fail(SPRING_REORDER_E_STATE, "no consensus loaded (spring_decode_seq_from_*)");
  }
  const int dev = ctx->dev;
  DBuf d[SPRING_STREAMS_NUM];
  const uint8_t *dp[SPRING_STREAMS_NUM] = {nullptr};
  const uint64_t *tab[SPRING_STREAMS_NUM] = {nullptr};
  for (int s = 0; s < ns; s++) {
    DALLOC(d[s], n[s]);
    if (n[s]) HIPCHK(hipMemcpyAsync(d[s].p, bytes[s], n[s], hipMemcpyHostToDevice, ctx->st));
    dp[s] = d[s].as<uint8_t>();
    tab[s] = block_off[s];
  }
  r = decode_core(ctx, dp, n, tab, first_block, num_blocks, num_reads, paired_end != 0, preserve_order != 0,
                  num_reads_per_block, info);
  (void)hipStreamSynchronize(ctx->st);
  return r;
}

int spring_decode_download(spring_decode_ctx *ctx, int32_t mate, char *bases, uint64_t *read_off) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing decoded yet");
  if (mate < 0 || mate > 1 || !ctx->off[mate].p) return fail(SPRING_REORDER_E_ARG, "bad mate %d", mate);
  HIPCHK(hipSetDevice(ctx->dev));
  if (bases && ctx->info.bases[mate]) HIPCHK(rd(ctx->st, bases, ctx->out[mate].p, ctx->info.bases[mate]));
  if (read_off) HIPCHK(rd(ctx->st, read_off, ctx->off[mate].p, (ctx->info.num_units + 1) * 8));
  return 0;
}

int spring_decode_get_info(spring_decode_ctx *ctx, spring_decode_info *info) {
  if (!ctx || !info) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing decoded yet");
  *info = ctx->info;
  return 0;
}

}  // extern "C"

namespace sr {
int decode_view(spring_decode_ctx *ctx, DecodeView *v) {
  if (!ctx || !v) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing decoded yet");
  v->dev = ctx->dev;
  v->info = ctx->info;
  v->paired_end = ctx->off[1].p != nullptr;
  for (int m = 0; m < 2; m++) { v->bases[m] = ctx->out[m].as<uint8_t>(); v->read_off[m] = ctx->off[m].as<uint64_t>(); }
  return 0;
}
}  // namespace sr

// ------------------------------------------------------------------ file contract
namespace {

const char *const FILE_NAME[SPRING_STREAMS_NUM] = {"read_flag.txt", "read_pos.bin", "read_noise.txt", "read_noisepos.bin",
                                                   "read_rev.txt", "read_unaligned.txt", "read_lengths.bin",
                                                   "read_pos_pair.bin", "read_rev_pair.txt"};

int slurp_append(const std::string &path, std::vector<uint8_t> &buf) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return fail(SPRING_REORDER_E_IO, "cannot open %s", path.c_str());
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  if (n < 0) { fclose(f); return fail(SPRING_REORDER_E_IO, "cannot size %s", path.c_str()); }
  const size_t o = buf.size();
  buf.resize(o + (size_t)n);
  const size_t got = n ? fread(buf.data() + o, 1, (size_t)n, f) : 0;
  fclose(f);
  if (got != (size_t)n) return fail(SPRING_REORDER_E_IO, "short read of %s", path.c_str());
  return 0;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

extern "C" int spring_decode_seq_from_files(spring_decode_ctx *ctx, const char *temp_dir, int32_t num_thr_e) {
  if (!temp_dir || num_thr_e < 0) return fail(SPRING_REORDER_E_ARG, "bad argument");
  const std::string base = std::string(temp_dir) + "/read_seq.bin.";
  std::vector<uint8_t> packed, tails(4 * (size_t)std::max(num_thr_e, 1), 0), tl;
  std::vector<uint64_t> len(std::max(num_thr_e, 1), 0);
  int r;
  for (int t = 0; t < num_thr_e; t++) {
    const size_t o = packed.size();
    tl.clear();
    if ((r = slurp_append(base + std::to_string(t), packed)) || (r = slurp_append(base + std::to_string(t) + ".tail", tl)))
      return r;
    if (tl.size() > 3) return fail(SPRING_REORDER_E_ARG, "read_seq.bin.%d.tail holds %zu bases", t, tl.size());
    memcpy(tails.data() + 4 * t, tl.data(), tl.size());
    len[t] = 4 * (packed.size() - o) + tl.size();
  }
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if ((r = spring_decode_seq_from_host(ctx, num_thr_e, len.data(), packed.data(), (const char *)tails.data())))
    return r;
  for (int t = 0; t < num_thr_e; t++) {   // decompress.cpp:656-657 and :119
    remove((base + std::to_string(t)).c_str());
    remove((base + std::to_string(t) + ".tail").c_str());
  }
  return 0;
}

extern "C" int spring_decode_from_files(spring_decode_ctx *ctx, const char *temp_dir, uint32_t first_block,
                                        uint32_t num_blocks, uint32_t num_reads, int32_t paired_end,
                                        int32_t preserve_order, uint32_t num_reads_per_block, spring_decode_info *info) {
  const auto t0 = std::chrono::steady_clock::now();
  if (!temp_dir) return fail(SPRING_REORDER_E_ARG, "temp_dir is NULL");
  const std::string base(temp_dir);
  const int ns = paired_end ? SPRING_STREAMS_NUM : SPRING_STREAMS_POS_PAIR;
  std::vector<std::vector<uint8_t>> data(ns);
  std::vector<std::vector<uint64_t>> tab(ns, std::vector<uint64_t>((size_t)num_blocks + 1, 0));
  int r;
  for (int s = 0; s < ns; s++)
    for (uint32_t b = 0; b < num_blocks; b++) {
      if ((r = slurp_append(base + "/" + FILE_NAME[s] + "." + std::to_string((uint64_t)first_block + b), data[s])))
        return r;
      tab[s][b + 1] = data[s].size();
    }
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  const uint8_t *bytes[SPRING_STREAMS_NUM] = {nullptr};
  const uint64_t *off[SPRING_STREAMS_NUM] = {nullptr};
  for (int s = 0; s < ns; s++) {
    bytes[s] = data[s].data();
    off[s] = tab[s].data();
  }
  spring_decode_info I;
  if ((r = spring_decode_from_host(ctx, bytes, off, first_block, num_blocks, num_reads, paired_end, preserve_order,
                                   num_reads_per_block, &I)))
    return r;
  for (int s = 0; s < ns; s++)   // decompress.cpp:334-353
    for (uint32_t b = 0; b < num_blocks; b++)
      remove((base + "/" + FILE_NAME[s] + "." + std::to_string((uint64_t)first_block + b)).c_str());
  I.ms_file = ms_since(t0);
  ctx->info.ms_file = I.ms_file;
  if (info) *info = I;
  return 0;
}
