// spring_amd/csrc/qualid.hip -- row g3: the quality and id side of preprocess and reorder_compress_quality_id
// (reference src/preprocess.cpp:200-250, src/reorder_compress_quality_id.cpp:34-235) up to their codec calls, on the
// device (include/spring_qualid.h).
//
//   newline index (fastq_kernels.hip)  ->  per slot: start and length (CR trimmed) of the line it holds, gathered
//   through the inverse of order_array  ->  exclusive scan of the lengths (off[]; block b starts at off[b * B])
//   ->  the slot of every 4 KiB of output  ->  the copy.
//
// The copy is the destination-driven copy of copy_words.h with the slots as its pieces: a lane owns one 16-byte-aligned
// word of the output, walks over as many lines as the word spans, applies the quantization table from LDS and stores
// the word.  Id lines get their '\n' from the kernel: with NL = 1 slot s starts at off[s] + s.
#include <algorithm>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "copy_words.h"
#include "encoder_internal.h"
#include "fastq_out_internal.h"
#include "reorder_device.h"
#include "reorder_internal.h"
#include "spring_qualid.h"
#include "stage_host.h"

using namespace sr;

namespace {

// error bits of the device checks
constexpr uint32_t ERR_PERM = 1, ERR_QLEN = 2, ERR_LONG = 4, ERR_BYTE = 8;
constexpr int CHANGED_SLOTS = 1024;      // counters the copy's blocks spread their bytes_changed over

// ------------------------------------------------------------------ order -> the line of every slot
__global__ void k_perm_check(const uint32_t *__restrict__ order, uint32_t n, uint32_t *__restrict__ hits,
                             uint32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t o = order[i];
  if (o >= n || atomicAdd(&hits[o], 1u)) atomicOr(err, ERR_PERM);
}
// Single-end: order_array[order[i]] = i (reorder_compress_quality_id.cpp:116-125), so slot i holds line order[i]: the
// order itself.  Paired-end: if (order[i] < n/2) order_array[order[i]] = pos++ (:101-115), so slot pos holds line
// order[i]; pos = exclusive scan of the flags.
__global__ void k_flag_file1(const uint32_t *__restrict__ order, uint32_t n, uint32_t half, uint32_t *__restrict__ f) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) f[i] = order[i] < half ? 1u : 0u;
}
__global__ void k_rec_pe(const uint32_t *__restrict__ order, const uint32_t *__restrict__ pos, uint32_t n,
                         uint32_t half, uint32_t *__restrict__ rec) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && order[i] < half) rec[pos[i]] = order[i];
}

// ------------------------------------------------------------------ lines
// line_end[j] is the position of the '\n' of line j (nbytes for an unterminated last line)
__device__ __forceinline__ uint64_t no_cr(const uint8_t *__restrict__ txt, uint64_t a, uint64_t b) {
  return b > a && txt[b - 1] == '\r' ? b - 1 : b;   // remove_CR_from_end
}
__device__ __forceinline__ void put_line(uint64_t *__restrict__ start, uint32_t *__restrict__ len, uint64_t s,
                                         uint64_t a, uint64_t b, uint32_t *__restrict__ err) {
  uint64_t l = b - a;
  if (l > 0xffffffffull) { atomicOr(err, ERR_LONG); l = 0; }
  start[s] = a;
  len[s] = (uint32_t)l;
}
// Slot s holds record rec[s] (s itself without an order) of a FASTQ: start and length of its id (line 0) and of its
// quality (line 3), whichever is asked for, in slot order; the quality has to be as long as the read (line 1).
__global__ void k_lines_fastq(const uint8_t *__restrict__ txt, const uint64_t *__restrict__ line_end, uint64_t U,
                              const uint32_t *__restrict__ rec, uint64_t *__restrict__ start_q,
                              uint32_t *__restrict__ len_q, uint64_t *__restrict__ start_i, uint32_t *__restrict__ len_i,
                              uint32_t *__restrict__ err) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s == 0) {
    if (len_q) len_q[U] = 0;
    if (len_i) len_i[U] = 0;
  }
  if (s >= U) return;
  const uint64_t i = rec ? rec[s] : s;
  const uint64_t *e = line_end + 4 * i;
  const uint64_t a0 = i ? e[-1] + 1 : 0, e0 = e[0], e1 = e[1], e2 = e[2], e3 = e[3];
  const uint64_t qb = no_cr(txt, e2 + 1, e3);
  if (no_cr(txt, e0 + 1, e1) - (e0 + 1) != qb - (e2 + 1)) atomicOr(err, ERR_QLEN);
  if (len_q) put_line(start_q, len_q, s, e2 + 1, qb, err);
  if (len_i) put_line(start_i, len_i, s, a0, no_cr(txt, a0, e0), err);
}
// the same for an image with one line per unit, taken as it is
__global__ void k_lines_plain(const uint64_t *__restrict__ line_end, uint64_t U, const uint32_t *__restrict__ rec,
                              uint64_t *__restrict__ start, uint32_t *__restrict__ len, uint32_t *__restrict__ err) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s == 0) len[U] = 0;
  if (s >= U) return;
  const uint64_t i = rec ? rec[s] : s;
  put_line(start, len, s, i ? line_end[i - 1] + 1 : 0, line_end[i], err);
}

// ------------------------------------------------------------------ the copy
// the offset of slot s in the output: the key of the copy's searches (copy_words.h)
template <int NL>
struct Offs {
  const uint64_t *__restrict__ off;
  __device__ __forceinline__ uint64_t operator()(uint64_t s) const { return off[s] + (NL ? s : 0); }
};

// out[off[s] + NL * s ..) = line of slot s (+ '\n' when NL), for all slots; total = off[U] + NL * U bytes.
// TAB: every byte b becomes table[b] (b < 128; else ERR_BYTE); changed[CHANGED_SLOTS] together count the bytes that
// differ (one atomic per block, spread over the counters: a single counter serializes the whole grid).
template <int NL, bool TAB>
__global__ __launch_bounds__(256) void k_copy_words(const uint8_t *__restrict__ txt, const uint64_t *__restrict__ start,
                                                    const uint32_t *__restrict__ len, const uint64_t *__restrict__ off,
                                                    const uint32_t *__restrict__ bs, uint64_t total,
                                                    const uint8_t *__restrict__ table, uint8_t *__restrict__ out,
                                                    unsigned long long *__restrict__ changed, uint32_t *__restrict__ err) {
  __shared__ uint8_t tab[128];
  __shared__ uint64_t soff[COPY_LDS_OFFSETS];
  __shared__ uint32_t wave_changed[4];
  if (TAB && threadIdx.x < 128) tab[threadIdx.x] = table[threadIdx.x];
  const Offs<NL> eoff{off};
  const uint64_t p = (uint64_t)blockIdx.x * COPY_BLOCK_BYTES + (uint64_t)threadIdx.x * 16;
  uint64_t s = block_piece(eoff, bs, p, p < total, soff);   // synchronises: tab is there as well
  uint32_t nchanged = 0;
  if (p < total) {
    const uint64_t end = min(p + 16, total);
    uint64_t so = eoff(s), q = p;
    u128 acc = 0;
    while (q < end) {
      const uint32_t l = len[s];
      const uint64_t k = q - so;
      if (k < l) {
        const uint32_t c = (uint32_t)min((uint64_t)l - k, end - q);
        acc |= fetch(txt, start[s] + k, c, ~0ull) << (8 * (uint32_t)(q - p));   // txt is padded: no last word
        q += c;
      } else if (NL && k == l) {
        acc |= (u128)'\n' << (8 * (uint32_t)(q - p));
        q++;
      }
      if (q >= so + l + NL) { so += (uint64_t)l + NL; s++; }   // on to the next slot (it may be empty)
    }
    const uint32_t nb = (uint32_t)(end - p);
    if (TAB) {
      uint32_t w[4] = {(uint32_t)acc, (uint32_t)(acc >> 32), (uint32_t)(acc >> 64), (uint32_t)(acc >> 96)};
      uint32_t bad = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint32_t x = w[i];
        uint32_t r = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) r |= (uint32_t)tab[(x >> (8 * j)) & 127] << (8 * j);
        // the bytes of this dword that belong to the output (all of them but in the last word)
        const uint32_t valid = nb >= 4u * i + 4 ? 0xffffffffu : nb <= 4u * i ? 0u : (1u << (8 * (nb - 4u * i))) - 1;
        const uint32_t d = (r ^ x) & valid;
        nchanged += __popc((((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d) & 0x80808080u);   // nonzero bytes of d
        bad |= x & 0x80808080u;   // bytes past the output are zero
        w[i] = r;
      }
      if (bad) atomicOr(err, ERR_BYTE);
      acc = (u128)w[3] << 96 | (u128)w[2] << 64 | (u128)w[1] << 32 | w[0];
    }
    put16(out, p, nb, acc);
  }
  if (TAB) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nchanged += __shfl_xor(nchanged, o, 64);
    if ((threadIdx.x & 63) == 0) wave_changed[threadIdx.x >> 6] = nchanged;
    __syncthreads();
    const uint32_t c = wave_changed[0] + wave_changed[1] + wave_changed[2] + wave_changed[3];
    if (threadIdx.x == 0 && c) atomicAdd(&changed[blockIdx.x % CHANGED_SLOTS], (unsigned long long)c);
  }
}

// tab[b] = offset of slot min(b * B, U), b = 0 .. nb
__global__ void k_block_table(const uint64_t *__restrict__ off, int nl, uint64_t U, uint64_t B, uint64_t nb,
                              uint64_t *__restrict__ tab) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b > nb) return;
  const uint64_t s = min(b * B, U);
  tab[b] = off[s] + (nl ? s : 0);
}

// ------------------------------------------------------------------ paired ids
// check_id_pattern (util.cpp:220-253); codes 1 and 3 never match an empty id
__device__ bool id_match(int code, const uint8_t *__restrict__ x, const uint8_t *__restrict__ y, uint64_t len) {
  if (code == 2) {
    for (uint64_t i = 0; i < len; i++)
      if (x[i] != y[i]) return false;
    return true;
  }
  if (len == 0) return false;
  if (code == 1) {
    if (x[len - 1] != '1' || y[len - 1] != '2') return false;
    for (uint64_t i = 0; i + 1 < len; i++)
      if (x[i] != y[i]) return false;
    return true;
  }
  uint64_t i = 0;
  for (; i < len; i++) {
    if (x[i] != y[i]) break;
    if (x[i] == ' ') {
      if (i + 1 < len && x[i + 1] == '1' && y[i + 1] == '2') i++;
      else break;
    }
  }
  return i == len;
}
__global__ void k_id_check(const uint8_t *__restrict__ t1, const uint64_t *__restrict__ le1,
                           const uint8_t *__restrict__ t2, const uint64_t *__restrict__ le2, uint64_t nrec, int code,
                           uint32_t *__restrict__ ok) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrec) return;
  const uint64_t a1 = i ? le1[4 * i - 1] + 1 : 0, a2 = i ? le2[4 * i - 1] + 1 : 0;
  const uint64_t b1 = no_cr(t1, a1, le1[4 * i]), b2 = no_cr(t2, a2, le2[4 * i]);
  if (b1 - a1 != b2 - a2 || !id_match(code, t1 + a1, t2 + a2, b1 - a1)) atomicAnd(ok, 0u);
}

// ------------------------------------------------------------------ host side

// A text in HBM with its newline index: line_end[j] = position of the '\n' of line j, nbytes for an unterminated
// last line.  The buffer is padded so that the aligned 16-byte loads of the copy stay inside it.
struct Text {
  DBuf txt, le;
  uint64_t nbytes = 0, nlines = 0;
};
int index_text(int dev, hipStream_t st, const uint8_t *text, size_t nbytes, Text &T, hipEvent_t after_copy) {
  T.nbytes = nbytes;
  T.nlines = 0;
  DALLOC(T.txt, nbytes + 32);
  if (nbytes) HIPCHK(hipMemcpyAsync(T.txt.p, text, nbytes, hipMemcpyHostToDevice, st));
  if (after_copy) HIPCHK(hipEventRecord(after_copy, st));
  if (!nbytes) { DALLOC(T.le, 16); return 0; }
  const uint64_t nblk = (nbytes + sr::NL_CHUNK_BYTES - 1) / sr::NL_CHUNK_BYTES;
  DBuf blk_cnt, blk_off, tmp;
  DALLOC(blk_cnt, nblk * 4); DALLOC(blk_off, nblk * 8);
  size_t tb = 0;
  HIPCHK(sr::excl_scan_u32_to_u64(st, nullptr, tb, nullptr, nullptr, nblk));
  DALLOC(tmp, tb + 16);
  sr::launch_nl_count(st, T.txt.as<uint8_t>(), nbytes, blk_cnt.as<uint32_t>(), nblk);
  HIPCHK(sr::excl_scan_u32_to_u64(st, tmp.p, tb, blk_cnt.as<uint32_t>(), blk_off.as<uint64_t>(), nblk));
  uint64_t last_off = 0;
  uint32_t last_cnt = 0;
  HIPCHK(hipMemcpyAsync(&last_off, blk_off.as<uint64_t>() + (nblk - 1), 8, hipMemcpyDeviceToHost, st));
  HIPCHK(rd(st, &last_cnt, blk_cnt.as<uint32_t>() + (nblk - 1), 4));
  const uint64_t nl = last_off + last_cnt;
  const bool unterminated = text[nbytes - 1] != '\n';
  T.nlines = nl + (unterminated ? 1 : 0);
  DALLOC(T.le, (T.nlines + 1) * 8);
  sr::launch_nl_fill(st, T.txt.as<uint8_t>(), nbytes, blk_off.as<uint64_t>(), T.le.as<uint64_t>(), nblk);
  if (unterminated) {
    const uint64_t e = nbytes;
    HIPCHK(hipMemcpyAsync(T.le.as<uint64_t>() + nl, &e, 8, hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipStreamSynchronize(st));   // the scratch buffers go back to the pool on return
  return 0;
}

}  // namespace

struct spring_qualid_ctx {
  int dev = 0;
  hipStream_t st = nullptr;
  bool have_order = false, pe = false;
  uint32_t num_reads = 0;
  uint64_t U = 0;
  DBuf rec;                // slot -> line (U entries); unset = identity
  bool have = false;       // a result of the last from_* call exists
  bool have_kind[2] = {false, false};
  spring_qualid_info info;
  uint32_t B = 0;          // num_reads_per_block of the result
  DBuf out[2], len[2];
  std::vector<uint64_t> table[2];   // num_blocks + 1 block offsets
};

namespace {

void drop_results(spring_qualid_ctx *ctx) {
  ctx->have = false;
  for (int k = 0; k < 2; k++) { ctx->have_kind[k] = false; ctx->out[k].release(); ctx->len[k].release(); ctx->table[k].clear(); }
  memset(&ctx->info, 0, sizeof(ctx->info));
}

// d_order: device, num_reads entries, or null (identity)
int set_order(spring_qualid_ctx *ctx, const uint32_t *d_order, uint32_t n, bool pe) {
  const int dev = ctx->dev;
  hipStream_t st = ctx->st;
  ctx->have_order = false;
  ctx->rec.release();
  drop_results(ctx);
  if (pe && (n & 1)) return fail(SPRING_REORDER_E_ARG, "paired-end data needs an even num_reads (got %u)", n);
  const uint32_t half = n / 2;
  const uint64_t U = pe ? half : n;
  if (d_order && n) {
    DBuf hits, d_err, pos, tmp;
    DALLOC(hits, (uint64_t)n * 4); DALLOC(d_err, 4);
    HIPCHK(hipMemsetAsync(hits.p, 0, (uint64_t)n * 4, st));
    HIPCHK(hipMemsetAsync(d_err.p, 0, 4, st));
    hipLaunchKernelGGL(k_perm_check, grid(n), dim3(256), 0, st, d_order, n, hits.as<uint32_t>(), d_err.as<uint32_t>());
    uint32_t herr = 0;
    HIPCHK(rd(st, &herr, d_err.p, 4));
    if (herr) return fail(SPRING_REORDER_E_ARG, "read_order.bin is not a permutation of [0, %u)", n);
    DALLOC(ctx->rec, U * 4);
    if (!pe) {
      HIPCHK(hipMemcpyAsync(ctx->rec.p, d_order, (uint64_t)n * 4, hipMemcpyDeviceToDevice, st));
    } else {
      size_t tb = 0;
      HIPCHK(sr::excl_scan_u32(st, nullptr, tb, nullptr, nullptr, n));
      DALLOC(tmp, tb + 16); DALLOC(pos, (uint64_t)n * 4);
      hipLaunchKernelGGL(k_flag_file1, grid(n), dim3(256), 0, st, d_order, n, half, hits.as<uint32_t>());
      HIPCHK(sr::excl_scan_u32(st, tmp.p, tb, hits.as<uint32_t>(), pos.as<uint32_t>(), n));
      hipLaunchKernelGGL(k_rec_pe, grid(n), dim3(256), 0, st, d_order, pos.as<uint32_t>(), n, half,
                         ctx->rec.as<uint32_t>());
    }
    HIPCHK(hipStreamSynchronize(st));
  }
  ctx->num_reads = n; ctx->pe = pe; ctx->U = U;
  ctx->have_order = true;
  return 0;
}

struct Kind {   // per-kind scratch of one run
  DBuf start, off, bs;
  uint64_t total = 0;
};

// text: a FASTQ (fastq = true; want: bit 0 quality, bit 1 id) or one line per read (want has the one bit of its kind)
int run_core(spring_qualid_ctx *ctx, const uint8_t *text, size_t nbytes, bool fastq, int want, const uint8_t *table,
             uint32_t B, spring_qualid_info *info_out) {
  const int dev = ctx->dev;
  hipStream_t st = ctx->st;
  drop_results(ctx);
  if (B == 0) return fail(SPRING_REORDER_E_ARG, "num_reads_per_block must be > 0");
  const uint64_t U = ctx->U;
  Events ev;
  HIPCHK(hipEventCreate(&ev.a)); HIPCHK(hipEventCreate(&ev.b));
  Text T;
  int r = index_text(dev, st, text, nbytes, T, ev.a);
  if (r) return r;
  if (fastq && T.nlines % 4) return fail(SPRING_REORDER_E_ARG, "Invalid FASTQ(A) file. Number of lines not multiple of 4(2)");
  const uint64_t nunits = fastq ? T.nlines / 4 : T.nlines;
  if (nunits != U)
    return fail(SPRING_REORDER_E_ARG, "the input holds %llu %s, the order is for %llu", (unsigned long long)nunits,
                fastq ? "records" : "lines", (unsigned long long)U);
  const uint64_t nb = (U + B - 1) / B;
  spring_qualid_info info;
  memset(&info, 0, sizeof(info));
  info.num_units = U; info.num_blocks = nb;
  DBuf d_err, d_changed, d_table, d_max, d_tab, tmp;
  Kind K[2];
  DALLOC(d_err, 4); DALLOC(d_changed, CHANGED_SLOTS * 8); DALLOC(d_max, 8); DALLOC(d_tab, (nb + 1) * 8);
  HIPCHK(hipMemsetAsync(d_err.p, 0, 4, st));
  HIPCHK(hipMemsetAsync(d_changed.p, 0, CHANGED_SLOTS * 8, st));
  HIPCHK(hipMemsetAsync(d_max.p, 0, 8, st));
  if (table && (want & 1)) {
    DALLOC(d_table, 128);
    HIPCHK(hipMemcpyAsync(d_table.p, table, 128, hipMemcpyHostToDevice, st));
  }
  size_t tb = 0, t2 = 0;
  HIPCHK(sr::excl_scan_u32_to_u64(st, nullptr, tb, nullptr, nullptr, U + 1));
  if (U) HIPCHK(sr::reduce_max_u32(st, nullptr, t2, nullptr, nullptr, U));
  tb = std::max(tb, t2);
  DALLOC(tmp, tb + 16);
  const uint32_t *rec = ctx->rec.as<uint32_t>();
  for (int k = 0; k < 2; k++)
    if (want >> k & 1) { DALLOC(K[k].start, U * 8); DALLOC(K[k].off, (U + 1) * 8); DALLOC(ctx->len[k], (U + 1) * 4); }
  if (fastq)
    hipLaunchKernelGGL(k_lines_fastq, grid(U), dim3(256), 0, st, T.txt.as<uint8_t>(), T.le.as<uint64_t>(), U, rec,
                       K[0].start.as<uint64_t>(), ctx->len[0].as<uint32_t>(), K[1].start.as<uint64_t>(),
                       ctx->len[1].as<uint32_t>(), d_err.as<uint32_t>());
  else
    hipLaunchKernelGGL(k_lines_plain, grid(U), dim3(256), 0, st, T.le.as<uint64_t>(), U, rec,
                       K[want >> 1].start.as<uint64_t>(), ctx->len[want >> 1].as<uint32_t>(), d_err.as<uint32_t>());
  for (int k = 0; k < 2; k++) {
    if (!(want >> k & 1)) continue;
    HIPCHK(sr::excl_scan_u32_to_u64(st, tmp.p, t2 = tb, ctx->len[k].as<uint32_t>(), K[k].off.as<uint64_t>(), U + 1));
    if (U) HIPCHK(sr::reduce_max_u32(st, tmp.p, t2 = tb, ctx->len[k].as<uint32_t>(), d_max.as<uint32_t>() + k, U));
    HIPCHK(hipMemcpyAsync(&K[k].total, K[k].off.as<uint64_t>() + U, 8, hipMemcpyDeviceToHost, st));
  }
  uint32_t herr = 0;
  HIPCHK(rd(st, &herr, d_err.p, 4));
  if (herr & ERR_QLEN) { drop_results(ctx); return fail(SPRING_REORDER_E_ARG, "Read length does not match quality length."); }
  if (herr & ERR_LONG) { drop_results(ctx); return fail(SPRING_REORDER_E_ARG, "a line is longer than 2^32 - 1 bytes"); }
  for (int k = 0; k < 2; k++) {
    if (!(want >> k & 1)) continue;
    const int nl = k == SPRING_QUALID_ID;
    const uint64_t total = K[k].total + (nl ? U : 0);
    DALLOC(ctx->out[k], total + 16);
    if (total) {
      const dim3 g = grid(total, COPY_BLOCK_BYTES);
      const uint64_t nblk = g.x;
      DALLOC(K[k].bs, (nblk + 1) * 4);
      if (nl) hipLaunchKernelGGL(k_block_pieces<Offs<1>>, grid(nblk + 1), dim3(256), 0, st, Offs<1>{K[k].off.as<uint64_t>()}, U, nblk, K[k].bs.as<uint32_t>());
      else hipLaunchKernelGGL(k_block_pieces<Offs<0>>, grid(nblk + 1), dim3(256), 0, st, Offs<0>{K[k].off.as<uint64_t>()}, U, nblk, K[k].bs.as<uint32_t>());
#define COPY(NLV, TABV)                                                                                          \
  hipLaunchKernelGGL((k_copy_words<NLV, TABV>), g, dim3(256), 0, st, T.txt.as<uint8_t>(), K[k].start.as<uint64_t>(), \
                     ctx->len[k].as<uint32_t>(), K[k].off.as<uint64_t>(), K[k].bs.as<uint32_t>(), total, d_table.as<uint8_t>(), \
                     ctx->out[k].as<uint8_t>(), d_changed.as<unsigned long long>(), d_err.as<uint32_t>())
      if (nl) COPY(1, false);
      else if (d_table.p) COPY(0, true);
      else COPY(0, false);
#undef COPY
    }
    hipLaunchKernelGGL(k_block_table, grid(nb + 1), dim3(256), 0, st, K[k].off.as<uint64_t>(), nl, U, (uint64_t)B, nb,
                       d_tab.as<uint64_t>());
    ctx->table[k].assign(nb + 1, 0);
    HIPCHK(rd(st, ctx->table[k].data(), d_tab.p, (nb + 1) * 8));
    info.bytes[k] = total;
  }
  HIPCHK(hipEventRecord(ev.b, st));
  uint32_t mx[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(mx, d_max.p, 8, hipMemcpyDeviceToHost, st));
  std::vector<uint64_t> changed(CHANGED_SLOTS);
  HIPCHK(hipMemcpyAsync(changed.data(), d_changed.p, CHANGED_SLOTS * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(rd(st, &herr, d_err.p, 4));
  for (uint64_t c : changed) info.bytes_changed += c;
  if (herr & ERR_BYTE) {
    drop_results(ctx);
    return fail(SPRING_REORDER_E_ARG, "a quality value >= 128 cannot be binned (the table has 128 entries)");
  }
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
  info.max_len[0] = mx[0]; info.max_len[1] = mx[1];
  info.ms_device = ms;
  ctx->info = info;
  ctx->B = B;
  for (int k = 0; k < 2; k++) ctx->have_kind[k] = (want >> k & 1) != 0;
  ctx->have = true;
  if (info_out) *info_out = info;
  return 0;
}

// the first line of a text without its '\n' and a trailing '\r'
void first_line(const uint8_t *t, size_t n, const uint8_t *&p, size_t &len) {
  const void *e = n ? memchr(t, '\n', n) : nullptr;
  len = e ? (size_t)((const uint8_t *)e - t) : n;
  if (len && t[len - 1] == '\r') len--;
  p = t;
}
bool host_id_match(int code, const uint8_t *x, const uint8_t *y, size_t len) {
  if (code == 2) return len == 0 || memcmp(x, y, len) == 0;
  if (len == 0) return false;
  if (code == 1) return x[len - 1] == '1' && y[len - 1] == '2' && memcmp(x, y, len - 1) == 0;
  size_t i = 0;
  for (; i < len; i++) {
    if (x[i] != y[i]) break;
    if (x[i] == ' ') {
      if (i + 1 < len && x[i + 1] == '1' && y[i + 1] == '2') i++;
      else break;
    }
  }
  return i == len;
}

}  // namespace

extern "C" {

int spring_qualid_create(int device, spring_qualid_ctx **out) {
  if (!out) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  const int r = stage_device(&device, "the quality / id stage");
  if (r) return r;
  spring_qualid_ctx *c = new spring_qualid_ctx();
  c->dev = device;
  memset(&c->info, 0, sizeof(c->info));
  *out = c;
  return 0;
}

void spring_qualid_destroy(spring_qualid_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->dev);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  drop_results(ctx);
  ctx->rec.release();
  if (ctx->st) (void)hipStreamDestroy(ctx->st);
  delete ctx;
}

int spring_qualid_order_from_host(spring_qualid_ctx *ctx, const uint32_t *order, uint32_t num_reads, int32_t paired_end) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  int r = stream_begin(ctx->dev, &ctx->st);
  if (r) return r;
  const int dev = ctx->dev;
  DBuf d_order;
  if (order && num_reads) {
    DALLOC(d_order, (uint64_t)num_reads * 4);
    HIPCHK(hipMemcpyAsync(d_order.p, order, (uint64_t)num_reads * 4, hipMemcpyHostToDevice, ctx->st));
  }
  r = set_order(ctx, d_order.as<uint32_t>(), num_reads, paired_end != 0);
  (void)hipStreamSynchronize(ctx->st);
  return r;
}

int spring_qualid_order_from_encoder(spring_qualid_ctx *ctx, spring_encoder_ctx *enc, uint32_t num_reads,
                                     int32_t paired_end) {
  if (!ctx || !enc) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  sr::EncoderView V;
  int r = sr::encoder_view(enc, &V);
  if (r) return r;
  if (V.dev != ctx->dev) return fail(SPRING_REORDER_E_ARG, "encoder and quality / id contexts live on different devices");
  if ((r = stream_begin(ctx->dev, &ctx->st))) return r;
  if (V.info.n_total != num_reads) {
    ctx->have_order = false;
    drop_results(ctx);
    return fail(SPRING_REORDER_E_ARG, "the encoder holds %llu reads, num_reads is %u", (unsigned long long)V.info.n_total,
                num_reads);
  }
  r = set_order(ctx, num_reads ? V.order : nullptr, num_reads, paired_end != 0);
  (void)hipStreamSynchronize(ctx->st);
  return r;
}

int spring_qualid_from_fastq(spring_qualid_ctx *ctx, const uint8_t *fastq, size_t nbytes, int32_t want,
                             const uint8_t *table, uint32_t num_reads_per_block, spring_qualid_info *info) {
  if (!ctx || (nbytes && !fastq)) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  int r = stream_begin(ctx->dev, &ctx->st);
  if (r) return r;
  drop_results(ctx);
  if (!ctx->have_order) return fail(SPRING_REORDER_E_STATE, "no order set (spring_qualid_order_from_host / _from_encoder)");
  if (want < 1 || want > 3) return fail(SPRING_REORDER_E_ARG, "want: bit 0 quality, bit 1 id (got %d)", want);
  std::vector<uint8_t> unz;
  if ((r = sr::gunzip_if_needed(fastq, nbytes, unz))) return r;
  r = run_core(ctx, fastq, nbytes, true, want, table, num_reads_per_block, info);
  (void)hipStreamSynchronize(ctx->st);
  return r;
}

int spring_qualid_from_lines(spring_qualid_ctx *ctx, int32_t kind, const uint8_t *lines, size_t nbytes,
                             const uint8_t *table, uint32_t num_reads_per_block, spring_qualid_info *info) {
  if (!ctx || (nbytes && !lines)) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  int r = stream_begin(ctx->dev, &ctx->st);
  if (r) return r;
  drop_results(ctx);
  if (!ctx->have_order) return fail(SPRING_REORDER_E_STATE, "no order set (spring_qualid_order_from_host / _from_encoder)");
  if (kind != SPRING_QUALID_QUALITY && kind != SPRING_QUALID_ID) return fail(SPRING_REORDER_E_ARG, "bad kind %d", kind);
  r = run_core(ctx, lines, nbytes, false, 1 << kind, kind == SPRING_QUALID_QUALITY ? table : nullptr,
               num_reads_per_block, info);
  (void)hipStreamSynchronize(ctx->st);
  return r;
}

int spring_qualid_get_info(spring_qualid_ctx *ctx, spring_qualid_info *info) {
  if (!ctx || !info) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "no quality / id blocks computed yet");
  *info = ctx->info;
  return 0;
}

int spring_qualid_download(spring_qualid_ctx *ctx, int32_t kind, uint8_t *bytes, uint32_t *len, uint64_t *block_off) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (kind != SPRING_QUALID_QUALITY && kind != SPRING_QUALID_ID) return fail(SPRING_REORDER_E_ARG, "bad kind %d", kind);
  if (!ctx->have || !ctx->have_kind[kind]) return fail(SPRING_REORDER_E_STATE, "no %s blocks computed yet", kind ? "id" : "quality");
  HIPCHK(hipSetDevice(ctx->dev));
  if (block_off) memcpy(block_off, ctx->table[kind].data(), ctx->table[kind].size() * 8);
  if (bytes && ctx->info.bytes[kind]) HIPCHK(rd(ctx->st, bytes, ctx->out[kind].p, ctx->info.bytes[kind]));
  if (len && ctx->info.num_units) HIPCHK(rd(ctx->st, len, ctx->len[kind].p, ctx->info.num_units * 4));
  return 0;
}

int spring_quality_table(int32_t mode, uint32_t thr, uint32_t high, uint32_t low, uint8_t table[128]) {
  if (!table) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (mode == 1) {   // generate_illumina_binning_table
    static const struct { uint32_t last, to; } bins[] = {{1, 0}, {9, 6}, {19, 15}, {24, 22}, {29, 27}, {34, 33}, {39, 37}, {94, 40}};
    for (uint32_t c = 0; c < 128; c++) {
      uint32_t k = 0;
      while (c > 33 + bins[k].last) k++;
      table[c] = (uint8_t)(33 + bins[k].to);
    }
    return 0;
  }
  if (mode == 2) {   // generate_binary_binning_table
    if (high < thr || low > thr || high < low) return fail(SPRING_REORDER_E_ARG, "Options do not satisfy low <= thr <= high.");
    if (high > 94) return fail(SPRING_REORDER_E_ARG, "binary binning: high must be <= 94 (quality byte 127)");
    for (uint32_t c = 0; c < 128; c++) table[c] = (uint8_t)(c < 33 + thr ? 33 + low : 33 + high);
    return 0;
  }
  return fail(SPRING_REORDER_E_ARG, "quality table mode %d (1 = Illumina binning, 2 = binary)", mode);
}

int spring_id_pattern(const uint8_t *fastq_1, size_t nbytes_1, const uint8_t *fastq_2, size_t nbytes_2, int32_t device,
                      uint8_t *paired_id_code, double *ms_device) {
  if (!paired_id_code || (nbytes_1 && !fastq_1) || (nbytes_2 && !fastq_2)) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  *paired_id_code = 0;
  if (ms_device) *ms_device = 0;
  std::vector<uint8_t> unz[2];
  int r = sr::gunzip_if_needed(fastq_1, nbytes_1, unz[0]);
  if (!r) r = sr::gunzip_if_needed(fastq_2, nbytes_2, unz[1]);
  if (!r) r = stage_device(&device, "the id check");
  if (r) return r;
  const int dev = device;
  HIPCHK(hipSetDevice(dev));
  hipStream_t st = nullptr;   // the null stream
  Events ev;
  HIPCHK(hipEventCreate(&ev.a)); HIPCHK(hipEventCreate(&ev.b));
  Text T[2];
  if ((r = index_text(dev, st, fastq_1, nbytes_1, T[0], nullptr))) return r;
  if ((r = index_text(dev, st, fastq_2, nbytes_2, T[1], nullptr))) return r;
  if (T[0].nlines % 4 || T[1].nlines % 4)
    return fail(SPRING_REORDER_E_ARG, "Invalid FASTQ(A) file. Number of lines not multiple of 4(2)");
  if (T[0].nlines != T[1].nlines) return fail(SPRING_REORDER_E_ARG, "Number of reads in paired files do not match.");
  const uint64_t nrec = T[0].nlines / 4;
  if (!nrec) return 0;
  // find_id_pattern (util.cpp:196-218) on the first pair
  const uint8_t *x, *y;
  size_t lx, ly;
  first_line(fastq_1, nbytes_1, x, lx);
  first_line(fastq_2, nbytes_2, y, ly);
  int code = 0;
  if (lx == ly) {
    if (host_id_match(2, x, y, lx)) code = 2;
    else if (host_id_match(1, x, y, lx)) code = 1;
    else if (host_id_match(3, x, y, lx)) code = 3;
  }
  if (!code) return 0;
  DBuf ok;
  DALLOC(ok, 4);
  const uint32_t one = 1;
  HIPCHK(hipMemcpyAsync(ok.p, &one, 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(ev.a, st));
  hipLaunchKernelGGL(k_id_check, grid(nrec), dim3(256), 0, st, T[0].txt.as<uint8_t>(), T[0].le.as<uint64_t>(),
                     T[1].txt.as<uint8_t>(), T[1].le.as<uint64_t>(), nrec, code, ok.as<uint32_t>());
  HIPCHK(hipEventRecord(ev.b, st));
  uint32_t h = 0;
  HIPCHK(rd(st, &h, ok.p, 4));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
  if (ms_device) *ms_device = ms;
  *paired_id_code = h ? (uint8_t)code : 0;
  return 0;
}

}  // extern "C"

namespace sr {
int qualid_view(spring_qualid_ctx *ctx, QualIdView *v) {
  if (!ctx || !v) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "no quality / id blocks computed yet");
  v->dev = ctx->dev;
  v->info = ctx->info;
  v->num_reads_per_block = ctx->B;
  for (int k = 0; k < 2; k++) {
    v->have[k] = ctx->have_kind[k];
    v->bytes[k] = ctx->out[k].as<uint8_t>();
    v->len[k] = ctx->len[k].as<uint32_t>();
    v->table[k] = ctx->table[k].data();
  }
  return 0;
}
}  // namespace sr
