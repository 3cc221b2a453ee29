// spring_amd/csrc/bsc_frame.hip -- libbsc's bsc_compress blocks and the files of BSC_compress / BSC_str_array_compress
// for a batch of segments in HBM (include/spring_bsc.h).  The stage runs the block sort and the
// QLFC coder on the caller's contexts and then frames what they left on the device:
//
//   1  sums      Adler-32 of every input segment, read in place: one workgroup per tile of 4 KiB (bsc_frame_plan.h),
//                then one workgroup per segment folds its tiles in order
//   2  plan      per block the outcome of bsc_compress's store rule and the lengths of its pieces; per file its header;
//                an exclusive scan (rocPRIM) gives every piece its place; the headers' first 20 bytes, the cut headers
//                and the count bytes go to a small table.  The host reads the total and the four outcome counts
//   3  assembly  the destination-driven copy: one lane per 16-byte word of the output finds its first piece (last_le
//                of copy_words.h) and walks the pieces that overlap it; the loads are its own (absolute addresses)
//   1' sums      Adler-32 of every coded body, from the output; then one lane per block writes the last 8 bytes of its
//                header: the body's sum and the sum of the 24 bytes in front
//
// Every loop on the device is bounded by a count known before it starts; no kernel waits for another lane's result.
#include <algorithm>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "bsc_frame_plan.h"
#include "bwt_internal.h"
#include "copy_words.h"
#include "fastq_out_internal.h"
#include "reorder_internal.h"
#include "spring_bsc.h"
#include "stage_host.h"
#include "streams_internal.h"

using namespace sr;

static_assert(bscf::HEADER == SPRING_BSC_HEADER_BYTES, "spring_bsc.h and bsc_frame_plan.h disagree");
static_assert(bscf::CODED == SPRING_BSC_CODED && bscf::STORED_SMALL == SPRING_BSC_STORED_SMALL &&
                  bscf::STORED_CODER == SPRING_BSC_STORED_CODER && bscf::STORED_NO_GAIN == SPRING_BSC_STORED_NO_GAIN,
              "spring_bsc.h and bsc_frame_plan.h disagree");
static_assert(bscf::BLOCKS == SPRING_BSC_BLOCKS && bscf::BSC_FILE == SPRING_BSC_FILE && bscf::STR_ARRAY == SPRING_BSC_STR_ARRAY,
              "spring_bsc.h and bsc_frame_plan.h disagree");
static_assert(bscf::TILE == 256 * 16, "a tile is one 16-byte word per lane of a workgroup");

namespace {

using bscf::Sum;
using bscf::TILE;

__device__ __forceinline__ uint64_t mn(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t mx(uint64_t a, uint64_t b) { return a > b ? a : b; }

// ------------------------------------------------------------------ 1: segmented Adler-32
// The segments a sum pass walks: segment s is len[s] bytes at base + addr[s]; tfirst[s]: its first tile.
struct Segs {
  const uint64_t *addr, *len;
  const uint64_t *tfirst;   // S + 1
  uint64_t base;
  uint64_t S;
};

// One workgroup per tile, one aligned 16-byte word per lane.  A word that lies inside the segment is one 16-byte load;
// the words at the segment's two ends are read byte by byte, only the bytes that belong to it.  The grid may be larger
// than the number of tiles (the body sums are launched on a bound).
__global__ __launch_bounds__(256) void k_tiles(Segs G, uint2 *__restrict__ tiles) {
  __shared__ uint32_t sh[2][4];
  const uint64_t t = blockIdx.x;
  if (G.S == 0 || t >= G.tfirst[G.S]) return;   // uniform
  const uint64_t s = last_le(G.S, t, G.tfirst);
  const uint64_t A = G.base + G.addr[s], n = G.len[s], tt = t - G.tfirst[s];
  uint64_t lo, hi;
  bscf::tile_range(A, n, tt, &lo, &hi);
  const uint64_t tlo = A + lo, thi = A + hi;                       // the tile's bytes, as addresses
  const uint64_t wa = (A & ~15ull) + tt * TILE + 16 * threadIdx.x;   // this lane's word
  const uint64_t blo = mx(wa, tlo), bhi = mn(wa + 16, thi);
  uint32_t bytes = 0, weighted = 0;
  if (blo < bhi) {
    if (bhi - blo == 16) {
      const uint4 v = *reinterpret_cast<const uint4 *>(wa);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      const uint32_t top = (uint32_t)(thi - wa);   // the weight of the word's first byte
#pragma unroll
      for (int q = 0; q < 16; q++) {
        const uint32_t d = w[q >> 2] >> (8 * (q & 3)) & 0xff;
        bytes += d;
        weighted += (top - q) * d;
      }
    } else {
      for (uint64_t p = blo; p < bhi; p++) {
        const uint32_t d = *reinterpret_cast<const uint8_t *>(p);
        bytes += d;
        weighted += (uint32_t)(thi - p) * d;
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    bytes += __shfl_down(bytes, o);
    weighted += __shfl_down(weighted, o);
  }
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = bytes; sh[1][threadIdx.x >> 6] = weighted; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const Sum r = bscf::tile_sum(sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3], sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3],
                                 (uint32_t)(thi - tlo));
    tiles[t] = make_uint2(r.a, r.b);
  }
}

// One workgroup per segment: every lane folds a run of consecutive tiles, lane 0 folds the 256 runs in order.
__global__ __launch_bounds__(256) void k_fold(Segs G, const uint2 *__restrict__ tiles, uint32_t *__restrict__ sums) {
  __shared__ Sum part[256];
  __shared__ uint64_t plen[256];
  const uint64_t s = blockIdx.x;
  const uint64_t A = G.base + G.addr[s], n = G.len[s], t0 = G.tfirst[s], nt = G.tfirst[s + 1] - t0;
  const uint64_t per = (nt + 255) / 256;
  const uint64_t a = mn(nt, threadIdx.x * per), b = mn(nt, a + per);
  Sum acc{1, 0};
  uint64_t len = 0;
  for (uint64_t t = a; t < b; t++) {
    uint64_t lo, hi;
    bscf::tile_range(A, n, t, &lo, &hi);
    const uint2 v = tiles[t0 + t];
    acc = bscf::combine(acc, Sum{v.x, v.y}, hi - lo);
    len += hi - lo;
  }
  part[threadIdx.x] = acc;
  plen[threadIdx.x] = len;
  __syncthreads();
  if (threadIdx.x == 0) {
    Sum all{1, 0};
    for (int i = 0; i < 256; i++) all = bscf::combine(all, part[i], plen[i]);
    sums[s] = bscf::value(all);
  }
}

// ------------------------------------------------------------------ 2: plan
struct Batch {
  uint64_t S, F;              // blocks (= segments), files
  int framing;
  const uint64_t *off;        // S + 1: the segments' offsets in the batch
  const uint64_t *src;        // S: the device address of a segment's input
  const uint32_t *bfile;      // S: the block's file
  const uint64_t *file_first; // F + 1
  const int32_t *primary, *nidx, *indexes;             // the block sort's
  const uint64_t *coded_src, *coded_off;               // the coder's
  const int32_t *status;
  const uint32_t *sum_in;     // S: Adler-32 of the input
};

struct Pieces {
  uint64_t P;
  uint64_t *len;   // P + 1 (the last one 0); the scan's input
  uint64_t *dst;   // P + 1: offsets in the output; dst[P]: its size
  uint64_t *src;   // P: device addresses
};

struct Plan {
  uint8_t *meta;       // S x META_BYTES
  int32_t *filemeta;   // F: nBlocks
  int32_t *kind;       // S: the outcome
  uint64_t *block_off; // S: the block's header in the output
  uint64_t *file_off;  // F + 1
  uint64_t *body_off, *body_len, *body_tiles;   // S (+ 1): the coded bodies in the output, for the second sum pass
  unsigned long long *totals;   // [0]: bytes of the output, [1 .. 4]: blocks per outcome
};

__device__ __forceinline__ void block_facts(const Batch &B, uint64_t j, uint64_t *n, int *oc, uint64_t *r, uint32_t *k) {
  *n = B.off[j + 1] - B.off[j];
  *r = B.coded_off[j + 1] - B.coded_off[j];
  *k = (uint32_t)B.nidx[j];
  *oc = bscf::outcome(*n, B.status[j], *r, *k);
}

// One lane per block, then one per file: piece lengths and sources, the outcome, the file headers.
__global__ __launch_bounds__(256) void k_plan(Batch B, Pieces Q, Plan L) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  if (i == 0) Q.len[Q.P] = 0;
  if (i < B.S) {
    uint64_t n, r;
    uint32_t k;
    int oc;
    block_facts(B, i, &n, &oc, &r, &k);
    const uint64_t p = bscf::piece_of_block(i, B.bfile[i]);
    bscf::piece_lengths(Q.len + p, B.framing, n, oc, r, k);
    uint8_t *meta = L.meta + i * bscf::META_BYTES;
    Q.src[p + 0] = reinterpret_cast<uint64_t>(meta);
    Q.src[p + 1] = oc == bscf::CODED ? B.coded_src[i] : B.src[i];
    Q.src[p + 2] = reinterpret_cast<uint64_t>(B.indexes + i * SPRING_BWT_MAX_INDEXES);
    Q.src[p + 3] = reinterpret_cast<uint64_t>(meta + bscf::META_COUNT);
    L.kind[i] = oc;
    atomicAdd(&L.totals[1 + oc], 1ull);
  } else if (i < B.S + B.F) {
    const uint64_t f = i - B.S, p = bscf::piece_of_file(f, B.file_first[f]);
    Q.len[p] = bscf::file_header_bytes(B.framing);
    Q.src[p] = reinterpret_cast<uint64_t>(L.filemeta + f);
    L.filemeta[f] = (int32_t)(B.file_first[f + 1] - B.file_first[f]);
  }
}

// Behind the scan.  One lane per block: its meta bytes (cut header, the header's first 20 bytes, the count byte), where
// its header and its body lie.  One lane per file: where it starts.
__global__ __launch_bounds__(256) void k_meta(Batch B, Pieces Q, Plan L) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  if (i == 0) {
    L.file_off[B.F] = Q.dst[Q.P];
    L.totals[0] = Q.dst[Q.P];
    L.body_tiles[B.S] = 0;
  }
  if (i < B.F) L.file_off[i] = Q.dst[bscf::piece_of_file(i, B.file_first[i])];
  if (i >= B.S) return;
  uint64_t n, r;
  uint32_t k;
  int oc;
  block_facts(B, i, &n, &oc, &r, &k);
  const uint32_t f = B.bfile[i], ch = bscf::cut_header_bytes(B.framing);
  uint8_t m[bscf::META_BYTES] = {0};
  bscf::cut_header(m, B.framing, B.off[i] - B.off[B.file_first[f]]);
  bscf::header_front(m + ch, n, oc, r, k, B.primary[i], B.sum_in[i]);
  m[bscf::META_COUNT] = (uint8_t)bscf::kept_indexes(n, k);
  uint32_t *out = reinterpret_cast<uint32_t *>(L.meta + i * bscf::META_BYTES);
  for (uint32_t q = 0; q < bscf::META_BYTES / 4; q++)
    out[q] = m[4 * q] | m[4 * q + 1] << 8 | m[4 * q + 2] << 16 | (uint32_t)m[4 * q + 3] << 24;
  const uint64_t at = Q.dst[bscf::piece_of_block(i, f)] + ch;
  L.block_off[i] = at;
  L.body_off[i] = at + bscf::HEADER;
  L.body_len[i] = oc == bscf::CODED ? bscf::block_bytes(n, oc, r, k) - bscf::HEADER : 0;
  L.body_tiles[i] = bscf::num_tiles(L.body_off[i], L.body_len[i]);   // the output starts at a 16-byte boundary
}

// ------------------------------------------------------------------ 3: assembly
__device__ __forceinline__ void put_byte(uint64_t &lo, uint64_t &hi, uint32_t q, uint64_t d) {
  if (q < 8) lo |= d << (8 * q); else hi |= d << (8 * (q - 8));
}

// One lane per 16-byte word of the output.  It finds the piece its first byte lies in and walks the pieces up to the
// word's end.  Where one piece covers the whole word and the two aligned 16-byte words around the source bytes lie
// inside that piece, they are loaded whole and shifted across the source's misalignment; everything else is byte
// loads of the bytes that exist.  One 16-byte store (the output is padded to whole words).
__global__ __launch_bounds__(256) void k_assemble(Pieces Q, uint64_t total, uint8_t *__restrict__ out) {
  const uint64_t x0 = (blockIdx.x * 256ull + threadIdx.x) * 16;
  if (x0 >= total) return;
  const uint64_t x1 = mn(x0 + 16, total);
  uint64_t p = last_le(Q.P, x0, Q.dst);
  uint64_t lo = 0, hi = 0;
  for (; p < Q.P && Q.dst[p] < x1; p++) {
    const uint64_t d = Q.dst[p], len = Q.len[p];
    const uint64_t a = mx(d, x0), b = mn(d + len, x1);
    if (a >= b) continue;
    const uint64_t src = Q.src[p] + (a - d);   // the address of the byte that goes to a
    if (b - a == 16) {
      const uint64_t o = a - d, sh = src & 15;
      if (sh == 0) {
        const uint4 v = *reinterpret_cast<const uint4 *>(src);
        lo = (uint64_t)v.y << 32 | v.x;
        hi = (uint64_t)v.w << 32 | v.z;
        continue;
      }
      if (o >= sh && o - sh + 32 <= len) {
        const uint4 v = *reinterpret_cast<const uint4 *>(src - sh), w = *reinterpret_cast<const uint4 *>(src - sh + 16);
        const uint64_t q0 = (uint64_t)v.y << 32 | v.x, q1 = (uint64_t)v.w << 32 | v.z;
        const uint64_t q2 = (uint64_t)w.y << 32 | w.x, q3 = (uint64_t)w.w << 32 | w.z;
        if (sh < 8) {
          const uint32_t s = 8 * (uint32_t)sh;
          lo = q0 >> s | q1 << (64 - s);
          hi = q1 >> s | q2 << (64 - s);
        } else if (sh == 8) {
          lo = q1;
          hi = q2;
        } else {
          const uint32_t s = 8 * ((uint32_t)sh - 8);
          lo = q1 >> s | q2 << (64 - s);
          hi = q2 >> s | q3 << (64 - s);
        }
        continue;
      }
    }
    for (uint64_t x = a; x < b; x++) put_byte(lo, hi, (uint32_t)(x - x0), *reinterpret_cast<const uint8_t *>(src + (x - a)));
  }
  *reinterpret_cast<uint4 *>(out + x0) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}

// ------------------------------------------------------------------ 1': the last 8 bytes of every header
__global__ __launch_bounds__(256) void k_headers(Batch B, Plan L, const uint32_t *__restrict__ sum_body, uint8_t *__restrict__ out) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  if (i >= B.S) return;
  uint8_t h[bscf::HEADER];
  const uint8_t *front = L.meta + i * bscf::META_BYTES + bscf::cut_header_bytes(B.framing);
  for (int q = 0; q < 20; q++) h[q] = front[q];
  bscf::header_back(h, L.kind[i] == bscf::CODED ? sum_body[i] : B.sum_in[i]);
  uint8_t *at = out + L.block_off[i];
  for (int q = 20; q < 28; q++) at[q] = h[q];
}

}  // namespace

struct spring_bsc_ctx {
  int dev = 0;
  hipStream_t st = nullptr;
  bool have = false;
  spring_bsc_info info;
  DBuf out;
  std::vector<uint64_t> file_off, block_off, file_first;
  std::vector<int32_t> kind, file_stream;
  std::vector<uint32_t> file_block;
};

namespace {

void drop_result(spring_bsc_ctx *ctx) {
  ctx->have = false;
  ctx->out.release();
  ctx->file_off.clear();
  ctx->block_off.clear();
  ctx->file_first.clear();
  ctx->kind.clear();
  ctx->file_stream.clear();
  ctx->file_block.clear();
  memset(&ctx->info, 0, sizeof(ctx->info));
}

// Adler-32 of S segments: addr / len on the host when the tiles can be counted there (d_tfirst == nullptr), else all
// three arrays are the device's and `bound` is an upper bound of the number of tiles.
int sum_segments(int dev, hipStream_t st, uint64_t S, uint64_t base, const uint64_t *h_addr, const uint64_t *h_len,
                 const uint64_t *d_addr, const uint64_t *d_len, const uint64_t *d_tfirst, uint64_t bound, uint32_t *d_sums) {
  if (S == 0) return 0;
  DBuf a, l, tf, tiles;
  std::vector<uint64_t> tfirst;
  SyncOnExit sync_on_exit{st};
  if (!d_tfirst) {
    tfirst.assign(S + 1, 0);
    for (uint64_t s = 0; s < S; s++) tfirst[s + 1] = tfirst[s] + bscf::num_tiles(base + h_addr[s], h_len[s]);
    bound = tfirst[S];
    DALLOC(a, S * 8); DALLOC(l, S * 8); DALLOC(tf, (S + 1) * 8);
    HIPCHK(hipMemcpyAsync(a.p, h_addr, S * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(l.p, h_len, S * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(tf.p, tfirst.data(), (S + 1) * 8, hipMemcpyHostToDevice, st));
    d_addr = a.as<uint64_t>(); d_len = l.as<uint64_t>(); d_tfirst = tf.as<uint64_t>();
  }
  if (bound >= 0x7fffffffull || S >= 0x7fffffffull) return fail(SPRING_REORDER_E_ARG, "too many tiles or segments to sum");
  DALLOC(tiles, bound * 8);
  const Segs G{d_addr, d_len, d_tfirst, base, S};
  if (bound) hipLaunchKernelGGL(k_tiles, dim3((unsigned)bound), dim3(256), 0, st, G, tiles.as<uint2>());
  hipLaunchKernelGGL(k_fold, dim3((unsigned)S), dim3(256), 0, st, G, tiles.as<uint2>(), d_sums);
  HIPCHK(hipGetLastError());
  return 0;   // sync_on_exit: the uploads and the tiles are read until here
}

// Frames the results the two contexts hold.  src[j]: device address of the input of segment j; file_first / file_stream
// / file_block are already in ctx.
int frame(spring_bsc_ctx *ctx, spring_bwt_ctx *bwt, spring_qlfc_ctx *qlfc, int framing, const std::vector<uint64_t> &src,
          spring_bsc_info *info_out) {
  const int dev = ctx->dev;
  hipStream_t st = ctx->st;
  BwtView V;
  QlfcView C;
  int r = bwt_view(bwt, &V);
  if (r) return r;
  if ((r = qlfc_view(qlfc, &C))) return r;
  const uint64_t S = V.num_segments, F = ctx->file_first.size() - 1;
  if (C.num_segments != S || src.size() != S || ctx->file_first[F] != S)
    return fail(SPRING_REORDER_E_STATE, "the block-sort and QLFC contexts hold %llu and %llu segments, %llu were framed",
                (unsigned long long)S, (unsigned long long)C.num_segments, (unsigned long long)src.size());
  HIPCHK(hipSetDevice(dev));
  spring_bsc_info &I = ctx->info;
  I.num_files = F;
  I.num_blocks = S;
  I.bytes_in = V.bytes;
  std::vector<uint32_t> bfile(S);
  std::vector<uint64_t> len(S);
  for (uint64_t f = 0; f < F; f++)
    for (uint64_t j = ctx->file_first[f]; j < ctx->file_first[f + 1]; j++) bfile[j] = (uint32_t)f;
  for (uint64_t j = 0; j < S; j++) len[j] = V.off[j + 1] - V.off[j];
  const uint64_t P = F + bscf::BLOCK_PIECES * S;
  DBuf d_off, d_src, d_bfile, d_ff, sum_in, sum_body, plen, pdst, psrc, meta, filemeta, kind, block_off, file_off, body_off,
      body_len, body_tiles, body_tfirst, totals, tmp;
  Laps T{st};
  SyncOnExit sync_on_exit{st};
  DALLOC(d_off, (S + 1) * 8); DALLOC(d_src, S * 8); DALLOC(d_bfile, S * 4); DALLOC(d_ff, (F + 1) * 8);
  DALLOC(sum_in, S * 4); DALLOC(sum_body, S * 4);
  DALLOC(plen, (P + 1) * 8); DALLOC(pdst, (P + 1) * 8); DALLOC(psrc, (P + 1) * 8);
  DALLOC(meta, S * bscf::META_BYTES); DALLOC(filemeta, F * 4); DALLOC(kind, S * 4);
  DALLOC(block_off, S * 8); DALLOC(file_off, (F + 1) * 8);
  DALLOC(body_off, S * 8); DALLOC(body_len, S * 8); DALLOC(body_tiles, (S + 1) * 8); DALLOC(body_tfirst, (S + 1) * 8);
  DALLOC(totals, 5 * 8);
  size_t scan_bytes = 0, scan2 = 0;
  HIPCHK(rocprim::exclusive_scan(nullptr, scan_bytes, plen.as<uint64_t>(), pdst.as<uint64_t>(), (uint64_t)0, (size_t)(P + 1),
                                 rocprim::plus<uint64_t>(), st));
  HIPCHK(rocprim::exclusive_scan(nullptr, scan2, body_tiles.as<uint64_t>(), body_tfirst.as<uint64_t>(), (uint64_t)0,
                                 (size_t)(S + 1), rocprim::plus<uint64_t>(), st));
  scan_bytes = std::max(scan_bytes, scan2);
  DALLOC(tmp, scan_bytes + 16);
  HIPCHK(hipMemcpyAsync(d_off.p, V.off, (S + 1) * 8, hipMemcpyHostToDevice, st));
  if (S) HIPCHK(hipMemcpyAsync(d_src.p, src.data(), S * 8, hipMemcpyHostToDevice, st));
  if (S) HIPCHK(hipMemcpyAsync(d_bfile.p, bfile.data(), S * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_ff.p, ctx->file_first.data(), (F + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(totals.p, 0, 5 * 8, st));
  // ---- 1: the inputs' sums
  HIPCHK(T.begin(0));
  if ((r = sum_segments(dev, st, S, 0, src.data(), len.data(), nullptr, nullptr, nullptr, 0, sum_in.as<uint32_t>()))) return r;
  HIPCHK(T.end());
  // ---- 2: plan
  const Batch B{S, F, framing, d_off.as<uint64_t>(), d_src.as<uint64_t>(), d_bfile.as<uint32_t>(), d_ff.as<uint64_t>(),
                V.primary, V.num_indexes, V.indexes, C.d_src, C.d_off, C.d_status, sum_in.as<uint32_t>()};
  const Pieces Q{P, plen.as<uint64_t>(), pdst.as<uint64_t>(), psrc.as<uint64_t>()};
  const Plan L{meta.as<uint8_t>(), filemeta.as<int32_t>(), kind.as<int32_t>(), block_off.as<uint64_t>(), file_off.as<uint64_t>(),
               body_off.as<uint64_t>(), body_len.as<uint64_t>(), body_tiles.as<uint64_t>(), totals.as<unsigned long long>()};
  HIPCHK(T.begin(1));
  hipLaunchKernelGGL(k_plan, grid(S + F), dim3(256), 0, st, B, Q, L);
  size_t sb = scan_bytes;
  HIPCHK(rocprim::exclusive_scan(tmp.p, sb, plen.as<uint64_t>(), pdst.as<uint64_t>(), (uint64_t)0, (size_t)(P + 1),
                                 rocprim::plus<uint64_t>(), st));
  hipLaunchKernelGGL(k_meta, grid(std::max(S, F)), dim3(256), 0, st, B, Q, L);
  sb = scan_bytes;
  HIPCHK(rocprim::exclusive_scan(tmp.p, sb, body_tiles.as<uint64_t>(), body_tfirst.as<uint64_t>(), (uint64_t)0, (size_t)(S + 1),
                                 rocprim::plus<uint64_t>(), st));
  HIPCHK(T.end());
  HIPCHK(hipGetLastError());
  uint64_t h_totals[5];
  HIPCHK(rd(st, h_totals, totals.p, sizeof(h_totals)));
  const uint64_t total = h_totals[0];
  if (h_totals[1] + h_totals[2] + h_totals[3] + h_totals[4] != S || total > V.bytes + (S + F) * 64)
    return fail(SPRING_REORDER_E_STATE, "the plan gave %llu bytes for %llu blocks", (unsigned long long)total, (unsigned long long)S);
  // ---- 3: assembly
  DALLOC(ctx->out, (total + 15) / 16 * 16 + 16);
  uint8_t *out = ctx->out.as<uint8_t>();
  if (reinterpret_cast<uint64_t>(out) & 15) return fail(SPRING_REORDER_E_HIP, "the output buffer is not 16-byte aligned");
  if ((total + 15) / 16 >= 0x7fffffffull * 256) return fail(SPRING_REORDER_E_ARG, "more than 2^42 bytes of output");
  HIPCHK(T.begin(2));
  if (total) hipLaunchKernelGGL(k_assemble, grid((total + 15) / 16), dim3(256), 0, st, Q, total, out);
  HIPCHK(T.end());
  HIPCHK(hipGetLastError());
  // ---- 1': the bodies' sums from the output, then the headers' last 8 bytes
  HIPCHK(T.begin(0));
  if ((r = sum_segments(dev, st, S, reinterpret_cast<uint64_t>(out), nullptr, nullptr, body_off.as<uint64_t>(), body_len.as<uint64_t>(),
                        body_tfirst.as<uint64_t>(), total / TILE + 2 * S + 1, sum_body.as<uint32_t>())))
    return r;
  if (S) hipLaunchKernelGGL(k_headers, grid(S), dim3(256), 0, st, B, L, sum_body.as<uint32_t>(), out);
  HIPCHK(T.end());
  HIPCHK(hipGetLastError());
  ctx->file_off.resize(F + 1);
  ctx->block_off.resize(S);
  ctx->kind.resize(S);
  HIPCHK(rd(st, ctx->file_off.data(), file_off.p, (F + 1) * 8));
  if (S) HIPCHK(rd(st, ctx->block_off.data(), block_off.p, S * 8));
  if (S) HIPCHK(rd(st, ctx->kind.data(), kind.p, S * 4));
  HIPCHK(hipStreamSynchronize(st));
  if ((r = T.collect(I.ms_pass, &I.ms_device))) return r;
  I.bytes_out = total;
  I.coded = h_totals[1 + bscf::CODED];
  I.stored_small = h_totals[1 + bscf::STORED_SMALL];
  I.stored_coder = h_totals[1 + bscf::STORED_CODER];
  I.stored_no_gain = h_totals[1 + bscf::STORED_NO_GAIN];
  ctx->have = true;
  if (info_out) *info_out = I;
  return 0;
}

// What every from_* call starts with: no result, the three contexts on one device, the coder's tables there.
int begin(spring_bsc_ctx *ctx, spring_bwt_ctx *bwt, spring_qlfc_ctx *qlfc) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  (void)hipSetDevice(ctx->dev);
  drop_result(ctx);
  if (!bwt || !qlfc) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  bool tables = false;
  if (bwt_device(bwt) != ctx->dev || qlfc_device(qlfc, &tables) != ctx->dev)
    return fail(SPRING_REORDER_E_ARG, "block-sort, QLFC and framing contexts live on different devices");
  if (!tables) return fail(SPRING_REORDER_E_STATE, "spring_qlfc_set_state_tables has not been called on the QLFC context");
  return stream_begin(ctx->dev, &ctx->st);
}

int finish(spring_bsc_ctx *ctx, int r) {
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  if (r) drop_result(ctx);
  return r;
}

struct Slice {
  int32_t stream;
  uint32_t block;
  const uint8_t *at;   // device: its first byte
  uint64_t bytes;
};

// The files of a batch whose segments are the cuts of (stream, block) slices: one file per slice, in their order.  The
// cuts of a slice are consecutive segments that follow each other in it, so their lengths place them: src[j] is where
// the block sort read segment j.
int group_by_slice(spring_bsc_ctx *ctx, const BwtView &V, const std::vector<Slice> &slices, std::vector<uint64_t> *src) {
  ctx->file_first.assign(1, 0);
  src->resize(V.num_segments);
  uint64_t j = 0;
  for (const Slice &sl : slices) {
    const uint64_t j0 = j;
    for (; j < V.num_segments && V.seg_stream[j] == sl.stream && V.seg_block[j] == sl.block; j++)
      (*src)[j] = reinterpret_cast<uint64_t>(sl.at + (V.off[j] - V.off[j0]));
    if (V.off[j] - V.off[j0] != sl.bytes)
      return fail(SPRING_REORDER_E_STATE, "the block sort's segments of stream %d, block %u hold %llu bytes, the slice %llu", sl.stream,
                  sl.block, (unsigned long long)(V.off[j] - V.off[j0]), (unsigned long long)sl.bytes);
    ctx->file_first.push_back(j);
    ctx->file_stream.push_back(sl.stream);
    ctx->file_block.push_back(sl.block);
  }
  if (j != V.num_segments) return fail(SPRING_REORDER_E_STATE, "the block sort's segments do not follow the slices");
  return 0;
}

int upload_batch(spring_bsc_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const uint64_t *seg_off, uint64_t num_segments,
                 uint64_t max_segment, DBuf *up, std::vector<uint64_t> *src) {
  const int dev = ctx->dev;
  if (nbytes && !bytes) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (num_segments >= 0x7fffffffull) return fail(SPRING_REORDER_E_ARG, "too many segments");
  if (seg_off[0] != 0 || seg_off[num_segments] != nbytes)
    return fail(SPRING_REORDER_E_ARG, "the segment offsets do not start at 0 and end at the %llu bytes", (unsigned long long)nbytes);
  for (uint64_t s = 0; s < num_segments; s++)
    if (seg_off[s + 1] < seg_off[s]) return fail(SPRING_REORDER_E_ARG, "the segment offsets decrease");
  for (uint64_t s = 0; s < num_segments; s++)   // before anything is uploaded
    if (seg_off[s + 1] - seg_off[s] > max_segment)
      return fail(SPRING_REORDER_E_ARG, "a segment of %llu bytes: more than 1 GiB", (unsigned long long)(seg_off[s + 1] - seg_off[s]));
  DALLOC(*up, nbytes + 32);
  if (nbytes) HIPCHK(hipMemcpyAsync(up->p, bytes, nbytes, hipMemcpyHostToDevice, ctx->st));
  src->resize(num_segments);
  for (uint64_t s = 0; s < num_segments; s++) (*src)[s] = reinterpret_cast<uint64_t>(up->as<uint8_t>() + seg_off[s]);
  return 0;
}

}  // namespace

extern "C" {

int spring_bsc_create(int device, spring_bsc_ctx **out) {
  if (!out) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  const int r = stage_device(&device, "the BSC framing stage");
  if (r) return r;
  spring_bsc_ctx *c = new spring_bsc_ctx();
  c->dev = device;
  memset(&c->info, 0, sizeof(c->info));
  *out = c;
  return 0;
}

void spring_bsc_destroy(spring_bsc_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->dev);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  drop_result(ctx);
  if (ctx->st) (void)hipStreamDestroy(ctx->st);
  delete ctx;
}

int spring_bsc_from_streams(spring_bsc_ctx *ctx, spring_bwt_ctx *bwt, spring_qlfc_ctx *qlfc, spring_streams_ctx *streams,
                            uint32_t stream_mask, spring_bsc_info *info) {
  int r = begin(ctx, bwt, qlfc);
  if (r) return r;
  if (!streams) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if ((r = spring_bwt_from_streams(bwt, streams, stream_mask, nullptr))) return r;
  if ((r = spring_qlfc_from_bwt(qlfc, bwt, nullptr))) return r;
  StreamsView SV;
  BwtView V;
  if ((r = streams_view(streams, &SV)) || (r = bwt_view(bwt, &V))) return r;
  const uint64_t nb = SV.info.num_blocks;
  std::vector<Slice> slices;
  for (int s = 0; s < SPRING_STREAMS_NUM; s++)
    if (stream_mask >> s & 1) {
      const uint64_t *tab = SV.table + (uint64_t)s * (nb + 1);
      for (uint64_t b = 0; b < nb; b++) slices.push_back(Slice{s, (uint32_t)b, SV.bytes[s] + tab[b], tab[b + 1] - tab[b]});
    }
  std::vector<uint64_t> src;
  if ((r = group_by_slice(ctx, V, slices, &src))) return finish(ctx, r);
  return finish(ctx, frame(ctx, bwt, qlfc, bscf::BSC_FILE, src, info));
}

int spring_bsc_from_qualid(spring_bsc_ctx *ctx, spring_bwt_ctx *bwt, spring_qlfc_ctx *qlfc, spring_qualid_ctx *q,
                           int32_t kind, uint64_t block_bytes, spring_bsc_info *info) {
  int r = begin(ctx, bwt, qlfc);
  if (r) return r;
  if (!q) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if ((r = spring_bwt_from_qualid(bwt, q, kind, block_bytes, nullptr))) return r;
  if ((r = spring_qlfc_from_bwt(qlfc, bwt, nullptr))) return r;
  QualIdView QV;
  BwtView V;
  if ((r = qualid_view(q, &QV)) || (r = bwt_view(bwt, &V))) return r;
  const int32_t origin = kind == SPRING_QUALID_QUALITY ? SPRING_BWT_SRC_QUALITY : SPRING_BWT_SRC_ID;
  const uint64_t *tab = QV.table[kind];
  std::vector<Slice> slices;
  for (uint64_t b = 0; b < QV.info.num_blocks; b++)
    slices.push_back(Slice{origin, (uint32_t)b, QV.bytes[kind] + tab[b], tab[b + 1] - tab[b]});
  std::vector<uint64_t> src;
  if ((r = group_by_slice(ctx, V, slices, &src))) return finish(ctx, r);
  return finish(ctx, frame(ctx, bwt, qlfc, bscf::STR_ARRAY, src, info));
}

int spring_bsc_from_host(spring_bsc_ctx *ctx, spring_bwt_ctx *bwt, spring_qlfc_ctx *qlfc, const uint8_t *bytes,
                         uint64_t nbytes, const uint64_t *seg_off, uint64_t num_segments, int32_t framing,
                         const uint64_t *file_first, uint64_t num_files, spring_bsc_info *info) {
  int r = begin(ctx, bwt, qlfc);
  if (r) return r;
  if (framing < bscf::BLOCKS || framing > bscf::STR_ARRAY)
    return fail(SPRING_REORDER_E_ARG, "framing must be 0 (blocks), 1 (BSC file) or 2 (string-array file), got %d", framing);
  const uint64_t one[2] = {0, nbytes};
  if (!seg_off) { seg_off = one; num_segments = 1; }
  if (file_first) {
    if (file_first[0] != 0 || file_first[num_files] != num_segments)
      return fail(SPRING_REORDER_E_ARG, "file_first does not start at 0 and end at the %llu segments", (unsigned long long)num_segments);
    for (uint64_t f = 0; f < num_files; f++)
      if (file_first[f + 1] < file_first[f]) return fail(SPRING_REORDER_E_ARG, "file_first decreases");
  }
  DBuf up;
  std::vector<uint64_t> src;
  SyncOnExit sync_on_exit{ctx->st};   // behind up: the input is read until the framing ends
  if ((r = upload_batch(ctx, bytes, nbytes, seg_off, num_segments, SPRING_BWT_MAX_SEGMENT, &up, &src))) return r;
  if ((r = spring_bwt_from_host(bwt, bytes, nbytes, seg_off, num_segments, nullptr))) return r;
  if ((r = spring_qlfc_from_bwt(qlfc, bwt, nullptr))) return r;
  if (file_first) {
    ctx->file_first.assign(file_first, file_first + num_files + 1);
  } else {
    num_files = num_segments;
    ctx->file_first.resize(num_files + 1);
    for (uint64_t f = 0; f <= num_files; f++) ctx->file_first[f] = f;
  }
  ctx->file_stream.assign(num_files, -1);
  ctx->file_block.resize(num_files);
  for (uint64_t f = 0; f < num_files; f++) ctx->file_block[f] = (uint32_t)f;
  return finish(ctx, frame(ctx, bwt, qlfc, framing, src, info));
}

int spring_bsc_get_info(spring_bsc_ctx *ctx, spring_bsc_info *info) {
  if (!ctx || !info) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing framed yet");
  *info = ctx->info;
  return 0;
}

int spring_bsc_download(spring_bsc_ctx *ctx, uint8_t *bytes, uint64_t *file_off, uint64_t *block_off, int32_t *block_kind) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing framed yet");
  HIPCHK(hipSetDevice(ctx->dev));
  const uint64_t S = ctx->info.num_blocks, F = ctx->info.num_files;
  if (file_off) memcpy(file_off, ctx->file_off.data(), (F + 1) * 8);
  if (block_off && S) memcpy(block_off, ctx->block_off.data(), S * 8);
  if (block_kind && S) memcpy(block_kind, ctx->kind.data(), S * 4);
  if (bytes && ctx->info.bytes_out) HIPCHK(rd(ctx->st, bytes, ctx->out.p, ctx->info.bytes_out));
  return 0;
}

int spring_bsc_files(spring_bsc_ctx *ctx, int32_t *stream, uint32_t *block, uint64_t *first_segment) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing framed yet");
  const uint64_t F = ctx->info.num_files;
  if (stream && F) memcpy(stream, ctx->file_stream.data(), F * 4);
  if (block && F) memcpy(block, ctx->file_block.data(), F * 4);
  if (first_segment && F) memcpy(first_segment, ctx->file_first.data(), F * 8);
  return 0;
}

int spring_bsc_adler32(spring_bsc_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const uint64_t *seg_off,
                       uint64_t num_segments, uint32_t *sums) {
  if (!ctx || !sums) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  int r = stream_begin(ctx->dev, &ctx->st);
  if (r) return r;
  const int dev = ctx->dev;
  const uint64_t one[2] = {0, nbytes};
  if (!seg_off) { seg_off = one; num_segments = 1; }
  DBuf up, d_sums;
  std::vector<uint64_t> src, len(num_segments);
  SyncOnExit sync_on_exit{ctx->st};
  if ((r = upload_batch(ctx, bytes, nbytes, seg_off, num_segments, ~0ull, &up, &src))) return r;
  for (uint64_t s = 0; s < num_segments; s++) len[s] = seg_off[s + 1] - seg_off[s];
  DALLOC(d_sums, num_segments * 4);
  if ((r = sum_segments(dev, ctx->st, num_segments, 0, src.data(), len.data(), nullptr, nullptr, nullptr, 0, d_sums.as<uint32_t>())))
    return r;
  if (num_segments) HIPCHK(rd(ctx->st, sums, d_sums.p, num_segments * 4));
  return 0;
}

int spring_bsc_compress(spring_bsc_ctx *ctx, spring_bwt_ctx *bwt, spring_qlfc_ctx *qlfc, const uint8_t *in, uint8_t *out,
                        int32_t n) {
  if (!ctx || n < 0 || !out || (n && !in)) return fail(SPRING_REORDER_E_ARG, "bad argument");
  const int r = spring_bsc_from_host(ctx, bwt, qlfc, in, (uint64_t)n, nullptr, 0, bscf::BLOCKS, nullptr, 0, nullptr);
  if (r) return r;
  if (ctx->info.bytes_out > (uint64_t)n + bscf::HEADER)
    return fail(SPRING_REORDER_E_STATE, "a block of %llu bytes for %d", (unsigned long long)ctx->info.bytes_out, n);
  const int r2 = spring_bsc_download(ctx, out, nullptr, nullptr, nullptr);
  return r2 ? r2 : (int)ctx->info.bytes_out;
}

}  // extern "C"
