// spring_amd/csrc/fastq_out.hip -- the FASTQ text decompress_short finally writes (reference src/decompress.cpp:357-419,
// write_fastq_block of src/util.cpp:56-69, modify_id of src/util.cpp:255-267), assembled on the device from decoded
// reads, quality lines and id lines (include/spring_fastq_out.h).
//
//   newline index of the id lines (fastq_kernels.hip), or the digit counts of numbered ids  ->  per unit: start and
//   length of its id, the offset of the byte modify_id changes, the size of its record  ->  exclusive scan of the sizes
//   (rec_off[])  ->  the record of every 4 KiB of output  ->  the copy.
//
// The copy is the destination-driven copy of copy_words.h with the records as its pieces: a lane owns one
// 16-byte-aligned word of the text and walks the segments id '\n' read '\n' "+\n" quality '\n' of every record that
// overlaps the word.  The three sources are addressed by absolute byte indices from 16-byte-aligned bases, each with
// the limit behind which nothing is read (the decode context's bases have no padding behind them).
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "copy_words.h"
#include "fastq_out_internal.h"
#include "reorder_device.h"
#include "reorder_internal.h"
#include "spring_fastq_out.h"
#include "stage_host.h"

using namespace sr;

namespace {

// error bits of the device checks
constexpr uint32_t ERR_OFF = 1, ERR_LONG = 2, ERR_IDNL = 4, ERR_QTAB = 8, ERR_ITAB = 16, ERR_ID1 = 32, ERR_ID3 = 64;
const char *const ERR_TEXT[7] = {"the read offsets do not start at 0 or decrease",
                                 "a read or an id is longer than 2^30 bytes",
                                 "the id lines do not end in a newline",
                                 "the quality block table does not match the read lengths of its blocks",
                                 "the id block table does not match the lines of its blocks",
                                 "paired id code 1 on an empty id",
                                 "paired id code 3 on an id without a space, or with its first space at the end"};
constexpr uint64_t MAX_LINE = 1ull << 30;
constexpr uint32_t NO_PATCH = 0xffffffffu;
constexpr int NUMBERED_MAX = 13;         // '@' + 10 digits + '/' + mate

// A source of bytes on the device: t is 16-byte aligned, the window's bytes are t[lo, lo + n), and t[0, limit) exists.
struct Src {
  const uint8_t *t = nullptr;
  uint64_t lo = 0, n = 0, limit = 0;
};

// ------------------------------------------------------------------ lines
struct LinesArg {
  const uint64_t *roff;    // nu + 1 read offsets of the window
  uint64_t nu, r0, r1;     // units of the window, the range
  const uint8_t *idt;      // stored ids: the text ...
  const uint64_t *le;      // ... and le[u] = index in idt of the '\n' of line u
  uint64_t id_lo, id_n;
  uint64_t g0;             // global slot of unit 0
  int numbered, code, quality;
  uint64_t *idstart;       // from here on indexed by u - r0
  uint32_t *idlen, *patch, *recsz;
};
__device__ __forceinline__ uint32_t digits_of(uint64_t v) {
  uint32_t d = 1;
  while (v >= 10) { v /= 10; d++; }
  return d;
}
// One thread per unit of the window: the checks for all of them, the id start / length, the patch offset of modify_id
// and the record size for those of the range.
__global__ void k_lines(LinesArg A, uint32_t *__restrict__ err) {
  const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t n = A.r1 - A.r0;
  if (u == 0) {
    A.idlen[n] = 0;
    A.recsz[n] = 0;
    if (A.roff[0] != 0) atomicOr(err, ERR_OFF);
    if (!A.numbered && A.id_n && A.idt[A.id_lo + A.id_n - 1] != '\n') atomicOr(err, ERR_IDNL);
  }
  if (u >= A.nu) return;
  uint32_t bad = 0;
  const uint64_t a = A.roff[u], b = A.roff[u + 1];
  uint64_t rl = b - a;
  if (b < a) { bad |= ERR_OFF; rl = 0; }
  if (rl > MAX_LINE) { bad |= ERR_LONG; rl = 0; }
  uint64_t s = 0, idl;
  uint32_t pk = NO_PATCH;
  if (A.numbered) {
    idl = 3 + digits_of(A.g0 + u + 1);
  } else {
    s = u ? A.le[u - 1] + 1 : A.id_lo;
    idl = A.le[u] - s;
    if (idl > MAX_LINE) { bad |= ERR_LONG; idl = 0; }
    if (A.code == 1) {          // id.back() = '2'
      if (idl == 0) bad |= ERR_ID1;
      else pk = (uint32_t)idl - 1;
    } else if (A.code == 3) {   // while (id[i] != ' ') i++; id[i + 1] = '2'
      uint64_t i = 0;
      while (i < idl && A.idt[s + i] != ' ') i++;
      if (i + 1 >= idl) bad |= ERR_ID3;
      else pk = (uint32_t)i + 1;
    }
  }
  if (bad) atomicOr(err, bad);
  if (u < A.r0 || u >= A.r1) return;
  const uint64_t i = u - A.r0;
  A.idstart[i] = s;
  A.idlen[i] = (uint32_t)idl;
  A.patch[i] = pk;
  A.recsz[i] = (uint32_t)(idl + rl + 2 + (A.quality ? rl + 3 : 0));
}

// numbered ids written out: "@" + decimal(g + 1) + "/" + decimal(mate + 1) at idstart[i] (the scan of idlen)
__global__ void k_numbered(const uint64_t *__restrict__ idstart, const uint32_t *__restrict__ idlen, uint64_t n,
                           uint64_t g_first, int mate, uint8_t *__restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t *o = out + idstart[i];
  const uint32_t l = idlen[i];
  uint64_t v = g_first + i + 1;
  o[0] = '@';
  for (uint32_t k = l - 3; k >= 1; k--) { o[k] = (uint8_t)('0' + v % 10); v /= 10; }
  o[l - 2] = '/';
  o[l - 1] = (uint8_t)('1' + mate);
}

// Block b of the window starts at unit min(b * B, nu): the quality table must be the read offsets there, the id table
// the start of that line.  qtab / itab: nb + 1 entries each, or null.
__global__ void k_tables(const uint64_t *__restrict__ qtab, const uint64_t *__restrict__ itab,
                         const uint64_t *__restrict__ roff, const uint64_t *__restrict__ le, uint64_t id_lo, uint64_t nu,
                         uint64_t B, uint64_t nb, uint32_t *__restrict__ err) {
  const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b > nb) return;
  const uint64_t s = min(b * B, nu);
  if (qtab && qtab[b] - qtab[0] != roff[s]) atomicOr(err, ERR_QTAB);
  if (itab && itab[b] - itab[0] != (s ? le[s - 1] + 1 - id_lo : 0)) atomicOr(err, ERR_ITAB);
}

// ------------------------------------------------------------------ the copy
struct CopyArg {
  Src id, bases, qual;       // id.lo is not used: idstart[] are indices into id.t
  const uint64_t *roff;      // read offsets from the first unit of the range on (n + 1)
  const uint64_t *idstart;
  const uint32_t *idlen, *patch;
  const uint64_t *rec_off;   // n + 1
  const uint32_t *bs;
  uint64_t n, total;
  uint8_t *out;
};

// k_assemble's own search, the largest r in [lo, hi] with off[r] <= p (off[lo] is): last_le of copy_words.h without the
// step counter, which costs this kernel 0.04 ms of its 11.7 at 20 M records (profiles/copy_words_before_after.txt).  It
// ends because hi - lo at least halves with every step.
template <class I>
__device__ __forceinline__ I find_rec(const uint64_t *__restrict__ off, uint64_t p, I lo, I hi) {
  while (lo < hi) {
    const I mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= p) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// out[rec_off[i] ..) = id '\n' read '\n' (Q: '+' '\n' quality '\n') of unit i, for all units of the range.
template <bool Q>
__global__ __launch_bounds__(256) void k_assemble(CopyArg A) {
  __shared__ uint64_t soff[COPY_LDS_OFFSETS];
  // block_piece of copy_words.h with find_rec as its search: the records this block's 4 KiB of output fall into go to
  // LDS, where every lane looks up its own; more of them than fit there are searched in memory
  const uint64_t s_lo = A.bs[blockIdx.x], s_hi = A.bs[blockIdx.x + 1];
  const uint64_t cnt = s_hi - s_lo + 1;
  const bool in_lds = cnt <= COPY_LDS_OFFSETS;
  if (in_lds)
    for (uint32_t t = threadIdx.x; t < cnt; t += 256) soff[t] = A.rec_off[s_lo + t];
  __syncthreads();
  const uint64_t p = (uint64_t)blockIdx.x * COPY_BLOCK_BYTES + (uint64_t)threadIdx.x * 16;
  if (p >= A.total) return;
  const uint64_t end = min(p + 16, A.total);
  uint64_t r = in_lds ? s_lo + find_rec<uint32_t>(soff, p, 0, (uint32_t)cnt - 1) : find_rec<uint64_t>(A.rec_off, p, s_lo, s_hi);
  uint64_t ro = A.rec_off[r], q = p;
  u128 acc = 0;
  while (q < end) {   // a record is at least two bytes: at most eight of them meet a word
    const uint64_t idl = A.idlen[r], ra = A.roff[r], rl = A.roff[r + 1] - ra;
    const uint64_t b1 = idl, b2 = b1 + 1, b3 = b2 + rl, b4 = b3 + 1;       // ends of id, '\n', read, '\n'
    const uint64_t b5 = b4 + 2, b6 = b5 + rl, size = Q ? b6 + 1 : b4;      // ends of "+\n", quality; the record
    uint64_t k = q - ro;
    while (q < end && k < size) {
      const uint64_t left = end - q;
      uint32_t c = 1;
      u128 v = '\n';
      if (k < b1) {
        c = (uint32_t)min(b1 - k, left);
        v = fetch(A.id.t, A.idstart[r] + k, c, A.id.limit);
        const uint64_t pk = A.patch[r];   // modify_id: one byte of the id becomes '2'
        if (pk != NO_PATCH && pk >= k && pk < k + c) {
          const uint32_t s = 8 * (uint32_t)(pk - k);
          v = (v & ~((u128)0xff << s)) | ((u128)'2' << s);
        }
      } else if (k >= b2 && k < b3) {
        c = (uint32_t)min(b3 - k, left);
        v = fetch(A.bases.t, A.bases.lo + ra + (k - b2), c, A.bases.limit);
      } else if (Q && k == b4) {
        v = '+';
      } else if (Q && k >= b5 && k < b6) {
        c = (uint32_t)min(b6 - k, left);
        v = fetch(A.qual.t, A.qual.lo + ra + (k - b5), c, A.qual.limit);
      }   // else: one of the newlines
      acc |= v << (8 * (uint32_t)(q - p));
      q += c;
      k += c;
    }
    ro += size;
    r++;
  }
  put16(A.out, p, (uint32_t)(end - p), acc);
}

// ------------------------------------------------------------------ host side

// the window's geometry (as the decoder's); -> 0 or E_ARG
int window(uint32_t first_block, uint32_t num_blocks, uint32_t N, bool pe, uint32_t B, uint64_t *U_out, uint64_t *nu) {
  if (B == 0) return fail(SPRING_REORDER_E_ARG, "num_reads_per_block must be > 0");
  if (pe && (N & 1)) return fail(SPRING_REORDER_E_ARG, "paired-end data needs an even num_reads (got %u)", N);
  const uint64_t U = pe ? N / 2 : N, total = (U + B - 1) / B;
  if ((uint64_t)first_block + num_blocks > total)
    return fail(SPRING_REORDER_E_ARG, "blocks [%u, %llu) outside the file's %llu blocks", first_block,
                (unsigned long long)first_block + num_blocks, (unsigned long long)total);
  const uint64_t u0 = (uint64_t)first_block * B, u1 = std::min<uint64_t>(((uint64_t)first_block + num_blocks) * B, U);
  *U_out = U;
  *nu = u1 > u0 ? u1 - u0 : 0;
  return 0;
}

// a host block table of the window: starts at 0, monotone, spans the bytes
int check_table(const uint64_t *t, uint32_t nb, uint64_t bytes, const char *what) {
  if (t[0] != 0 || t[nb] != bytes)
    return fail(SPRING_REORDER_E_ARG, "the %s block table does not span its %llu bytes", what, (unsigned long long)bytes);
  for (uint32_t b = 0; b < nb; b++)
    if (t[b + 1] < t[b]) return fail(SPRING_REORDER_E_ARG, "the %s block table is not monotone", what);
  return 0;
}

}  // namespace

struct spring_fastq_out_ctx {
  int dev = 0;
  hipStream_t st = nullptr;
  bool have = false;
  spring_fastq_out_info info;
  DBuf text, rec_off;
};

namespace {

void drop_result(spring_fastq_out_ctx *ctx) {
  ctx->have = false;
  ctx->text.release();
  ctx->rec_off.release();
  memset(&ctx->info, 0, sizeof(ctx->info));
}

// n host bytes into a device buffer at the host pointer's own offset inside a 16-byte word, so that the copy meets the
// misalignment the caller's buffer has; the bytes before them are zero, 16 bytes of padding follow
int upload(int dev, hipStream_t st, const void *host, uint64_t n, DBuf &buf, Src &S) {
  const uint64_t lo = (uint64_t)((uintptr_t)host & 15);
  DALLOC(buf, lo + n + 32);
  HIPCHK(hipMemsetAsync(buf.p, 0, 16, st));
  if (n) HIPCHK(hipMemcpyAsync(buf.as<uint8_t>() + lo, host, n, hipMemcpyHostToDevice, st));
  S.t = buf.as<uint8_t>(); S.lo = lo; S.n = n; S.limit = lo + n;
  return 0;
}

// the newline index of t[0, nbytes): *nl newlines, le[k] = index of the k-th
int index_lines(int dev, hipStream_t st, const uint8_t *t, uint64_t nbytes, DBuf &le, uint64_t *nl) {
  *nl = 0;
  if (!nbytes) { DALLOC(le, 16); return 0; }
  const uint64_t nblk = (nbytes + sr::NL_CHUNK_BYTES - 1) / sr::NL_CHUNK_BYTES;
  DBuf blk_cnt, blk_off, tmp;
  DALLOC(blk_cnt, nblk * 4); DALLOC(blk_off, nblk * 8);
  size_t tb = 0;
  HIPCHK(sr::excl_scan_u32_to_u64(st, nullptr, tb, nullptr, nullptr, nblk));
  DALLOC(tmp, tb + 16);
  sr::launch_nl_count(st, t, nbytes, blk_cnt.as<uint32_t>(), nblk);
  HIPCHK(sr::excl_scan_u32_to_u64(st, tmp.p, tb, blk_cnt.as<uint32_t>(), blk_off.as<uint64_t>(), nblk));
  uint64_t last_off = 0;
  uint32_t last_cnt = 0;
  HIPCHK(hipMemcpyAsync(&last_off, blk_off.as<uint64_t>() + (nblk - 1), 8, hipMemcpyDeviceToHost, st));
  HIPCHK(rd(st, &last_cnt, blk_cnt.as<uint32_t>() + (nblk - 1), 4));
  *nl = last_off + last_cnt;
  DALLOC(le, (*nl + 1) * 8);
  sr::launch_nl_fill(st, t, nbytes, blk_off.as<uint64_t>(), le.as<uint64_t>(), nblk);
  HIPCHK(hipStreamSynchronize(st));   // the scratch buffers go back to the pool on return
  return 0;
}

int assemble(spring_fastq_out_ctx *ctx, const spring_fastq_out_params &P, const spring_fastq_out_sources &S,
             spring_fastq_out_info *info_out) {
  const int dev = ctx->dev;
  const bool pe = P.paired_end != 0, Q = P.preserve_quality != 0;
  const uint32_t B = P.num_reads_per_block, nb = P.num_blocks, fb = P.first_block;
  // ---- everything that is refused before any allocation
  if (P.mate < 0 || P.mate > 1) return fail(SPRING_REORDER_E_ARG, "bad mate %d", P.mate);
  if (P.id_mode < SPRING_FASTQ_OUT_ID_STORED || P.id_mode > SPRING_FASTQ_OUT_ID_FROM_MATE_1)
    return fail(SPRING_REORDER_E_ARG, "bad id_mode %d", P.id_mode);
  const bool numbered = P.id_mode == SPRING_FASTQ_OUT_ID_NUMBERED;
  const int code = P.id_mode == SPRING_FASTQ_OUT_ID_FROM_MATE_1 ? P.paired_id_code : 0;
  const bool have_reads = S.decode || S.read_off, have_ids = S.id_ctx || S.ids || S.id_bytes || S.id_block_off;
  const bool have_qual = S.quality_ctx || S.quality || S.quality_bytes || S.quality_block_off;
  if (!have_reads) return fail(SPRING_REORDER_E_STATE, "no reads given (a decode context, or bases and read offsets)");
  sr::DecodeView DV;
  sr::QualIdView QV[2];   // [0] the quality source, [1] the id source
  int r;
  if (S.decode && (r = sr::decode_view(S.decode, &DV))) return r;
  if (Q && S.quality_ctx) {
    if ((r = sr::qualid_view(S.quality_ctx, &QV[0]))) return r;
    if (!QV[0].have[SPRING_QUALID_QUALITY]) return fail(SPRING_REORDER_E_STATE, "the quality context holds no quality blocks");
  }
  if (!numbered && S.id_ctx) {
    if ((r = sr::qualid_view(S.id_ctx, &QV[1]))) return r;
    if (!QV[1].have[SPRING_QUALID_ID]) return fail(SPRING_REORDER_E_STATE, "the id context holds no id blocks");
  }
  if (P.mate == 1 && (!pe || (S.decode && !DV.paired_end)))
    return fail(SPRING_REORDER_E_ARG, "mate 1 of single-end data");
  if (S.decode && DV.paired_end != pe) return fail(SPRING_REORDER_E_ARG, "the decode is %s-end, the call is not", pe ? "single" : "paired");
  if (numbered && have_ids) return fail(SPRING_REORDER_E_ARG, "stored ids given together with numbered ids");
  if (!numbered && !have_ids) return fail(SPRING_REORDER_E_ARG, "no id source (and ids are not numbered)");
  if (Q && !have_qual) return fail(SPRING_REORDER_E_ARG, "preserve_quality without a quality source");
  if (P.id_mode == SPRING_FASTQ_OUT_ID_FROM_MATE_1 && P.mate != 1)
    return fail(SPRING_REORDER_E_ARG, "ids from mate 1 are for mate 1 (file 2) only");
  if (P.id_mode == SPRING_FASTQ_OUT_ID_FROM_MATE_1 && (code < 1 || code > 3))
    return fail(SPRING_REORDER_E_ARG, "Invalid paired id code %d", P.paired_id_code);
  uint64_t U = 0, nu = 0;
  if ((r = window(fb, nb, P.num_reads, pe, B, &U, &nu))) return r;
  if (S.decode) {
    if (DV.dev != dev) return fail(SPRING_REORDER_E_ARG, "decode and assembler contexts live on different devices");
    if (DV.info.first_block != fb || DV.info.num_blocks != nb || DV.info.num_units != nu)
      return fail(SPRING_REORDER_E_ARG, "the decode holds blocks [%llu, %llu) with %llu units, the call asks for [%u, %llu) with %llu",
                  (unsigned long long)DV.info.first_block, (unsigned long long)(DV.info.first_block + DV.info.num_blocks),
                  (unsigned long long)DV.info.num_units, fb, (unsigned long long)fb + nb, (unsigned long long)nu);
  }
  for (int k = 0; k < 2; k++) {
    if (k == 0 ? !(Q && S.quality_ctx) : !(!numbered && S.id_ctx)) continue;
    if (QV[k].dev != dev) return fail(SPRING_REORDER_E_ARG, "quality / id and assembler contexts live on different devices");
    if (QV[k].info.num_units != U || QV[k].num_reads_per_block != B)
      return fail(SPRING_REORDER_E_ARG, "the %s context holds %llu units in blocks of %u, the file has %llu in blocks of %u",
                  k ? "id" : "quality", (unsigned long long)QV[k].info.num_units, QV[k].num_reads_per_block,
                  (unsigned long long)U, B);
  }
  const uint64_t r0 = P.range_start, r1 = P.range_end == SPRING_FASTQ_OUT_TO_END ? nu : P.range_end;
  if (r0 > r1 || r1 > nu)
    return fail(SPRING_REORDER_E_ARG, "units [%llu, %llu) outside the window's %llu", (unsigned long long)r0,
                (unsigned long long)r1, (unsigned long long)nu);
  const uint64_t n = r1 - r0;
  if (!S.decode && !S.bases && S.read_off[nu]) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (Q && !S.quality_ctx) {
    if (S.quality_bytes && !S.quality) return fail(SPRING_REORDER_E_ARG, "NULL argument");
    if (S.quality_block_off && (r = check_table(S.quality_block_off, nb, S.quality_bytes, "quality"))) return r;
  }
  if (!numbered && !S.id_ctx) {
    if (S.id_bytes && !S.ids) return fail(SPRING_REORDER_E_ARG, "NULL argument");
    if (S.id_block_off && (r = check_table(S.id_block_off, nb, S.id_bytes, "id"))) return r;
  }
  // ---- the sources on the device
  if ((r = stream_begin(ctx->dev, &ctx->st))) return r;
  hipStream_t st = ctx->st;
  Events ev;
  HIPCHK(hipEventCreate(&ev.a)); HIPCHK(hipEventCreate(&ev.b));
  DBuf up_bases, up_roff, up_qual, up_ids, d_qtab, d_itab, numbered_ids, le_buf, d_err, idstart, idlen, patch, recsz, tmp, bs;
  SyncOnExit sync_on_exit{st};
  Src bases, qual, ids;
  const uint64_t *roff = nullptr;
  const uint64_t *h_qtab = nullptr, *h_itab = nullptr;   // host tables of the window (nb + 1), or none
  if (S.decode) {
    bases.t = DV.bases[P.mate]; bases.n = bases.limit = DV.info.bases[P.mate];
    roff = DV.read_off[P.mate];
  } else {
    if ((r = upload(dev, st, S.bases, S.read_off[nu], up_bases, bases))) return r;
    DALLOC(up_roff, (nu + 1) * 8);
    HIPCHK(hipMemcpyAsync(up_roff.p, S.read_off, (nu + 1) * 8, hipMemcpyHostToDevice, st));
    roff = up_roff.as<uint64_t>();
  }
  if (Q) {
    if (S.quality_ctx) {
      h_qtab = QV[0].table[SPRING_QUALID_QUALITY] + fb;
      qual.t = QV[0].bytes[SPRING_QUALID_QUALITY]; qual.lo = h_qtab[0]; qual.n = h_qtab[nb] - h_qtab[0];
      qual.limit = QV[0].info.bytes[SPRING_QUALID_QUALITY];
    } else {
      if ((r = upload(dev, st, S.quality, S.quality_bytes, up_qual, qual))) return r;
      h_qtab = S.quality_block_off;
    }
    if (qual.n != bases.n)
      return fail(SPRING_REORDER_E_ARG, "the quality lines hold %llu bytes, the reads %llu", (unsigned long long)qual.n,
                  (unsigned long long)bases.n);
  }
  if (!numbered) {
    if (S.id_ctx) {
      h_itab = QV[1].table[SPRING_QUALID_ID] + fb;
      ids.t = QV[1].bytes[SPRING_QUALID_ID]; ids.lo = h_itab[0]; ids.n = h_itab[nb] - h_itab[0];
      ids.limit = QV[1].info.bytes[SPRING_QUALID_ID];
    } else {
      if ((r = upload(dev, st, S.ids, S.id_bytes, up_ids, ids))) return r;
      h_itab = S.id_block_off;
    }
  }
  if (h_qtab) {
    DALLOC(d_qtab, ((uint64_t)nb + 1) * 8);
    HIPCHK(hipMemcpyAsync(d_qtab.p, h_qtab, ((uint64_t)nb + 1) * 8, hipMemcpyHostToDevice, st));
  }
  if (h_itab) {
    DALLOC(d_itab, ((uint64_t)nb + 1) * 8);
    HIPCHK(hipMemcpyAsync(d_itab.p, h_itab, ((uint64_t)nb + 1) * 8, hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipEventRecord(ev.a, st));
  // ---- the id lines: a newline index from the 16-byte word the window's ids start in.  The bytes of that word
  // before the window belong to the block before it (a context's whole-file buffer): their newlines are skipped.
  const uint64_t *le = nullptr;
  if (!numbered) {
    const uint64_t A0 = ids.lo & ~15ull;
    ids.t += A0; ids.lo -= A0; ids.limit -= A0;
    uint64_t nl = 0, skip = 0;
    if ((r = index_lines(dev, st, ids.t, ids.lo + ids.n, le_buf, &nl))) return r;
    if (S.id_ctx && ids.lo) {
      uint8_t head[16];
      HIPCHK(rd(st, head, ids.t, ids.lo));
      for (uint64_t i = 0; i < ids.lo; i++) skip += head[i] == '\n';
    }
    if (nl - skip != nu)
      return fail(SPRING_REORDER_E_ARG, "the ids hold %llu lines, the window %llu units", (unsigned long long)(nl - skip),
                  (unsigned long long)nu);
    le = le_buf.as<uint64_t>() + skip;
  }
  // ---- lines, tables, record offsets
  DALLOC(d_err, 4);
  HIPCHK(hipMemsetAsync(d_err.p, 0, 4, st));
  DALLOC(idstart, (n + 1) * 8); DALLOC(idlen, (n + 1) * 4); DALLOC(patch, (n + 1) * 4); DALLOC(recsz, (n + 1) * 4);
  DALLOC(ctx->rec_off, (n + 1) * 8);
  size_t tb = 0;
  HIPCHK(sr::excl_scan_u32_to_u64(st, nullptr, tb, nullptr, nullptr, n + 1));
  DALLOC(tmp, tb + 16);
  const uint64_t g0 = (uint64_t)fb * B;
  LinesArg L;
  L.roff = roff; L.nu = nu; L.r0 = r0; L.r1 = r1; L.idt = ids.t; L.le = le; L.id_lo = ids.lo; L.id_n = ids.n; L.g0 = g0;
  L.numbered = numbered; L.code = code; L.quality = Q;
  L.idstart = idstart.as<uint64_t>(); L.idlen = idlen.as<uint32_t>(); L.patch = patch.as<uint32_t>();
  L.recsz = recsz.as<uint32_t>();
  hipLaunchKernelGGL(k_lines, grid(nu), dim3(256), 0, st, L, d_err.as<uint32_t>());
  if (d_qtab.p || d_itab.p)
    hipLaunchKernelGGL(k_tables, grid((uint64_t)nb + 1), dim3(256), 0, st, d_qtab.as<uint64_t>(), d_itab.as<uint64_t>(), roff,
                       le, ids.lo, nu, (uint64_t)B, (uint64_t)nb, d_err.as<uint32_t>());
  if (numbered) {   // the ids written out, so that the copy has one path
    size_t t2 = tb;
    HIPCHK(sr::excl_scan_u32_to_u64(st, tmp.p, t2, idlen.as<uint32_t>(), idstart.as<uint64_t>(), n + 1));
    DALLOC(numbered_ids, n * NUMBERED_MAX + 16);
    if (n) hipLaunchKernelGGL(k_numbered, grid(n), dim3(256), 0, st, idstart.as<uint64_t>(), idlen.as<uint32_t>(), n, g0 + r0,
                              P.mate, numbered_ids.as<uint8_t>());
    ids.t = numbered_ids.as<uint8_t>(); ids.lo = 0; ids.limit = n * NUMBERED_MAX;
  }
  {
    size_t t2 = tb;
    HIPCHK(sr::excl_scan_u32_to_u64(st, tmp.p, t2, recsz.as<uint32_t>(), ctx->rec_off.as<uint64_t>(), n + 1));
  }
  uint64_t total = 0;
  uint32_t herr = 0;
  HIPCHK(hipMemcpyAsync(&total, ctx->rec_off.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(rd(st, &herr, d_err.p, 4));   // the one look at the error word: the copy below adds nothing to it
  if (herr) {
    drop_result(ctx);
    std::string msg;
    for (int k = 0; k < 7; k++)
      if (herr & (1u << k)) msg += std::string(msg.empty() ? "" : "; ") + ERR_TEXT[k];
    return fail(SPRING_REORDER_E_ARG, "refused: %s", msg.c_str());
  }
  // ---- the copy
  DALLOC(ctx->text, total + 16);
  if (total) {
    const dim3 g = grid(total, COPY_BLOCK_BYTES);
    const uint64_t nblk = g.x;
    DALLOC(bs, (nblk + 1) * 4);
    hipLaunchKernelGGL(k_block_pieces<ArrayKey<uint64_t>>, grid(nblk + 1), dim3(256), 0, st,
                       ArrayKey<uint64_t>{ctx->rec_off.as<uint64_t>()}, n, nblk, bs.as<uint32_t>());
    CopyArg C;
    C.id = ids; C.bases = bases; C.qual = qual;
    C.roff = roff + r0; C.idstart = idstart.as<uint64_t>(); C.idlen = idlen.as<uint32_t>(); C.patch = patch.as<uint32_t>();
    C.rec_off = ctx->rec_off.as<uint64_t>(); C.bs = bs.as<uint32_t>(); C.n = n; C.total = total;
    C.out = ctx->text.as<uint8_t>();
    if (Q) hipLaunchKernelGGL(k_assemble<true>, g, dim3(256), 0, st, C);
    else hipLaunchKernelGGL(k_assemble<false>, g, dim3(256), 0, st, C);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev.b, st));
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b));
  ctx->info.num_units = n;
  ctx->info.first_slot = g0 + r0;
  ctx->info.bytes = total;
  ctx->info.ms_device = ms;
  ctx->info.ms_file = 0;
  ctx->have = true;
  if (info_out) *info_out = ctx->info;
  return 0;
}

}  // namespace

int sr::fastq_out_view(spring_fastq_out_ctx *ctx, FastqOutView *v) {
  if (!ctx || !v) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "no text assembled yet");
  v->dev = ctx->dev;
  v->info = ctx->info;
  v->text = ctx->text.as<uint8_t>();
  v->rec_off = ctx->rec_off.as<uint64_t>();
  return 0;
}

extern "C" {

int spring_fastq_out_create(int device, spring_fastq_out_ctx **out) {
  if (!out) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  const int r = stage_device(&device, "the FASTQ assembler");
  if (r) return r;
  spring_fastq_out_ctx *c = new spring_fastq_out_ctx();
  c->dev = device;
  memset(&c->info, 0, sizeof(c->info));
  *out = c;
  return 0;
}

void spring_fastq_out_destroy(spring_fastq_out_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->dev);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  drop_result(ctx);
  if (ctx->st) (void)hipStreamDestroy(ctx->st);
  delete ctx;
}

int spring_fastq_out_assemble(spring_fastq_out_ctx *ctx, const spring_fastq_out_params *params,
                              const spring_fastq_out_sources *sources, spring_fastq_out_info *info) {
  if (!ctx || !params || !sources) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  (void)hipSetDevice(ctx->dev);
  drop_result(ctx);
  const int r = assemble(ctx, *params, *sources, info);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  if (r) drop_result(ctx);
  return r;
}

int spring_fastq_out_get_info(spring_fastq_out_ctx *ctx, spring_fastq_out_info *info) {
  if (!ctx || !info) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "no text assembled yet");
  *info = ctx->info;
  return 0;
}

int spring_fastq_out_download(spring_fastq_out_ctx *ctx, uint8_t *text, uint64_t *rec_off) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "no text assembled yet");
  HIPCHK(hipSetDevice(ctx->dev));
  if (text && ctx->info.bytes) HIPCHK(rd(ctx->st, text, ctx->text.p, ctx->info.bytes));
  if (rec_off) HIPCHK(rd(ctx->st, rec_off, ctx->rec_off.p, (ctx->info.num_units + 1) * 8));
  return 0;
}

int spring_fastq_out_write(spring_fastq_out_ctx *ctx, const char *path, int32_t append, spring_fastq_out_info *info) {
  if (!ctx || !path) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "no text assembled yet");
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
  const uint64_t total = ctx->info.bytes, nchunk = (total + sr::PIN_CHUNK - 1) / sr::PIN_CHUNK;
  for (int k = 0; k < 2 && (uint64_t)k < nchunk; k++) {
    if (!(R.pin[k] = sr::pinned_get())) return fail(SPRING_REORDER_E_HIP, "cannot pin a staging chunk for the text");
    HIPCHK(hipEventCreateWithFlags(&R.ev[k], hipEventDisableTiming));
  }
  auto chunk_len = [&](uint64_t i) { return (size_t)std::min<uint64_t>(sr::PIN_CHUNK, total - i * sr::PIN_CHUNK); };
  auto issue = [&](uint64_t i) -> hipError_t {
    hipError_t e = hipMemcpyAsync(R.pin[i & 1], ctx->text.as<uint8_t>() + i * sr::PIN_CHUNK, chunk_len(i),
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
