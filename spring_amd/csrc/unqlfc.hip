// spring_amd/csrc/unqlfc.hip -- libbsc's bsc_coder_decompress (LIBBSC_CODER_QLFC_STATIC, fast mode) for a batch of coded
// segments in HBM (include/spring_unqlfc.h), one sub-batch of whole segments at a time.
//
// Which predictor a decision reads depends on what has been decoded, so a chunk is one serial walk; the batch has as
// many walks in flight as it has coded chunks.
//
//   1  plan: one lane per segment reads k and the chunk table; the host applies the header rules and lays out jobs
//      (coded chunks), pieces (raw chunks) and sub-batches
//   2  decode: the predictors of every chunk of the sub-batch are set to 2048 in the workspace; one wavefront per chunk
//      walks its payload.  Everything the walk decides on is uniform across the wave; the lanes hold what is wide: 64
//      units of the payload, four entries each of the move-to-front list, one predictor each of a decision's three, and
//      they write a run together.
//   3  raw chunks: one copy kernel
//
// Every loop on the device is bounded by a number known before it starts: at most n runs for a chunk of n bytes, 256 x 8
// steps of the symbol table, exponents below 8 and 32, payload / 2 units.  No kernel waits on a flag or on another
// lane's result.  A violation of the rules stops the chunk and is left in its result, which the host reads before it
// publishes anything.
#include <algorithm>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "bwt_internal.h"
#include "reorder_internal.h"
#include "spring_unqlfc.h"
#include "stage_host.h"
#include "unqlfc_plan.h"

using namespace sr;

static_assert(unqlfc::MODEL_BYTES == SPRING_UNQLFC_MODEL_BYTES, "spring_unqlfc.h and unqlfc_plan.h disagree");
static_assert(unqlfc::MAX_SEGMENT == SPRING_UNQLFC_MAX_SEGMENT, "spring_unqlfc.h and unqlfc_plan.h disagree");
static_assert(unqlfc::MAX_SEGMENT == SPRING_QLFC_MAX_SEGMENT, "the coder and the decoder disagree");

namespace {

constexpr int NPASS = SPRING_UNQLFC_PASSES;
constexpr uint32_t PLAN_STRIDE = 8;         // chunk-table entries read per segment at first: what the coder writes
constexpr uint64_t MAX_SUB_CHUNKS = 2048;   // coded chunks of a sub-batch: eight waves on every CU

// qlfc_params.h, in the order of qlfc::Family and qlfc::Kind
#define QLFC_ROW_(f, k, th0, ar0, th1, ar1) {th0, ar0, th1, ar1},
#define QLFC_MIX_(f, a, b, c) {a, b, c},
#define QLFC_NONE_(...)
__constant__ int c_rows[QLFC_FAMILIES * QLFC_KINDS][4] = {QLFC_PARAM_TABLE(QLFC_ROW_, QLFC_NONE_)};
__constant__ int c_mix[QLFC_FAMILIES][QLFC_KINDS] = {QLFC_PARAM_TABLE(QLFC_NONE_, QLFC_MIX_)};

struct Job {       // a coded chunk
  uint64_t src;    // device address of its payload
  uint64_t dst;    // device address of its n bytes
  uint32_t n;      // its size as the header states it
  uint32_t len;    // bytes of the payload
};
struct Res {
  uint32_t violation, runs;
  uint64_t events;
};
struct Piece {     // a raw chunk
  uint64_t src, dst, len;
};

// ------------------------------------------------------------------ 1: plan
// k[s]: the segment's first byte (0 for a segment without bytes); tab[(s * stride + j) * 2 ..]: entry j of its chunk
// table, where the table fits the segment and the stride.  Bytes, not words: a segment starts anywhere.
__global__ __launch_bounds__(256) void k_plan(const uint64_t *__restrict__ src, const uint64_t *__restrict__ off, uint32_t S,
                                              uint32_t stride, uint32_t *__restrict__ k_out, int32_t *__restrict__ tab) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= S) return;
  const uint64_t len = off[s + 1] - off[s];
  const uint8_t *p = reinterpret_cast<const uint8_t *>(src[s]);
  const uint32_t k = len ? p[0] : 0;
  k_out[s] = k;
  if (k < 2 || k > stride || 1 + 8ull * k > len) return;
  for (uint32_t j = 0; j < 2 * k; j++) {
    const uint8_t *q = p + 1 + 4 * j;
    tab[(size_t)s * stride * 2 + j] = (int32_t)((uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24);
  }
}

// ------------------------------------------------------------------ 2: decode
__global__ __launch_bounds__(256) void k_fill(uint4 *__restrict__ models, uint64_t n16) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  const uint32_t w = 2048u | 2048u << 16;
  if (i < n16) models[i] = make_uint4(w, w, w, w);
}

__device__ __forceinline__ uint32_t lane_value(uint32_t v, uint32_t lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// The range decoder (rangecoder.h:152-180).  Lane i of the window holds unit base + i of the payload, put together from
// two byte loads.  A unit beyond the payload reads as 0 and sets `bad`, which stops the chunk at its next check.
struct Decoder {
  const uint8_t *src;
  uint32_t nunits, at = 0, base = 0, win = 0, lane;
  uint32_t code = 0, range = 0xffffffffu;
  bool bad = false;
  uint64_t events = 0;
  __device__ __forceinline__ void load() {
    const uint32_t u = base + lane;
    uint32_t v = 0;
    if (u < nunits) v = (uint32_t)src[2 * (size_t)u] | (uint32_t)src[2 * (size_t)u + 1] << 8;
    win = v;
  }
  __device__ __forceinline__ uint32_t unit() {
    if (at >= nunits) { bad = true; return 0; }
    if (at - base >= 64) { base += 64; load(); }
    return lane_value(win, at++ - base);
  }
  __device__ __forceinline__ uint32_t bit(uint32_t p) {
    const uint32_t r = (range >> 12) * p;
    uint32_t b;
    if (code >= r) { code -= r; range -= r; b = 1; } else { range = r; b = 0; }
    if (range < 0x10000u) { range <<= 16; code = code << 16 | unit(); }
    return b;
  }
};

struct Params {   // of lane 0, 1, 2: the row and the weight of its kind, per family
  int th0[QLFC_FAMILIES], ar0[QLFC_FAMILIES], th1[QLFC_FAMILIES], ar1[QLFC_FAMILIES], w[QLFC_FAMILIES];
};

// One decision of family FAM at `place`: lanes 0, 1 and 2 load the predictor of the run's byte, of the context state
// and the shared one; the weighted sum is taken from the values as loaded; then each of the three updates and stores
// its own (predictor.h:45-53 through a short).
template <int FAM>
__device__ __forceinline__ uint32_t decide(Decoder &d, const Params &P, int16_t *__restrict__ model, uint32_t sym, uint32_t state,
                                           uint32_t place) {
  constexpr uint32_t L = unqlfc::places(FAM), B = unqlfc::family_base(FAM);
  const uint32_t l = d.lane;
  const uint32_t who = (l == 0 ? sym : state) & 255u;
  const uint32_t idx = B + (l < 2 ? (l * 256 + who) * L : 512 * L) + (place & (L - 1));
  int v = 0;
  if (l < 3) v = model[idx];
  const int wv = v * P.w[FAM];
  const int p = ((int)lane_value((uint32_t)wv, 0) + (int)lane_value((uint32_t)wv, 1) + (int)lane_value((uint32_t)wv, 2)) >> 5;
  const uint32_t b = d.bit((uint32_t)p);
  if (l < 3) {
    const int nv = b ? v - (((v - P.th1[FAM]) * P.ar1[FAM]) >> 12) : v + (((4096 - P.th0[FAM] - v) * P.ar0[FAM]) >> 12);
    model[idx] = (int16_t)nv;
  }
  d.events++;
  return b;
}

// Is any of the bytes lo .. lo + len - 1 (len a power of two up to 128, lo a multiple of it) in the 256-bit mask?
__device__ __forceinline__ bool any_in(uint64_t m0, uint64_t m1, uint64_t m2, uint64_t m3, uint32_t lo, uint32_t len) {
  const uint32_t q = lo >> 6;
  if (len == 128) return q == 0 ? (m0 | m1) != 0 : (m2 | m3) != 0;
  const uint64_t m = q == 0 ? m0 : q == 1 ? m1 : q == 2 ? m2 : m3;
  if (len == 64) return m != 0;
  return ((m >> (lo & 63)) & ((1ull << len) - 1)) != 0;
}

// `len` bytes c from p on, by all lanes: byte stores up to the first 16-byte boundary and behind the last, 16-byte
// stores in between.  Nothing outside p[0 .. len).
__device__ __forceinline__ void write_run(uint8_t *p, uint32_t len, uint32_t c, uint32_t l) {
  if (len <= 64) {
    if (l < len) p[l] = (uint8_t)c;
    return;
  }
  const uint32_t head = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u;
  if (l < head) p[l] = (uint8_t)c;
  p += head;
  len -= head;
  const uint32_t w = c * 0x01010101u, q = len >> 4;
  const uint4 v = make_uint4(w, w, w, w);
  for (uint32_t j = l; j < q; j += 64) reinterpret_cast<uint4 *>(p)[j] = v;
  if (l < (len & 15u)) p[(size_t)q * 16 + l] = (uint8_t)c;
}

#define STOP(v)                                        \
  do {                                                 \
    if (l == 0) res[c] = Res{(uint32_t)(d.bad ? unqlfc::V_UNITS : (v)), runs, d.events}; \
    return;                                            \
  } while (0)

// One wavefront per coded chunk (qlfc.cpp:1038-1297).
__global__ __launch_bounds__(64) void k_decode(const Job *__restrict__ jobs, int16_t *__restrict__ models,
                                               const uint8_t *__restrict__ rank_tab, const uint8_t *__restrict__ run_tab,
                                               Res *__restrict__ res) {
  __shared__ uint8_t hist[2][256];   // rankHistory, runHistory
  const uint32_t c = blockIdx.x, l = threadIdx.x;
  for (uint32_t i = l; i < 256; i += 64) hist[0][i] = hist[1][i] = 0;
  __syncthreads();
  const Job J = jobs[c];
  int16_t *model = models + (size_t)c * (unqlfc::MODEL_BYTES / 2);
  uint8_t *dst = reinterpret_cast<uint8_t *>(J.dst);
  const uint32_t n = J.n;
  Params P;
  const int kind = l < 2 ? (int)l : 2;
#pragma unroll
  for (int f = 0; f < QLFC_FAMILIES; f++) {
    P.th0[f] = c_rows[3 * f + kind][0];
    P.ar0[f] = c_rows[3 * f + kind][1];
    P.th1[f] = c_rows[3 * f + kind][2];
    P.ar1[f] = c_rows[3 * f + kind][3];
    P.w[f] = l < 3 ? c_mix[f][kind] : 0;
  }
  Decoder d;
  d.src = reinterpret_cast<const uint8_t *>(J.src);
  d.nunits = J.len >> 1;
  d.lane = l;
  d.load();
  uint32_t runs = 0;
  for (int k = 0; k < 3; k++) d.code = d.code << 16 | d.unit();
  uint32_t size = 0;
  for (int b = 0; b < 32; b++) size += size + d.bit(2048);
  if (d.bad || size != n) STOP(unqlfc::V_SIZE);
  // ---- the symbol table (:1061-1105): a bit is read only where both of its values are still possible among the
  // bytes not yet listed and the one listed last.  Entry e of the move-to-front list is m[e / 64] of lane e % 64.
  uint64_t a0 = ~0ull, a1 = ~0ull, a2 = ~0ull, a3 = ~0ull;
  auto mark = [&](uint32_t byte, bool on) {   // selects, so that the four words stay in registers
    const uint64_t bitm = 1ull << (byte & 63);
    const uint32_t q = byte >> 6;
    a0 = q != 0 ? a0 : on ? a0 | bitm : a0 & ~bitm;
    a1 = q != 1 ? a1 : on ? a1 | bitm : a1 & ~bitm;
    a2 = q != 2 ? a2 : on ? a2 | bitm : a2 & ~bitm;
    a3 = q != 3 ? a3 : on ? a3 | bitm : a3 & ~bitm;
  };
  uint32_t m[4] = {0, 0, 0, 0};
  uint32_t entries = 0, prev = 256;
  int maxrank = 7;
  for (uint32_t rank = 0; rank < 256; rank++) {
    if (prev < 256) mark(prev, true);
    uint32_t cur = 0;
    for (int b = 7; b >= 0; b--) {
      const uint32_t lo = cur << (b + 1), half = 1u << b;
      const bool zero = any_in(a0, a1, a2, a3, lo, half), one = any_in(a0, a1, a2, a3, lo + half, half);
      cur += cur + (zero && one ? d.bit(2048) : one ? 1u : 0u);
    }
    if (prev < 256) mark(prev, false);
    if (l == (rank & 63)) {
      if ((rank >> 6) == 0) m[0] = cur; else if ((rank >> 6) == 1) m[1] = cur; else if ((rank >> 6) == 2) m[2] = cur; else m[3] = cur;
    }
    entries = rank + 1;
    if (cur == prev) {
      maxrank = qlfc::log2i(rank - 1);
      break;
    }
    mark(cur, false);
    prev = cur;
  }
  if (d.bad) STOP(unqlfc::V_UNITS);
  // ---- the runs
  uint32_t ctx0 = 0, ctx4 = 0, ctxrun = 0, avg = 0, i = 0;
  for (uint32_t r = 0; r < n && i < n; r++) {
    const uint32_t cur = lane_value(m[0], 0);
    const uint32_t hr = uniform(hist[0][cur]);
    uint32_t state = rank_tab[ctxrun << 11 | ctx4 << 3 | (hr & 7u)];
    uint32_t rank = 1, newhr = 0;
    if (avg < 32) {
      if (decide<qlfc::RANK_TOP>(d, P, model, cur, state, 0)) {
        if (maxrank < 1) STOP(unqlfc::V_RANK);   // one or two symbols: no rank but 1
        uint32_t e = 1;
        for (int t = 0; t < 7 && (int)e != maxrank; t++) {
          if (!decide<qlfc::RANK_EXP>(d, P, model, cur, state, e - 1)) break;
          e++;
        }
        newhr = e;
        for (uint32_t t = 0; t < e; t++) rank += rank + decide<qlfc::RANK_MAN>(d, P, model, cur, state, unqlfc::rank_man_place(e, rank));
      }
    } else {
      uint32_t ctx = 1;
      rank = 0;
      for (int b = maxrank; b >= 0; b--) {
        const uint32_t bit = decide<qlfc::RANK_ESC>(d, P, model, cur, state, ctx);
        ctx += ctx + bit;
        rank += rank + bit;
      }
      if (rank == 0) STOP(unqlfc::V_RANK);
      newhr = (uint32_t)qlfc::log2i(rank);
    }
    if (d.bad || rank >= entries) STOP(unqlfc::V_RANK);
    hist[0][cur] = (uint8_t)newhr;   // every lane writes the same byte
    // the list moves in one step: entry e takes entry e + 1 below the rank, the run's byte at the rank
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (64u * k <= rank) {   // uniform
        uint32_t up = (uint32_t)__shfl_down((int)m[k], 1);
        const uint32_t over = k < 3 ? lane_value(m[k < 3 ? k + 1 : 3], 0) : 0;
        if (l == 63) up = over;
        const uint32_t e = 64u * k + l;
        m[k] = e < rank ? up : e == rank ? cur : m[k];
      }
    }
    avg = (avg * 124 + rank * 4) >> 7;
    const uint32_t rk = rank - 1;
    const uint32_t hu = uniform(hist[1][cur]);
    state = run_tab[ctx0 << 10 | ctxrun << 6 | min(rk, 7u) << 3 | min(hu, 7u)];
    uint32_t run = 1, newhu = (hu + 2) >> 2;
    if (decide<qlfc::RUN_TOP>(d, P, model, cur, state, 0)) {
      uint32_t e = 1;
      for (int t = 0; t < 31; t++) {
        if (!decide<qlfc::RUN_EXP>(d, P, model, cur, state, e - 1)) break;
        e++;
      }
      if (d.bad || e >= 32) STOP(unqlfc::V_EXPONENT);
      newhu = (hu + 3 * e + 3) >> 2;
      uint32_t ctx = 1;
      for (uint32_t t = 0; t < e; t++) {
        const uint32_t bit = decide<qlfc::RUN_MAN>(d, P, model, cur, state, unqlfc::run_man_place(e, ctx));
        run += run + bit;
        ctx = e <= 5 ? ctx + ctx + bit : ctx + 1;   // above exponent 5 the context is the bit's position
      }
    }
    hist[1][cur] = (uint8_t)newhu;
    ctx0 = (ctx0 << 1 | (rk == 0)) & 7;
    ctx4 = (ctx4 << 2 | min(rk, 3u)) & 0xff;
    ctxrun = (ctxrun << 1 | (run < 3)) & 0xf;
    if (d.bad || run > n - i) STOP(unqlfc::V_RUN);
    write_run(dst + i, run, cur, l);
    i += run;
    runs++;
  }
  if (l == 0) res[c] = Res{unqlfc::V_NONE, runs, d.events};
}
#undef STOP

// ------------------------------------------------------------------ 3: raw chunks
__global__ __launch_bounds__(256) void k_copy(const Piece *__restrict__ pieces) {
  const Piece P = pieces[blockIdx.x];
  const uint8_t *s = reinterpret_cast<const uint8_t *>(P.src);
  uint8_t *t = reinterpret_cast<uint8_t *>(P.dst);
  for (uint64_t i = blockIdx.y * 256ull + threadIdx.x; i < P.len; i += 256ull * gridDim.y) t[i] = s[i];
}

}  // namespace

struct spring_unqlfc_ctx {
  int dev = 0;
  hipStream_t st = nullptr;
  uint64_t workspace_bytes = 0;   // 0: from the free HBM
  bool have_tables = false, have = false;
  DBuf rank_tab, run_tab;
  spring_unqlfc_info info;
  std::vector<uint64_t> off;      // num_segments + 1: the decoded segments in out
  DBuf out;
};

namespace {

void drop_result(spring_unqlfc_ctx *ctx) {
  ctx->have = false;
  ctx->out.release();
  ctx->off.clear();
  memset(&ctx->info, 0, sizeof(ctx->info));
}

// The batch: S coded segments at the device addresses src with the offsets coded_off, out_size[s] bytes each decoded.
int decode_batch(spring_unqlfc_ctx *ctx, const std::vector<uint64_t> &coded_off, const std::vector<uint64_t> &src,
                 const uint64_t *out_size, spring_unqlfc_info *info_out) {
  const int dev = ctx->dev;
  hipStream_t st = ctx->st;
  const uint64_t S = src.size();
  spring_unqlfc_info &I = ctx->info;
  memset(&I, 0, sizeof(I));
  I.num_segments = S;
  I.bytes_in = coded_off[S];
  if (S >= 0x7fffffffull) return fail(SPRING_REORDER_E_ARG, "too many segments");
  ctx->off.assign(S + 1, 0);
  for (uint64_t s = 0; s < S; s++) {
    if (coded_off[s + 1] - coded_off[s] > unqlfc::MAX_SEGMENT || out_size[s] > unqlfc::MAX_SEGMENT)
      return fail(SPRING_REORDER_E_ARG, "segment %llu: %llu coded bytes for %llu: more than 1 GiB", (unsigned long long)s,
                  (unsigned long long)(coded_off[s + 1] - coded_off[s]), (unsigned long long)out_size[s]);
    ctx->off[s + 1] = ctx->off[s] + out_size[s];
  }
  const std::vector<uint64_t> &off = ctx->off;
  I.bytes_out = off[S];
  DALLOC(ctx->out, I.bytes_out + 16);
  uint8_t *out = ctx->out.as<uint8_t>();
  const bool own_budget = ctx->workspace_bytes != 0;
  uint64_t budget = 0;
  if (int r = workspace_budget(ctx->workspace_bytes, 0, &budget)) return r;
  I.workspace_bytes = budget;
  if (S == 0) {
    ctx->have = true;
    if (info_out) *info_out = I;
    return 0;
  }
  Laps T{st};
  DBuf d_off, d_src, d_k, d_tab, d_jobs, d_res, d_pieces, models;
  SyncOnExit sync_on_exit{st};
  // ---- 1: k and the chunk tables
  DALLOC(d_off, (S + 1) * 8);
  DALLOC(d_src, S * 8);
  DALLOC(d_k, S * 4);
  HIPCHK(hipMemcpyAsync(d_off.p, coded_off.data(), (S + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_src.p, src.data(), S * 8, hipMemcpyHostToDevice, st));
  std::vector<uint32_t> h_k(S);
  std::vector<int32_t> h_tab;
  uint32_t stride = PLAN_STRIDE;
  for (int attempt = 0; attempt < 2; attempt++) {   // again with the widest stride where a segment has more chunks
    DALLOC(d_tab, S * stride * 8);
    HIPCHK(T.begin(0));
    hipLaunchKernelGGL(k_plan, grid(S), dim3(256), 0, st, d_src.as<uint64_t>(), d_off.as<uint64_t>(), (uint32_t)S, stride,
                       d_k.as<uint32_t>(), d_tab.as<int32_t>());
    HIPCHK(T.end());
    HIPCHK(hipGetLastError());
    HIPCHK(rd(st, h_k.data(), d_k.p, S * 4));
    if (*std::max_element(h_k.begin(), h_k.end()) <= stride) break;
    stride = 255;
  }
  h_tab.resize(S * stride * 2);
  HIPCHK(rd(st, h_tab.data(), d_tab.p, S * stride * 8));
  // ---- the header rules; jobs, pieces
  std::vector<Job> jobs;
  std::vector<Piece> pieces;
  std::vector<uint64_t> job0(S + 1, 0);   // the first job of every segment
  for (uint64_t s = 0; s < S; s++) {
    job0[s] = jobs.size();
    const uint64_t len = coded_off[s + 1] - coded_off[s], n = out_size[s], k = h_k[s];
    auto bad = [&](uint32_t v) {
      return fail(SPRING_REORDER_E_ARG, "segment %llu: its %llu coded bytes for %llu are malformed (%s, %llu chunks)",
                  (unsigned long long)s, (unsigned long long)len, (unsigned long long)n, unqlfc::violation_name(v),
                  (unsigned long long)k);
    };
    if (len == 0 && n == 0) { I.skipped++; continue; }
    if (len == 0 || k == 0) return bad(unqlfc::V_CHUNKS);
    uint8_t *dst = out + off[s];
    if (k == 1) {
      jobs.push_back(Job{src[s] + 1, reinterpret_cast<uint64_t>(dst), (uint32_t)n, (uint32_t)(len - 1)});
      I.chunks++;
      continue;
    }
    if (1 + 8 * k > len) return bad(unqlfc::V_TABLE);
    const int32_t *T = &h_tab[s * stride * 2];
    uint64_t sum_in = 0, sum_coded = 0;
    for (uint64_t j = 0; j < k; j++) {
      if (T[2 * j] < 0 || T[2 * j + 1] < 0 || T[2 * j + 1] > T[2 * j]) return bad(unqlfc::V_ENTRY);
      sum_in += (uint64_t)T[2 * j];
      sum_coded += (uint64_t)T[2 * j + 1];
    }
    if (sum_in != n) return bad(unqlfc::V_SUM);
    if (1 + 8 * k + sum_coded != len) return bad(unqlfc::V_LENGTH);
    uint64_t in_at = 1 + 8 * k, out_at = 0;
    for (uint64_t j = 0; j < k; j++) {
      const uint64_t a = (uint64_t)T[2 * j], b = (uint64_t)T[2 * j + 1];
      if (a == b) {
        if (a) pieces.push_back(Piece{src[s] + in_at, reinterpret_cast<uint64_t>(dst + out_at), a});
        I.chunks_raw++;
      } else {
        jobs.push_back(Job{src[s] + in_at, reinterpret_cast<uint64_t>(dst + out_at), (uint32_t)a, (uint32_t)b});
      }
      I.chunks++;
      in_at += b;
      out_at += a;
    }
  }
  job0[S] = jobs.size();
  // ---- sub-batches of whole segments
  std::vector<uint64_t> first(1, 0);
  uint64_t most = 0;
  for (uint64_t s = 0, s0 = 0; s <= S; s++) {
    const uint64_t have = job0[s] - job0[s0];
    if (s == S) {
      first.push_back(S);
      most = std::max(most, have);
      break;
    }
    const uint64_t mine = job0[s + 1] - job0[s];
    if (unqlfc::workspace_need(out_size[s], mine) > budget)
      return fail(SPRING_REORDER_E_ARG, "segment %llu of %llu coded chunks needs %llu bytes of workspace, the budget is %llu",
                  (unsigned long long)s, (unsigned long long)mine, (unsigned long long)unqlfc::workspace_need(out_size[s], mine),
                  (unsigned long long)budget);
    if (s > s0 && (unqlfc::workspace_need(off[s + 1] - off[s0], have + mine) > budget || (!own_budget && have + mine > MAX_SUB_CHUNKS))) {
      first.push_back(s);
      most = std::max(most, have);
      s0 = s;
    }
  }
  I.sub_batches = first.size() - 1;
  // ---- 2: decode
  std::vector<Res> h_res(jobs.size());
  if (!jobs.empty()) {
    DALLOC(d_jobs, jobs.size() * sizeof(Job));
    DALLOC(d_res, jobs.size() * sizeof(Res));
    DALLOC(models, most * unqlfc::MODEL_BYTES);
    HIPCHK(hipMemcpyAsync(d_jobs.p, jobs.data(), jobs.size() * sizeof(Job), hipMemcpyHostToDevice, st));
    for (size_t b = 0; b + 1 < first.size(); b++) {
      const uint64_t j0 = job0[first[b]], cnt = job0[first[b + 1]] - j0;
      if (!cnt) continue;
      const uint64_t n16 = cnt * (unqlfc::MODEL_BYTES / 16);
      HIPCHK(T.begin(1));
      hipLaunchKernelGGL(k_fill, grid(n16), dim3(256), 0, st, models.as<uint4>(), n16);
      hipLaunchKernelGGL(k_decode, dim3((unsigned)cnt), dim3(64), 0, st, d_jobs.as<Job>() + j0, models.as<int16_t>(),
                         ctx->rank_tab.as<uint8_t>(), ctx->run_tab.as<uint8_t>(), d_res.as<Res>() + j0);
      HIPCHK(T.end());
      HIPCHK(hipGetLastError());
    }
    HIPCHK(rd(st, h_res.data(), d_res.p, jobs.size() * sizeof(Res)));
  }
  for (uint64_t s = 0; s < S; s++)
    for (uint64_t j = job0[s]; j < job0[s + 1]; j++) {
      I.runs += h_res[j].runs;
      I.events += h_res[j].events;
      if (h_res[j].violation)
        return fail(SPRING_REORDER_E_ARG, "segment %llu: its %llu coded bytes for %llu are malformed (%s, in coded chunk %llu after %u runs)",
                    (unsigned long long)s, (unsigned long long)(coded_off[s + 1] - coded_off[s]), (unsigned long long)out_size[s],
                    unqlfc::violation_name(h_res[j].violation), (unsigned long long)(j - job0[s]), h_res[j].runs);
    }
  // ---- 3: raw chunks
  if (!pieces.empty()) {
    DALLOC(d_pieces, pieces.size() * sizeof(Piece));
    HIPCHK(hipMemcpyAsync(d_pieces.p, pieces.data(), pieces.size() * sizeof(Piece), hipMemcpyHostToDevice, st));
    HIPCHK(T.begin(2));
    hipLaunchKernelGGL(k_copy, dim3((unsigned)pieces.size(), 64), dim3(256), 0, st, d_pieces.as<Piece>());
    HIPCHK(T.end());
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(st));   // jobs and pieces are read until here
  if (int r = T.collect(I.ms_pass, &I.ms_device)) return r;
  ctx->have = true;
  if (info_out) *info_out = I;
  return 0;
}

int begin(spring_unqlfc_ctx *ctx) {
  (void)hipSetDevice(ctx->dev);
  drop_result(ctx);
  if (!ctx->have_tables) return fail(SPRING_REORDER_E_STATE, "spring_unqlfc_set_state_tables has not been called");
  return 0;
}

int finish(spring_unqlfc_ctx *ctx, int r) {
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  if (r) drop_result(ctx);
  return r;
}

}  // namespace

extern "C" {

int spring_unqlfc_create(int device, spring_unqlfc_ctx **out) {
  if (!out) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  const int r = stage_device(&device, "the QLFC decoder stage");
  if (r) return r;
  spring_unqlfc_ctx *c = new spring_unqlfc_ctx();
  c->dev = device;
  memset(&c->info, 0, sizeof(c->info));
  *out = c;
  return 0;
}

void spring_unqlfc_destroy(spring_unqlfc_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->dev);
  if (ctx->st) (void)hipStreamSynchronize(ctx->st);
  drop_result(ctx);
  ctx->rank_tab.release();
  ctx->run_tab.release();
  if (ctx->st) (void)hipStreamDestroy(ctx->st);
  delete ctx;
}

int spring_unqlfc_set_state_tables(spring_unqlfc_ctx *ctx, const uint8_t *rank_table, const uint8_t *run_table) {
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

int spring_unqlfc_set_workspace_bytes(spring_unqlfc_ctx *ctx, uint64_t workspace_bytes) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  ctx->workspace_bytes = workspace_bytes;
  return 0;
}

uint64_t spring_unqlfc_workspace_need(uint64_t bytes_out, uint64_t chunks) { return unqlfc::workspace_need(bytes_out, chunks); }

int spring_unqlfc_from_host(spring_unqlfc_ctx *ctx, const uint8_t *coded, uint64_t ncoded, const uint64_t *coded_off,
                            const uint64_t *out_size, uint64_t num_segments, spring_unqlfc_info *info) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  int r = begin(ctx);
  if (r) return r;
  if ((ncoded && !coded) || !coded_off || (num_segments && !out_size)) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (num_segments >= 0x7fffffffull) return fail(SPRING_REORDER_E_ARG, "too many segments");
  if (coded_off[0] != 0 || coded_off[num_segments] != ncoded)
    return fail(SPRING_REORDER_E_ARG, "the segment offsets do not start at 0 and end at the %llu bytes", (unsigned long long)ncoded);
  for (uint64_t s = 0; s < num_segments; s++)
    if (coded_off[s + 1] < coded_off[s]) return fail(SPRING_REORDER_E_ARG, "the segment offsets decrease");
  for (uint64_t s = 0; s < num_segments; s++)   // before anything is uploaded
    if (coded_off[s + 1] - coded_off[s] > unqlfc::MAX_SEGMENT || out_size[s] > unqlfc::MAX_SEGMENT)
      return fail(SPRING_REORDER_E_ARG, "segment %llu: %llu coded bytes for %llu: more than 1 GiB", (unsigned long long)s,
                  (unsigned long long)(coded_off[s + 1] - coded_off[s]), (unsigned long long)out_size[s]);
  if ((r = stream_begin(ctx->dev, &ctx->st))) return r;
  const int dev = ctx->dev;
  DBuf up;
  DALLOC(up, ncoded + 32);
  if (ncoded) HIPCHK(hipMemcpyAsync(up.p, coded, ncoded, hipMemcpyHostToDevice, ctx->st));
  std::vector<uint64_t> off(coded_off, coded_off + num_segments + 1), src(num_segments);
  for (uint64_t s = 0; s < num_segments; s++) src[s] = reinterpret_cast<uint64_t>(up.as<uint8_t>() + coded_off[s]);
  return finish(ctx, decode_batch(ctx, off, src, out_size, info));
}

int spring_unqlfc_from_qlfc(spring_unqlfc_ctx *ctx, spring_qlfc_ctx *qlfc, spring_unqlfc_info *info) {
  if (!ctx || !qlfc) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  int r = begin(ctx);
  if (r) return r;
  sr::QlfcView V;
  if ((r = sr::qlfc_view(qlfc, &V))) return r;
  if (V.dev != ctx->dev) return fail(SPRING_REORDER_E_ARG, "QLFC and decoder contexts live on different devices");
  if ((r = stream_begin(ctx->dev, &ctx->st))) return r;
  const uint64_t S = V.num_segments;
  std::vector<uint64_t> off(V.coded_off, V.coded_off + S + 1), src(S), out_size(S);
  if (S) HIPCHK(rd(ctx->st, src.data(), V.d_src, S * 8));
  for (uint64_t s = 0; s < S; s++) out_size[s] = V.status[s] == 0 ? V.in_off[s + 1] - V.in_off[s] : 0;
  return finish(ctx, decode_batch(ctx, off, src, out_size.data(), info));
}

int spring_unqlfc_get_info(spring_unqlfc_ctx *ctx, spring_unqlfc_info *info) {
  if (!ctx || !info) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing decoded yet");
  *info = ctx->info;
  return 0;
}

int spring_unqlfc_download(spring_unqlfc_ctx *ctx, uint8_t *bytes, uint64_t *seg_off) {
  if (!ctx) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing decoded yet");
  HIPCHK(hipSetDevice(ctx->dev));
  if (seg_off) memcpy(seg_off, ctx->off.data(), (ctx->info.num_segments + 1) * 8);
  if (bytes && ctx->info.bytes_out) HIPCHK(rd(ctx->st, bytes, ctx->out.p, ctx->info.bytes_out));
  return 0;
}

int spring_unqlfc_decompress(spring_unqlfc_ctx *ctx, const uint8_t *in, int32_t in_size, uint8_t *out, int32_t out_size) {
  if (!ctx || in_size < 0 || out_size < 0 || (in_size && !in) || (out_size && !out)) return fail(SPRING_REORDER_E_ARG, "bad argument");
  const uint64_t off[2] = {0, (uint64_t)in_size}, n = (uint64_t)out_size;
  const int r = spring_unqlfc_from_host(ctx, in, (uint64_t)in_size, off, &n, 1, nullptr);
  if (r) return r;
  const int r2 = spring_unqlfc_download(ctx, out, nullptr);
  return r2 ? r2 : out_size;
}

}  // extern "C"

namespace sr {
int unqlfc_view(spring_unqlfc_ctx *ctx, UnqlfcView *v) {
  if (!ctx || !v) return fail(SPRING_REORDER_E_ARG, "NULL argument");
  if (!ctx->have) return fail(SPRING_REORDER_E_STATE, "nothing decoded yet");
  *v = UnqlfcView{ctx->dev, ctx->info.num_segments, ctx->info.bytes_out, ctx->off.data(), ctx->out.as<uint8_t>()};
  return 0;
}
}  // namespace sr
