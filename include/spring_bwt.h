/*
 * include/spring_bwt.h -- C ABI of the MI355X (gfx950) block-sort stage: libbsc's bsc_bwt_encode for a batch of byte
 * segments in HBM.
 *
 * Replaces the bsc_bwt_encode call of bsc_compress (reference src/libbsc/libbsc/libbsc/libbsc.cpp:158 and :254,
 * divsufsort.c:1667-1760) for the stream blocks reorder_compress_streams hands to BSC_compress.  For a segment T[0..n),
 * n >= 1:
 *
 *   order      the n suffixes T[i..n) sorted by unsigned bytes; a suffix that is a proper prefix of another sorts
 *              first.  rank[i] is the 0-based place of suffix i.
 *   bytes      out[0] = T[n-1], then T[i-1] for every suffix i > 0 in rank order: n bytes.
 *   primary    rank[0] + 1.
 *   indexes    mod = n / 8 with its highest set bit smeared downwards, then >> 1; step = mod + 1;
 *              num_indexes = (uint8_t)((n - 1) / step); indexes[k] = rank[(k + 1) * step] for k < num_indexes.  Always
 *              reported (bsc_compress drops them below 64 KiB: that is the caller's rule).
 *   n = 0      zero bytes, primary 0, no indexes.
 *
 * A batch is S segments back to back with S + 1 offsets; no comparison ever reads across a segment boundary.  The batch
 * is worked off in sub-batches of whole segments that fit the workspace budget (info.sub_batches).
 *
 *   from_host     offsets start at 0, do not decrease and end at nbytes; NULL offsets mean one segment.
 *   from_streams  every non-empty (stream, block) slice of a finished streams context whose stream is in stream_mask
 *                 (bit s = stream id s of spring_streams.h), read in place in HBM and left as it was, cut every
 *                 block_bytes bytes as BSC's Compression() cuts a file (bsc.cpp:149-190: the last cut is the short
 *                 one; an empty slice gives no segment).  Order: stream, then block, then cut; spring_bwt_segments
 *                 says which is which.
 *   from_qualid   every non-empty block of the quality (or id) result of a finished quality / id context
 *                 (spring_qualid.h), read in place in HBM and left as it was, cut every block_bytes bytes as
 *                 BSC_str_array_compress's Compression() cuts its input (bsc_str_array.cpp:183-250: at byte multiples
 *                 regardless of line ends; the last cut is the short one; an empty block gives no segment).
 *                 block_bytes 0 = 64 MiB, the "-b64" SPRING passes (bsc_str_array.cpp:864-865); the context's own
 *                 block_bytes is for from_streams only.  Order: block, then cut; spring_bwt_segments reports
 *                 SPRING_BWT_SRC_QUALITY or SPRING_BWT_SRC_ID as the stream.
 *
 * Run-aware first keys (spring_bwt_set_run_keys; off by default): the same results from a first
 * key that also orders the positions inside a run of one byte by what follows the run, for content with few symbols and
 * long runs.  With them on a position costs 76 bytes of workspace, not 72.
 *
 * Refused before any result: offsets that do not start at 0, decrease or do not end at nbytes, a NULL buffer with
 * nbytes > 0, a streams context on another device, a segment above 1 GiB (as bsc_compress refuses it) or one that does
 * not fit the workspace budget, a kind outside 0 / 1, a block_bytes above 2^30, a quality / id context on another device,
 * a cap_bits above a sub-batch's own run field (SPRING_REORDER_E_ARG); a streams context without a run, a quality / id
 * context without a result of that kind (SPRING_REORDER_E_STATE).  A refused call leaves the context without a result;
 * download / segments / get_info / round_entries without a result give SPRING_REORDER_E_STATE.
 *
 * Return value: 0 on success, negative SPRING_REORDER_E_* on error; text in spring_reorder_last_error().
 */
#ifndef SPRING_BWT_H_
#define SPRING_BWT_H_

#include <stddef.h>
#include <stdint.h>

#include "spring_qualid.h"
#include "spring_streams.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPRING_BWT_MAX_INDEXES 256
#define SPRING_BWT_MAX_SEGMENT (1u << 30)   /* bsc_compress: n > 1073741824 is LIBBSC_BAD_PARAMETER */
#define SPRING_BWT_SRC_QUALITY (-2)         /* spring_bwt_segments: the stream of a segment from from_qualid */
#define SPRING_BWT_SRC_ID (-3)

typedef struct spring_bwt_ctx spring_bwt_ctx;

typedef struct {
  uint64_t num_segments;
  uint64_t bytes;
  uint64_t max_segment;     /* the longest segment                                                    */
  uint64_t sub_batches;
  uint64_t rounds;          /* sort rounds (the first sort included) of the sub-batch that took most   */
  uint64_t rounds_total;    /* ... summed over the sub-batches                                         */
  uint64_t workspace_bytes; /* the budget the sub-batches were planned for                             */
  double ms_device;         /* HIP events around the device passes, input copies excluded              */
  double ms_pass[5];        /* keys (the run scan included), sort, re-rank, compaction of the unresolved,
                               gather + indexes                                                        */
  uint64_t run_positions;   /* positions whose first key carried a run (0 with run keys off)           */
} spring_bwt_info;

int spring_bwt_create(int device, spring_bwt_ctx **out);
void spring_bwt_destroy(spring_bwt_ctx *ctx);

/* The cut inside a stream slice for spring_bwt_from_streams: 1 .. 2^30; default 25 * 1024 * 1024, BSC's paramBlockSize
 * (bsc.cpp:80). */
int spring_bwt_set_block_bytes(spring_bwt_ctx *ctx, uint64_t block_bytes);
/* Device workspace the per-position arrays of a sub-batch may use; 0 (the default) takes it from the free HBM at the
 * time of the call.  The sort's fixed tables (at most 8 MiB) come on top.  spring_bwt_workspace_need: what a sub-batch
 * of `bytes` bytes in `segments` segments takes of it. */
int spring_bwt_set_workspace_bytes(spring_bwt_ctx *ctx, uint64_t workspace_bytes);
uint64_t spring_bwt_workspace_need(uint64_t bytes, uint64_t segments);
/* Run-aware first keys for every from_* call and encode_inplace that follows; off by default.  cap_bits: run lengths
 * are told apart up to 2^cap_bits - 1 (longer runs tie and are resolved by the doubling rounds); 0 = the width of the
 * layout's run field (20 bits up to 256 segments in a sub-batch, else 16), else 2 .. that width.  With run keys on a
 * sub-batch takes 4 bytes a position more than spring_bwt_workspace_need says. */
int spring_bwt_set_run_keys(spring_bwt_ctx *ctx, int32_t on, uint32_t cap_bits);

int spring_bwt_from_host(spring_bwt_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const uint64_t *seg_off,
                         uint64_t num_segments, spring_bwt_info *info);
int spring_bwt_from_streams(spring_bwt_ctx *ctx, spring_streams_ctx *streams, uint32_t stream_mask,
                            spring_bwt_info *info);
/* kind: SPRING_QUALID_QUALITY or SPRING_QUALID_ID; block_bytes: 0 (64 MiB) or 1 .. 2^30. */
int spring_bwt_from_qualid(spring_bwt_ctx *ctx, spring_qualid_ctx *q, int32_t kind, uint64_t block_bytes,
                           spring_bwt_info *info);

/* bwt: info.bytes bytes; seg_off: info.num_segments + 1 offsets into bwt; primary, num_indexes: one int32 per segment;
 * indexes: SPRING_BWT_MAX_INDEXES int32 per segment, the first num_indexes of them set, the rest 0.  Any may be NULL. */
int spring_bwt_download(spring_bwt_ctx *ctx, uint8_t *bwt, uint64_t *seg_off, int32_t *primary, int32_t *num_indexes,
                        int32_t *indexes);
/* Where a segment came from, one entry per segment: stream id (-1 after from_host, SPRING_BWT_SRC_QUALITY / _ID after
 * from_qualid), block (from_host: the segment's number) and cut inside the block.  Any may be NULL. */
int spring_bwt_segments(spring_bwt_ctx *ctx, int32_t *stream, uint32_t *block, uint32_t *cut);

int spring_bwt_get_info(spring_bwt_ctx *ctx, spring_bwt_info *info);
/* entries[k], k < max_entries: the entries round k sorted (round 0: every position), summed over the sub-batches; 0
 * behind the last round (info.rounds). */
int spring_bwt_round_entries(spring_bwt_ctx *ctx, uint64_t *entries, uint64_t max_entries);

/* bsc_bwt_encode's own contract (libbsc/bwt/bwt.h): T[0..n) on the host is transformed in place; returns the primary
 * index or a negative SPRING_REORDER_E_*.  n = 0 returns 0; num_indexes and indexes may be NULL. */
int spring_bwt_encode_inplace(spring_bwt_ctx *ctx, uint8_t *T, int32_t n, uint8_t *num_indexes, int32_t *indexes);

#ifdef __cplusplus
}
#endif
#endif
