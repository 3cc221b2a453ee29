/*
 * include/spring_unbwt.h -- C ABI of the MI355X (gfx950) inverse block-sort stage: libbsc's bsc_bwt_decode for a batch
 * of transformed segments in HBM.  The exact inverse of spring_bwt.h.
 *
 * Replaces the bsc_bwt_decode call of bsc_decompress (reference src/libbsc/libbsc/libbsc/libbsc.cpp; the function
 * itself: bwt/bwt.cpp:180, bsc_unbwt_mergedTL_serial at bwt.cpp:54-84).  A segment is L[0..n) with a primary index;
 * for n >= 1 the primary index must satisfy 1 <= primary <= n.  Think of n + 1 rows:
 *
 *   rows       row 0 is the empty suffix.  Byte L[q] sits in row q for q < primary and in row q + 1 for q >= primary;
 *              row `primary` holds no byte: it is the suffix that starts the text.
 *   LF         sort the n bytes stably; the byte that lands at place t (0-based) came from row r: LF[r] = t + 1.
 *   text       start at row 0 and write backwards: T[n-1] = byte(row 0), then row = LF[row], and so on.  After n steps
 *              the walk stands on row `primary`.
 *
 * LF is a bijection from the rows other than `primary` onto the rows 1..n, so the rows form one path from row 0 to row
 * `primary` plus, possibly, cycles.  The segment is the transform of some text if and only if that path has n steps.
 *
 *   shorter path   refused: SPRING_REORDER_E_ARG, the first such segment named in spring_reorder_last_error(), no
 *                  result left.  (bsc_bwt_decode writes garbage there.)  No store for such a segment leaves the
 *                  segment's own n bytes.
 *   wrong primary  a primary index that is in range and whose path is complete gives a different text: a valid result.
 *   n = 0          primary 0: an empty segment; any other primary is SPRING_REORDER_E_ARG.
 *   n = 1          the byte itself.
 *   indexes        libbsc's secondary indexes are not needed for the result and are not read.
 *
 * A batch is S segments back to back with S + 1 offsets and S primary indexes, worked off in sub-batches of whole
 * segments that fit the workspace budget (info.sub_batches).
 *
 *   from_host   offsets start at 0, do not decrease and end at nbytes; NULL offsets mean one segment.
 *   from_bwt    the result of a finished block-sort context (spring_bwt.h), read in place in HBM and left as it was:
 *               its segments, offsets and primary indexes.
 *   from_unqlfc the decoded segments of a finished QLFC decoder context (spring_unqlfc.h), read where they lie in HBM
 *               and left as they were, with one primary index per segment from the caller (the block headers hold
 *               them); a segment that context left empty takes primary index 0.
 *
 * Refused before any result: offsets that do not start at 0, decrease or do not end at nbytes, a NULL buffer with
 * nbytes > 0, a NULL primary array, a primary index out of range, a block-sort context on another device, a segment
 * above 1 GiB or one that does not fit the workspace budget (SPRING_REORDER_E_ARG); a block-sort context without a
 * result (SPRING_REORDER_E_STATE).  A refused call leaves the context without a result; download / get_info without a
 * result give SPRING_REORDER_E_STATE.
 *
 * Return value: 0 on success, negative SPRING_REORDER_E_* on error; text in spring_reorder_last_error().
 */
#ifndef SPRING_UNBWT_H_
#define SPRING_UNBWT_H_

#include <stddef.h>
#include <stdint.h>

#include "spring_bwt.h"
#include "spring_unqlfc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPRING_UNBWT_PASSES 6

typedef struct spring_unbwt_ctx spring_unbwt_ctx;

typedef struct {
  uint64_t num_segments;
  uint64_t bytes;
  uint64_t max_segment;     /* the longest segment                                                        */
  uint64_t sub_batches;
  uint64_t heads;           /* sublist heads, summed over the sub-batches (row 0 and primary rows included) */
  uint64_t head_spacing;    /* K: one regular head in every K rows                                         */
  uint64_t max_walk;        /* the longest sublist: steps from a head to the next head                     */
  uint64_t rank_rounds;     /* pointer-doubling rounds of the sub-batch that took most                     */
  uint64_t workspace_bytes; /* the budget the sub-batches were planned for                                 */
  double ms_device;         /* HIP events around the device passes, input copies excluded                  */
  double ms_pass[SPRING_UNBWT_PASSES]; /* keys, sort, LF scatter, sublist walk, ranking + check, write     */
} spring_unbwt_info;

int spring_unbwt_create(int device, spring_unbwt_ctx **out);
void spring_unbwt_destroy(spring_unbwt_ctx *ctx);

/* Device workspace the per-row arrays of a sub-batch may use; 0 (the default) takes it from the free HBM at the time of
 * the call.  The sort's fixed tables (at most 8 MiB) come on top.  spring_unbwt_workspace_need: what a sub-batch of
 * `bytes` bytes in `segments` segments takes of it. */
int spring_unbwt_set_workspace_bytes(spring_unbwt_ctx *ctx, uint64_t workspace_bytes);
uint64_t spring_unbwt_workspace_need(uint64_t bytes, uint64_t segments);
/* K, the distance between two regular sublist heads: a power of two in 16 .. 1024; 0 (the default) is 64.  The result
 * does not depend on it. */
int spring_unbwt_set_head_spacing(spring_unbwt_ctx *ctx, uint32_t head_spacing);

int spring_unbwt_from_host(spring_unbwt_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const uint64_t *seg_off,
                           const int32_t *primary, uint64_t num_segments, spring_unbwt_info *info);
int spring_unbwt_from_bwt(spring_unbwt_ctx *ctx, spring_bwt_ctx *bwt, spring_unbwt_info *info);
int spring_unbwt_from_unqlfc(spring_unbwt_ctx *ctx, spring_unqlfc_ctx *unqlfc, const int32_t *primary /* [num_segments] */,
                             spring_unbwt_info *info);

/* text: info.bytes bytes, the segments back to back; seg_off: info.num_segments + 1 offsets into it.  Either may be
 * NULL. */
int spring_unbwt_download(spring_unbwt_ctx *ctx, uint8_t *text, uint64_t *seg_off);

int spring_unbwt_get_info(spring_unbwt_ctx *ctx, spring_unbwt_info *info);

/* bsc_bwt_decode's own contract (libbsc/bwt/bwt.h): T[0..n) on the host, a transform with primary index `index`, is
 * replaced by its text; returns 0 or a negative SPRING_REORDER_E_* (T is untouched then).  num_indexes and indexes
 * are accepted as bsc_bwt_decode takes them and not read; indexes may be NULL.  n = 0 with index 0 returns 0. */
int spring_unbwt_decode_inplace(spring_unbwt_ctx *ctx, uint8_t *T, int32_t n, int32_t index, uint8_t num_indexes,
                                const int32_t *indexes);

#ifdef __cplusplus
}
#endif
#endif
