/*
 * include/spring_qlfc.h -- C ABI of the MI355X (gfx950) QLFC stage: libbsc's bsc_coder_compress with
 * LIBBSC_CODER_QLFC_STATIC in fast mode for a batch of byte segments in HBM (INTEGRATION.md
 * section 14).
 *
 * Replaces the bsc_coder_compress call of bsc_compress (reference src/libbsc/libbsc/libbsc/libbsc.cpp:171-187; the
 * coder is libbsc/coder/coder.cpp:110-160 and bsc_qlfc_static_encode, libbsc/coder/qlfc/qlfc.cpp:448-752) for the
 * block-sorted segments the block-sort stage leaves in HBM.  For a segment of n >= 1 bytes:
 *
 *   chunks     1 below 256 KiB, 2 below 4 MiB, 4 below 16 MiB, else 8, cut as bsc_coder_split_blocks cuts: the positions
 *              1, 33, 65, ... whose byte differs from the one before are counted; if there are more than chunks, every
 *              (count / chunks)-th of them is a cut, else the chunks are n / chunks bytes and the last takes the rest.
 *   bytes      one chunk: [1][payload].  Several: [k][k x (int32 input size, int32 coded size)][payloads].
 *   payload    the 32 bits of the chunk's size, the symbol table, the runs (rank, then length; every binary decision
 *              coded with the weighted sum of three adaptive predictors), three closing shifts of the range coder.
 *   a chunk fails  when the coder has written output_size - 16 bytes or more at the start of its last run;
 *              output_size is n - 1 for a single chunk, else min(chunk size, n - bytes of the segment so far).  A
 *              failed chunk of several is stored raw (coded size == input size) if bytes so far + chunk size < n.
 *   status     0: coded.  1: not compressible (a single chunk failed, or a failed chunk could not be stored raw): no
 *              bytes; the reference returns LIBBSC_NOT_COMPRESSIBLE and bsc_compress stores the block, which stays
 *              the caller's rule.  n = 0: status 1, no bytes (the reference is never called so, libbsc.cpp:123).
 *
 * The two state tables that map a run's context to a predictor (libbsc's model_rank_state_table[32768] and
 * model_run_state_table[8192], coder/common/tables.h) come from the caller: spring_qlfc_set_state_tables.  The library
 * holds no copy of them.
 *
 * A batch is S segments back to back with S + 1 offsets.  It is worked off in sub-batches of whole segments that fit
 * the workspace budget (info.sub_batches); a sub-batch whose events turn out not to fit is halved.
 *
 *   from_host   offsets start at 0, do not decrease and end at nbytes; NULL offsets mean one segment.
 *   from_bwt    the transformed segments of a finished block-sort context (spring_bwt.h), read in place in HBM and left
 *               as they were; same segments, same order.
 *
 * Refused before any result: offsets that do not start at 0, decrease or do not end at nbytes, a NULL buffer with
 * nbytes > 0, a segment above 1 GiB (as bsc_compress refuses it) or one that does not fit the workspace budget, a
 * block-sort context on another device (SPRING_REORDER_E_ARG); any coding call before spring_qlfc_set_state_tables, a
 * block-sort context without a result (SPRING_REORDER_E_STATE).  A refused call leaves the context without a result;
 * download / get_info without a result give SPRING_REORDER_E_STATE.
 *
 * Return value: 0 on success, negative SPRING_REORDER_E_* on error; text in spring_reorder_last_error().
 */
#ifndef SPRING_QLFC_H_
#define SPRING_QLFC_H_

#include <stddef.h>
#include <stdint.h>

#include "spring_bwt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPRING_QLFC_RANK_TABLE 32768
#define SPRING_QLFC_RUN_TABLE 8192
#define SPRING_QLFC_MAX_SEGMENT (1u << 30)
#define SPRING_QLFC_PASSES 6
#define SPRING_QLFC_NOT_COMPRESSIBLE (-16)   /* spring_qlfc_compress: where bsc_coder_compress returns LIBBSC_NOT_COMPRESSIBLE */

typedef struct spring_qlfc_ctx spring_qlfc_ctx;

typedef struct {
  uint64_t num_segments;
  uint64_t bytes_in;
  uint64_t bytes_out;
  uint64_t chunks;
  uint64_t runs;
  uint64_t events;            /* binary decisions coded with predictors (the size and symbol-table bits are not events) */
  uint64_t not_compressible;  /* segments with status 1                                                  */
  uint64_t chunks_raw;        /* chunks stored raw                                                       */
  uint64_t sub_batches;
  uint64_t workspace_bytes;   /* the budget the sub-batches were planned for                             */
  double ms_device;           /* HIP events around the device passes, input copies excluded              */
  double ms_pass[SPRING_QLFC_PASSES]; /* runs and ranks, contexts and events, slots (sort + chains),
                                 probabilities, range coder, assembly                                    */
} spring_qlfc_info;

int spring_qlfc_create(int device, spring_qlfc_ctx **out);
void spring_qlfc_destroy(spring_qlfc_ctx *ctx);

/* The two state tables, copied to the device; they stay until they are set again. */
int spring_qlfc_set_state_tables(spring_qlfc_ctx *ctx, const uint8_t *rank_table /* [32768] */,
                                 const uint8_t *run_table /* [8192] */);
/* Device workspace a sub-batch may use; 0 (the default) takes it from the free HBM at the time of the call.
 * spring_qlfc_workspace_need: what a sub-batch of `bytes` bytes in `segments` segments takes of it before its events
 * are counted; an event takes SPRING_QLFC_EVENT_BYTES more. */
int spring_qlfc_set_workspace_bytes(spring_qlfc_ctx *ctx, uint64_t workspace_bytes);
uint64_t spring_qlfc_workspace_need(uint64_t bytes, uint64_t segments);
#define SPRING_QLFC_EVENT_BYTES 160

int spring_qlfc_from_host(spring_qlfc_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const uint64_t *seg_off,
                          uint64_t num_segments, spring_qlfc_info *info);
int spring_qlfc_from_bwt(spring_qlfc_ctx *ctx, spring_bwt_ctx *bwt, spring_qlfc_info *info);

/* coded: info.bytes_out bytes, the coded segments back to back; coded_off: num_segments + 1 offsets into coded; status:
 * one int32 per segment.  Any may be NULL. */
int spring_qlfc_download(spring_qlfc_ctx *ctx, uint8_t *coded, uint64_t *coded_off, int32_t *status);
int spring_qlfc_get_info(spring_qlfc_ctx *ctx, spring_qlfc_info *info);

/* bsc_coder_compress's own contract on host buffers (libbsc/coder/coder.h): in[0..n) is coded into out, which holds
 * at least n bytes; returns the coded size, SPRING_QLFC_NOT_COMPRESSIBLE, or a negative SPRING_REORDER_E_*. */
int spring_qlfc_compress(spring_qlfc_ctx *ctx, const uint8_t *in, uint8_t *out, int32_t n);

#ifdef __cplusplus
}
#endif
#endif
