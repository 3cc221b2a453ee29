/*
 * include/spring_unqlfc.h -- C ABI of the MI355X (gfx950) QLFC decoder stage: libbsc's bsc_coder_decompress with
 * LIBBSC_CODER_QLFC_STATIC in fast mode for a batch of coded segments in HBM (INTEGRATION.md
 * section 17).  The exact inverse of spring_qlfc.h.
 *
 * Replaces the bsc_coder_decompress call of bsc_decompress (reference libbsc/coder/coder.cpp:171-217; the decoder is
 * bsc_qlfc_static_decode, libbsc/coder/qlfc/qlfc.cpp:1038-1297, over the range decoder of coder/common/rangecoder.h:
 * 152-205).  On every well-formed segment the bytes are the reference's.  A coded segment is, as spring_qlfc.h writes it:
 *
 *   bytes      one chunk: [1][payload].  Several: [k][k x (int32 input size, int32 coded size)][payloads].  A chunk of
 *              several whose coded size equals its input size is raw and is copied.
 *   payload    16-bit units, little-endian, at whatever address the segment and its header put them: the 32 bits of the
 *              chunk's size, the symbol table (the chunk's symbols in the order they first occur, then the last one again
 *              unless all 256 are listed; a bit is there only where both of its values are still possible), then per
 *              run its rank in the move-to-front list and its length, every binary decision read with the weighted sum
 *              of three adaptive predictors.  The decoder reads three units to start and one per normalisation.
 *   out_size   the size of the decoded segment, which the block header holds (bsc_decompress gets it from there).  It
 *              is required: it sizes the output and bounds every loop.
 *
 * Well-formedness.  bsc_coder_decompress trusts its input; where it would read or write outside its buffers the stage
 * refuses instead.  A segment is malformed when
 *
 *   chunks     k = 0, or the segment has no bytes although out_size > 0
 *   table      the chunk table does not fit the coded length (1 + 8 k bytes)
 *   entry      a table entry is negative, or its coded size is above its input size
 *   sum        the input sizes do not add up to out_size
 *   length     1 + 8 k + the coded sizes is not the coded length (one chunk: the payload is the coded length - 1)
 *   size       the 32-bit size decoded from a payload is not the chunk's input size
 *   rank       a decoded rank is 0, or is not below the number of entries of the chunk's symbol table (its symbols,
 *              plus one where the last symbol is listed again)
 *   exponent   a run-length exponent reaches 32
 *   run        a run passes the end of its chunk
 *   units      the decoder needs a 16-bit unit beyond its payload.  A well-formed payload is read exactly to its end:
 *              the encoder writes one unit per normalisation plus three (tests/test_unqlfc_cpu.py asserts it on every
 *              case)
 *
 * A malformed segment refuses the call: SPRING_REORDER_E_ARG, the first such segment and its rule named in
 * spring_reorder_last_error(), no result left.  No store for a malformed segment leaves that segment's own out_size
 * bytes.  A segment without coded bytes and with out_size 0 is empty (info.skipped): what a QLFC context leaves for a
 * segment that is not compressible, whose block the caller stores.
 *
 * The two state tables come from the caller, as in spring_qlfc.h.  A batch is S coded segments back to back with S + 1
 * offsets and S output sizes, worked off in sub-batches of whole segments that fit the workspace budget
 * (info.sub_batches): every coded chunk takes SPRING_UNQLFC_MODEL_BYTES of it for its predictors.
 *
 *   from_host   offsets start at 0, do not decrease and end at ncoded.
 *   from_qlfc   the coded segments of a finished QLFC context (spring_qlfc.h), read in place in HBM and left as they
 *               were; the output sizes are that context's input sizes, 0 for a segment it left not compressible.
 *
 * Refused before any result: offsets that do not start at 0, decrease or do not end at ncoded, a NULL buffer with
 * ncoded > 0, NULL offsets or sizes with S > 0, a coded or decoded segment above 1 GiB or one that does not fit the
 * workspace budget, a QLFC context on another device (SPRING_REORDER_E_ARG); any decoding call before
 * spring_unqlfc_set_state_tables, a QLFC context without a result (SPRING_REORDER_E_STATE).  A refused call leaves the
 * context without a result; download / get_info without a result give SPRING_REORDER_E_STATE.
 *
 * Return value: 0 on success, negative SPRING_REORDER_E_* on error; text in spring_reorder_last_error().
 */
#ifndef SPRING_UNQLFC_H_
#define SPRING_UNQLFC_H_

#include <stddef.h>
#include <stdint.h>

#include "spring_qlfc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPRING_UNQLFC_PASSES 3
#define SPRING_UNQLFC_MAX_SEGMENT (1u << 30)
#define SPRING_UNQLFC_MODEL_BYTES 1619200   /* the predictors of one coded chunk in the workspace */

typedef struct spring_unqlfc_ctx spring_unqlfc_ctx;

typedef struct {
  uint64_t num_segments;
  uint64_t bytes_in;          /* coded bytes                                                             */
  uint64_t bytes_out;         /* decoded bytes                                                           */
  uint64_t chunks;            /* raw ones included                                                       */
  uint64_t chunks_raw;
  uint64_t runs;
  uint64_t events;            /* binary decisions read with predictors (size and symbol-table bits are not events) */
  uint64_t skipped;           /* segments without coded bytes                                            */
  uint64_t sub_batches;
  uint64_t workspace_bytes;   /* the budget the sub-batches were planned for                             */
  double ms_device;           /* HIP events around the device passes, input copies excluded              */
  double ms_pass[SPRING_UNQLFC_PASSES]; /* plan (chunk tables), decode (predictor fill + walk), raw copies */
} spring_unqlfc_info;

int spring_unqlfc_create(int device, spring_unqlfc_ctx **out);
void spring_unqlfc_destroy(spring_unqlfc_ctx *ctx);

/* The two state tables, copied to the device; they stay until they are set again. */
int spring_unqlfc_set_state_tables(spring_unqlfc_ctx *ctx, const uint8_t *rank_table /* [32768] */,
                                   const uint8_t *run_table /* [8192] */);
/* Device workspace a sub-batch may use; 0 (the default) takes it from the free HBM at the time of the call.
 * spring_unqlfc_workspace_need: what a sub-batch that decodes `bytes_out` bytes in `chunks` chunks takes of it. */
int spring_unqlfc_set_workspace_bytes(spring_unqlfc_ctx *ctx, uint64_t workspace_bytes);
uint64_t spring_unqlfc_workspace_need(uint64_t bytes_out, uint64_t chunks);

int spring_unqlfc_from_host(spring_unqlfc_ctx *ctx, const uint8_t *coded, uint64_t ncoded, const uint64_t *coded_off,
                            const uint64_t *out_size, uint64_t num_segments, spring_unqlfc_info *info);
int spring_unqlfc_from_qlfc(spring_unqlfc_ctx *ctx, spring_qlfc_ctx *qlfc, spring_unqlfc_info *info);

/* bytes: info.bytes_out bytes, the decoded segments back to back; seg_off: num_segments + 1 offsets into bytes.  Either
 * may be NULL. */
int spring_unqlfc_download(spring_unqlfc_ctx *ctx, uint8_t *bytes, uint64_t *seg_off);
int spring_unqlfc_get_info(spring_unqlfc_ctx *ctx, spring_unqlfc_info *info);

/* bsc_coder_decompress's contract on host buffers (libbsc/coder/coder.h) plus the two sizes it leaves to its caller:
 * in[0..in_size) is decoded into out[0..out_size); returns the decoded size (out_size) or a negative
 * SPRING_REORDER_E_* (out is untouched then). */
int spring_unqlfc_decompress(spring_unqlfc_ctx *ctx, const uint8_t *in, int32_t in_size, uint8_t *out, int32_t out_size);

#ifdef __cplusplus
}
#endif
#endif
