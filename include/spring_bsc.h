/*
 * include/spring_bsc.h -- C ABI of the MI355X (gfx950) BSC framing stage: libbsc's bsc_compress blocks and the files
 * BSC_compress / BSC_str_array_compress write, made in HBM from the block sort and the QLFC coder (DESIGN.md
 * section 19).
 *
 * Replaces what bsc_compress does around bsc_bwt_encode and bsc_coder_compress (reference
 * src/libbsc/libbsc/libbsc/libbsc.cpp:77-90 and :201-305) and what Compression() writes around it (libbsc/bsc.cpp:149-156,
 * :306-379; libbsc/bsc_str_array.cpp:183-250, :451-458) under SPRING's settings: no LZP, block sorter BWT, static QLFC,
 * recordSize 1, contexts following -- mode = 1 | 1 << 5.
 *
 * Block of a segment of n bytes with primary index p, k secondary indexes and r coded bytes; k' = 0 for n < 65536,
 * else k.  Seven little-endian 32-bit words, then the body:
 *
 *   coded            r + 1 + 4 k' + 28, n, mode, p, adler32(input), adler32(body), adler32(the 24 bytes before);
 *                    body = the coded bytes, k' int32 indexes, the byte k'
 *   stored           n + 28, n, 0, 0, adler32(input), adler32(input), adler32(the 24 bytes before); body = the input.
 *                    Where n <= 28 (SPRING_BSC_STORED_SMALL), where the coder reports not compressible
 *                    (SPRING_BSC_STORED_CODER) and where r + 1 + 4 k' >= n (SPRING_BSC_STORED_NO_GAIN).
 *
 * Files (framing): SPRING_BSC_BLOCKS -- bare blocks, one file per group of segments.  SPRING_BSC_FILE -- int32 nBlocks,
 * then per cut the packed 10 bytes {int64 offset of the cut in the file's input, int8 1, int8 1} and the block.
 * SPRING_BSC_STR_ARRAY -- int32 nBlocks, then per cut the 2 bytes {1, 1} and the block.  A file without cuts is the 4
 * bytes of nBlocks = 0 (no bytes with SPRING_BSC_BLOCKS).
 *
 * The from_* calls run the two stages in front themselves, on contexts the caller owns: spring_bwt_from_* with the
 * block-sort context's own block_bytes, run-key and workspace settings, then spring_qlfc_from_bwt, then the framing.
 * Both contexts keep their results.  The input is read in place: the streams or quality / id context must stay as it
 * is until the call returns.
 *
 *   from_streams  one SPRING_BSC_FILE file per (stream, block) slice whose stream is in stream_mask, in (stream,
 *                 block) order, the empty slices included.
 *   from_qualid   one SPRING_BSC_STR_ARRAY file per quality (or id) block; block_bytes as spring_bwt_from_qualid.
 *   from_host     segments as spring_bwt_from_host takes them; file_first[num_files + 1] groups consecutive segments
 *                 into files (it starts at 0, does not decrease and ends at num_segments), NULL: one file a segment.
 *                 A cut's offset is the sum of the segments before it in its file.
 *
 * Refused: a NULL context, contexts on different devices, offsets or a file_first that do not start at 0, decrease or
 * do not end where they must, a framing outside 0 .. 2 (SPRING_REORDER_E_ARG); a QLFC context without state tables,
 * download / files / get_info without a result (SPRING_REORDER_E_STATE).  An error of an inner stage is passed on.  A
 * refused or failed call leaves the context without a result.
 *
 * Return value: 0 on success, negative SPRING_REORDER_E_* on error; text in spring_reorder_last_error().
 */
#ifndef SPRING_BSC_H_
#define SPRING_BSC_H_

#include <stddef.h>
#include <stdint.h>

#include "spring_bwt.h"
#include "spring_qlfc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPRING_BSC_HEADER_BYTES 28 /* LIBBSC_HEADER_SIZE */
#define SPRING_BSC_PASSES 3
#define SPRING_BSC_BLOCKS 0 /* framing */
#define SPRING_BSC_FILE 1
#define SPRING_BSC_STR_ARRAY 2
#define SPRING_BSC_CODED 0 /* block_kind */
#define SPRING_BSC_STORED_SMALL 1
#define SPRING_BSC_STORED_CODER 2
#define SPRING_BSC_STORED_NO_GAIN 3

typedef struct spring_bsc_ctx spring_bsc_ctx;

typedef struct {
  uint64_t num_files;
  uint64_t num_blocks;
  uint64_t bytes_in;
  uint64_t bytes_out;
  uint64_t coded;           /* blocks per outcome */
  uint64_t stored_small;
  uint64_t stored_coder;
  uint64_t stored_no_gain;
  double ms_device;         /* HIP events around the framing's own passes; the inner stages report theirs */
  double ms_pass[SPRING_BSC_PASSES]; /* sums (input, body, header), plan (outcomes, scans, headers' fields), assembly */
} spring_bsc_info;

int spring_bsc_create(int device, spring_bsc_ctx **out);
void spring_bsc_destroy(spring_bsc_ctx *ctx);

int spring_bsc_from_streams(spring_bsc_ctx *ctx, spring_bwt_ctx *bwt, spring_qlfc_ctx *qlfc, spring_streams_ctx *streams,
                            uint32_t stream_mask, spring_bsc_info *info);
int spring_bsc_from_qualid(spring_bsc_ctx *ctx, spring_bwt_ctx *bwt, spring_qlfc_ctx *qlfc, spring_qualid_ctx *q,
                           int32_t kind, uint64_t block_bytes, spring_bsc_info *info);
int spring_bsc_from_host(spring_bsc_ctx *ctx, spring_bwt_ctx *bwt, spring_qlfc_ctx *qlfc, const uint8_t *bytes,
                         uint64_t nbytes, const uint64_t *seg_off, uint64_t num_segments, int32_t framing,
                         const uint64_t *file_first, uint64_t num_files, spring_bsc_info *info);

/* bytes: info.bytes_out bytes, the files back to back; file_off: info.num_files + 1 offsets into bytes; block_off:
 * per block the offset of its header in bytes; block_kind: per block SPRING_BSC_CODED .. _STORED_NO_GAIN.  Any may be
 * NULL. */
int spring_bsc_download(spring_bsc_ctx *ctx, uint8_t *bytes, uint64_t *file_off, uint64_t *block_off, int32_t *block_kind);
/* Per file: stream id and block as spring_bwt_segments reports them (from_host: -1 and the file's number), and its
 * first segment (the next file's is where its own end).  Any may be NULL. */
int spring_bsc_files(spring_bsc_ctx *ctx, int32_t *stream, uint32_t *block, uint64_t *first_segment);
int spring_bsc_get_info(spring_bsc_ctx *ctx, spring_bsc_info *info);

/* The sum kernel alone: bsc_adler32 of every segment of a host batch, 1 for an empty one.  Leaves the context's result
 * as it is. */
int spring_bsc_adler32(spring_bsc_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const uint64_t *seg_off,
                       uint64_t num_segments, uint32_t *sums);

/* bsc_compress's own contract (libbsc/libbsc.h) on host buffers that do not overlap: out holds n + 28 bytes; returns
 * the size of the block, stored where bsc_compress (or BSC_compress behind it) stores, or a negative
 * SPRING_REORDER_E_*. */
int spring_bsc_compress(spring_bsc_ctx *ctx, spring_bwt_ctx *bwt, spring_qlfc_ctx *qlfc, const uint8_t *in, uint8_t *out,
                        int32_t n);

#ifdef __cplusplus
}
#endif
#endif
