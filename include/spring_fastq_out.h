/*
 * include/spring_fastq_out.h -- C ABI of the MI355X (gfx950) FASTQ assembler: the text decompress_short finally
 * writes, built on the device from decoded reads, quality lines and id lines (INTEGRATION.md
 * section 9).
 *
 * Replaces the tail of spring::decompress_short (reference src/decompress.cpp:357-419: fake ids, modify_id, the
 * start_num / end_num cut) and the plain-text branch of write_fastq_block (src/util.cpp:56-69) with modify_id
 * (src/util.cpp:255-267), after their codec calls (BSC_str_array_decompress, decompress_id_block):
 *
 *   window    blocks [first_block, first_block + num_blocks) of one mate j (0 = read 1 / file 1, 1 = read 2 / file 2).
 *             Block b of the file holds slots [b * B, min((b + 1) * B, U)), B = num_reads_per_block, U = num_reads
 *             (single-end) or num_reads / 2 (pairs).  The window's units u = 0 .. nu - 1 have global slot
 *             g = first_block * B + u.
 *   record    id[u] '\n' read[u] '\n'                         preserve_quality = 0
 *             id[u] '\n' read[u] '\n' '+' '\n' qual[u] '\n'   preserve_quality = 1
 *             in slot order, back to back: one contiguous text plus n + 1 record offsets.
 *   reads     bases back to back plus nu + 1 offsets: a spring_decode_ctx holding a successful decode of exactly this
 *             window (mate j is read in HBM, the decode context is left as it was), or host memory as
 *             spring_decode_download gives it.
 *   quality   the window's lines back to back without separators; line u is as long as read u (BSC_str_array_decompress
 *             with read_lengths_array).  A spring_qualid_ctx holding a quality result of the whole file (read in HBM),
 *             or host memory.  Bytes pass through unchanged.  A block table (num_blocks + 1 offsets), when given, must
 *             start at 0, be monotone, span the bytes, and block b must hold exactly the sum of its units' read
 *             lengths; the total must equal the bases of the mate.
 *   ids       SPRING_FASTQ_OUT_ID_STORED: the window's lines, each ended by '\n' (the id result of the quality / id
 *             stage; the string array decompress_id_block fills), from a spring_qualid_ctx or host memory: exactly nu
 *             lines, the last byte '\n'; a block table, when given, must start at 0, be monotone, span the bytes, and
 *             block b must hold exactly its units' lines.
 *             SPRING_FASTQ_OUT_ID_NUMBERED (preserve_id = 0): "@" + decimal(g + 1) + "/" + decimal(j + 1); g + 1
 *             counts from the start of the file (num_reads_done + i + 1).  No id source may be given.
 *             SPRING_FASTQ_OUT_ID_FROM_MATE_1 (paired_id_match, j = 1 only): the stored ids of file 1 with
 *             modify_id(paired_id_code): 2 unchanged; 1 the last byte becomes '2'; 3 the byte after the first ' '
 *             becomes '2'.  Where the reference has undefined behaviour the call is refused: an empty id under code 1;
 *             an id without a space, or with its first space as the last byte, under code 3.  A code outside 1..3
 *             is refused.
 *   range     units [range_start, range_end) of the window (start_num % B and the end_num cut); range_end =
 *             SPRING_FASTQ_OUT_TO_END means nu.  The checks cover the whole window, the text the range only; numbered
 *             ids keep their global numbers.  An empty range gives an empty text and is no error.
 *
 * Refused with SPRING_REORDER_E_ARG before any allocation: mate 1 of single-end data, a decode whose window differs
 * from the one asked for, a quality / id context whose num_units or num_reads_per_block does not fit, an id source
 * together with numbered ids, a missing quality or id source, mate 0 with ID_FROM_MATE_1, a code outside 1..3, a
 * range outside the window.  Everything else is checked on the device, one bit of an error word each, read once:
 * read offsets that do not start at 0 or decrease, a read or id longer than 2^30 bytes, the line count and final
 * '\n' of the ids, both block tables, the modify_id cases above.  Any refusal leaves the context without a result.
 * A call without reads, a source context without a result, and a download / write without a result give
 * SPRING_REORDER_E_STATE.
 *
 * Return value: 0 on success, negative SPRING_REORDER_E_* on error; text in spring_reorder_last_error().
 */
#ifndef SPRING_FASTQ_OUT_H_
#define SPRING_FASTQ_OUT_H_

#include <stddef.h>
#include <stdint.h>

#include "spring_decode.h"
#include "spring_qualid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPRING_FASTQ_OUT_ID_STORED 0
#define SPRING_FASTQ_OUT_ID_NUMBERED 1
#define SPRING_FASTQ_OUT_ID_FROM_MATE_1 2
#define SPRING_FASTQ_OUT_TO_END UINT64_MAX

typedef struct spring_fastq_out_ctx spring_fastq_out_ctx;

typedef struct {
  uint32_t first_block, num_blocks;   /* the window                                                            */
  uint32_t num_reads;                 /* cp.num_reads                                                          */
  uint32_t num_reads_per_block;
  int32_t paired_end;
  int32_t mate;                       /* j: 0 or 1                                                             */
  int32_t preserve_quality;
  int32_t id_mode;                    /* SPRING_FASTQ_OUT_ID_*                                                 */
  int32_t paired_id_code;             /* ID_FROM_MATE_1 only                                                   */
  int32_t pad;
  uint64_t range_start, range_end;    /* units of the window; range_end = SPRING_FASTQ_OUT_TO_END: all of them */
} spring_fastq_out_params;

/* For each of reads / quality / ids: the context, or else the host pointers (both NULL: no such source). */
typedef struct {
  spring_decode_ctx *decode;          /* reads of params.mate in HBM                                           */
  const char *bases;                  /* or: host, read_off[nu] bytes                                          */
  const uint64_t *read_off;           /*     host, nu + 1 offsets from 0                                       */
  spring_qualid_ctx *quality_ctx;     /* quality result of the whole file in HBM                               */
  const uint8_t *quality;             /* or: host, quality_bytes bytes of the window                           */
  uint64_t quality_bytes;
  const uint64_t *quality_block_off;  /*     host, num_blocks + 1 offsets from 0, or NULL                      */
  spring_qualid_ctx *id_ctx;          /* id result of the whole file in HBM                                    */
  const uint8_t *ids;                 /* or: host, id_bytes bytes of the window                                */
  uint64_t id_bytes;
  const uint64_t *id_block_off;       /*     host, num_blocks + 1 offsets from 0, or NULL                      */
} spring_fastq_out_sources;

typedef struct {
  uint64_t num_units;     /* records in the text (the range)                                     */
  uint64_t first_slot;    /* global slot g of the first of them                                  */
  uint64_t bytes;         /* length of the text                                                  */
  double ms_device;       /* HIP events around the device passes, input copies excluded          */
  double ms_file;         /* spring_fastq_out_write: wall time of the last call                  */
} spring_fastq_out_info;

int spring_fastq_out_create(int device, spring_fastq_out_ctx **out);
void spring_fastq_out_destroy(spring_fastq_out_ctx *ctx);

/* Builds the text of one mate over one window in HBM.  The source contexts are read in place and left as they were;
 * they must live on the device of ctx. */
int spring_fastq_out_assemble(spring_fastq_out_ctx *ctx, const spring_fastq_out_params *params,
                              const spring_fastq_out_sources *sources, spring_fastq_out_info *info);

/* text: info.bytes bytes; rec_off: info.num_units + 1 offsets into text.  Either may be NULL. */
int spring_fastq_out_download(spring_fastq_out_ctx *ctx, uint8_t *text, uint64_t *rec_off);
/* The text to a plain file through a ring of pinned staging chunks (gzip output: include/spring_gzip.h).  append = 0
 * truncates.  A file that cannot be opened or written gives SPRING_REORDER_E_IO. */
int spring_fastq_out_write(spring_fastq_out_ctx *ctx, const char *path, int32_t append, spring_fastq_out_info *info);

int spring_fastq_out_get_info(spring_fastq_out_ctx *ctx, spring_fastq_out_info *info);

#ifdef __cplusplus
}
#endif
#endif
