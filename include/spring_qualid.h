/*
 * include/spring_qualid.h -- C ABI of the MI355X (gfx950) quality and id stage: the quality lines and id lines of a
 * FASTQ put into the final read order and cut into blocks.
 *
 * Replaces the quality / id side of spring::preprocess (reference src/preprocess.cpp:200-250, the quantize_quality
 * table lookup of util.cpp:143-149 included) and spring::reorder_compress_quality_id
 * (src/reorder_compress_quality_id.cpp:34-235) up to, not including, their codec calls (quantize_quality_qvz,
 * BSC_str_array_compress, compress_id_block).  compress_id_block is the id codec stage (spring_idcodec.h), which takes
 * the id result of a context where it lies in HBM; the block sort of BSC_str_array_compress is spring_bwt.h:
 *
 *   order     read_order.bin as the encoder leaves it, BEFORE pe_encode (spring.cpp:176-206).  Single-end:
 *             order_array[order[i]] = i, U = num_reads units.  Paired-end: for i < num_reads, if order[i] <
 *             num_reads/2 then order_array[order[i]] = pos++; U = num_reads/2 units, and the same order_array serves
 *             file 1 and file 2.  Line j of a file goes to slot order_array[j].  No order (NULL) = identity, the
 *             blocks preprocess.cpp:231-250 cuts under preserve_order.
 *   blocks    block b holds slots [b * B, min((b + 1) * B, U)), B = num_reads_per_block; ceil(U / B) blocks.
 *   quality   a block is its lines back to back without separators (the input of BSC_str_array_compress,
 *             bsc_str_array.cpp:125-175) plus their lengths.  A 128-byte table (spring_quality_table, or any other)
 *             is applied to every byte on the way; a byte >= 128 under a table is refused (the reference indexes a
 *             128-entry table with it).
 *   id        a block is its lines, each terminated by '\n' (the std::string array of compress_id_block), plus
 *             their lengths without the '\n'.
 *   FASTQ     id = line 0 of a record, whole, with its '@'; quality = line 3; a trailing '\r' is dropped from each
 *             (util.cpp:31-54); a missing final newline is accepted.
 *
 * Everything is checked before a result exists: an order that is not a permutation of [0, num_reads), an odd
 * num_reads for paired-end data, a line count that differs from U, num_reads_per_block == 0, a quality byte >= 128
 * under a table, "Read length does not match quality length." (preprocess.cpp:200-202), a line count that is no
 * multiple of 4, a line longer than uint32.  Each gives SPRING_REORDER_E_ARG; a call before an order is set and a
 * download after a refused call give SPRING_REORDER_E_STATE.
 *
 * Return value: 0 on success, negative SPRING_REORDER_E_* on error; text in spring_reorder_last_error().
 */
#ifndef SPRING_QUALID_H_
#define SPRING_QUALID_H_

#include <stddef.h>
#include <stdint.h>

#include "spring_encoder.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPRING_QUALID_QUALITY 0
#define SPRING_QUALID_ID 1

typedef struct spring_qualid_ctx spring_qualid_ctx;

typedef struct {
  uint64_t num_units;     /* reads (single-end) or pairs (paired-end)                                           */
  uint64_t num_blocks;    /* ceil(num_units / num_reads_per_block)                                              */
  uint64_t bytes[2];      /* output bytes of the quality / id result of the last call (0 = not asked for)       */
  uint64_t bytes_changed; /* quality bytes the table altered                                                    */
  uint32_t max_len[2];    /* longest quality / id line (without the id's '\n')                                  */
  double ms_device;       /* HIP events around the device passes, input copy excluded                           */
} spring_qualid_info;

int spring_qualid_create(int device, spring_qualid_ctx **out);
void spring_qualid_destroy(spring_qualid_ctx *ctx);

/* order = image of read_order.bin before pe_encode (num_reads entries); NULL = identity (preserve_order).  Setting an
 * order drops the results of earlier calls; a refused order leaves the context without one. */
int spring_qualid_order_from_host(spring_qualid_ctx *ctx, const uint32_t *order, uint32_t num_reads, int32_t paired_end);
/* The encoder's order in HBM (spring_encoder_encode_reorder / _encode_host): nothing leaves the device, and the
 * encoder context is left as it was.  num_reads must equal the encoder's n_total. */
int spring_qualid_order_from_encoder(spring_qualid_ctx *ctx, spring_encoder_ctx *enc, uint32_t num_reads,
                                     int32_t paired_end);

/* One input file (mate 0 or 1), plain text or a gzip image (what spring_reorder_load_fastq takes).
 * want: bit 0 quality, bit 1 id.  table: 128 bytes or NULL (lossless). */
int spring_qualid_from_fastq(spring_qualid_ctx *ctx, const uint8_t *fastq, size_t nbytes, int32_t want,
                             const uint8_t *table, uint32_t num_reads_per_block, spring_qualid_info *info);
/* Image of quality_j / id_j as preprocess writes them: one '\n'-terminated line per read, file order.  kind =
 * SPRING_QUALID_QUALITY or SPRING_QUALID_ID; table is read for quality lines only. */
int spring_qualid_from_lines(spring_qualid_ctx *ctx, int32_t kind, const uint8_t *lines, size_t nbytes,
                             const uint8_t *table, uint32_t num_reads_per_block, spring_qualid_info *info);

/* bytes: all blocks back to back (info.bytes[kind] bytes); len: num_units line lengths in slot order (without the
 * id's '\n'); block_off: num_blocks + 1 offsets into bytes.  Any pointer may be NULL. */
int spring_qualid_download(spring_qualid_ctx *ctx, int32_t kind, uint8_t *bytes, uint32_t *len, uint64_t *block_off);
int spring_qualid_get_info(spring_qualid_ctx *ctx, spring_qualid_info *info);

/* Host only.  mode 1 = Illumina 8-level binning (util.cpp:166-180), 2 = binary (util.cpp:182-188: byte < 33 + thr ->
 * 33 + low, else 33 + high; refused unless low <= thr <= high, spring.cpp:124-126, and high <= 94). */
int spring_quality_table(int32_t mode, uint32_t thr, uint32_t high, uint32_t low, uint8_t table[128]);

/* paired_id_code 0..3 of two FASTQ texts (util.cpp:196-253): find_id_pattern on the first pair on the host, then
 * check_id_pattern on every pair on the device; 0 unless every pair matches.  For an empty id codes 1 and 3 are
 * "no match" (the reference reads id[len - 1]); equal empty ids still give code 2. */
int spring_id_pattern(const uint8_t *fastq_1, size_t nbytes_1, const uint8_t *fastq_2, size_t nbytes_2, int32_t device,
                      uint8_t *paired_id_code, double *ms_device);

#ifdef __cplusplus
}
#endif
#endif
