/*
 * include/spring_streams.h -- C ABI of the MI355X (gfx950) per-block read streams, the last stage of SPRING's read
 * side.
 *
 * Replaces what spring::reorder_compress_streams (reference src/reorder_compress_streams.cpp:31-441) computes up to,
 * not including, its BSC_compress calls: the encoder's flat streams (read_pos.bin, read_noise.txt,
 * read_noisepos.bin, read_rev.txt, read_order.bin, read_lengths.bin, read_unaligned.txt) scattered into the final
 * read order and cut into blocks of num_reads_per_block reads (pairs for paired-end data).  The output for block b
 * and stream s is byte for byte the file <stream>.<b> the reference compresses into <stream>.<b>.bsc, i.e. what
 * decompress_short gets back from BSC_decompress (decompress.cpp:223-321).
 *
 * The input is checked before anything is written (the reference checks none of it): n_total == num_reads, order
 * a permutation of [0, num_reads) when it is used (paired-end or preserve_order), an even num_reads for paired-end
 * data, num_reads_per_block > 0, one noise line per aligned read, one noise position per noise character, unaligned
 * records that match read_lengths.bin and hold only the codes A G C T N.  Violations give SPRING_REORDER_E_ARG.
 *
 * Return value: 0 on success, negative SPRING_REORDER_E_* on error; text in spring_reorder_last_error().
 */
#ifndef SPRING_STREAMS_H_
#define SPRING_STREAMS_H_

#include <stdint.h>

#include "spring_encoder.h"

#ifdef __cplusplus
extern "C" {
#endif

/* stream ids: the order of the BSC calls of reorder_compress_streams.cpp:376-424 is not kept, these are fixed ids */
#define SPRING_STREAMS_FLAG 0      /* read_flag.txt      '0'..'4' per pair ('0' / '2' per single-end read)     */
#define SPRING_STREAMS_POS 1       /* read_pos.bin       u64 absolute, or u16 delta / 65535 + u64 escape       */
#define SPRING_STREAMS_NOISE 2     /* read_noise.txt     noise characters + '\n' per aligned read              */
#define SPRING_STREAMS_NOISEPOS 3  /* read_noisepos.bin  u16 per noise character (as the encoder stored them)  */
#define SPRING_STREAMS_REV 4       /* read_rev.txt       'd' / 'r'                                             */
#define SPRING_STREAMS_UNALIGNED 5 /* read_unaligned.txt bases of the unaligned reads, no separators           */
#define SPRING_STREAMS_LENGTHS 6   /* read_lengths.bin   u16 per read (both reads of a pair)                   */
#define SPRING_STREAMS_POS_PAIR 7  /* read_pos_pair.bin  int16 pos2 - pos1 (paired-end, flag 0)                */
#define SPRING_STREAMS_REV_PAIR 8  /* read_rev_pair.txt  '0' orientations differ, '1' same (paired-end, flag 0) */
#define SPRING_STREAMS_NUM 9

typedef struct spring_streams_ctx spring_streams_ctx;

typedef struct {
  uint64_t num_units;                    /* reads (single-end) or pairs (paired-end)                          */
  uint64_t num_blocks;                   /* ceil(num_units / num_reads_per_block)                              */
  uint64_t bytes[SPRING_STREAMS_NUM];    /* all blocks of a stream together                                    */
  uint64_t flag_count[5];                /* units per flag value                                               */
  uint64_t pos_escapes;                  /* 65535 escapes written to read_pos.bin (not preserve_order)         */
  uint64_t n_aligned;                    /* aligned reads of the input                                         */
  double ms_device;                      /* HIP-event time of the device passes (input copies and pe_encode excluded) */
  double ms_file;                        /* spring_streams_run only: wall time of the whole file contract      */
} spring_streams_info;

int spring_streams_create(int device, spring_streams_ctx **out);
void spring_streams_destroy(spring_streams_ctx *ctx);

/* From the streams an encoder context holds in HBM (spring_encoder_encode_reorder / _encode_host): nothing leaves the
 * device.  num_reads = cp.num_reads (must equal the encoder's n_total).  apply_pe_encode = 1 (paired-end data without
 * preserve_order only) runs pe_encode (pe_encode.cpp:24-84) on the device on a private copy of the encoder's order:
 * the encoder context is left as it was, so reorder_compress_quality_id can still read its read_order.bin.  With
 * apply_pe_encode = 0 the encoder's order is taken as it is. */
int spring_streams_from_encoder(spring_streams_ctx *ctx, spring_encoder_ctx *enc, uint32_t num_reads, int32_t paired_end,
                                int32_t preserve_order, uint32_t num_reads_per_block, int32_t apply_pe_encode,
                                spring_streams_info *info);

/* From the in-memory images of the encoder's files, for streams of any encoder (the reference's included):
 *   pos[n_aligned] read_pos.bin; rc[n_aligned] read_rev.txt; noise read_noise.txt; noisepos read_noisepos.bin;
 *   order[n_total] read_order.bin (read only for paired-end or preserve_order data, may be NULL otherwise; already
 *   through pe_encode for paired-end data without preserve_order, as spring.cpp:190-206 runs it);
 *   rlen[n_total] read_lengths.bin; unaligned read_unaligned.txt (write_dnaN_in_bits records). */
int spring_streams_from_host(spring_streams_ctx *ctx, const uint64_t *pos, const char *rc, uint64_t n_aligned,
                             const char *noise, uint64_t noise_bytes, const uint16_t *noisepos, uint64_t n_noisepos,
                             const uint32_t *order, const uint16_t *rlen, uint64_t n_total, const uint8_t *unaligned,
                             uint64_t unaligned_bytes, uint32_t num_reads, int32_t paired_end, int32_t preserve_order,
                             uint32_t num_reads_per_block, spring_streams_info *info);

/* Copy stream_id of the last successful call to the host: bytes (info.bytes[stream_id] bytes, all blocks back to back)
 * and block_off (num_blocks + 1 offsets into bytes: block b is [block_off[b], block_off[b + 1])).  Either pointer may
 * be NULL. */
int spring_streams_download(spring_streams_ctx *ctx, int32_t stream_id, uint8_t *bytes, uint64_t *block_off);

int spring_streams_get_info(spring_streams_ctx *ctx, spring_streams_info *info);

/* File contract of reorder_compress_streams(temp_dir, cp) up to, not including, its BSC calls: reads the files
 * encoder_main, spring_encoder_run or spring_reorder_encode_run leave in temp_dir (read_order.bin after pe_encode for
 * paired-end data without preserve_order), writes temp_dir/<stream>.<b> for every stream and block (read_pos_pair.bin
 * and read_rev_pair.txt for paired-end data only) and removes its inputs as reorder_compress_streams.cpp:145-182 does,
 * read_unaligned.txt.count included.  The caller runs BSC_compress(f, f + ".bsc") and remove(f) on every output
 * (INTEGRATION.md section 6).  If the input fails a check, nothing is written and nothing is removed.
 * num_reads = cp.num_reads, num_reads_per_block = cp.num_reads_per_block. */
int spring_streams_run(const char *temp_dir, uint32_t num_reads, int32_t paired_end, int32_t preserve_order,
                       uint32_t num_reads_per_block, int32_t device, spring_streams_info *info);

#ifdef __cplusplus
}
#endif
#endif
