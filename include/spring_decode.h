/*
 * include/spring_decode.h -- C ABI of the MI355X (gfx950) decoder of SPRING's per-block read streams: the read part
 * of decompress_short (reference src/decompress.cpp:107-119, :201-321, :615-662), the inverse of
 * include/spring_streams.h.
 *
 * The consensus is loaded once (seq_from_*), then any window of blocks [first_block, first_block + num_blocks) is
 * decoded (from_*) into the reads of its units in slot order, read 1 and read 2 of paired-end data into two outputs
 * (fout[0] / fout[1] of the reference).  Block b of the file holds min(num_reads_per_block, U - b *
 * num_reads_per_block) units, U = num_reads (single-end) or num_reads / 2 (pairs); num_reads = cp.num_reads.
 *
 * The input is checked on the device and refused with SPRING_REORDER_E_ARG unless the reader would consume every
 * stream of every block exactly and read only what exists: a flag outside '0' '2' (single-end) or '0'..'4'
 * (paired-end); an orientation other than 'd' / 'r', a relative orientation other than '0' / '1'; a noise character
 * outside '0'..'3'; a noise position >= the read's length; a read that reaches past the consensus, by a u64 position,
 * a u16 delta or pos1 + int16; a stream that is under- or over-consumed in any block (a truncated escape, trailing
 * bytes, and read_pos.bin of a block that opens with an unaligned read 1 followed by an aligned one, where the
 * reader expects the u64 at the first aligned read 1 and the writer puts it at the first unit, all land here); an
 * unaligned byte other than A C G T N; block tables that do not start at 0, are not monotone or do not match the
 * byte counts.  Without a consensus a decode returns SPRING_REORDER_E_STATE.
 * Noise positions are decoded as the reader does: each is a u16 delta from the previous one of the same read (u16
 * arithmetic, so it may wrap), a repeated position is changed again, through dec_noise of its current base.
 * After a refusal the context holds no result: download returns SPRING_REORDER_E_STATE.
 *
 * Return value: 0 on success, negative SPRING_REORDER_E_* on error; text in spring_reorder_last_error().
 */
#ifndef SPRING_DECODE_H_
#define SPRING_DECODE_H_

#include <stdint.h>

#include "spring_encoder.h"
#include "spring_streams.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spring_decode_ctx spring_decode_ctx;

typedef struct {
  uint64_t seq_len;                 /* consensus bases held                                          */
  uint64_t first_block, num_blocks, num_units;
  uint64_t bases[2];                /* output bytes of read 1 / read 2 (read 2: paired-end only)     */
  uint64_t n_aligned, n_unaligned;  /* reads decoded from the consensus / copied from read_unaligned */
  uint64_t pos_escapes;             /* 65535 escapes met in read_pos.bin                             */
  double ms_device;                 /* HIP events around the decode passes (input copies excluded)  */
  double ms_file;                   /* _files entry points only: wall time of the whole call        */
} spring_decode_info;

int spring_decode_create(int device, spring_decode_ctx **out);
void spring_decode_destroy(spring_decode_ctx *ctx);

/* The consensus, held on the device until the next seq_from_* call or destroy. */
/* From an encoder context in HBM (HBM to HBM copy; the encoder context may be destroyed afterwards). */
int spring_decode_seq_from_encoder(spring_decode_ctx *ctx, spring_encoder_ctx *enc);
/* From the images spring_encoder_download_seq_packed gives: seq_len_tid[num_thr_e] bases per tid, packed = the
 * floor(len / 4) bytes of every tid back to back (A0 C1 G2 T3, first base in the low bits), tail = 4 characters per
 * tid of which the first len % 4 are used. */
int spring_decode_seq_from_host(spring_decode_ctx *ctx, int32_t num_thr_e, const uint64_t *seq_len_tid,
                                const uint8_t *packed, const char *tail);
/* From temp_dir/read_seq.bin.<tid> (packed, as BSC_decompress leaves it) and read_seq.bin.<tid>.tail for tid <
 * num_thr_e.  On success both files of every tid are removed (decompress.cpp:119, :656-657); on an error none.  The
 * files are read before ctx is looked at: a missing file gives SPRING_REORDER_E_IO before any device call. */
int spring_decode_seq_from_files(spring_decode_ctx *ctx, const char *temp_dir, int32_t num_thr_e);

/* The blocks. */
/* Every block of the last run of s, with that run's parameters (nothing leaves the device). */
int spring_decode_from_streams(spring_decode_ctx *ctx, spring_streams_ctx *s, spring_decode_info *info);
/* bytes[s] / block_off[s] for the stream ids SPRING_STREAMS_* (as spring_streams_download gives them, restricted to
 * the window): the window's blocks back to back and num_blocks + 1 offsets starting at 0.  Ids 7 and 8 are read for
 * paired-end data only (NULL allowed otherwise); bytes[s] may be NULL when the stream is empty. */
int spring_decode_from_host(spring_decode_ctx *ctx, const uint8_t *const *bytes, const uint64_t *const *block_off,
                            uint32_t first_block, uint32_t num_blocks, uint32_t num_reads, int32_t paired_end,
                            int32_t preserve_order, uint32_t num_reads_per_block, spring_decode_info *info);
/* From temp_dir/<stream>.<b> for every stream and block of the window (what BSC_decompress leaves).  On success they
 * are removed (decompress.cpp:334-353); on an error none.  File errors give SPRING_REORDER_E_IO before ctx is looked
 * at or any device call is made. */
int spring_decode_from_files(spring_decode_ctx *ctx, const char *temp_dir, uint32_t first_block, uint32_t num_blocks,
                             uint32_t num_reads, int32_t paired_end, int32_t preserve_order,
                             uint32_t num_reads_per_block, spring_decode_info *info);

/* The reads of mate 0 (read 1) or 1 (read 2, paired-end) of the last successful decode: bases = info.bases[mate]
 * bytes, the reads back to back in slot order; read_off = num_units + 1 offsets into bases.  Either may be NULL. */
int spring_decode_download(spring_decode_ctx *ctx, int32_t mate, char *bases, uint64_t *read_off);

int spring_decode_get_info(spring_decode_ctx *ctx, spring_decode_info *info);

#ifdef __cplusplus
}
#endif
#endif
