/*
 * include/spring_gzip.h -- C ABI of the MI355X (gfx950) gzip stage: a byte buffer plus member cuts becomes a series of
 * RFC 1952 members, compressed on the device.
 *
 * Replaces the gzip_flag branch of write_fastq_block (reference src/util.cpp:70-110, `spring -d -g`): there every thread
 * deflates 1 + (num_reads - 1) / num_thr records of a block into a member of its own and the members are written back
 * to back.  What that file is, is only defined by what it inflates to; so is this one:
 *
 *   source    the text of a spring_fastq_out_ctx, read in place in HBM and left as it was, or any host buffer.
 *   members   from a fastq_out context: cut every member_records records from the start of the text (its rec_off[] on
 *             the device); 0 means one member.  From the host: num_members + 1 byte offsets that start at 0, increase
 *             strictly and end at nbytes; NULL means one member.  An empty input gives zero members and zero bytes and
 *             is no error.
 *   member    1f 8b 08 00, mtime 0, XFL 0, OS 255; a raw deflate stream; CRC-32 and length mod 2^32 of the member's
 *             bytes.
 *   chunks    a member is cut every chunk_bytes bytes (info.chunk_bytes).  A chunk becomes a dynamic-Huffman block
 *             followed by an empty stored block, so that it ends on a byte boundary, or stored blocks of at most 65535
 *             bytes when that is not smaller.  The last block of a member carries BFINAL.  A match never reaches before
 *             the start of its member; it may reach up to 32768 bytes back into earlier chunks of the same member.
 *             Hence  bytes_out <= bytes_in + 18 * members + 5 * sum over chunks of ceil(chunk_len / 65535).
 *   mode      SPRING_GZIP_STORED: stored blocks only; SPRING_GZIP_DEFLATE: the compressor.
 *
 * The output is a function of the input bytes, the cuts, mode and chunk_bytes only.
 *
 * Refused before any result: cuts that do not start at 0, do not increase strictly or do not end at nbytes, a NULL
 * buffer with nbytes > 0, a mode outside 0 .. 1, a fastq_out context on another device (SPRING_REORDER_E_ARG); a
 * fastq_out context without a text (SPRING_REORDER_E_STATE).  A refused call leaves the context without a result;
 * download / write / get_info without a result give SPRING_REORDER_E_STATE.
 *
 * Return value: 0 on success, negative SPRING_REORDER_E_* on error; text in spring_reorder_last_error().
 */
#ifndef SPRING_GZIP_H_
#define SPRING_GZIP_H_

#include <stddef.h>
#include <stdint.h>

#include "spring_fastq_out.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPRING_GZIP_STORED 0
#define SPRING_GZIP_DEFLATE 1

typedef struct spring_gzip_ctx spring_gzip_ctx;

typedef struct {
  uint64_t num_members;
  uint64_t bytes_in;
  uint64_t bytes_out;
  uint64_t chunk_bytes;     /* the library's cut inside a member                                   */
  uint64_t num_chunks;
  uint64_t chunks_stored;   /* chunks written as stored blocks                                     */
  double ms_device;         /* HIP events around the device passes, input copies excluded          */
  double ms_file;           /* spring_gzip_write: wall time of the last call                       */
  double ms_pass[6];        /* chunk table, match + parse, codes, emit, CRC-32, compaction         */
  uint64_t num_batches;     /* batches the chunks were matched, coded and emitted in (0: stored)   */
} spring_gzip_info;

int spring_gzip_create(int device, spring_gzip_ctx **out);
void spring_gzip_destroy(spring_gzip_ctx *ctx);

/* chunk_bytes for the calls that follow: a multiple of 4096 in 4096 .. 65536 (for measurements; the default is the
 * measured choice of DESIGN.md section 14).  The match window is min(32768, 65536 - chunk_bytes). */
int spring_gzip_set_chunk_bytes(spring_gzip_ctx *ctx, uint32_t chunk_bytes);
/* Token scratch of one batch of chunks for the calls that follow; 0 selects the default of 1 GiB.  Chunks are matched,
 * coded and emitted max(1, bytes / (chunk_bytes * 4)) at a time (info.num_batches batches).  For tests and
 * measurements: the output does not depend on it. */
int spring_gzip_set_token_bytes(spring_gzip_ctx *ctx, uint64_t bytes);

int spring_gzip_from_fastq_out(spring_gzip_ctx *ctx, spring_fastq_out_ctx *text, uint64_t member_records, int32_t mode,
                               spring_gzip_info *info);
int spring_gzip_from_host(spring_gzip_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, const uint64_t *member_off,
                          uint64_t num_members, int32_t mode, spring_gzip_info *info);

/* gz: info.bytes_out bytes; member_off: info.num_members + 1 offsets into gz.  Either may be NULL. */
int spring_gzip_download(spring_gzip_ctx *ctx, uint8_t *gz, uint64_t *member_off);
/* The members to a file through the ring of pinned staging chunks spring_fastq_out_write uses.  append = 0 truncates.
 * A file that cannot be opened or written gives SPRING_REORDER_E_IO and leaves the result. */
int spring_gzip_write(spring_gzip_ctx *ctx, const char *path, int32_t append, spring_gzip_info *info);

int spring_gzip_get_info(spring_gzip_ctx *ctx, spring_gzip_info *info);

#ifdef __cplusplus
}
#endif
#endif
