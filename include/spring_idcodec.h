/*
 * include/spring_idcodec.h -- C ABI of the MI355X (gfx950) id codec stage: the id blocks of a run, where they lie in
 * HBM, turned into the exact bytes compress_id_block writes to id_N.<block> (INTEGRATION.md
 * section 13).
 *
 * Replaces compress_id_block (reference src/util.cpp:113-126; the codec is src/id_compression/) as spring::preprocess
 * calls it under preserve_order (preprocess.cpp:232-239) and spring::reorder_compress_quality_id calls it otherwise.
 * Two kernel groups:
 *
 *   tokens   one lane per id line: the token symbols of an id are a function of that id and the id before it in the
 *            block (the first id of a block has an empty one before it).  A symbol is one 32-bit word: value in bits
 *            0-7, kind in bits 8-10 (SPRING_IDCODEC_K_*), context in bits 11-22 (the token number; for
 *            SPRING_IDCODEC_K_INT 4 * token number + byte index).
 *   coder    one wavefront per block: the adaptive models (all counts 1; + 10 per coded symbol; halved as
 *            (count >> 1) + 1 once their sum reaches 2^20) and the 26-bit arithmetic coder, bits packed most
 *            significant first, the byte in progress always written at the end.  Blocks are independent; those beyond
 *            what the workspace holds models for are worked off in sub-batches of whole blocks (info.sub_batches).
 *
 * Refused before any result, because the reference is undefined or lossy there (SPRING_REORDER_E_ARG): an id longer
 * than 1 023 bytes (its ID[1024] buffers and 1 024 contexts), an id byte 0 or >= 128 (isalpha / isdigit on a signed
 * char), a letter run or a zero run longer than 255 (its uint8_t length wraps), num_reads_per_block == 0, lines that are
 * not '\n'-terminated, a line count that differs from num_lines, a qualid context on another device, a workspace cap
 * below one block's models.  A qualid context without an id result gives SPRING_REORDER_E_STATE.  A refused call leaves
 * the context without a result; download / symbols / get_info without a result give SPRING_REORDER_E_STATE.
 *
 * Return value: 0 on success, negative SPRING_REORDER_E_* on error; text in spring_reorder_last_error().
 */
#ifndef SPRING_IDCODEC_H_
#define SPRING_IDCODEC_H_

#include <stddef.h>
#include <stdint.h>

#include "spring_qualid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPRING_IDCODEC_MAX_ID 1023   /* bytes of an id, without its '\n' */
#define SPRING_IDCODEC_MAX_RUN 255   /* letters of a letter run, zeros of a zero run */

/* kinds of a symbol word: the model family it is coded with */
#define SPRING_IDCODEC_K_TYPE 0      /* token type, alphabet 10: ALPHA 0, DIGIT 1, CHAR 2, MATCH 3, ZEROS 4, DELTA 5, END 6 */
#define SPRING_IDCODEC_K_ALEN 1      /* length of a letter run */
#define SPRING_IDCODEC_K_ABYTE 2     /* a byte of a letter run */
#define SPRING_IDCODEC_K_CHAR 3
#define SPRING_IDCODEC_K_DELTA 4
#define SPRING_IDCODEC_K_ZEROS 5     /* length of a zero run */
#define SPRING_IDCODEC_K_INT 6       /* a byte of a number, low byte first */

typedef struct spring_idcodec_ctx spring_idcodec_ctx;

typedef struct {
  uint64_t num_lines;
  uint64_t num_blocks;    /* ceil(num_lines / num_reads_per_block)                                   */
  uint64_t num_symbols;
  uint64_t bytes;         /* compressed bytes of all blocks                                          */
  uint64_t max_tokens;    /* largest token count of an id: the model tables hold max_tokens + 1 contexts */
  uint64_t sub_batches;
  double ms_tokens;       /* HIP events around the tokenizer's passes, copies excluded               */
  double ms_coder;        /* ... around the coder's passes                                           */
} spring_idcodec_info;

int spring_idcodec_create(int device, spring_idcodec_ctx **out);
void spring_idcodec_destroy(spring_idcodec_ctx *ctx);

/* Device memory the model tables of a sub-batch may use; 0 (the default) takes it from the free HBM at the time of the
 * call.  spring_idcodec_workspace_need: what `blocks` blocks take of it at a largest token count of max_tokens. */
int spring_idcodec_set_workspace_bytes(spring_idcodec_ctx *ctx, uint64_t workspace_bytes);
uint64_t spring_idcodec_workspace_need(uint64_t blocks, uint64_t max_tokens);

/* The id result of a finished quality / id context, read in place in HBM and left as it was. */
int spring_idcodec_from_qualid(spring_idcodec_ctx *ctx, spring_qualid_ctx *q, spring_idcodec_info *info);
/* lines: num_lines '\n'-terminated ids in slot order (nbytes bytes); block b holds lines
 * [b * B, min((b + 1) * B, num_lines)), B = num_reads_per_block. */
int spring_idcodec_from_host(spring_idcodec_ctx *ctx, const uint8_t *lines, uint64_t nbytes, uint64_t num_lines,
                             uint32_t num_reads_per_block, spring_idcodec_info *info);

/* bytes: all compressed blocks back to back (info.bytes bytes); block_off: num_blocks + 1 offsets into bytes.  Any
 * pointer may be NULL. */
int spring_idcodec_download(spring_idcodec_ctx *ctx, uint8_t *bytes, uint64_t *block_off);
/* words: info.num_symbols symbol words; block_off: num_blocks + 1 offsets into words.  Any pointer may be NULL. */
int spring_idcodec_symbols(spring_idcodec_ctx *ctx, uint32_t *words, uint64_t *block_off);
int spring_idcodec_get_info(spring_idcodec_ctx *ctx, spring_idcodec_info *info);

#ifdef __cplusplus
}
#endif
#endif
