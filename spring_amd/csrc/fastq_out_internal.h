// spring_amd/csrc/fastq_out_internal.h -- what the FASTQ assembler (fastq_out.hip) reads in place from a decode
// context (decode.hip) and from a quality / id context (qualid.hip): the device buffers of their last result, with the
// sizes that bound them; and what the gzip stage (gzip.hip) reads in place from the assembler's own context.  Internal
// to the library.
#ifndef SPRING_FASTQ_OUT_INTERNAL_H_
#define SPRING_FASTQ_OUT_INTERNAL_H_

#include <stdint.h>

#include "spring_decode.h"
#include "spring_fastq_out.h"
#include "spring_qualid.h"

namespace sr {

struct DecodeView {
  int dev;
  spring_decode_info info;        // first_block, num_blocks, num_units; bases[m] = bytes held by bases[m]
  bool paired_end;                // the decode filled mate 1 as well
  const uint8_t *bases[2];        // device: the reads of mate 0 / 1 back to back (no padding behind them)
  const uint64_t *read_off[2];    // device: num_units + 1 offsets
};
int decode_view(spring_decode_ctx *ctx, DecodeView *v);   // fails unless the context holds a decode

struct QualIdView {
  int dev;
  spring_qualid_info info;        // num_units, num_blocks, bytes[kind]
  uint32_t num_reads_per_block;
  bool have[2];                   // a result of this kind exists
  const uint8_t *bytes[2];        // device: all blocks back to back (info.bytes[kind] bytes)
  const uint32_t *len[2];         // device: num_units line lengths in slot order (without the id's '\n')
  const uint64_t *table[2];       // host: num_blocks + 1 block offsets
};
int qualid_view(spring_qualid_ctx *ctx, QualIdView *v);   // fails unless the context holds a result

struct FastqOutView {
  int dev;
  spring_fastq_out_info info;     // num_units, bytes
  const uint8_t *text;            // device: info.bytes bytes from a 16-byte-aligned start, 16 bytes of padding behind them
  const uint64_t *rec_off;        // device: num_units + 1 offsets into text
};
int fastq_out_view(spring_fastq_out_ctx *ctx, FastqOutView *v);   // fails unless the context holds a text

}  // namespace sr
#endif
