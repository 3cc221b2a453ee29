// spring_amd/csrc/streams_internal.h -- what the decoder (decode.hip) needs from a finished streams context without a
// round trip through the host: the device buffers of the last run, its block tables and its parameters.  Internal to
// the library.
#ifndef SPRING_STREAMS_INTERNAL_H_
#define SPRING_STREAMS_INTERNAL_H_

#include <stdint.h>

#include "spring_streams.h"

namespace sr {

struct StreamsView {
  int dev;
  spring_streams_info info;                 // num_units, num_blocks, bytes[] size the buffers below
  const uint8_t *bytes[SPRING_STREAMS_NUM];  // device: all blocks of a stream back to back
  const uint64_t *table;                    // host: SPRING_STREAMS_NUM x (num_blocks + 1) block offsets
  uint32_t num_reads, num_reads_per_block;
  bool paired_end, preserve_order;
};
int streams_view(spring_streams_ctx *ctx, StreamsView *v);   // fails unless the context holds a run

}  // namespace sr
#endif
