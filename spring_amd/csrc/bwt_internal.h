// spring_amd/csrc/bwt_internal.h -- what the inverse stage (unbwt.hip) needs from a finished block-sort context without
// a round trip through the host: the device buffers of its result and the segment offsets.  Internal to the library.
#ifndef SPRING_BWT_INTERNAL_H_
#define SPRING_BWT_INTERNAL_H_

#include <stdint.h>

#include "spring_bwt.h"

namespace sr {

struct BwtView {
  int dev;
  uint64_t num_segments, bytes;
  const uint8_t *bwt;       // device: the transformed segments back to back
  const int32_t *primary;   // device: one per segment
  const uint64_t *off;      // host: num_segments + 1 offsets into bwt
};
int bwt_view(spring_bwt_ctx *ctx, BwtView *v);   // fails unless the context holds a result

}  // namespace sr
#endif
