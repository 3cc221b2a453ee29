// spring_amd/csrc/bwt_internal.h -- what the stages behind the block sort (unbwt.hip, qlfc.hip, bsc_frame.hip,
// unqlfc.hip) need from a finished block-sort, QLFC or QLFC decoder context without a round trip through the host: the
// device buffers of its result and the segment offsets.  Internal to the library.
#ifndef SPRING_BWT_INTERNAL_H_
#define SPRING_BWT_INTERNAL_H_

#include <stdint.h>

#include "spring_bwt.h"
#include "spring_qlfc.h"
#include "spring_unqlfc.h"

namespace sr {

struct BwtView {
  int dev;
  uint64_t num_segments, bytes;
  const uint8_t *bwt;       // device: the transformed segments back to back
  const int32_t *primary;   // device: one per segment
  const uint64_t *off;      // host: num_segments + 1 offsets into bwt
  const int32_t *num_indexes;   // device: one per segment
  const int32_t *indexes;       // device: SPRING_BWT_MAX_INDEXES per segment
  const int32_t *seg_stream;    // host, one per segment: where it came from (spring_bwt_segments)
  const uint32_t *seg_block, *seg_cut;
};
int bwt_view(spring_bwt_ctx *ctx, BwtView *v);   // fails unless the context holds a result
int bwt_device(spring_bwt_ctx *ctx);             // with or without a result

struct QlfcView {
  int dev;
  uint64_t num_segments, bytes;
  const uint64_t *coded_off;   // host: num_segments + 1 offsets into the coded bytes
  const int32_t *status;       // host: 0 coded, 1 not compressible
  const uint64_t *d_src;       // device, one per segment: the device address of its coded bytes
  const uint64_t *d_off;       // device: coded_off
  const int32_t *d_status;     // device: status
  const uint64_t *in_off;      // host: num_segments + 1 offsets of the segments as they came in
};
// Fails unless the context holds a result.  The device copies of the offsets and the status are made on the first call
// behind a result and go with it.
int qlfc_view(spring_qlfc_ctx *ctx, QlfcView *v);
int qlfc_device(spring_qlfc_ctx *ctx, bool *have_tables);   // with or without a result

struct UnqlfcView {
  int dev;
  uint64_t num_segments, bytes;
  const uint64_t *off;         // host: num_segments + 1 offsets into out
  const uint8_t *out;          // device: the decoded segments back to back
};
int unqlfc_view(spring_unqlfc_ctx *ctx, UnqlfcView *v);   // fails unless the context holds a result

}  // namespace sr
#endif
