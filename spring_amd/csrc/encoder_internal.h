// spring_amd/csrc/encoder_internal.h -- what the streams stage (streams.hip) needs from a finished encoder context
// without a round trip through the host: device pointers of the encoder's output streams.  Internal to the library.
#ifndef SPRING_ENCODER_INTERNAL_H_
#define SPRING_ENCODER_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spring_encoder.h"

namespace sr {

struct EncoderView {
  int dev;
  spring_encoder_info info;   // n_aligned, n_total, noise_bytes, n_noisepos, unaligned_bytes size the arrays below
  const uint64_t *pos;        // read_pos.bin
  const char *noise;          // read_noise.txt
  const uint16_t *noisepos;   // read_noisepos.bin
  const uint32_t *order;      // read_order.bin
  const uint16_t *rlen;       // read_lengths.bin
  const char *rc;             // read_rev.txt
  const uint8_t *unaligned;   // read_unaligned.txt (write_dnaN_in_bits records)
  const uint8_t *refc;        // the consensus, one byte per base, SPRING code A0 G1 C2 T3 (info.seq_len bases)
  int num_thr;                // tids of the consensus
  const uint64_t *tid_seq;    // host: num_thr + 1 offsets into refc (tid t holds [tid_seq[t], tid_seq[t + 1]))
};
int encoder_view(spring_encoder_ctx *ctx, EncoderView *v);   // fails unless the context holds an encode

// pe_encode (pe_encode.cpp:24-84) on device arrays: out[i] for order[i], n even (order_ops.hip)
int pe_encode_device(hipStream_t st, const uint32_t *order, uint32_t n, uint32_t *out);

}  // namespace sr
#endif
