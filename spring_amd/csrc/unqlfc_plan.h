// spring_amd/csrc/unqlfc_plan.h -- the arithmetic of the QLFC decoder stage that host and device share (DESIGN.md
// section 20): where a chunk's predictors lie in its workspace, the violation codes, workspace need.  Internal to the
// library.
#ifndef SPRING_UNQLFC_PLAN_H_
#define SPRING_UNQLFC_PLAN_H_

#include <stdint.h>

#include "qlfc_plan.h"

namespace unqlfc {

constexpr uint64_t MAX_SEGMENT = 1ull << 30;

// The well-formedness rules of spring_unqlfc.h, in its order; 0: none.
enum Violation { V_NONE, V_CHUNKS, V_TABLE, V_ENTRY, V_SUM, V_LENGTH, V_SIZE, V_RANK, V_EXPONENT, V_RUN, V_UNITS };
inline const char *violation_name(uint32_t v) {
  static const char *const names[] = {"none", "chunks", "table", "entry", "sum", "length", "size", "rank", "exponent", "run", "units"};
  return v <= V_UNITS ? names[v] : "?";
}

// The predictors of one chunk: 16-bit values, family after family.  Inside a family of L places per byte: the 256 * L
// of kind CHAR, the 256 * L of kind STATE (who * L + place), then the L of kind STATIC.  The place of a decision:
//   RANK_TOP, RUN_TOP   0
//   RANK_EXP, RUN_EXP   the position in the unary exponent (0 .. 6, 0 .. 30)
//   RANK_MAN            exponent e = 1 .. 7 with the bits so far ctx = 1 .. 2^e - 1: 2^e - e - 2 + ctx (0 .. 246)
//   RANK_ESC            the bits so far, 1 .. 255
//   RUN_MAN             exponent e = 1 .. 31, ctx = 1 .. 31: e << 5 | ctx
QLFC_HD constexpr uint32_t places(int family) {
  return family == qlfc::RANK_EXP ? 8 : family == qlfc::RANK_MAN || family == qlfc::RANK_ESC ? 256
       : family == qlfc::RUN_EXP ? 32 : family == qlfc::RUN_MAN ? 1024 : 1;
}
QLFC_HD constexpr uint32_t family_base(int family) {
  uint32_t b = 0;
  for (int f = 0; f < family; f++) b += 513 * places(f);
  return b;
}
constexpr uint32_t MODEL_ENTRIES = family_base(QLFC_FAMILIES);
constexpr uint64_t MODEL_BYTES = ((uint64_t)MODEL_ENTRIES * 2 + 255) / 256 * 256;
QLFC_HD uint32_t rank_man_place(uint32_t e, uint32_t ctx) { return (1u << e) - e - 2 + ctx; }
QLFC_HD uint32_t run_man_place(uint32_t e, uint32_t ctx) { return e << 5 | ctx; }

// Workspace of a sub-batch: the predictors of every coded chunk, per chunk its job and its three results, per decoded
// byte nothing (the output is the result's own buffer).
constexpr uint64_t CHUNK_NEED = MODEL_BYTES + 64, FIXED_NEED = 1 << 20;
inline uint64_t workspace_need(uint64_t bytes_out, uint64_t chunks) { (void)bytes_out; return chunks * CHUNK_NEED + FIXED_NEED; }

}  // namespace unqlfc
#endif
