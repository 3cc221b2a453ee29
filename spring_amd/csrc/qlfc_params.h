// spring_amd/csrc/qlfc_params.h -- the predictor parameters of libbsc's static QLFC coder in fast mode (reference
// libbsc/coder/qlfc/qlfc_model.h:115-176), restated as one table of this project's own layout.
// qlfc.hip expands it into device constants; tests/qlfc_model.py reads the same rows with a regular expression, so keep
// one ROW / MIX per line and plain decimal numbers.
//
// A family is one group of predictors of the coder; a kind is which of the three predictors of a decision: the one
// indexed by the run's byte (CHAR), the one indexed by the context state (STATE), the one shared by all (STATIC).
//
//   ROW(family, kind, th0, ar0, th1, ar1)   on a 0: p += ((4096 - th0 - p) * ar0) >> 12
//                                           on a 1: p -= ((p - th1) * ar1) >> 12      (predictor.h:45-53; p starts at 2048)
//   MIX(family, w_char, w_state, w_static)  probability of a 0 = (char * w_char + state * w_state + static * w_static) >> 5
//
// Slot class = 3 * family + kind, families and kinds in the order below.
#ifndef SPRING_QLFC_PARAMS_H_
#define SPRING_QLFC_PARAMS_H_

#define QLFC_FAMILIES 7
#define QLFC_KINDS 3

#define QLFC_PARAM_TABLE(ROW, MIX)                                                  \
  /* rank: is it 1?  (qlfc_model.h:115-122) */                                      \
  ROW(RANK_TOP, CHAR, -2, 282, 12, 274)                                             \
  ROW(RANK_TOP, STATE, -116, 33, -78, 34)                                           \
  ROW(RANK_TOP, STATIC, 4, 697, 55, 1185)                                           \
  MIX(RANK_TOP, 17, 14, 1)                                                          \
  /* rank: unary exponent  (:124-131) */                                            \
  ROW(RANK_EXP, CHAR, -14, 271, 3, 308)                                             \
  ROW(RANK_EXP, STATE, -177, 23, -370, 11)                                          \
  ROW(RANK_EXP, STATIC, -3, 788, 135, 1364)                                         \
  MIX(RANK_EXP, 22, 6, 4)                                                           \
  /* rank: mantissa bits  (:133-140) */                                             \
  ROW(RANK_MAN, CHAR, -55, 73, -54, 74)                                             \
  ROW(RANK_MAN, STATE, -254, 16, -177, 20)                                          \
  ROW(RANK_MAN, STATIC, -6, 575, 1670, 1173)                                        \
  MIX(RANK_MAN, 15, 10, 7)                                                          \
  /* rank: the escape path, all bits  (:142-149) */                                 \
  ROW(RANK_ESC, CHAR, -33, 120, -25, 157)                                           \
  ROW(RANK_ESC, STATE, -126, 32, -126, 32)                                          \
  ROW(RANK_ESC, STATIC, -6, 585, 150, 275)                                          \
  MIX(RANK_ESC, 16, 11, 5)                                                          \
  /* run length: is it 1?  (:151-158) */                                            \
  ROW(RUN_TOP, CHAR, -4, 221, -13, 231)                                             \
  ROW(RUN_TOP, STATE, -68, 38, -112, 36)                                            \
  ROW(RUN_TOP, STATIC, 0, 0, 0, 0)                                                  \
  MIX(RUN_TOP, 14, 18, 0)                                                           \
  /* run length: unary exponent  (:160-167) */                                      \
  ROW(RUN_EXP, CHAR, -3, 325, -11, 341)                                             \
  ROW(RUN_EXP, STATE, -90, 45, -92, 44)                                             \
  ROW(RUN_EXP, STATIC, 24, 887, -4, 765)                                            \
  MIX(RUN_EXP, 14, 15, 3)                                                           \
  /* run length: mantissa bits  (:169-176) */                                       \
  ROW(RUN_MAN, CHAR, -18, 191, -15, 241)                                            \
  ROW(RUN_MAN, STATE, -275, 14, -185, 22)                                           \
  ROW(RUN_MAN, STATIC, -73, 54, -214, 19)                                           \
  MIX(RUN_MAN, 7, 15, 10)

#endif
