// What the kernels that read a dense prediction [B,C,H,W] next to its label share: the criterion (loss.hip) and the task
// metrics (meter.hip).  Grid sizing, the shape and alignment checks of an entry point, the label-dtype dispatch and the lane
// geometry of a channels-last pixel, the loss record.  The fixed-order sums all of them end in are reduce_dev.h's.
#pragma once
#include "reduce_dev.h"
#include <math.h>

namespace m3 {

constexpr int LS_THREADS = 256;
constexpr int LS_MAX_BLOCKS = M3_LOSS_MAX_BLOCKS;   // 4 workgroups per CU; with two pieces per thread the bytes in flight of 8 per CU

// the eight words of a loss record (M3_LOSS_REC_*, include/m3vit_hip.h); words 6 and 7 are reserved and written as zero
__device__ __forceinline__ void write_loss_record(int32_t *__restrict__ rec, float value, float coef, float coef2, int n_valid,
                                                  int n_aux, int n_bad) {
  ((float *)rec)[M3_LOSS_REC_VALUE] = value;
  ((float *)rec)[M3_LOSS_REC_COEF] = coef;
  ((float *)rec)[M3_LOSS_REC_COEF2] = coef2;
  rec[M3_LOSS_REC_N_VALID] = n_valid;
  rec[M3_LOSS_REC_N_AUX] = n_aux;
  rec[M3_LOSS_REC_N_BAD] = n_bad;
  rec[6] = rec[7] = 0;
}

static inline int blocks_for(int64_t units, int per_block) {
  const int64_t b = (units + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : (b > LS_MAX_BLOCKS ? LS_MAX_BLOCKS : b));
}
static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

struct LossShape { int B, C, H, W, HW, npix; int64_t n; };

static inline int shape_ok(int B, int C, int H, int W, int cmin, int cmax, int layout, int dtype, const char *who, LossShape *s) {
  M3_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: B, H, W must be positive (got %d, %d, %d)", who, B, H, W);
  M3_REQUIRE(C >= cmin && C <= cmax, "%s: C = %d outside [%d, %d]", who, C, cmin, cmax);
  M3_REQUIRE(layout == M3_LAYOUT_NCHW || layout == M3_LAYOUT_NHWC, "%s: bad layout code %d", who, layout);
  M3_REQUIRE(dtype_ok(dtype), "%s: bad dtype code %d", who, dtype);
  const int64_t n = (int64_t)B * C * H * W;
  M3_REQUIRE(n < ((int64_t)1 << 31) - ((int64_t)1 << 20), "%s: %lld elements: the kernels index with 32 bits", who, (long long)n);
  s->B = B; s->C = C; s->H = H; s->W = W; s->HW = H * W; s->npix = B * H * W; s->n = n;
  return 0;
}

static inline bool label_dtype_ok(int ldt) { return ldt == M3_LABEL_F32 || ldt == M3_LABEL_I64 || ldt == M3_LABEL_U8; }

// f(IntTag<L>{}), L the label dtype code that label_dtype_ok() has accepted
template <typename F> static inline void by_label(int ldt, F &&f) {
  if (!by_int<M3_LABEL_I64, M3_LABEL_U8>(ldt, f)) f(IntTag<M3_LABEL_F32>{});
}

static inline int group_shift(int nch) {                 // lanes per channels-last pixel: the power of two >= nch, at most 64
  int sh = 0;
  while ((1 << sh) < nch && sh < 6) ++sh;
  return sh;
}

}  // namespace m3
