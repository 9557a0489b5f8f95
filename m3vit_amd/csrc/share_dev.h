// The lane's view of a row, shared by the row kernels of the token path (share.hip, token_ffn.hip): a lane owns the
// 8-element chunks lane, lane + 64 of a row (D <= M3_SHARE_MAX_D = 1024, D % 8 == 0): 16-byte accesses for fp16 / bf16, two
// per chunk for fp32.
#pragma once
#include "common.h"

namespace m3 {

constexpr int SHARE_CH = 8;                         // elements per lane chunk

template <typename T, int NCH> struct RowIO {
  // chunk i of this lane starts at element off[i]; chunks past D read chunk 0 (an address that exists) and become zeros
  static __device__ __forceinline__ void load(const void *row, int D, int lane, float (&v)[NCH][SHARE_CH]) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int d = (lane + 64 * i) * SHARE_CH;
      Pack<T, SHARE_CH>::load((const T *)row + (d < D ? d : 0), v[i]);
    }
  }
  static __device__ __forceinline__ void mask(int D, int lane, float (&v)[NCH][SHARE_CH]) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const bool ok = (lane + 64 * i) * SHARE_CH < D;
#pragma unroll
      for (int j = 0; j < SHARE_CH; ++j) v[i][j] = ok ? v[i][j] : 0.f;
    }
  }
  static __device__ __forceinline__ void store(void *row, int D, int lane, const float (&v)[NCH][SHARE_CH]) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int d = (lane + 64 * i) * SHARE_CH;
      if (d < D) Pack<T, SHARE_CH>::store((T *)row + d, v[i]);
    }
  }
};

}  // namespace m3
