// The routing scan, shared by m3_route_build's second launch (route.hip) and the workgroup that rides along with the balance
// reduction (gate.hip).  Integer work, bit-exact against oracle/gate_route.c.
#pragma once
#include "common.h"

namespace m3 {

// Exclusive scan of the per-block expert histograms blk_counts [nblk][E] along the block axis into blk_base, one WAVE per
// expert (64 blocks per step, shuffle scan), then the expert totals, offsets and 128-row tile prefix by one thread.
// One workgroup of THREADS threads; MAX_E >= E words of LDS.
template <int THREADS, int MAX_E>
__device__ __forceinline__ void route_scan(const int32_t *blk_counts, int nblk, int E, int32_t *blk_base, int32_t *counts,
                                           int32_t *offsets, int32_t *tile_starts, int64_t *counts64) {
  __shared__ int32_t tot[MAX_E];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int e = wave; e < E; e += THREADS / 64) {
    int32_t carry = 0;
    for (int b0 = 0; b0 < nblk; b0 += 64) {
      const int b = b0 + lane;
      const int32_t v = b < nblk ? blk_counts[(int64_t)b * E + e] : 0;
      int32_t inc = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int32_t up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
      }
      if (b < nblk) blk_base[(int64_t)b * E + e] = carry + inc - v;
      carry += __shfl(inc, 63, 64);
    }
    if (lane == 0) {
      tot[e] = carry;
      counts[e] = carry;
      if (counts64) counts64[e] = carry;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t o = 0, ts = 0;
    for (int i = 0; i < E; ++i) {
      offsets[i] = o;
      tile_starts[i] = ts;
      o += tot[i];
      ts += (tot[i] + 127) / 128;
    }
    offsets[E] = o;
    tile_starts[E] = ts;
  }
}

}  // namespace m3
