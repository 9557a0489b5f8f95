// The fixed-order reduction of the kernels that turn a tensor into a few scalars - the criterion (loss.hip), the task meters
// (meter.hip), the pretraining losses and eval counters (pretrain.hip), the optimizer's global norm (optim.hip) - and the
// all-reduce over the lanes of a channels-last pixel.  No atomics: the same inputs give the same bits on every run, because
// every addition has its place in ONE order, stated here and nowhere else:
//
//   stage 1, inside a workgroup of 256 threads: the xor butterfly of a wave (wave_sum / wave_sum_i / wave_max, common.h:
//     offsets 32, 16, ... 1 - symmetric, so every lane ends with the same bits), then the four wave results added
//     ((w0 + w1) + w2) + w3.  block_partials() leaves that in column blockIdx.x of row k of a [rows][nblk] workspace;
//     block_sum() / block_max() / block_sum_i() hand it to every thread instead.
//   stage 2, one workgroup of 256 threads in a launch of its own (reduce_partials): thread t adds partials t, t + 256, ... of
//     a row in that order - float rows in double, int32 rows in int64 - and the 256 thread results are added 0, 1, ... 255.
//
// A kernel that needs such a sum calls these; it does not write the loops again.
#pragma once
#include "common.h"

namespace m3 {

// ------------------------------------------------------------------------------------------------------------ stage 1
// NF sums and NI counts per thread -> rows [NF + NI][nblk] of the workspace, nblk = gridDim.x, column blockIdx.x.  The barrier
// inside also orders what the caller stored to LDS before the call against what it reads after it.
template <int NF, int NI>
__device__ __forceinline__ void block_partials_rows(const float *s, const int *c, float *__restrict__ ws) {
  __shared__ float sh_f[NF][4];
  __shared__ int sh_i[NI ? NI : 1][4];
  const int t = threadIdx.x, nblk = gridDim.x, b = blockIdx.x;
#pragma unroll
  for (int k = 0; k < NF; ++k) {
    const float w = wave_sum(s[k]);
    if ((t & 63) == 0) sh_f[k][t >> 6] = w;
  }
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    const int w = wave_sum_i(c[k]);
    if ((t & 63) == 0) sh_i[k][t >> 6] = w;
  }
  __syncthreads();
  if (t < NF) ws[t * nblk + b] = ((sh_f[t][0] + sh_f[t][1]) + sh_f[t][2]) + sh_f[t][3];
  else if (t < NF + NI) ((int32_t *)ws)[t * nblk + b] = sh_i[t - NF][0] + sh_i[t - NF][1] + sh_i[t - NF][2] + sh_i[t - NF][3];
}
template <int NF, int NI>
__device__ __forceinline__ void block_partials(const float (&s)[NF], const int (&c)[NI], float *__restrict__ ws) {
  block_partials_rows<NF, NI>(s, c, ws);
}
template <int NF> __device__ __forceinline__ void block_partials(const float (&s)[NF], float *__restrict__ ws) {   // no counts
  block_partials_rows<NF, 0>(s, nullptr, ws);
}

// The broadcast form: every thread returns the same bits.  sh: 4 words of LDS; the leading barrier lets a caller reuse it for
// the next reduction.
__device__ __forceinline__ float block_sum(float v, float *sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
__device__ __forceinline__ float block_max(float v, float *sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
__device__ __forceinline__ int block_sum_i(int v, float *sh) {
  v = wave_sum_i(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) ((int *)sh)[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((int *)sh)[0] + ((int *)sh)[1] + ((int *)sh)[2] + ((int *)sh)[3];
}

// ------------------------------------------------------------------------------------------------------------ stage 2
// the totals of NF float rows, then NI int32 rows, of n partials each; row k starts at ws + k * stride
template <int NF, int NI> struct Totals { double s[NF]; long long c[NI ? NI : 1]; };

// Called by all 256 threads of the one workgroup of a finalize launch; every thread returns every total.  Thread k adds the
// 256 thread results of row k, so the rows go side by side, and the totals pass through LDS behind a second barrier.
template <int NF, int NI>
__device__ __forceinline__ Totals<NF, NI> reduce_partials(const float *__restrict__ ws, int n, int stride) {
  constexpr int NC = NI ? NI : 1;
  __shared__ double sh_s[NF][256], tot_s[NF];
  __shared__ long long sh_c[NC][256], tot_c[NC];
  const int t = threadIdx.x;
  const int32_t *wi = (const int32_t *)ws + NF * stride;
  Totals<NF, NI> r;
#pragma unroll
  for (int k = 0; k < NF; ++k) r.s[k] = 0.0;
#pragma unroll
  for (int k = 0; k < NC; ++k) r.c[k] = 0;
  for (int i = t; i < n; i += 256) {                             // thread t: partials t, t + 256, ... in order
#pragma unroll
    for (int k = 0; k < NF; ++k) r.s[k] += (double)ws[k * stride + i];
#pragma unroll
    for (int k = 0; k < NI; ++k) r.c[k] += wi[k * stride + i];
  }
#pragma unroll
  for (int k = 0; k < NF; ++k) sh_s[k][t] = r.s[k];
#pragma unroll
  for (int k = 0; k < NI; ++k) sh_c[k][t] = r.c[k];
  __syncthreads();
  if (t < NF) {
    double a = 0.0;
    for (int i = 0; i < 256; ++i) a += sh_s[t][i];
    tot_s[t] = a;
  } else if (t < NF + NI) {
    long long a = 0;
    for (int i = 0; i < 256; ++i) a += sh_c[t - NF][i];
    tot_c[t - NF] = a;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NF; ++k) r.s[k] = tot_s[k];
#pragma unroll
  for (int k = 0; k < NI; ++k) r.c[k] = tot_c[k];
  return r;
}

// ------------------------------------------------------------------------------------ the lanes of a channels-last pixel
// one DPP row operation (quad permutes, row mirrors): full-rate VALU, no LDS round trip
template <int CTRL, typename T> __device__ __forceinline__ T dpp(T v) {
  return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}

struct OpSum { static __device__ __forceinline__ float of(float a, float b) { return a + b; } };
struct OpMax {
  static __device__ __forceinline__ float of(float a, float b) { return fmaxf(a, b); }
  static __device__ __forceinline__ uint32_t of(uint32_t a, uint32_t b) { return a > b ? a : b; }
};
struct OpMin { static __device__ __forceinline__ uint32_t of(uint32_t a, uint32_t b) { return a < b ? a : b; } };

// All-reduce of U values at once over each group of 2^gsh neighbouring lanes; every lane of a group ends with the same bits.
// The first four levels are DPP row operations, only groups of 32 and 64 lanes go on to a shuffle (an LDS round trip).
template <typename Op, typename T, int U>
__device__ __forceinline__ void group_allreduce(T (&v)[U], int gsh) {
  if (gsh >= 1) {
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = Op::of(v[u], dpp<0xB1>(v[u]));             // quad_perm [1,0,3,2]
  }
  if (gsh >= 2) {
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = Op::of(v[u], dpp<0x4E>(v[u]));             // quad_perm [2,3,0,1]
  }
  if (gsh >= 3) {
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = Op::of(v[u], dpp<0x141>(v[u]));            // row_half_mirror: the other quad of 8 lanes
  }
  if (gsh >= 4) {
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = Op::of(v[u], dpp<0x140>(v[u]));            // row_mirror: the other half of 16 lanes
  }
  if (gsh >= 5) {
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = Op::of(v[u], __shfl_xor(v[u], 16, 64));
  }
  if (gsh >= 6) {
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = Op::of(v[u], __shfl_xor(v[u], 32, 64));
  }
}

}  // namespace m3
