// The MoE combine of gfx950 and the row movement around it: the weighted sum of a token's k expert outputs (+ residual),
// its backward, the branch-point backward that also takes the gate's share, and the row gather with an optional k-way sum.
// HBM-bound: one wave owns one token row; every access is a 16-byte (fp32) or 8-byte (16-bit) vector per lane, fully
// coalesced along D.
//
//   combine : bmm(gate_score[T,1,k], moe_outp[T,k,D]), models/moe/ckpt/custom_moe_layer.py:298-305,
//             fused with x = x + moe_output, models/moe/ckpt/vision_transformer_moe.py:450
//   gather  : MOEScatter / MOEGather row movement of fastmoe behind custom_moe_layer.py:263-265
#include "common.h"

namespace m3 {

// KT: top-k as a template constant (1, 2, 4, 8; 0 = run-time k).  With a run-time trip count the k row loads of a token
// are issued one dependent iteration at a time; unrolled, all k rows of a 16-byte column are in flight together.
template <typename T, int KT>
__global__ __launch_bounds__(ROW_THREADS) void combine_fwd_kernel(const T *__restrict__ y, const float *__restrict__ score,
                                                                  const float *__restrict__ residual, int64_t T_,
                                                                  int k_rt, int D, float *__restrict__ out) {
  const int k = KT ? KT : k_rt;
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * (ROW_THREADS / 64) + (threadIdx.x >> 6);
  if (t >= T_) return;
  const float *sc = score + t * k;
  if constexpr (KT > 0) {
    float sv[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) sv[j] = sc[j];
    for (int d = lane * 4; d < D; d += 256) {
      f32x4 v[KT];
#pragma unroll
      for (int j = 0; j < KT; ++j) v[j] = Vec4<T>::load(y + (t * KT + j) * D + d);
      f32x4 acc = residual ? *(const f32x4 *)(residual + t * D + d) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < KT; ++j) {                       // (same order as the run-time loop: j = 0, 1, ...)
        acc[0] = __builtin_fmaf(sv[j], v[j][0], acc[0]); acc[1] = __builtin_fmaf(sv[j], v[j][1], acc[1]);
        acc[2] = __builtin_fmaf(sv[j], v[j][2], acc[2]); acc[3] = __builtin_fmaf(sv[j], v[j][3], acc[3]);
      }
      *(f32x4 *)(out + t * D + d) = acc;
    }
  } else {
    for (int d = lane * 4; d < D; d += 256) {
      f32x4 acc = residual ? *(const f32x4 *)(residual + t * D + d) : f32x4{0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < k; ++j) {
        const f32x4 v = Vec4<T>::load(y + (t * k + j) * D + d);
        const float s = sc[j];
        acc[0] = __builtin_fmaf(s, v[0], acc[0]); acc[1] = __builtin_fmaf(s, v[1], acc[1]);
        acc[2] = __builtin_fmaf(s, v[2], acc[2]); acc[3] = __builtin_fmaf(s, v[3], acc[3]);
      }
      *(f32x4 *)(out + t * D + d) = acc;
    }
  }
}

template <typename T, int KT>
__global__ __launch_bounds__(ROW_THREADS) void combine_bwd_kernel(const float *__restrict__ dout, const T *__restrict__ y,
                                                                  const float *__restrict__ score, int64_t T_, int k_rt,
                                                                  int D, T *__restrict__ dy, float *__restrict__ dscore) {
  const int k = KT ? KT : k_rt;
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * (ROW_THREADS / 64) + (threadIdx.x >> 6);
  if (t >= T_) return;
  if constexpr (KT > 0) {
    // one pass over the token's gradient row for all k routed rows: dout is read once, the k dot products run side by side
    float dot[KT], sv[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) { dot[j] = 0.f; sv[j] = score[t * KT + j]; }
    for (int d = lane * 4; d < D; d += 256) {
      const f32x4 g = *(const f32x4 *)(dout + t * D + d);
      f32x4 v[KT];
#pragma unroll
      for (int j = 0; j < KT; ++j) v[j] = Vec4<T>::load(y + (t * KT + j) * D + d);
#pragma unroll
      for (int j = 0; j < KT; ++j) {
        dot[j] += g[0] * v[j][0] + g[1] * v[j][1] + g[2] * v[j][2] + g[3] * v[j][3];
        if (dy) Vec4<T>::store(dy + (t * KT + j) * D + d, f32x4{sv[j] * g[0], sv[j] * g[1], sv[j] * g[2], sv[j] * g[3]});
      }
    }
#pragma unroll
    for (int j = 0; j < KT; ++j) {
      const float s = wave_sum(dot[j]);
      if (lane == 0) dscore[t * KT + j] = s;
    }
  } else {
    for (int j = 0; j < k; ++j) {
      const float s = score[t * k + j];
      float dot = 0.f;
      for (int d = lane * 4; d < D; d += 256) {
        const f32x4 g = *(const f32x4 *)(dout + t * D + d);
        const f32x4 v = Vec4<T>::load(y + (t * k + j) * D + d);
        dot += g[0] * v[0] + g[1] * v[1] + g[2] * v[2] + g[3] * v[3];
        if (dy) Vec4<T>::store(dy + (t * k + j) * D + d, f32x4{s * g[0], s * g[1], s * g[2], s * g[3]});
      }
      dot = wave_sum(dot);
      if (lane == 0) dscore[t * k + j] = dot;
    }
  }
}

// Input gradient of an MoE layer's branch point: the k routed copies of a token (MOEScatter's backward: a gather-sum,
// custom_moe_layer.py:254-259 / fmoe functions.py MOEScatter.backward) plus the gate's share d logits @ w_gate^T
// (the backward of `inp @ w_gate`, noisy_gate_vmoe.py:91).  A wave takes CG_ROWS rows per pass; the E rows of w_gate^T live
// in LDS as [E][D + 4] fp32 (a lane reads its 4 columns of every expert row as one 16-byte access, shared by the pass's
// rows), the tokens' E logit gradients are wave-uniform scalars.  Replaces a [T,k,D] -> [T,D] sum pass plus a K = E GEMM pass that re-read and re-wrote the
// fp32 [T,D] result.
constexpr int CG_THREADS = 512;    // 8 waves share one LDS image of w_gate^T
constexpr int CG_ROWS = 2;         // rows per wave and pass (4: 142 VGPRs, 3 waves per SIMD)
template <typename T, typename TO, int KT, int NCH>
__global__ __launch_bounds__(CG_THREADS) void combine_gate_bwd_kernel(const T *__restrict__ dxe, int64_t T_, int k_rt, int D,
                                                                      const float *__restrict__ dl,
                                                                      const float *__restrict__ wg, int E,
                                                                      TO *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float s_w[];        // [E][D + 4]: the transposing fill below walks e
  const int DP = D + 4;     // fastest, and a row stride of D (a multiple of the 32 banks) would put all 64 lanes on one bank
  const int k = KT ? KT : k_rt;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int q = threadIdx.x * 4; q < D * E; q += CG_THREADS * 4) {    // w_gate is [D][E]: transpose on the way in
    const f32x4 v = *(const f32x4 *)(wg + q);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int d = (q + i) / E, e = (q + i) - d * E;
      s_w[e * DP + d] = v[i];
    }
  }
  __syncthreads();
  constexpr int WPB = CG_THREADS / 64, RW = CG_ROWS; // RW rows per wave and pass: every LDS read of w_gate^T feeds RW rows
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  // lanes past D in the last column chunk read column 0 again and never store: every load stays unconditional (a
  // predicated load becomes its own basic block with its own wait - the row's loads would go out one latency at a time)
  bool on[NCH];
  int col[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) { on[c] = c * 256 + lane * 4 < D; col[c] = on[c] ? c * 256 + lane * 4 : 0; }
  const int64_t ngrp = (T_ + RW - 1) / RW;
  for (int64_t gq = (int64_t)blockIdx.x * WPB + wave; gq < ngrp; gq += (int64_t)gridDim.x * WPB) {
    const int64_t t0 = gq * RW;
    // every load of the RW rows first (RW x k rows x NCH column chunks in flight), then the E-step fma chains side by side
    f32x4 acc[RW][NCH];
    if constexpr (KT > 0) {
      typename Vec4<T>::type raw[RW][NCH][KT];                       // as loaded: converted only after all are on their way
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const int64_t t = t0 + r < T_ ? t0 + r : T_ - 1;           // (rows past T: a valid row again, never stored)
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
          for (int j = 0; j < KT; ++j)
            raw[r][c][j] = *(const typename Vec4<T>::type *)(dxe + (t * KT + j) * D + col[c]);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          acc[r][c] = f32x4{(float)raw[r][c][0][0], (float)raw[r][c][0][1], (float)raw[r][c][0][2], (float)raw[r][c][0][3]};
#pragma unroll
          for (int j = 1; j < KT; ++j)
            acc[r][c] = acc[r][c] + f32x4{(float)raw[r][c][j][0], (float)raw[r][c][j][1], (float)raw[r][c][j][2], (float)raw[r][c][j][3]};
        }
    } else {
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const int64_t t = t0 + r < T_ ? t0 + r : T_ - 1;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};
          for (int j = 0; j < k; ++j) acc[r][c] = acc[r][c] + Vec4<T>::load(dxe + (t * k + j) * D + col[c]);
        }
      }
    }
    const float *u[RW];                                              // wave-uniform addresses: scalar loads
#pragma unroll
    for (int r = 0; r < RW; ++r) u[r] = dl + (t0 + r < T_ ? t0 + r : T_ - 1) * E;
#pragma unroll 4
    for (int e = 0; e < E; ++e) {
      float ue[RW];
#pragma unroll
      for (int r = 0; r < RW; ++r) ue[r] = u[r][e];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const f32x4 w = *(const f32x4 *)(s_w + e * DP + col[c]);
        const f32x2 wl = f32x2{w[0], w[1]}, wh = f32x2{w[2], w[3]};
#pragma unroll
        for (int r = 0; r < RW; ++r) {                              // packed fp32 fma: two columns per instruction
          const f32x2 uu = f32x2{ue[r], ue[r]};
          f32x2 lo = f32x2{acc[r][c][0], acc[r][c][1]}, hi = f32x2{acc[r][c][2], acc[r][c][3]};
          lo = __builtin_elementwise_fma(uu, wl, lo);
          hi = __builtin_elementwise_fma(uu, wh, hi);
          acc[r][c] = f32x4{lo[0], lo[1], hi[0], hi[1]};
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
      for (int c = 0; c < NCH; ++c)
        if (on[c] && t0 + r < T_) Vec4<TO>::store(out + (t0 + r) * D + c * 256 + lane * 4, acc[r][c]);
  }
}

// ---- row gather with optional k-way sum: dst[i,:] = sum_{j<k} src[idx[i*k+j] / div, :]
// (k = 1: MOEScatter / MOEGather row movement of fastmoe behind custom_moe_layer.py:263-265;
//  k > 1: the backward of MOEScatter, which sums the k routed copies of a token)
template <typename T>
__global__ __launch_bounds__(ROW_THREADS) void gather_rows_kernel(const T *__restrict__ src, const int32_t *__restrict__ idx,
                                                                  int div, int64_t nout, int k, int D,
                                                                  T *__restrict__ dst) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * (ROW_THREADS / 64) + (threadIdx.x >> 6);
  if (i >= nout) return;
  for (int d = lane * 4; d < D; d += 256) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < k; ++j) {
      const int64_t r = idx[i * k + j] / div;
      acc += Vec4<T>::load(src + r * D + d);
    }
    Vec4<T>::store(dst + i * D + d, acc);
  }
}

}  // namespace m3

using namespace m3;

extern "C" int m3_combine_fwd(const void *y, int dtype, const float *score, const float *residual, int64_t T, int k,
                              int D, float *out, void *stream) {
  M3_REQUIRE(y && score && out, "m3_combine_fwd: null operand");
  M3_REQUIRE(dtype_ok(dtype), "m3_combine_fwd: bad dtype");
  M3_REQUIRE(D % 4 == 0 && D > 0 && k >= 1, "m3_combine_fwd: D must be a multiple of 4");
  if (T == 0) return M3_OK;
  hipStream_t s = (hipStream_t)stream;
  by_dtype(dtype, [&](auto tt) {
    typedef typename decltype(tt)::type TT;
    auto go = [&](auto kt) {
      hipLaunchKernelGGL((combine_fwd_kernel<TT, decltype(kt)::value>), dim3(row_blocks(T)), dim3(ROW_THREADS), 0, s,
                         (const TT *)y, score, residual, T, k, D, out);
    };
    if (!by_int<4, 2, 1, 8>(k, go)) go(IntTag<0>{});
  });
  return check_launch("m3_combine_fwd");
}

extern "C" int m3_combine_bwd(const float *dout, const void *y, int dtype, const float *score, int64_t T, int k, int D,
                              void *dy, float *dscore, void *stream) {
  M3_REQUIRE(dout && y && score && dscore, "m3_combine_bwd: null operand");
  M3_REQUIRE(dtype_ok(dtype), "m3_combine_bwd: bad dtype");
  M3_REQUIRE(D % 4 == 0 && D > 0 && k >= 1, "m3_combine_bwd: D must be a multiple of 4");
  if (T == 0) return M3_OK;
  hipStream_t s = (hipStream_t)stream;
  by_dtype(dtype, [&](auto tt) {
    typedef typename decltype(tt)::type TT;
    auto go = [&](auto kt) {
      hipLaunchKernelGGL((combine_bwd_kernel<TT, decltype(kt)::value>), dim3(row_blocks(T)), dim3(ROW_THREADS), 0, s, dout,
                         (const TT *)y, score, T, k, D, (TT *)dy, dscore);
    };
    if (!by_int<4, 2, 1, 8>(k, go)) go(IntTag<0>{});
  });
  return check_launch("m3_combine_bwd");
}

extern "C" int m3_combine_gate_bwd(const void *dxe, int dtype, int64_t T, int k, int D, const float *d_logits,
                                   const float *w_gate, int E, void *dh, int dh_dtype, void *stream) {
  M3_REQUIRE(dxe && d_logits && w_gate && dh, "m3_combine_gate_bwd: null operand");
  M3_REQUIRE(dtype_ok(dtype), "m3_combine_gate_bwd: bad dtype");
  M3_REQUIRE(dh_dtype == M3_F32 || dh_dtype == dtype, "m3_combine_gate_bwd: dh is fp32 or the activation dtype");
  M3_REQUIRE(D % 4 == 0 && D > 0 && k >= 1 && E >= 1, "m3_combine_gate_bwd: D must be a multiple of 4");
  const size_t lds = (size_t)E * (D + 4) * sizeof(float);
  M3_REQUIRE(lds <= 64 * 1024, "m3_combine_gate_bwd: w_gate [D=%d][E=%d] does not fit the 64 KB LDS image", D, E);
  if (T == 0) return M3_OK;
  hipStream_t s = (hipStream_t)stream;
  // grid-stride over the rows: two 16-wave workgroups per CU (all 32 wave slots), each filling its LDS image of w_gate once
  const int64_t rb = ((T + CG_ROWS - 1) / CG_ROWS + CG_THREADS / 64 - 1) / (CG_THREADS / 64);
  const unsigned grid = (unsigned)(rb < 1024 ? rb : 1024);
  const int nch = (D + 255) / 256;
  M3_REQUIRE(nch <= 4 && (D * E) % 4 == 0 && ((uintptr_t)w_gate % 16) == 0, "m3_combine_gate_bwd: D <= 1024, w_gate 16-byte aligned");
  by_dtype(dtype, [&](auto tt) {
    typedef typename decltype(tt)::type TT;
    auto with_out = [&](auto to) {                         // dh: fp32, or the activation dtype
      typedef typename decltype(to)::type TO;
      auto with_k = [&](auto kt) {
        auto go = [&](auto nc) {
          hipLaunchKernelGGL((combine_gate_bwd_kernel<TT, TO, decltype(kt)::value, decltype(nc)::value>), dim3(grid),
                             dim3(CG_THREADS), lds, s, (const TT *)dxe, T, k, D, d_logits, w_gate, E, (TO *)dh);
        };
        if (!by_int<1, 2, 3>(nch, go)) go(IntTag<4>{});
      };
      if (!by_int<4, 2>(k, with_k)) with_k(IntTag<0>{});
    };
    if (dh_dtype == M3_F32) with_out(DtypeTag<float>{}); else with_out(tt);
  });
  return check_launch("m3_combine_gate_bwd");
}

extern "C" int m3_gather_rows(const void *src, int dtype, const int32_t *idx, int div, int64_t nout, int k, int D,
                              void *dst, void *stream) {
  M3_REQUIRE(src && idx && dst && D % 4 == 0 && D > 0 && k >= 1 && div >= 1, "m3_gather_rows: bad args");
  M3_REQUIRE(dtype_ok(dtype), "m3_gather_rows: bad dtype");
  if (nout == 0) return M3_OK;
  hipStream_t s = (hipStream_t)stream;
  by_dtype(dtype, [&](auto tt) {
    typedef typename decltype(tt)::type TT;
    hipLaunchKernelGGL(gather_rows_kernel<TT>, dim3(row_blocks(nout)), dim3(ROW_THREADS), 0, s, (const TT *)src, idx, div,
                       nout, k, D, (TT *)dst);
  });
  return check_launch("m3_gather_rows");
}
