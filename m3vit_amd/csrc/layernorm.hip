// LayerNorm on the fp32 residual stream for gfx950: forward, backward, and the batched reduction of the backward's
// per-workgroup dgamma / dbeta partials.  HBM-bound: one wave owns one token row at a time; a row is ceil(D / 256) 16-byte
// vectors per lane, held in registers between the passes.
//
//   norm1 / norm2 = nn.LayerNorm(eps 1e-6), models/moe/ckpt/vision_transformer_moe.py:441-442,567
#include "common.h"

namespace m3 {

template <typename T, int NCH>
__global__ __launch_bounds__(ROW_THREADS) void layernorm_fwd_kernel(const float *__restrict__ x, int64_t T_, int D,
                                                                    const float *__restrict__ gamma,
                                                                    const float *__restrict__ beta, float eps,
                                                                    T *__restrict__ y, float *__restrict__ mean,
                                                                    float *__restrict__ rstd) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * (ROW_THREADS / 64) + (threadIdx.x >> 6);
  if (t >= T_) return;
  const float *xr = x + t * D;
  // NCH = ceil(D / 256) 16-byte vectors per lane, kept in registers between the passes.  Every load of the row - and gamma /
  // beta, which are only needed after the two reductions - is unconditional (lanes past D re-read column 0 and contribute
  // zeros) and issued up front: a load under `if (d < D)` is its own basic block with its own wait (see layernorm_bwd_kernel).
  f32x4 v[NCH], g[NCH], b[NCH];
  bool on[NCH];
  int col[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    on[i] = lane * 4 + i * 256 < D;
    col[i] = on[i] ? lane * 4 + i * 256 : 0;
    v[i] = *(const f32x4 *)(xr + col[i]);
  }
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    g[i] = *(const f32x4 *)(gamma + col[i]);
    b[i] = *(const f32x4 *)(beta + col[i]);
  }
  __builtin_amdgcn_sched_barrier(0);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    if (!on[i]) v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
  }
  const float mu = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    if (on[i]) {
      const f32x4 c = v[i] - mu;
      q += c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + c[3] * c[3];
    }
  }
  const float var = wave_sum(q) / (float)D;
  const float rs = 1.0f / sqrtf(var + eps);
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    if (on[i]) {
      const f32x4 o = (v[i] - mu) * rs * g[i] + b[i];
      Vec4<T>::store(y + t * D + col[i], o);
    }
  }
  if (lane == 0) { mean[t] = mu; rstd[t] = rs; }
}

// dx = dx_res + rstd * (g*dy - mean(g*dy) - xhat * mean(g*dy*xhat)); per-block partial
// dgamma/dbeta (rows of a block summed in row order).
// Geometry: ln_bwd_waves() waves per workgroup (8; M3_LN_WAVES overrides it for tuning), each wave owns `rpw` consecutive
// rows (default LNB_RPW; M3_LN_ROWS).  Measured at T = 25 216, D = 384 (tools/ln_bench.py, operands streamed; then the
// two-stream training step, same box): 4 waves x 1 / 2 / 4 / 8 / 16 rows 34.7 / 36.7 / 41.7 / 39.7 / 60.5 us per launch,
// 16 waves x 1 / 2 / 4 rows 42.1 / 41.4 / 40.5 us, 8 waves x 8 rows 38.0 us.  Fewer rows per wave stream faster by
// themselves but leave one dgamma / dbeta partial row per workgroup (6304 rows x 2 x D floats at one row per wave: 12 % of
// the kernel's bytes), and 1024-thread workgroups cannot be placed beside the other task stream's kernels (the step went
// 18.16 -> 18.57 ms with them); 8 x 8 is the fastest INSIDE the step.  The partials are summed by ONE batched launch for
// many layers (m3_layernorm_bwd_reduce) instead of a 24-workgroup reduce launch behind every LayerNorm backward.
constexpr int LNB_RPW = 8;                 // default rows per wave
static inline int ln_bwd_waves(int D) {
  static int forced = -1;                    // M3_LN_WAVES = 4 / 8 / 16 (tuning; 16 only while the image fits 64 KiB)
  if (forced < 0) { const char *e = getenv("M3_LN_WAVES"); forced = e ? atoi(e) : 0; }
  if (forced == 4 || forced == 8 || (forced == 16 && D <= 512)) return forced;
  return 8;
}
static int ln_rows_per_wave() {
  static int rpw = 0;
  if (rpw == 0) {
    const char *e = getenv("M3_LN_ROWS");
    const int v = e ? atoi(e) : LNB_RPW;
    rpw = (v >= 1 && v <= 64) ? v : LNB_RPW;
  }
  return rpw;
}

// NCH = ceil(D / 256): 16-byte chunks per lane (registers are sized for the row width in use: D = 384 -> 2, not 4,
// which takes the kernel from 116 to ~70 VGPRs and from 4 to 7 waves per SIMD)
template <typename T, typename TA, int NCH, int LNB_WAVES>
__global__ __launch_bounds__(LNB_WAVES * 64) void layernorm_bwd_kernel(const T *__restrict__ dy, const float *__restrict__ x,
                                                                    const float *__restrict__ mean,
                                                                    const float *__restrict__ rstd,
                                                                    const float *__restrict__ gamma,
                                                                    const float *__restrict__ dx_res, int64_t T_, int D,
                                                                    float *__restrict__ dx, float *__restrict__ part,
                                                                    TA *__restrict__ dx_act, int rpw) {
  extern __shared__ float sred[];   // [LNB_WAVES][2][D]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nblk = gridDim.x;
  f32x4 dg[NCH], db[NCH], gam[NCH];
  // lanes past D in the last 256-column chunk read column 0 again, contribute zeros and never store: every load of a row is
  // unconditional and issued before the first use.  (A load under `if (d < D)` is its own basic block with its own wait: the
  // row's chunks, and the residual behind them, then cost one memory latency EACH - four per row at D = 384 - and a wave's
  // rows run one after the other.)
  bool on[NCH];
  int col[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    on[i] = lane * 4 + i * 256 < D;
    col[i] = on[i] ? lane * 4 + i * 256 : 0;
    dg[i] = f32x4{0.f, 0.f, 0.f, 0.f}; db[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    gam[i] = *(const f32x4 *)(gamma + col[i]);
  }
  // (two rows side by side - their loads in flight together, their shuffle chains interleaved - was measured in round 3:
  // 41.2 us against 38.0 us for this loop at T = 25 216, D = 384: the second row's registers cost more occupancy than the
  // overlap wins)
  for (int r = 0; r < rpw; ++r) {
    const int64_t t = ((int64_t)blockIdx.x * LNB_WAVES + wave) * rpw + r;
    if (t >= T_) break;
    const float mu = mean[t], rs = rstd[t];
    typename Vec4<T>::type dyr[NCH];
    f32x4 xr[NCH], rr[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      dyr[i] = *(const typename Vec4<T>::type *)(dy + t * D + col[i]);
      xr[i] = *(const f32x4 *)(x + t * D + col[i]);
    }
    if (dx_res) {
#pragma unroll
      for (int i = 0; i < NCH; ++i) rr[i] = *(const f32x4 *)(dx_res + t * D + col[i]);
    } else {
#pragma unroll
      for (int i = 0; i < NCH; ++i) rr[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x4 gdy[NCH], xh[NCH];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      f32x4 dyv = f32x4{(float)dyr[i][0], (float)dyr[i][1], (float)dyr[i][2], (float)dyr[i][3]};
      if (!on[i]) dyv = f32x4{0.f, 0.f, 0.f, 0.f};
      xh[i] = (xr[i] - mu) * rs;
      gdy[i] = dyv * gam[i];
      s1 += gdy[i][0] + gdy[i][1] + gdy[i][2] + gdy[i][3];
      s2 += gdy[i][0] * xh[i][0] + gdy[i][1] * xh[i][1] + gdy[i][2] * xh[i][2] + gdy[i][3] * xh[i][3];
      dg[i] += dyv * xh[i];
      db[i] += dyv;
    }
    const float m1 = wave_sum(s1) / (float)D, m2 = wave_sum(s2) / (float)D;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      if (on[i]) {
        const f32x4 o = (gdy[i] - m1 - xh[i] * m2) * rs + rr[i];
        *(f32x4 *)(dx + t * D + col[i]) = o;
        if (dx_act) Vec4<TA>::store(dx_act + t * D + col[i], o);   // activation-dtype copy for the next GEMMs
      }
    }
  }
  // block partials: waves in order
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int d = lane * 4 + i * 256;
    if (d < D) {
      *(f32x4 *)(sred + (wave * 2 + 0) * D + d) = dg[i];
      *(f32x4 *)(sred + (wave * 2 + 1) * D + d) = db[i];
    }
  }
  __syncthreads();
  for (int d = threadIdx.x; d < D; d += LNB_WAVES * 64) {
    float a = 0.f, b = 0.f;
    for (int w = 0; w < LNB_WAVES; ++w) { a += sred[(w * 2 + 0) * D + d]; b += sred[(w * 2 + 1) * D + d]; }
    part[(int64_t)blockIdx.x * D + d] = a;
    part[((int64_t)nblk + blockIdx.x) * D + d] = b;
  }
}

}  // namespace m3

using namespace m3;

extern "C" int m3_layernorm_fwd(const float *x, int64_t T, int D, const float *gamma, const float *beta, float eps,
                                void *y, int y_dtype, float *mean, float *rstd, void *stream) {
  M3_REQUIRE(x && gamma && beta && y && mean && rstd, "m3_layernorm_fwd: null operand");
  M3_REQUIRE(dtype_ok(y_dtype), "m3_layernorm_fwd: bad dtype");
  M3_REQUIRE(D % 4 == 0 && D > 0 && D <= 1024, "m3_layernorm_fwd: D must be a multiple of 4 and <= 1024 (got %d)", D);
  if (T == 0) return M3_OK;
  hipStream_t s = (hipStream_t)stream;
  const int nch = (D + 255) / 256;
  by_dtype(y_dtype, [&](auto tt) {
    typedef typename decltype(tt)::type TT;
    auto go = [&](auto nc) {
      hipLaunchKernelGGL((layernorm_fwd_kernel<TT, decltype(nc)::value>), dim3(row_blocks(T)), dim3(ROW_THREADS), 0, s, x, T,
                         D, gamma, beta, eps, (TT *)y, mean, rstd);
    };
    if (!by_int<1, 2, 3>(nch, go)) go(IntTag<4>{});
  });
  return check_launch("m3_layernorm_fwd");
}

extern "C" int m3_ln_bwd_blocks(int64_t T, int D) {
  const int64_t rows = (int64_t)ln_bwd_waves(D) * ln_rows_per_wave();
  return (int)((T + rows - 1) / rows);
}

extern "C" int m3_layernorm_bwd(const void *dy, int dy_dtype, const float *x, const float *mean, const float *rstd,
                                const float *gamma, const float *dx_res, int64_t T, int D, float *dx, float *ws,
                                float *dgamma, float *dbeta, int beta, void *dx_act, int dx_act_dtype, void *stream) {
  M3_REQUIRE(dy && x && mean && rstd && gamma && dx && ws, "m3_layernorm_bwd: null operand");
  M3_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), "m3_layernorm_bwd: dgamma and dbeta go together");
  M3_REQUIRE(dtype_ok(dy_dtype), "m3_layernorm_bwd: bad dtype");
  M3_REQUIRE(!dx_act || dtype_ok(dx_act_dtype), "m3_layernorm_bwd: bad dx_act dtype");
  M3_REQUIRE(D % 4 == 0 && D > 0 && D <= 1024, "m3_layernorm_bwd: D must be a multiple of 4 and <= 1024");
  if (T == 0) return M3_OK;
  hipStream_t s = (hipStream_t)stream;
  const int nblk = m3_ln_bwd_blocks(T, D), rpw = ln_rows_per_wave(), nw = ln_bwd_waves(D);
  const size_t lds = (size_t)2 * nw * D * sizeof(float);
  const int nch = (D + 255) / 256;
  // (the activation-dtype copy of dx has the dtype of the incoming gradient or is fp32; mixed 16-bit pairs are not built)
  const int act_dtype = dx_act ? dx_act_dtype : M3_F32;
  M3_REQUIRE(dy_dtype == M3_F32 || act_dtype == M3_F32 || act_dtype == dy_dtype,
             "m3_layernorm_bwd: dy fp16 with dx_act bf16 (or the reverse) is not supported");
  by_dtype(dy_dtype, [&](auto tt) {
    typedef typename decltype(tt)::type TT;
    auto with_act = [&](auto ta) {
      typedef typename decltype(ta)::type TA;
      auto with_nch = [&](auto nc) {
        auto go = [&](auto nwt) {
          constexpr int NW = decltype(nwt)::value;
          hipLaunchKernelGGL((layernorm_bwd_kernel<TT, TA, decltype(nc)::value, NW>), dim3(nblk), dim3(NW * 64), lds, s,
                             (const TT *)dy, x, mean, rstd, gamma, dx_res, T, D, dx, ws, (TA *)dx_act, rpw);
        };
        if (!by_int<16, 8>(nw, go)) go(IntTag<4>{});
      };
      if (!by_int<1, 2, 3>(nch, with_nch)) with_nch(IntTag<4>{});
    };
    // the seven (dy, dx_act) pairs that are built: (f32, f16) (f32, bf16) (f32, f32) (f16, f16) (f16, f32) (bf16, bf16)
    // (bf16, f32) - `if constexpr` keeps (f16, bf16) and (bf16, f16) from being instantiated
    if constexpr (sizeof(TT) == 4) by_dtype(act_dtype, with_act);             // fp32 dy: dx_act of any dtype
    else if (act_dtype == dy_dtype) with_act(tt);                             // 16-bit dy: its own dtype ...
    else with_act(DtypeTag<float>{});                                         // ... or fp32
  });
  int rc = check_launch("m3_layernorm_bwd");
  if (rc || !dgamma) return rc;                  // no dgamma / dbeta: the partials stay in ws for m3_layernorm_bwd_reduce
  return launch_reduce_rows2_f32(ws, nblk, D, dgamma, dbeta, beta, s);
}

extern "C" int m3_layernorm_bwd_reduce(const float *ws, int64_t layer_stride, int nblk, int D,
                                       const m3_ln_param_grads *grads_dev, int first, int count, int beta, void *stream) {
  M3_REQUIRE(ws && grads_dev && nblk >= 1 && D > 0 && first >= 0 && count >= 0 && layer_stride >= (int64_t)2 * nblk * D,
             "m3_layernorm_bwd_reduce: bad args");
  if (count == 0) return M3_OK;
  return launch_reduce_rows2_batch_f32(ws, layer_stride, nblk, D, grads_dev, first, count, beta, (hipStream_t)stream);
}
