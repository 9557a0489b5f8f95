// Step 5 of TokenBlock.forward for the blocks that need no router (models/moe/token/vision_transformer_moe.py): the second
// sublayer x + drop_path(mlp(norm2(x))) computed ONLY over the rows that differ - the private rows of every task and one
// row per shared position - and the broadcast of the shared result.  The dense block (dense_mlp_stage + shared_dense_forward
// + apply_shared_broadcast, :443-515, :966-984) is mode M3_TOKEN_FFN_ALL; the shared branch of an MoE block
// (shared_x + drop_path(shared_ffn(norm2(shared_x))), then the broadcast, :1002-1014) is mode M3_TOKEN_FFN_SHARED.
//
//   work list      segment t < T lists the positions where bit t of bits[p] is clear (mode ALL only), segment T the
//                  positions with bits[p] != 0; segment-major, ascending p.  A mark launch turns (seg, p) into an id of 0
//                  or -1 (dropped), m3_route_build with ONE group gives the stable slots, offsets and tile prefix in the form
//                  every grouped GEMM / weight-gradient kernel reads, a last launch writes rows / slot_of / count.  The row
//                  count R never leaves the device: buffers and launches are sized by the bound (T P, or P in mode SHARED).
//   LN-gather      h[r] = LayerNorm(source row of work row r), mean[r], rstd[r]; two-pass variance
//   (FC1, FC2)     m3_gemm_nt grouped calls with G = 1 and the work list's offsets: no GEMM code here
//   scatter        one pass over the positions writes every y_t[p] from x_t, shared_x, f[slot_of] and the two DropPath factors
//   backward       gather: d f[r] = factor * d y (private) or factor * sum over the set bits of d y_t (shared);
//                  (FC2 dgrad with gelu', FC1 dgrad, two m3_wgrad_tn calls with G = 1);
//                  position pass: d x_t[p] and d shared_x[p] = pass-through gradient + LayerNorm backward of d h[slot], or
//                  exact zero; per-workgroup d gamma / d beta partial rows, added in a fixed order by reduce.hip's column sum
//
// Row kernels as in share.hip: one WAVE per row (a position or a work row), four per workgroup, grid-stride; a lane owns the
// 8-element chunks lane, lane + 64 (share_dev.h).  Every row load is unconditional: a slot of -1 reads row 0 of the compact
// buffer (an address that exists; M_ub >= 1 whenever a kernel runs) and the value is discarded by a select, never multiplied
// by zero - the compact buffers hold whatever the allocator left at and past row R.  All arithmetic fp32, no atomics.
#include "share_dev.h"

#pragma clang fp contract(off)

namespace m3 {

constexpr int TOK_MAX_BLOCKS = 2048;                 // work-row kernels: workgroups of a grid-stride launch

struct TokListDev {
  const int64_t *bits; int64_t P; int nt; int mode; int64_t n;
  int32_t *ids;                                      // mark
  const int32_t *pos, *ros, *offsets;                // finish: m3_route_build's outputs
  int32_t *rows, *slot_of, *count; int64_t M_ub;
};

struct TokLnDev {
  m3_share_rows x; const void *sx;
  int64_t P, M_ub; int nt, D;
  const int32_t *rows, *count;
  const float *gamma, *beta; float eps;
  void *h; float *mean, *rstd;
};

struct TokScatDev {
  m3_share_rows x, y; const void *sx, *f;
  const int32_t *slot_of; const int64_t *bits;
  const float *ps, *sps;                             // path_scale [P / N], shared_path_scale [P]; NULL = 1
  int64_t P; int N, D;
};

struct TokGatDev {
  m3_share_rows dy; const int64_t *bits;
  const int32_t *rows, *count;
  const float *ps, *sps;
  int64_t P, M_ub; int N, D;
  void *df;
};

struct TokBwdDev {
  m3_share_rows x, dy, dx; const void *sx; void *dsx;
  const void *dh; const float *mean, *rstd;
  const int32_t *slot_of; const int64_t *bits;
  const float *gamma;
  int64_t P; int D;
  float *part;                                       // [2][gridDim.x][D]: d gamma rows, then d beta rows
};

// the tensor a segment's rows come from: task seg < T, else the shared representative (a wave-uniform select chain: the
// table lives in the kernel arguments, a run-time index into it would go through scratch)
__device__ __forceinline__ const void *tok_source(const m3_share_rows &x, const void *sx, int seg, int T) {
  const void *b = sx;
#pragma unroll
  for (int t = 0; t < M3_SHARE_MAX_T; ++t) b = (t < T && seg == t) ? x.p[t] : b;
  return b;
}

// ---------------------------------------------------------------------------------------------------------- work list
__global__ __launch_bounds__(256) void tok_mark_kernel(const TokListDev p) {
  const unsigned tmask = (1u << p.nt) - 1u;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.n; i += (int64_t)gridDim.x * 256) {
    const int seg = (int)(i / p.P);
    const int64_t pos = i - (int64_t)seg * p.P;
    const unsigned b = (unsigned)p.bits[pos] & tmask;
    const bool listed = seg < p.nt ? (p.mode == M3_TOKEN_FFN_ALL && !((b >> seg) & 1u)) : b != 0u;
    p.ids[i] = listed ? 0 : -1;
  }
}

__global__ __launch_bounds__(256) void tok_finish_kernel(const TokListDev p) {
  const int64_t c = p.offsets[1] < p.M_ub ? p.offsets[1] : p.M_ub;      // (R <= M_ub by the derived bound)
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.n; i += (int64_t)gridDim.x * 256) {
    p.slot_of[i] = p.ids[i] == 0 ? p.pos[i] : -1;
    if (i < c) p.rows[i] = p.ros[i];
    if (i == 0) p.count[0] = (int32_t)c;
  }
}

// ---------------------------------------------------------------------------------------------------- LayerNorm-gather
template <typename T, int NCH>
__global__ __launch_bounds__(ROW_THREADS) void tok_ln_fwd_kernel(const TokLnDev p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D = p.D, P = (int)p.P;
  const int64_t n = *p.count < p.M_ub ? (int64_t)*p.count : p.M_ub;
  float ga[NCH][SHARE_CH], be[NCH][SHARE_CH];
  RowIO<float, NCH>::load(p.gamma, D, lane, ga);
  RowIO<float, NCH>::load(p.beta, D, lane, be);
  const float invD = 1.f / (float)D;
  const int64_t step = (int64_t)gridDim.x * 4;
  int64_t r = (int64_t)blockIdx.x * 4 + wave;
  if (r >= n) return;
  int32_t e = p.rows[r];
  for (; r < n; r += step) {
    const int32_t cur = __builtin_amdgcn_readfirstlane(e);
    e = p.rows[r + step < n ? r + step : r];                    // the next row's entry is under way before this row's load
    const int seg = cur / P;
    const int64_t pos = cur - seg * P;
    const T *src = (const T *)tok_source(p.x, p.sx, seg, p.nt) + pos * D;
    float v[NCH][SHARE_CH];
    RowIO<T, NCH>::load(src, D, lane, v);
    RowIO<T, NCH>::mask(D, lane, v);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int j = 0; j < SHARE_CH; ++j) s += v[i][j];
    const float mean = wave_sum(s) * invD;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const bool ok = (lane + 64 * i) * SHARE_CH < D;
#pragma unroll
      for (int j = 0; j < SHARE_CH; ++j) {
        v[i][j] = ok ? v[i][j] - mean : 0.f;
        q = __builtin_fmaf(v[i][j], v[i][j], q);
      }
    }
    const float rstd = 1.f / sqrtf(wave_sum(q) * invD + p.eps);
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int j = 0; j < SHARE_CH; ++j) v[i][j] = __builtin_fmaf(v[i][j] * rstd, ga[i][j], be[i][j]);
    RowIO<T, NCH>::store((T *)p.h + r * D, D, lane, v);
    if (lane == 0) {
      p.mean[r] = mean;
      p.rstd[r] = rstd;
    }
  }
}

// ------------------------------------------------------------------------------------------------------ scatter forward
// shared_out = sx + sps * f[slot_of[T][p]] (rounded once, the same bits for every task that takes it);
// y_t = bit t ? shared_out : slot_of[t][p] >= 0 ? x_t + ps * f[slot] : x_t's own bits.  ALL = false (mode SHARED): no
// private row is listed, so the f rows of the tasks are not loaded at all.
template <typename T, int NT, int NCH, bool ALL>
__global__ __launch_bounds__(ROW_THREADS) void tok_scatter_fwd_kernel(const TokScatDev p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D = p.D;
  for (int64_t pos = (int64_t)blockIdx.x * 4 + wave; pos < p.P; pos += (int64_t)gridDim.x * 4) {
    const unsigned m = (unsigned)p.bits[pos] & ((1u << NT) - 1u);
    int sl[NT + 1];
#pragma unroll
    for (int t = 0; t <= NT; ++t) sl[t] = (ALL || t == NT) ? p.slot_of[(int64_t)t * p.P + pos] : -1;
    const float a_p = p.ps ? p.ps[pos / p.N] : 1.f, a_s = p.sps ? p.sps[pos] : 1.f;
    float so[NCH][SHARE_CH], fs[NCH][SHARE_CH];
    RowIO<T, NCH>::load((const T *)p.sx + pos * D, D, lane, so);
    RowIO<T, NCH>::load((const T *)p.f + (int64_t)(sl[NT] > 0 ? sl[NT] : 0) * D, D, lane, fs);
    constexpr bool UP = (2 * NT + 2) * NCH <= 24;                 // all rows of the position in flight at once where they fit
    constexpr int NB = UP ? NT : 1;
    float x[NB][NCH][SHARE_CH], f[ALL ? NB : 1][NCH][SHARE_CH];
    if constexpr (UP) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        RowIO<T, NCH>::load((const T *)p.x.p[t] + pos * D, D, lane, x[t]);
        if constexpr (ALL) RowIO<T, NCH>::load((const T *)p.f + (int64_t)(sl[t] > 0 ? sl[t] : 0) * D, D, lane, f[t]);
      }
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int j = 0; j < SHARE_CH; ++j) so[i][j] = __builtin_fmaf(a_s, fs[i][j], so[i][j]);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int b = UP ? t : 0;
      if constexpr (!UP) {
        RowIO<T, NCH>::load((const T *)p.x.p[t] + pos * D, D, lane, x[0]);
        if constexpr (ALL) RowIO<T, NCH>::load((const T *)p.f + (int64_t)(sl[t] > 0 ? sl[t] : 0) * D, D, lane, f[0]);
      }
      T *yr = (T *)p.y.p[t] + pos * D;
      if ((m >> t) & 1u) {
        RowIO<T, NCH>::store(yr, D, lane, so);
      } else {
        if constexpr (ALL) {
          if (sl[t] >= 0) {
#pragma unroll
            for (int i = 0; i < NCH; ++i)
#pragma unroll
              for (int j = 0; j < SHARE_CH; ++j) x[b][i][j] = __builtin_fmaf(a_p, f[b][i][j], x[b][i][j]);
          }
        }
        RowIO<T, NCH>::store(yr, D, lane, x[b]);                 // a pass-through row keeps its bits (16-bit -> fp32 -> 16-bit)
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------ backward gather
template <typename T, int NT, int NCH>
__global__ __launch_bounds__(ROW_THREADS) void tok_gather_bwd_kernel(const TokGatDev p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D = p.D, P = (int)p.P;
  const int64_t n = *p.count < p.M_ub ? (int64_t)*p.count : p.M_ub;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n; r += (int64_t)gridDim.x * 4) {
    const int32_t cur = __builtin_amdgcn_readfirstlane(p.rows[r]);
    const int seg = cur / P;
    const int64_t pos = cur - seg * P;
    float o[NCH][SHARE_CH];
    if (seg < NT) {                                              // (wave-uniform)
      const float a = p.ps ? p.ps[pos / p.N] : 1.f;
      RowIO<T, NCH>::load((const T *)tok_source(p.dy, p.dy.p[0], seg, NT) + pos * D, D, lane, o);
#pragma unroll
      for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int j = 0; j < SHARE_CH; ++j) o[i][j] *= a;
    } else {
      float v[NT][NCH][SHARE_CH];
#pragma unroll
      for (int t = 0; t < NT; ++t) RowIO<T, NCH>::load((const T *)p.dy.p[t] + pos * D, D, lane, v[t]);
      const unsigned m = (unsigned)p.bits[pos];
      const float a = p.sps ? p.sps[pos] : 1.f;
#pragma unroll
      for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int j = 0; j < SHARE_CH; ++j) {
          float acc = 0.f;
#pragma unroll
          for (int t = 0; t < NT; ++t) acc += ((m >> t) & 1u) ? v[t][i][j] : 0.f;
          o[i][j] = a * acc;
        }
    }
    RowIO<T, NCH>::store((T *)p.df + r * D, D, lane, o);
  }
}

// ----------------------------------------------------------------------------------------------- position pass backward
// LayerNorm backward of one listed row, added to `out`: g = d h * gamma, out += rstd (g - mean(g) - xhat mean(g xhat)),
// xhat = (x - mean) rstd; d gamma += d h xhat, d beta += d h.  x, dh: chunks past D are zero.
template <int NCH>
__device__ __forceinline__ void tok_ln_bwd_row(const float (&x)[NCH][SHARE_CH], const float (&dh)[NCH][SHARE_CH],
                                               const float (&ga)[NCH][SHARE_CH], float mean, float rstd, float invD, int D,
                                               int lane, float (&out)[NCH][SHARE_CH], float (&dG)[NCH][SHARE_CH],
                                               float (&dB)[NCH][SHARE_CH]) {
  float xh[NCH][SHARE_CH], g[NCH][SHARE_CH];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const bool ok = (lane + 64 * i) * SHARE_CH < D;
#pragma unroll
    for (int j = 0; j < SHARE_CH; ++j) {
      xh[i][j] = ok ? (x[i][j] - mean) * rstd : 0.f;
      g[i][j] = dh[i][j] * ga[i][j];
      s1 += g[i][j];
      s2 = __builtin_fmaf(g[i][j], xh[i][j], s2);
    }
  }
  const float c1 = wave_sum(s1) * invD, c2 = wave_sum(s2) * invD;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const bool ok = (lane + 64 * i) * SHARE_CH < D;
#pragma unroll
    for (int j = 0; j < SHARE_CH; ++j) {
      const float d = rstd * ((g[i][j] - c1) - xh[i][j] * c2);
      out[i][j] += ok ? d : 0.f;
      dG[i][j] = __builtin_fmaf(dh[i][j], xh[i][j], dG[i][j]);
      dB[i][j] += dh[i][j];
    }
  }
}

template <typename T, int NT, int NCH, bool ALL>
__global__ __launch_bounds__(ROW_THREADS) void tok_scatter_bwd_kernel(const TokBwdDev p) {
  __shared__ float sG[4][NCH * 64 * SHARE_CH];
  __shared__ float sB[4][NCH * 64 * SHARE_CH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D = p.D;
  const float invD = 1.f / (float)D;
  float ga[NCH][SHARE_CH], dG[NCH][SHARE_CH], dB[NCH][SHARE_CH];
  RowIO<float, NCH>::load(p.gamma, D, lane, ga);
  RowIO<float, NCH>::mask(D, lane, ga);
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int j = 0; j < SHARE_CH; ++j) dG[i][j] = dB[i][j] = 0.f;

  for (int64_t pos = (int64_t)blockIdx.x * 4 + wave; pos < p.P; pos += (int64_t)gridDim.x * 4) {
    const unsigned m = (unsigned)p.bits[pos] & ((1u << NT) - 1u);
    int sl[NT + 1];
#pragma unroll
    for (int t = 0; t <= NT; ++t) sl[t] = (ALL || t == NT) ? p.slot_of[(int64_t)t * p.P + pos] : -1;
    float mu[NT + 1], rs[NT + 1];
#pragma unroll
    for (int t = 0; t <= NT; ++t) {
      const int s = sl[t] > 0 ? sl[t] : 0;
      mu[t] = (ALL || t == NT) ? p.mean[s] : 0.f;
      rs[t] = (ALL || t == NT) ? p.rstd[s] : 0.f;
    }
    float sxv[NCH][SHARE_CH], dhs[NCH][SHARE_CH], gs[NCH][SHARE_CH];
    RowIO<T, NCH>::load((const T *)p.sx + pos * D, D, lane, sxv);
    RowIO<T, NCH>::load((const T *)p.dh + (int64_t)(sl[NT] > 0 ? sl[NT] : 0) * D, D, lane, dhs);
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int j = 0; j < SHARE_CH; ++j) gs[i][j] = 0.f;
    constexpr bool UP = 3 * NT * NCH <= 24;                       // all rows of the position in flight at once where they fit
    constexpr int NB = (UP && ALL) ? NT : 1;
    float dy[NT][NCH][SHARE_CH], x[NB][NCH][SHARE_CH], dh[NB][NCH][SHARE_CH];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      RowIO<T, NCH>::load((const T *)p.dy.p[t] + pos * D, D, lane, dy[t]);
      if constexpr (UP && ALL) {
        RowIO<T, NCH>::load((const T *)p.x.p[t] + pos * D, D, lane, x[t]);
        RowIO<T, NCH>::load((const T *)p.dh + (int64_t)(sl[t] > 0 ? sl[t] : 0) * D, D, lane, dh[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int b = (UP && ALL) ? t : 0;
      if constexpr (!UP && ALL) {
        RowIO<T, NCH>::load((const T *)p.x.p[t] + pos * D, D, lane, x[0]);
        RowIO<T, NCH>::load((const T *)p.dh + (int64_t)(sl[t] > 0 ? sl[t] : 0) * D, D, lane, dh[0]);
      }
      RowIO<T, NCH>::mask(D, lane, dy[t]);
      T *dxr = (T *)p.dx.p[t] + pos * D;
      if ((m >> t) & 1u) {                                       // overwritten by the broadcast: its gradient goes to shared_x
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
          for (int j = 0; j < SHARE_CH; ++j) {
            gs[i][j] += dy[t][i][j];
            dy[t][i][j] = 0.f;
          }
      } else if (ALL && sl[t] >= 0) {
        if constexpr (ALL) {
          RowIO<T, NCH>::mask(D, lane, x[b]);
          RowIO<T, NCH>::mask(D, lane, dh[b]);
          tok_ln_bwd_row<NCH>(x[b], dh[b], ga, mu[t], rs[t], invD, D, lane, dy[t], dG, dB);
        }
      }
      RowIO<T, NCH>::store(dxr, D, lane, dy[t]);
    }
    if (m != 0u && sl[NT] >= 0) {
      RowIO<T, NCH>::mask(D, lane, sxv);
      RowIO<T, NCH>::mask(D, lane, dhs);
      tok_ln_bwd_row<NCH>(sxv, dhs, ga, mu[NT], rs[NT], invD, D, lane, gs, dG, dB);
    }
    RowIO<T, NCH>::store((T *)p.dsx + pos * D, D, lane, gs);     // exact zeros where bits == 0
  }

  // the workgroup's two partial rows: the four waves' sums added ((w0 + w1) + w2) + w3
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int j = 0; j < SHARE_CH; ++j) {
      sG[wave][(lane + 64 * i) * SHARE_CH + j] = dG[i][j];
      sB[wave][(lane + 64 * i) * SHARE_CH + j] = dB[i][j];
    }
  __syncthreads();
  float *rowG = p.part + (int64_t)blockIdx.x * D, *rowB = p.part + ((int64_t)gridDim.x + blockIdx.x) * D;
  for (int c = threadIdx.x; c < D; c += ROW_THREADS) {
    rowG[c] = ((sG[0][c] + sG[1][c]) + sG[2][c]) + sG[3][c];
    rowB[c] = ((sB[0][c] + sB[1][c]) + sB[2][c]) + sB[3][c];
  }
}

// ------------------------------------------------------------------------------------------------------------ host side
static int tok_shape_ok(const char *what, int dtype, int T, int64_t P, int D, int mode) {
  M3_REQUIRE(dtype_ok(dtype), "%s: bad dtype", what);
  M3_REQUIRE(mode == M3_TOKEN_FFN_ALL || mode == M3_TOKEN_FFN_SHARED, "%s: mode %d is neither M3_TOKEN_FFN_ALL nor M3_TOKEN_FFN_SHARED", what, mode);
  if (T < 2 || T > M3_SHARE_MAX_T) {
    set_error("%s: T=%d tasks outside [2, %d]", what, T, M3_SHARE_MAX_T);
    return M3_ERR_UNSUPPORTED;
  }
  if (D < SHARE_CH || D > M3_SHARE_MAX_D || D % SHARE_CH) {
    set_error("%s: D=%d must be a multiple of 8 in [8, %d]", what, D, M3_SHARE_MAX_D);
    return M3_ERR_UNSUPPORTED;
  }
  M3_REQUIRE(P >= 0 && (int64_t)(T + 1) * P < ((int64_t)1 << 31), "%s: (T + 1) * B*N = %lld outside [0, 2^31)", what,
             (long long)((int64_t)(T + 1) * P));
  return M3_OK;
}

static int tok_rows_ok(const char *what, const m3_share_rows *r, int T) {
  M3_REQUIRE(r, "%s: null row table", what);
  for (int t = 0; t < T; ++t)
    M3_REQUIRE(r->p[t] && ((uintptr_t)r->p[t] % 16) == 0, "%s: task tensor %d is null or not 16-byte aligned", what, t);
  return M3_OK;
}

static inline bool tok_al16(const void *p) { return ((uintptr_t)p % 16) == 0; }

static inline unsigned tok_row_grid(int64_t rows) {
  const int64_t b = (rows + 3) / 4;
  return (unsigned)(b < 1 ? 1 : b > TOK_MAX_BLOCKS ? TOK_MAX_BLOCKS : b);
}

// kernel<T, NT, NCH> for the run-time dtype, task count and row length
template <typename F> static inline void tok_instance(int dtype, int T, int D, F &&f) {
  by_dtype(dtype, [&](auto tt) {
    by_int<2, 3, 4, 5, 6, 7, 8>(T, [&](auto nt) {
      if (D <= 64 * SHARE_CH) f(tt, nt, IntTag<1>{});
      else f(tt, nt, IntTag<2>{});
    });
  });
}

}  // namespace m3

using namespace m3;

extern "C" int64_t m3_token_ffn_rows_ub(int64_t P, int T, int mode) { return mode == M3_TOKEN_FFN_ALL ? (int64_t)T * P : P; }

extern "C" int64_t m3_token_ffn_list_ws_elems(int64_t P, int T) {
  const int64_t n = (int64_t)(T + 1) * P;
  return 3 * n + 4 + m3_route_ws_elems(n, 1);
}

extern "C" int m3_token_ffn_worklist(const int64_t *bits, int64_t P, int T, int mode, int32_t *rows, int32_t *slot_of,
                                     int32_t *offsets, int32_t *tile_starts, int32_t *count, int32_t *ws, void *stream) {
  int rc = tok_shape_ok("m3_token_ffn_worklist", M3_F32, T, P, SHARE_CH, mode);
  if (rc) return rc;
  M3_REQUIRE(bits && rows && slot_of && offsets && tile_starts && count && ws, "m3_token_ffn_worklist: null operand");
  hipStream_t s = (hipStream_t)stream;
  TokListDev d;
  d.bits = bits; d.P = P; d.nt = T; d.mode = mode; d.n = (int64_t)(T + 1) * P;
  d.M_ub = m3_token_ffn_rows_ub(P, T, mode);
  int32_t *pos = ws + d.n, *ros = ws + 2 * d.n, *counts = ws + 3 * d.n;
  d.ids = ws; d.pos = pos; d.ros = ros; d.offsets = offsets; d.rows = rows; d.slot_of = slot_of; d.count = count;
  if (P == 0) {                                      // nothing to list: all-zero metadata
    if (hipMemsetAsync(offsets, 0, 2 * sizeof(int32_t), s) != hipSuccess || hipMemsetAsync(tile_starts, 0, 2 * sizeof(int32_t), s) != hipSuccess ||
        hipMemsetAsync(count, 0, sizeof(int32_t), s) != hipSuccess) {
      set_error("m3_token_ffn_worklist: hipMemsetAsync failed");
      return M3_ERR_LAUNCH;
    }
    return M3_OK;
  }
  const int64_t want = (d.n + 255) / 256;
  const dim3 grid((unsigned)(want > TOK_MAX_BLOCKS ? TOK_MAX_BLOCKS : want));
  hipLaunchKernelGGL(tok_mark_kernel, grid, dim3(256), 0, s, d);
  if ((rc = check_launch("m3_token_ffn_worklist(mark)"))) return rc;
  if ((rc = m3_route_build(d.ids, d.n, 1, counts, offsets, pos, ros, tile_starts, nullptr, ws + 3 * d.n + 4, stream))) return rc;
  hipLaunchKernelGGL(tok_finish_kernel, grid, dim3(256), 0, s, d);
  return check_launch("m3_token_ffn_worklist(finish)");
}

extern "C" int m3_token_ffn_ln_fwd(const m3_share_rows *x, const void *shared_x, int dtype, int T, int64_t P, int D,
                                   const int32_t *rows, const int32_t *count, int64_t M_ub, const float *gamma,
                                   const float *beta, float eps, void *h, float *mean, float *rstd, void *stream) {
  int rc = tok_shape_ok("m3_token_ffn_ln_fwd", dtype, T, P, D, M3_TOKEN_FFN_ALL);
  if (rc) return rc;
  if ((rc = tok_rows_ok("m3_token_ffn_ln_fwd(x)", x, T))) return rc;
  M3_REQUIRE(shared_x && rows && count && gamma && beta && h && mean && rstd, "m3_token_ffn_ln_fwd: null operand");
  M3_REQUIRE(tok_al16(shared_x) && tok_al16(h) && tok_al16(gamma) && tok_al16(beta),
             "m3_token_ffn_ln_fwd: shared_x, h, gamma and beta must be 16-byte aligned");
  M3_REQUIRE(M_ub >= 0 && M_ub <= (int64_t)T * P && eps >= 0.f, "m3_token_ffn_ln_fwd: M_ub outside [0, T * B*N] or negative eps");
  if (M_ub == 0) return M3_OK;
  TokLnDev d;
  d.x = *x; d.sx = shared_x; d.P = P; d.M_ub = M_ub; d.nt = T; d.D = D; d.rows = rows; d.count = count;
  d.gamma = gamma; d.beta = beta; d.eps = eps; d.h = h; d.mean = mean; d.rstd = rstd;
  const dim3 grid(tok_row_grid(M_ub));
  by_dtype(dtype, [&](auto tt) {
    typedef typename decltype(tt)::type TT;
    if (D <= 64 * SHARE_CH) hipLaunchKernelGGL((tok_ln_fwd_kernel<TT, 1>), grid, dim3(ROW_THREADS), 0, (hipStream_t)stream, d);
    else hipLaunchKernelGGL((tok_ln_fwd_kernel<TT, 2>), grid, dim3(ROW_THREADS), 0, (hipStream_t)stream, d);
  });
  return check_launch("m3_token_ffn_ln_fwd");
}

extern "C" int m3_token_ffn_scatter_fwd(const m3_share_rows *x, const void *shared_x, const void *f, int dtype, int T,
                                        int64_t P, int N, int D, int mode, const int32_t *slot_of, const int64_t *bits,
                                        const float *path_scale, const float *shared_path_scale, const m3_share_rows *y,
                                        void *stream) {
  int rc = tok_shape_ok("m3_token_ffn_scatter_fwd", dtype, T, P, D, mode);
  if (rc) return rc;
  if ((rc = tok_rows_ok("m3_token_ffn_scatter_fwd(x)", x, T))) return rc;
  if ((rc = tok_rows_ok("m3_token_ffn_scatter_fwd(y)", y, T))) return rc;
  M3_REQUIRE(shared_x && f && slot_of && bits, "m3_token_ffn_scatter_fwd: null operand");
  M3_REQUIRE(tok_al16(shared_x) && tok_al16(f), "m3_token_ffn_scatter_fwd: shared_x and f must be 16-byte aligned");
  M3_REQUIRE(N >= 1 && P % N == 0, "m3_token_ffn_scatter_fwd: N=%d tokens per sample must divide B*N=%lld", N, (long long)P);
  if (P == 0) return M3_OK;
  TokScatDev d;
  d.x = *x; d.y = *y; d.sx = shared_x; d.f = f; d.slot_of = slot_of; d.bits = bits; d.ps = path_scale; d.sps = shared_path_scale;
  d.P = P; d.N = N; d.D = D;
  const dim3 grid((unsigned)m3_share_num_blocks(P));
  hipStream_t s = (hipStream_t)stream;
  tok_instance(dtype, T, D, [&](auto tt, auto nt, auto nch) {
    typedef typename decltype(tt)::type TT;
    constexpr int NT = decltype(nt)::value, NCH = decltype(nch)::value;
    if (mode == M3_TOKEN_FFN_ALL) hipLaunchKernelGGL((tok_scatter_fwd_kernel<TT, NT, NCH, true>), grid, dim3(ROW_THREADS), 0, s, d);
    else hipLaunchKernelGGL((tok_scatter_fwd_kernel<TT, NT, NCH, false>), grid, dim3(ROW_THREADS), 0, s, d);
  });
  return check_launch("m3_token_ffn_scatter_fwd");
}

extern "C" int m3_token_ffn_gather_bwd(const m3_share_rows *dy, int dtype, int T, int64_t P, int N, int D,
                                       const int32_t *rows, const int32_t *count, int64_t M_ub, const int64_t *bits,
                                       const float *path_scale, const float *shared_path_scale, void *df, void *stream) {
  int rc = tok_shape_ok("m3_token_ffn_gather_bwd", dtype, T, P, D, M3_TOKEN_FFN_ALL);
  if (rc) return rc;
  if ((rc = tok_rows_ok("m3_token_ffn_gather_bwd(dy)", dy, T))) return rc;
  M3_REQUIRE(rows && count && bits && df && tok_al16(df), "m3_token_ffn_gather_bwd: null operand or df not 16-byte aligned");
  M3_REQUIRE(M_ub >= 0 && M_ub <= (int64_t)T * P, "m3_token_ffn_gather_bwd: M_ub outside [0, T * B*N]");
  M3_REQUIRE(N >= 1 && P % N == 0, "m3_token_ffn_gather_bwd: N=%d tokens per sample must divide B*N=%lld", N, (long long)P);
  if (M_ub == 0) return M3_OK;
  TokGatDev d;
  d.dy = *dy; d.bits = bits; d.rows = rows; d.count = count; d.ps = path_scale; d.sps = shared_path_scale;
  d.P = P; d.M_ub = M_ub; d.N = N; d.D = D; d.df = df;
  const dim3 grid(tok_row_grid(M_ub));
  tok_instance(dtype, T, D, [&](auto tt, auto nt, auto nch) {
    hipLaunchKernelGGL((tok_gather_bwd_kernel<typename decltype(tt)::type, decltype(nt)::value, decltype(nch)::value>), grid,
                       dim3(ROW_THREADS), 0, (hipStream_t)stream, d);
  });
  return check_launch("m3_token_ffn_gather_bwd");
}

extern "C" int64_t m3_token_ffn_bwd_ws_elems(int64_t P, int D) { return 2 * (int64_t)m3_share_num_blocks(P) * D; }

extern "C" int m3_token_ffn_scatter_bwd(const m3_share_rows *x, const void *shared_x, const m3_share_rows *dy, const void *dh,
                                        const float *mean, const float *rstd, int dtype, int T, int64_t P, int D, int mode,
                                        const int32_t *slot_of, const int64_t *bits, const float *gamma,
                                        const m3_share_rows *dx, void *d_shared_x, float *ws, float *d_gamma, float *d_beta,
                                        void *stream) {
  int rc = tok_shape_ok("m3_token_ffn_scatter_bwd", dtype, T, P, D, mode);
  if (rc) return rc;
  if ((rc = tok_rows_ok("m3_token_ffn_scatter_bwd(x)", x, T))) return rc;
  if ((rc = tok_rows_ok("m3_token_ffn_scatter_bwd(dy)", dy, T))) return rc;
  if ((rc = tok_rows_ok("m3_token_ffn_scatter_bwd(dx)", dx, T))) return rc;
  M3_REQUIRE(shared_x && dh && mean && rstd && slot_of && bits && gamma && d_shared_x && ws && d_gamma && d_beta,
             "m3_token_ffn_scatter_bwd: null operand");
  M3_REQUIRE(tok_al16(shared_x) && tok_al16(dh) && tok_al16(d_shared_x) && tok_al16(gamma),
             "m3_token_ffn_scatter_bwd: shared_x, dh, d_shared_x and gamma must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (P == 0) {
    if (hipMemsetAsync(d_gamma, 0, D * sizeof(float), s) != hipSuccess || hipMemsetAsync(d_beta, 0, D * sizeof(float), s) != hipSuccess) {
      set_error("m3_token_ffn_scatter_bwd: hipMemsetAsync failed");
      return M3_ERR_LAUNCH;
    }
    return M3_OK;
  }
  TokBwdDev d;
  d.x = *x; d.dy = *dy; d.dx = *dx; d.sx = shared_x; d.dsx = d_shared_x; d.dh = dh; d.mean = mean; d.rstd = rstd;
  d.slot_of = slot_of; d.bits = bits; d.gamma = gamma; d.P = P; d.D = D; d.part = ws;
  const int nblk = m3_share_num_blocks(P);
  const dim3 grid((unsigned)nblk);
  tok_instance(dtype, T, D, [&](auto tt, auto nt, auto nch) {
    typedef typename decltype(tt)::type TT;
    constexpr int NT = decltype(nt)::value, NCH = decltype(nch)::value;
    if (mode == M3_TOKEN_FFN_ALL) hipLaunchKernelGGL((tok_scatter_bwd_kernel<TT, NT, NCH, true>), grid, dim3(ROW_THREADS), 0, s, d);
    else hipLaunchKernelGGL((tok_scatter_bwd_kernel<TT, NT, NCH, false>), grid, dim3(ROW_THREADS), 0, s, d);
  });
  if ((rc = check_launch("m3_token_ffn_scatter_bwd"))) return rc;
  return launch_reduce_rows2_f32(ws, nblk, D, d_gamma, d_beta, 0, s);
}
