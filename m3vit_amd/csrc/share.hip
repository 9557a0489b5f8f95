// The token sharing stage of a TokenBlock (models/moe/token/): shareability predictor, merge / split transition and
// broadcast in ONE row pass over the T task tensors, its backward, the predictor alone, the masked mean of
// Aggregation / AggregationStage, and the compaction + statistics launch that replaces nonzero() and the .item() reads.
//
// Row kernels: one WAVE per position p in [0, B*N), four positions per workgroup, grid-stride over the positions (at most
// M3_SHARE_MAX_BLOCKS workgroups, so that what a wave prepares once - its slice of w_gate, the tasks' embedding logits -
// is shared by all its positions and the backward's parameter partials are one row per workgroup).  A lane owns the
// 8-element chunks lane, lane + 64 of a row (D <= M3_SHARE_MAX_D = 1024, D % 8 == 0): 16-byte accesses for fp16 / bf16, two
// per chunk for fp32.  Every load of a position - the T rows and, in the backward, the T gradient rows, d shared_x and
// shared_x - is issued before the first use; chunks past D load chunk 0 and are zeroed, so no load sits behind a branch.
//
// Arithmetic, stated once (tests/sharing_cases.py derives its bounds from this):
//   logit_j(t) = bias_j(t) + wave_sum(lane chain of fma(x_d, w[d][j], .)),  bias_j(t) = wave_sum(chain of task_emb[t][e] w[D+e][j])
//   z = ((l1 + n1) - (l0 + n0)) / tau;  soft = sigmoid(z) (the 2-way softmax's second entry);  G = soft, or (z > 0) when hard
//   M_t = G_t >= gamma, dropped where fewer than 2 tasks agree;  den = (sum_t G_t M_t, t ascending) + eps;  W_t = G_t M_t / den
//   shared_x = fma chain over t ascending of W_t x_t, rounded once to the activation dtype; y_t = that value or x_t's own bits
// No atomics anywhere: the parameter gradients are per-workgroup partials added in a fixed order by one reduce launch.
#include "share_dev.h"

#pragma clang fp contract(off)

namespace m3 {

constexpr int SHARE_SCAN = M3_SHARE_SCAN_WIDTH;     // positions per step of the compaction scan = its workgroup size

struct ShareFwdDev {
  m3_share_rows x, y;
  int64_t P; int D; int Dg;
  const float *w; const float *emb; const float *noise;
  float tau, gamma, eps; int hard;
  void *sx; int64_t *bits; float *g; float *soft;
};

struct ShareBwdDev {
  m3_share_rows x, dy, dx;
  int64_t P; int D; int Dg;
  const float *w; const float *emb;
  float tau, eps;
  const int64_t *bits; const float *g; const float *soft; const void *sx; const void *dsx; const float *dg;
  float *part;
};

struct ShareAggDev {
  m3_share_rows x, y;                               // backward: x = d y, y = d x
  int64_t P; int D;
  const int64_t *mask; const unsigned char *need; float eps;
  void *agg;                                        // forward: the dense mean (optional); backward: d agg (optional)
};

// the lane's slice of w_gate [D + Dg][2] (rows d of its chunks): column 0 and column 1
template <int NCH>
__device__ __forceinline__ void share_load_w(const float *w, int D, int lane, float (&w0)[NCH][SHARE_CH], float (&w1)[NCH][SHARE_CH]) {
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int d = (lane + 64 * i) * SHARE_CH;
    const bool ok = d < D;
    const f32x4 *p = (const f32x4 *)(w + (int64_t)(ok ? d : 0) * 2);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 v = p[q];
      w0[i][2 * q] = ok ? v[0] : 0.f; w1[i][2 * q] = ok ? v[1] : 0.f;
      w0[i][2 * q + 1] = ok ? v[2] : 0.f; w1[i][2 * q + 1] = ok ? v[3] : 0.f;
    }
  }
}

// the two logits a task's embedding adds at every position
__device__ __forceinline__ void share_emb_logits(const float *emb_t, const float *w, int D, int Dg, int lane, float &b0, float &b1) {
  float a0 = 0.f, a1 = 0.f;
  for (int e = lane; e < Dg; e += 64) {
    const float v = emb_t[e];
    a0 = __builtin_fmaf(v, w[(int64_t)(D + e) * 2], a0);
    a1 = __builtin_fmaf(v, w[(int64_t)(D + e) * 2 + 1], a1);
  }
  b0 = wave_sum(a0);
  b1 = wave_sum(a1);
}

// THE predictor of one row: the same code for m3_share_stage_fwd and m3_share_predict_fwd, so both give the same bits for
// the same row.  Every lane returns the same values.
template <int NCH>
__device__ __forceinline__ void share_score(const float (&x)[NCH][SHARE_CH], const float (&w0)[NCH][SHARE_CH],
                                            const float (&w1)[NCH][SHARE_CH], float b0, float b1, float n0, float n1, float tau,
                                            int hard, float &G, float &soft) {
  float a0 = 0.f, a1 = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int j = 0; j < SHARE_CH; ++j) {
      a0 = __builtin_fmaf(x[i][j], w0[i][j], a0);
      a1 = __builtin_fmaf(x[i][j], w1[i][j], a1);
    }
  const float l0 = (wave_sum(a0) + b0) + n0, l1 = (wave_sum(a1) + b1) + n1;
  const float z = (l1 - l0) / tau;
  const float e = expf(-fabsf(z));
  const float s = 1.f / (1.f + e);
  soft = z >= 0.f ? s : e * s;
  G = hard ? (z > 0.f ? 1.f : 0.f) : soft;          // a tie goes to index 0 (private), as max() does
}

// mask, denominator and weights of a position from its scores: forward and backward alike
template <int NT>
__device__ __forceinline__ void share_weights(const float (&G)[NT], unsigned m, float eps, float &den, float (&W)[NT]) {
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) s += ((m >> t) & 1u) ? G[t] : 0.f;
  den = s + eps;
#pragma unroll
  for (int t = 0; t < NT; ++t) W[t] = ((m >> t) & 1u) ? G[t] / den : 0.f;
}

// ----------------------------------------------------------------------------------------------------------- forward
// NT = 1 is the predictor alone (no y, shared_x, bits)
template <typename T, int NT, int NCH>
__global__ __launch_bounds__(ROW_THREADS) void share_fwd_kernel(const ShareFwdDev p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D = p.D;
  float w0[NCH][SHARE_CH], w1[NCH][SHARE_CH];
  share_load_w<NCH>(p.w, D, lane, w0, w1);
  float b0[NT], b1[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    b0[t] = 0.f; b1[t] = 0.f;
    if (p.emb) share_emb_logits(p.emb + (int64_t)t * p.Dg, p.w, D, p.Dg, lane, b0[t], b1[t]);
  }
  for (int64_t pos = (int64_t)blockIdx.x * 4 + wave; pos < p.P; pos += (int64_t)gridDim.x * 4) {
    float x[NT][NCH][SHARE_CH];
    float n0[NT], n1[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) RowIO<T, NCH>::load((const T *)p.x.p[t] + pos * D, D, lane, x[t]);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      n0[t] = p.noise ? p.noise[((int64_t)t * p.P + pos) * 2] : 0.f;
      n1[t] = p.noise ? p.noise[((int64_t)t * p.P + pos) * 2 + 1] : 0.f;
    }
    float G[NT], soft[NT];
    unsigned m = 0u;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      RowIO<T, NCH>::mask(D, lane, x[t]);
      share_score<NCH>(x[t], w0, w1, b0[t], b1[t], n0[t], n1[t], p.tau, p.hard, G[t], soft[t]);
      if (G[t] >= p.gamma) m |= 1u << t;
    }
    if (lane == 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        st_nt<true>(p.g + (int64_t)t * p.P + pos, G[t]);        // next read by the backward
        if (p.soft) st_nt<true>(p.soft + (int64_t)t * p.P + pos, soft[t]);
      }
    }
    if constexpr (NT > 1) {
      if (__builtin_popcount(m) < 2) m = 0u;
      float den, W[NT];
      share_weights<NT>(G, m, p.eps, den, W);
      float sx[NCH][SHARE_CH];
#pragma unroll
      for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int j = 0; j < SHARE_CH; ++j) {
          float a = 0.f;
#pragma unroll
          for (int t = 0; t < NT; ++t) a = __builtin_fmaf(W[t], x[t][i][j], a);
          sx[i][j] = a;                                          // zeros where nothing is shared (every W is 0)
        }
      if (lane == 0) p.bits[pos] = (int64_t)m;
      RowIO<T, NCH>::store((T *)p.sx + pos * D, D, lane, sx);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        T *yr = (T *)p.y.p[t] + pos * D;
        if ((m >> t) & 1u) RowIO<T, NCH>::store(yr, D, lane, sx);
        else RowIO<T, NCH>::store(yr, D, lane, x[t]);            // the row's own bits (16-bit -> fp32 -> 16-bit is exact)
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------------------- backward
// per position: g = d shared_x + sum_{t in M} d y_t;  d G_t = M_t <g, x_t - shared_x> / den + d g_t;
// d l1 = d G y (1 - y) / tau = -d l0;  d x_t = (M_t ? W_t g : d y_t) + d l1 (w[d][1] - w[d][0]).
// Parameter partials of the workgroup, one row of NC = D + Dg + NT * Dg floats:
//   [0, D)            A_d = sum d l1 x_t[d]            (d w_gate[d][1]; column 0 is its negative)
//   [D, D + Dg)       sum_t task_emb[t][e] R_t          (d w_gate[D + e][1]),  R_t = sum over positions of d l1(t)
//   then [t][e]       R_t (w[D + e][1] - w[D + e][0])   (d task_emb[t][e])
template <typename T, int NT, int NCH>
__global__ __launch_bounds__(ROW_THREADS) void share_bwd_kernel(const ShareBwdDev p) {
  __shared__ float sA[4][NCH * 64 * SHARE_CH];
  __shared__ float sR[4][NT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D = p.D, Dg = p.Dg;
  float wd[NCH][SHARE_CH];
  {
    float w0[NCH][SHARE_CH], w1[NCH][SHARE_CH];
    share_load_w<NCH>(p.w, D, lane, w0, w1);
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int j = 0; j < SHARE_CH; ++j) wd[i][j] = w1[i][j] - w0[i][j];
  }
  float A[NCH][SHARE_CH], R[NT];
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int j = 0; j < SHARE_CH; ++j) A[i][j] = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) R[t] = 0.f;

  for (int64_t pos = (int64_t)blockIdx.x * 4 + wave; pos < p.P; pos += (int64_t)gridDim.x * 4) {
    float x[NT][NCH][SHARE_CH], dy[NT][NCH][SHARE_CH], sx[NCH][SHARE_CH], g[NCH][SHARE_CH];
#pragma unroll
    for (int t = 0; t < NT; ++t) RowIO<T, NCH>::load((const T *)p.x.p[t] + pos * D, D, lane, x[t]);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (p.dy.p[t]) RowIO<T, NCH>::load((const T *)p.dy.p[t] + pos * D, D, lane, dy[t]);      // (a wave-uniform pointer test)
      else {
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
          for (int j = 0; j < SHARE_CH; ++j) dy[t][i][j] = 0.f;
      }
    }
    if (NT > 1 && p.dsx) RowIO<T, NCH>::load((const T *)p.dsx + pos * D, D, lane, g);
    else {
#pragma unroll
      for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int j = 0; j < SHARE_CH; ++j) g[i][j] = 0.f;
    }
    if constexpr (NT > 1) RowIO<T, NCH>::load((const T *)p.sx + pos * D, D, lane, sx);
    float G[NT], ys[NT], dgo[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      G[t] = ld_nt<true>(p.g + (int64_t)t * p.P + pos);
      ys[t] = p.soft ? ld_nt<true>(p.soft + (int64_t)t * p.P + pos) : G[t];
      dgo[t] = p.dg ? p.dg[(int64_t)t * p.P + pos] : 0.f;
    }
    const unsigned m = (NT > 1) ? (unsigned)p.bits[pos] : 0u;
    float den = 1.f, W[NT];
    if constexpr (NT > 1) share_weights<NT>(G, m, p.eps, den, W);
    else W[0] = 0.f;
    RowIO<T, NCH>::mask(D, lane, g);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      RowIO<T, NCH>::mask(D, lane, x[t]);
      RowIO<T, NCH>::mask(D, lane, dy[t]);
      if ((m >> t) & 1u) {
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
          for (int j = 0; j < SHARE_CH; ++j) g[i][j] += dy[t][i][j];
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const bool sh = (m >> t) & 1u;
      float dot = 0.f;
      if constexpr (NT > 1) {
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
          for (int j = 0; j < SHARE_CH; ++j) a = __builtin_fmaf(g[i][j], x[t][i][j] - sx[i][j], a);
        a = wave_sum(a);                      // (chunks past D: g is zero there)
        dot = sh ? a / den : 0.f;
      }
      const float dG = dot + dgo[t];
      const float dl1 = dG * ys[t] * (1.f - ys[t]) / p.tau;
      R[t] += dl1;
      float o[NCH][SHARE_CH];
#pragma unroll
      for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int j = 0; j < SHARE_CH; ++j) {
          A[i][j] = __builtin_fmaf(dl1, x[t][i][j], A[i][j]);
          o[i][j] = __builtin_fmaf(dl1, wd[i][j], sh ? W[t] * g[i][j] : dy[t][i][j]);
        }
      RowIO<T, NCH>::store((T *)p.dx.p[t] + pos * D, D, lane, o);
    }
  }

  // the workgroup's partial row: the four waves' sums added ((w0 + w1) + w2) + w3
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int j = 0; j < SHARE_CH; ++j) sA[wave][(lane + 64 * i) * SHARE_CH + j] = A[i][j];
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < NT; ++t) sR[wave][t] = R[t];
  }
  __syncthreads();
  const int NC = D + Dg + NT * Dg;
  float *row = p.part + (int64_t)blockIdx.x * NC;
  for (int c = threadIdx.x; c < NC; c += ROW_THREADS) {
    float v;
    if (c < D) {
      v = ((sA[0][c] + sA[1][c]) + sA[2][c]) + sA[3][c];
    } else if (c < D + Dg) {
      const int e = c - D;
      v = 0.f;
      for (int t = 0; t < NT; ++t) v = __builtin_fmaf(p.emb[(int64_t)t * Dg + e], ((sR[0][t] + sR[1][t]) + sR[2][t]) + sR[3][t], v);
    } else {
      const int t = (c - D - Dg) / Dg, e = (c - D - Dg) - t * Dg;
      v = (((sR[0][t] + sR[1][t]) + sR[2][t]) + sR[3][t]) * (p.w[(int64_t)(D + e) * 2 + 1] - p.w[(int64_t)(D + e) * 2]);
    }
    row[c] = v;
  }
}

// columns of the partial rows added in a fixed order (8 interleaved row lanes, then lanes 0 .. 7, as reduce.hip), written in
// the parameters' own layouts
__global__ __launch_bounds__(256) void share_bwd_reduce_kernel(const float *__restrict__ part, int nrows, int NC, int DW,
                                                               float *__restrict__ dw, float *__restrict__ demb) {
  __shared__ float s[8][33];
  const int c = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int n = blockIdx.x * 32 + c;
  float acc = 0.f;
  if (n < NC) {
#pragma unroll 4
    for (int r = rl; r < nrows; r += 8) acc += part[(int64_t)r * NC + n];
  }
  s[rl][c] = acc;
  __syncthreads();
  if (rl == 0 && n < NC) {
    float t = s[0][c];
#pragma unroll
    for (int i = 1; i < 8; ++i) t += s[i][c];
    if (n < DW) {
      dw[(int64_t)n * 2] = -t;
      dw[(int64_t)n * 2 + 1] = t;
    } else if (demb) {
      demb[n - DW] = t;
    }
  }
}

// ------------------------------------------------------------------------------------- Aggregation / AggregationStage
// forward: agg = sum_s v_s x_s / (count + eps), y_t = v_t ? agg : x_t, v = mask bits of the position where agg_needed.
// BWD: the same pass over d y -> d x with d agg joining the sum: d x_s = v_s (d agg + sum_{t in v} d y_t) / (count + eps)
// + (1 - v_s) d y_s
template <typename T, int NT, int NCH, bool BWD>
__global__ __launch_bounds__(ROW_THREADS) void share_agg_kernel(const ShareAggDev p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D = p.D;
  for (int64_t pos = (int64_t)blockIdx.x * 4 + wave; pos < p.P; pos += (int64_t)gridDim.x * 4) {
    float x[NT][NCH][SHARE_CH], a[NCH][SHARE_CH];
#pragma unroll
    for (int t = 0; t < NT; ++t) RowIO<T, NCH>::load((const T *)p.x.p[t] + pos * D, D, lane, x[t]);
    const bool extra = BWD && p.agg;
    if (extra) RowIO<T, NCH>::load((const T *)p.agg + pos * D, D, lane, a);
    else {
#pragma unroll
      for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int j = 0; j < SHARE_CH; ++j) a[i][j] = 0.f;
    }
    unsigned v = (unsigned)p.mask[pos] & ((1u << NT) - 1u);
    if (p.need && !p.need[pos]) v = 0u;
    const float inv = 1.f / ((float)__builtin_popcount(v) + p.eps);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if ((v >> t) & 1u) {
#pragma unroll
        for (int i = 0; i < NCH; ++i)
#pragma unroll
          for (int j = 0; j < SHARE_CH; ++j) a[i][j] += x[t][i][j];
      }
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int j = 0; j < SHARE_CH; ++j) a[i][j] = v ? a[i][j] * inv : 0.f;
    if (!BWD && p.agg) RowIO<T, NCH>::store((T *)p.agg + pos * D, D, lane, a);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      T *yr = (T *)p.y.p[t] + pos * D;
      if ((v >> t) & 1u) RowIO<T, NCH>::store(yr, D, lane, a);
      else RowIO<T, NCH>::store(yr, D, lane, x[t]);
    }
  }
}

// ------------------------------------------------------------------------------- compaction and statistics, one workgroup
// SHARE_SCAN positions per step, one per thread: the ballot of a wave gives the rank inside it, the 16 wave totals pass
// through LDS, the running count is carried from step to step (the scan of route_dev.h, over flags instead of histograms).
// Integer work: the same bits on every run.
__global__ __launch_bounds__(SHARE_SCAN) void share_compact_kernel(const int64_t *__restrict__ bits, const int64_t *__restrict__ prev,
                                                                   int64_t P, int T, int32_t *__restrict__ idx,
                                                                   int32_t *__restrict__ count, int64_t *__restrict__ stats) {
  constexpr int NW = SHARE_SCAN / 64, NS = 3 + M3_SHARE_MAX_T;
  __shared__ int wtot[2][NW];
  __shared__ int red[NW][NS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;
  int st[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) st[k] = 0;
  int64_t b = tid < P ? bits[tid] : 0, pb = (prev && tid < P) ? prev[tid] : 0;
  int step = 0;
  for (int64_t base = 0; base < P; base += SHARE_SCAN, ++step) {
    const int64_t pos = base + tid;
    const int64_t cur = b, curp = pb;
    const int64_t nxt = pos + SHARE_SCAN;                       // the next step's words are under way before this one's barrier
    b = nxt < P ? bits[nxt] : 0;
    pb = (prev && nxt < P) ? prev[nxt] : 0;
    const bool in = pos < P, flag = in && cur != 0;
    if (in) {
      const int pc = __builtin_popcountll((unsigned long long)cur);
      st[0] += pc;
      st[1] += (pc > 0 && pc < T) ? 1 : 0;
      st[2] += (prev && curp != cur) ? 1 : 0;
#pragma unroll
      for (int t = 0; t < M3_SHARE_MAX_T; ++t) st[3 + t] += (t < T) ? (int)((cur >> t) & 1) : 0;
    }
    const unsigned long long bal = __ballot(flag);
    const int before = __builtin_popcountll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[step & 1][wave] = __builtin_popcountll(bal);
    __syncthreads();                                            // double-buffered totals: one barrier per step
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const int v = wtot[step & 1][w];
      off += w < wave ? v : 0;
      tot += v;
    }
    if (flag && idx) idx[carry + off + before] = (int32_t)pos;
    carry += tot;
  }
  if (idx)
    for (int64_t i = carry + tid; i < P; i += SHARE_SCAN) idx[i] = -1;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const int v = wave_sum_i(st[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (tid < NS) {
    long long v = 0;
    for (int w = 0; w < NW; ++w) v += red[w][tid];
    if (tid == 0) stats[M3_SHARE_STAT_TASKTOKENS] = v;
    else if (tid == 1) stats[M3_SHARE_STAT_PARTIAL] = v;
    else if (tid == 2) stats[M3_SHARE_STAT_FLIPS] = v;
    else stats[M3_SHARE_STAT_S_T + tid - 3] = v;
  }
  if (tid == 0) {
    if (count) *count = carry;
    stats[M3_SHARE_STAT_POSITIONS] = carry;
    stats[M3_SHARE_STAT_PARTIAL_TOTAL] = P;
    stats[M3_SHARE_STAT_FLIP_TOTAL] = prev ? P : 0;
    stats[M3_SHARE_STAT_S] = carry;
  }
}

// ------------------------------------------------------------------------------------------------------------ host side
static int share_rows_ok(const char *what, const m3_share_rows *r, int T, bool may_be_null) {
  M3_REQUIRE(r, "%s: null row table", what);
  for (int t = 0; t < T; ++t) {
    M3_REQUIRE(may_be_null || r->p[t], "%s: null task tensor %d", what, t);
    M3_REQUIRE(((uintptr_t)r->p[t] % 16) == 0, "%s: task tensor %d is not 16-byte aligned", what, t);
  }
  return M3_OK;
}

static int share_shape_ok(const char *what, int dtype, int T, int tmin, int64_t P, int D, int Dg) {
  M3_REQUIRE(dtype_ok(dtype), "%s: bad dtype", what);
  if (T < tmin || T > M3_SHARE_MAX_T) {
    set_error("%s: T=%d tasks outside [%d, %d]", what, T, tmin, M3_SHARE_MAX_T);
    return M3_ERR_UNSUPPORTED;
  }
  if (D < SHARE_CH || D > M3_SHARE_MAX_D || D % SHARE_CH) {
    set_error("%s: D=%d must be a multiple of 8 in [8, %d]", what, D, M3_SHARE_MAX_D);
    return M3_ERR_UNSUPPORTED;
  }
  M3_REQUIRE(Dg >= 0, "%s: Dg=%d is negative", what, Dg);
  M3_REQUIRE(P >= 0 && P < ((int64_t)1 << 31), "%s: B*N=%lld outside [0, 2^31)", what, (long long)P);
  return M3_OK;
}

// kernel<T, NT, NCH> for the run-time dtype, task count and row length
template <int TMIN, typename F> static inline void share_instance(int dtype, int T, int D, F &&f) {
  by_dtype(dtype, [&](auto tt) {
    auto with_t = [&](auto nt) {
      if (D <= 64 * SHARE_CH) f(tt, nt, IntTag<1>{});
      else f(tt, nt, IntTag<2>{});
    };
    if constexpr (TMIN == 1) with_t(IntTag<1>{});
    else by_int<2, 3, 4, 5, 6, 7, 8>(T, with_t);
  });
}

}  // namespace m3

using namespace m3;

extern "C" int m3_share_num_blocks(int64_t P) {
  const int64_t b = (P + 3) / 4;
  return (int)(b < 1 ? 1 : b > M3_SHARE_MAX_BLOCKS ? M3_SHARE_MAX_BLOCKS : b);
}

extern "C" int64_t m3_share_bwd_ws_elems(int64_t P, int T, int D, int Dg) {
  return (int64_t)m3_share_num_blocks(P) * ((int64_t)D + Dg + (int64_t)T * Dg);
}

static int share_fwd_launch(const char *what, ShareFwdDev &d, int dtype, int T, hipStream_t s) {
  if (d.P == 0) return M3_OK;
  const dim3 grid((unsigned)m3_share_num_blocks(d.P));
  if (T == 1)
    share_instance<1>(dtype, T, d.D, [&](auto tt, auto nt, auto nch) {
      hipLaunchKernelGGL((share_fwd_kernel<typename decltype(tt)::type, 1, decltype(nch)::value>), grid, dim3(ROW_THREADS), 0, s, d);
    });
  else
    share_instance<2>(dtype, T, d.D, [&](auto tt, auto nt, auto nch) {
      hipLaunchKernelGGL((share_fwd_kernel<typename decltype(tt)::type, decltype(nt)::value, decltype(nch)::value>), grid,
                         dim3(ROW_THREADS), 0, s, d);
    });
  return check_launch(what);
}

static int share_bwd_launch(const char *what, ShareBwdDev &d, int dtype, int T, float *d_w_gate, float *d_task_emb, hipStream_t s) {
  if (d.P == 0) return M3_OK;
  const int nblk = m3_share_num_blocks(d.P);
  const dim3 grid((unsigned)nblk);
  if (T == 1)
    share_instance<1>(dtype, T, d.D, [&](auto tt, auto nt, auto nch) {
      hipLaunchKernelGGL((share_bwd_kernel<typename decltype(tt)::type, 1, decltype(nch)::value>), grid, dim3(ROW_THREADS), 0, s, d);
    });
  else
    share_instance<2>(dtype, T, d.D, [&](auto tt, auto nt, auto nch) {
      hipLaunchKernelGGL((share_bwd_kernel<typename decltype(tt)::type, decltype(nt)::value, decltype(nch)::value>), grid,
                         dim3(ROW_THREADS), 0, s, d);
    });
  int rc = check_launch(what);
  if (rc) return rc;
  const int NC = d.D + d.Dg + T * d.Dg;
  hipLaunchKernelGGL(share_bwd_reduce_kernel, dim3((NC + 31) / 32), dim3(256), 0, s, d.part, nblk, NC, d.D + d.Dg, d_w_gate,
                     d_task_emb);
  return check_launch(what);
}

extern "C" int m3_share_stage_fwd(const m3_share_rows *x, int dtype, int T, int64_t P, int D, const float *w_gate,
                                  const float *task_emb, int Dg, const float *noise, float tau, int hard, float gamma,
                                  float eps, const m3_share_rows *y, void *shared_x, int64_t *shared_bits, float *g,
                                  float *soft, void *stream) {
  int rc = share_shape_ok("m3_share_stage_fwd", dtype, T, 2, P, D, Dg);
  if (rc) return rc;
  if ((rc = share_rows_ok("m3_share_stage_fwd(x)", x, T, false))) return rc;
  if ((rc = share_rows_ok("m3_share_stage_fwd(y)", y, T, false))) return rc;
  M3_REQUIRE(w_gate && shared_x && shared_bits && g, "m3_share_stage_fwd: null operand");
  M3_REQUIRE(((uintptr_t)w_gate % 16) == 0 && ((uintptr_t)shared_x % 16) == 0, "m3_share_stage_fwd: w_gate and shared_x must be 16-byte aligned");
  M3_REQUIRE((Dg > 0) == (task_emb != nullptr), "m3_share_stage_fwd: task_emb goes with Dg > 0");
  M3_REQUIRE(tau > 0.f && eps >= 0.f, "m3_share_stage_fwd: tau must be positive, eps non-negative");
  M3_REQUIRE(!hard || soft, "m3_share_stage_fwd: hard mode writes the soft probability too");
  ShareFwdDev d;
  d.x = *x; d.y = *y; d.P = P; d.D = D; d.Dg = Dg; d.w = w_gate; d.emb = task_emb; d.noise = noise;
  d.tau = tau; d.gamma = gamma; d.eps = eps; d.hard = hard; d.sx = shared_x; d.bits = shared_bits; d.g = g; d.soft = soft;
  return share_fwd_launch("m3_share_stage_fwd", d, dtype, T, (hipStream_t)stream);
}

extern "C" int m3_share_predict_fwd(const void *x, int dtype, int64_t P, int D, const float *w_gate, const float *task_emb,
                                    int Dg, const float *noise, float tau, int hard, float *g, float *soft, void *stream) {
  int rc = share_shape_ok("m3_share_predict_fwd", dtype, 1, 1, P, D, Dg);
  if (rc) return rc;
  M3_REQUIRE(x && w_gate && g, "m3_share_predict_fwd: null operand");
  M3_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)w_gate % 16) == 0, "m3_share_predict_fwd: x and w_gate must be 16-byte aligned");
  M3_REQUIRE((Dg > 0) == (task_emb != nullptr), "m3_share_predict_fwd: task_emb goes with Dg > 0");
  M3_REQUIRE(tau > 0.f, "m3_share_predict_fwd: tau must be positive");
  M3_REQUIRE(!hard || soft, "m3_share_predict_fwd: hard mode writes the soft probability too");
  ShareFwdDev d;
  memset(&d, 0, sizeof(d));
  d.x.p[0] = (void *)x; d.P = P; d.D = D; d.Dg = Dg; d.w = w_gate; d.emb = task_emb; d.noise = noise;
  d.tau = tau; d.gamma = 0.5f; d.eps = 0.f; d.hard = hard; d.g = g; d.soft = soft;
  return share_fwd_launch("m3_share_predict_fwd", d, dtype, 1, (hipStream_t)stream);
}

extern "C" int m3_share_stage_bwd(const m3_share_rows *x, int dtype, int T, int64_t P, int D, const float *w_gate,
                                  const float *task_emb, int Dg, float tau, float eps, const int64_t *shared_bits,
                                  const float *g, const float *soft, const void *shared_x, const m3_share_rows *dy,
                                  const void *d_shared_x, const float *d_g, const m3_share_rows *dx, float *ws,
                                  float *d_w_gate, float *d_task_emb, void *stream) {
  int rc = share_shape_ok("m3_share_stage_bwd", dtype, T, 2, P, D, Dg);
  if (rc) return rc;
  if ((rc = share_rows_ok("m3_share_stage_bwd(x)", x, T, false))) return rc;
  if ((rc = share_rows_ok("m3_share_stage_bwd(dy)", dy, T, true))) return rc;
  if ((rc = share_rows_ok("m3_share_stage_bwd(dx)", dx, T, false))) return rc;
  M3_REQUIRE(w_gate && shared_bits && g && shared_x && ws && d_w_gate, "m3_share_stage_bwd: null operand");
  M3_REQUIRE(((uintptr_t)w_gate % 16) == 0 && ((uintptr_t)shared_x % 16) == 0 && ((uintptr_t)d_shared_x % 16) == 0,
             "m3_share_stage_bwd: w_gate, shared_x and d_shared_x must be 16-byte aligned");
  M3_REQUIRE((Dg > 0) == (task_emb != nullptr) && (Dg > 0) == (d_task_emb != nullptr),
             "m3_share_stage_bwd: task_emb and d_task_emb go with Dg > 0");
  M3_REQUIRE(tau > 0.f, "m3_share_stage_bwd: tau must be positive");
  ShareBwdDev d;
  d.x = *x; d.dy = *dy; d.dx = *dx; d.P = P; d.D = D; d.Dg = Dg; d.w = w_gate; d.emb = task_emb; d.tau = tau; d.eps = eps;
  d.bits = shared_bits; d.g = g; d.soft = soft; d.sx = shared_x; d.dsx = d_shared_x; d.dg = d_g; d.part = ws;
  return share_bwd_launch("m3_share_stage_bwd", d, dtype, T, d_w_gate, d_task_emb, (hipStream_t)stream);
}

extern "C" int m3_share_predict_bwd(const void *x, int dtype, int64_t P, int D, const float *w_gate, const float *task_emb,
                                    int Dg, float tau, const float *g, const float *soft, const float *d_g, void *dx,
                                    float *ws, float *d_w_gate, float *d_task_emb, void *stream) {
  int rc = share_shape_ok("m3_share_predict_bwd", dtype, 1, 1, P, D, Dg);
  if (rc) return rc;
  M3_REQUIRE(x && w_gate && g && d_g && dx && ws && d_w_gate, "m3_share_predict_bwd: null operand");
  M3_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)dx % 16) == 0 && ((uintptr_t)w_gate % 16) == 0,
             "m3_share_predict_bwd: x, dx and w_gate must be 16-byte aligned");
  M3_REQUIRE((Dg > 0) == (task_emb != nullptr) && (Dg > 0) == (d_task_emb != nullptr),
             "m3_share_predict_bwd: task_emb and d_task_emb go with Dg > 0");
  M3_REQUIRE(tau > 0.f, "m3_share_predict_bwd: tau must be positive");
  ShareBwdDev d;
  memset(&d, 0, sizeof(d));
  d.x.p[0] = (void *)x; d.dx.p[0] = dx; d.P = P; d.D = D; d.Dg = Dg; d.w = w_gate; d.emb = task_emb; d.tau = tau; d.eps = 0.f;
  d.g = g; d.soft = soft; d.dg = d_g; d.part = ws;
  return share_bwd_launch("m3_share_predict_bwd", d, dtype, 1, d_w_gate, d_task_emb, (hipStream_t)stream);
}

static int share_agg_launch(const char *what, bool bwd, const m3_share_rows *x, int dtype, int T, int64_t P, int D,
                            const int64_t *mask_bits, const void *agg_needed, float eps, const m3_share_rows *y, void *agg,
                            void *stream) {
  int rc = share_shape_ok(what, dtype, T, 2, P, D, 0);
  if (rc) return rc;
  if ((rc = share_rows_ok(what, x, T, false))) return rc;
  if ((rc = share_rows_ok(what, y, T, false))) return rc;
  M3_REQUIRE(mask_bits && ((uintptr_t)agg % 16) == 0 && eps >= 0.f, "%s: null mask, unaligned agg or negative eps", what);
  if (P == 0) return M3_OK;
  ShareAggDev d;
  d.x = *x; d.y = *y; d.P = P; d.D = D; d.mask = mask_bits; d.need = (const unsigned char *)agg_needed; d.eps = eps; d.agg = agg;
  const dim3 grid((unsigned)m3_share_num_blocks(P));
  hipStream_t s = (hipStream_t)stream;
  share_instance<2>(dtype, T, D, [&](auto tt, auto nt, auto nch) {
    typedef typename decltype(tt)::type TT;
    constexpr int NT = decltype(nt)::value, NCH = decltype(nch)::value;
    if (bwd) hipLaunchKernelGGL((share_agg_kernel<TT, NT, NCH, true>), grid, dim3(ROW_THREADS), 0, s, d);
    else hipLaunchKernelGGL((share_agg_kernel<TT, NT, NCH, false>), grid, dim3(ROW_THREADS), 0, s, d);
  });
  return check_launch(what);
}

extern "C" int m3_share_aggregate_fwd(const m3_share_rows *x, int dtype, int T, int64_t P, int D, const int64_t *mask_bits,
                                      const void *agg_needed, float eps, const m3_share_rows *y, void *agg, void *stream) {
  return share_agg_launch("m3_share_aggregate_fwd", false, x, dtype, T, P, D, mask_bits, agg_needed, eps, y, agg, stream);
}

extern "C" int m3_share_aggregate_bwd(const m3_share_rows *dy, int dtype, int T, int64_t P, int D, const int64_t *mask_bits,
                                      const void *agg_needed, float eps, const void *d_agg, const m3_share_rows *dx,
                                      void *stream) {
  return share_agg_launch("m3_share_aggregate_bwd", true, dy, dtype, T, P, D, mask_bits, agg_needed, eps, dx, (void *)d_agg, stream);
}

extern "C" int m3_share_compact(const int64_t *shared_bits, const int64_t *prev_shared_bits, int64_t P, int T,
                                int32_t *shared_flat_idx, int32_t *count, int64_t *stats, void *stream) {
  M3_REQUIRE(shared_bits && stats, "m3_share_compact: null operand");
  M3_REQUIRE(P >= 0 && P < ((int64_t)1 << 31), "m3_share_compact: B*N=%lld outside [0, 2^31)", (long long)P);
  if (T < 1 || T > M3_SHARE_MAX_T) {
    set_error("m3_share_compact: T=%d tasks outside [1, %d]", T, M3_SHARE_MAX_T);
    return M3_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL(share_compact_kernel, dim3(1), dim3(SHARE_SCAN), 0, (hipStream_t)stream, shared_bits, prev_shared_bits, P,
                     T, shared_flat_idx, count, stats);
  return check_launch("m3_share_compact");
}
