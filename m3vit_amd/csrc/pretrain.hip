// The recipe around an ImageNet pretraining step for gfx950 (pretrain/train.py, engine/train_one_epoch.py, engine/evaluate.py):
// Mixup / CutMix of the image batch with its batch-reversed self and the dense soft target that goes with it, the soft-target /
// label-smoothing cross-entropy of [B, C] logits (forward pair and one backward launch, record as in loss.hip), the evaluation
// loop's loss / top-1 / top-5 accumulation into a device-resident state, and the weight EMA of every tensor of a descriptor
// table in one launch.  Nothing is read back to the host.  No float atomics: a row is reduced by one workgroup (lanes of a
// wave by shuffles, then the four waves in order), rows are added in row order in double by one workgroup - the same bits from
// run to run.  Tails clamp their offsets and mask the stores.
#include "loss_dev.h"

namespace m3 {

constexpr int PT_THREADS = 256;

// ------------------------------------------------------------------------------------------------------ mix_batch
// one element of sample `self` whose partner is `other`: inside a non-empty box the partner's pixel, outside it the own one
// (both bit copies); with an empty box the Mixup blend - lam 1 and lam 0 are bit copies too (a -0 survives, a partner's Inf
// does not leak through 0 * Inf)
__device__ __forceinline__ float mix_one(float self, float other, float lam, float oml, bool empty, bool inbox) {
  const float blend = lam == 1.f ? self : (lam == 0.f ? other : __builtin_fmaf(oml, other, lam * self));
  return inbox ? other : (empty ? blend : self);
}

struct MixBox { int yl, yh, xl, xh; };

// Workgroups (x, pair): a thread owns the same V elements of BOTH samples of the pair (i, B - 1 - i), loads both, then writes
// both - so the call is valid in place and with per-sample parameters.  V = 4: W % 4 == 0, the four elements share an image row.
// x and out may be the same pointer: no __restrict__.
template <typename TO, int V>
__global__ __launch_bounds__(PT_THREADS) void mix_batch_kernel(const float *x, const float *__restrict__ lam,
                                                               const int32_t *__restrict__ box, int B, int N, int HW, int W,
                                                               TO *out) {
  const int i = blockIdx.y, j = B - 1 - i;
  const float li = lam[i], lj = lam[j], omli = 1.f - li, omlj = 1.f - lj;
  const MixBox bi = {box[4 * i], box[4 * i + 1], box[4 * i + 2], box[4 * i + 3]};
  const MixBox bj = {box[4 * j], box[4 * j + 1], box[4 * j + 2], box[4 * j + 3]};
  const bool ei = bi.yl == bi.yh || bi.xl == bi.xh, ej = bj.yl == bj.yh || bj.xl == bj.xh;
  const float *xi = x + (int64_t)i * N, *xj = x + (int64_t)j * N;
  TO *oi = out + (int64_t)i * N, *oj = out + (int64_t)j * N;
  const int units = N / V;
  for (int u0 = blockIdx.x * PT_THREADS; u0 < units; u0 += gridDim.x * PT_THREADS) {
    const int u = u0 + threadIdx.x;
    const bool on = u < units;
    const int e = (on ? u : units - 1) * V;
    float a[V], b[V], ra[V], rb[V];
    Pack<float, V>::load(xi + e, a);
    Pack<float, V>::load(xj + e, b);
    const int rem = e % HW, y = rem / W, x0 = rem - y * W;
    const bool yi = !ei && y >= bi.yl && y < bi.yh, yj = !ej && y >= bj.yl && y < bj.yh;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int col = x0 + k;
      ra[k] = mix_one(a[k], b[k], li, omli, ei, yi && col >= bi.xl && col < bi.xh);
      rb[k] = mix_one(b[k], a[k], lj, omlj, ej, yj && col >= bj.xl && col < bj.xh);
    }
    if (on) {
      Pack<TO, V>::store(oi + e, ra);
      Pack<TO, V>::store(oj + e, rb);
    }
  }
}

// ----------------------------------------------------------------------------------------------------- mix_target
// t[i, c] = lam_i s(y_i)[c] + (1 - lam_i) s(y_j)[c], j = B - 1 - i; s(y) = off everywhere and on at y.  A label outside [0, C)
// hits no class: the off floor only.  Workgroup 0 also counts those labels (an integer sum, written, not added).
__global__ __launch_bounds__(PT_THREADS) void mix_target_kernel(const int64_t *__restrict__ lab, const float *__restrict__ lam,
                                                                int B, int C, float off, float on, float *__restrict__ tgt,
                                                                int32_t *__restrict__ n_bad) {
  __shared__ float sh[4];
  const int n = B * C;
  for (int e = blockIdx.x * PT_THREADS + threadIdx.x; e < n; e += gridDim.x * PT_THREADS) {
    const int i = e / C, c = e - i * C;
    const float l = lam[i], oml = 1.f - l;
    const float si = lab[i] == (int64_t)c ? on : off, sj = lab[B - 1 - i] == (int64_t)c ? on : off;
    tgt[e] = l == 1.f ? si : __builtin_fmaf(oml, sj, l * si);
  }
  if (blockIdx.x == 0) {
    int bad = 0;
    for (int i = threadIdx.x; i < B; i += PT_THREADS) bad += (lab[i] < 0 || lab[i] >= (int64_t)C) ? 1 : 0;
    bad = block_sum_i(bad, sh);
    if (threadIdx.x == 0) *n_bad = bad;
  }
}

// ------------------------------------------------------------------------------------------- soft-target cross-entropy
// what a workgroup knows of one row of logits after one pass: lse = M + log sum exp(x - M) with a running maximum per thread
// (finite at |x| = 6e4), and two sums of the caller's choice
struct RowStats { float lse, s0, s1; };

// One workgroup per row (a loop over the rows past the grid).  A thread walks units t, t + 256, ... of V elements.  DENSE:
// s0 = sum_c t_c x_c, s1 = sum_c t_c; hard labels: s0 = sum_c x_c.
template <typename T, int V, bool DENSE>
__device__ __forceinline__ RowStats row_pass(const T *__restrict__ xr, const float *__restrict__ tr, int C, float *sh) {
  const int units = C / V;
  float m = -INFINITY, s = 0.f, a0 = 0.f, a1 = 0.f;
  for (int u0 = 0; u0 < units; u0 += PT_THREADS) {
    const int u = u0 + threadIdx.x;
    const bool on = u < units;
    const int e = (on ? u : units - 1) * V;
    float v[V], tv[V];
    Pack<T, V>::load(xr + e, v);
    if (DENSE) Pack<float, V>::load(tr + e, tv);
    if (on) {
      float cm = v[0];
#pragma unroll
      for (int k = 1; k < V; ++k) cm = fmaxf(cm, v[k]);
      const float mn = fmaxf(m, cm);
      float cs = 0.f;
#pragma unroll
      for (int k = 0; k < V; ++k) cs += __expf(v[k] - mn);
      s = __builtin_fmaf(s, __expf(m - mn), cs);                      // the first unit: s = 0, exp(-inf) = 0
      m = mn;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        if (DENSE) { a0 = __builtin_fmaf(tv[k], v[k], a0); a1 += tv[k]; }
        else a0 += v[k];
      }
    }
  }
  const float M = block_max(m, sh);
  s = m == -INFINITY ? 0.f : s * __expf(m - M);                       // a thread without a unit (C < 256 V) adds nothing
  RowStats r;
  r.lse = M + __logf(block_sum(s, sh));
  r.s0 = block_sum(a0, sh);
  r.s1 = DENSE ? block_sum(a1, sh) : 1.f;
  return r;
}

// ws: f32 [B] row losses, then i32 [B] bad-label flags
template <typename T, int V, bool DENSE>
__global__ __launch_bounds__(PT_THREADS) void softce_fwd_kernel(const T *__restrict__ x, const float *__restrict__ tgt,
                                                                const int64_t *__restrict__ lab, float w_on, float w_off, int B,
                                                                int C, float *__restrict__ lse, float *__restrict__ tsum,
                                                                float *__restrict__ ws) {
  __shared__ float sh[4];
  for (int row = blockIdx.x; row < B; row += gridDim.x) {
    const T *xr = x + (int64_t)row * C;
    const RowStats r = row_pass<T, V, DENSE>(xr, DENSE ? tgt + (int64_t)row * C : nullptr, C, sh);
    if (threadIdx.x == 0) {
      float loss;
      int bad = 0;
      if (DENSE) {
        loss = __builtin_fmaf(r.s1, r.lse, -r.s0);                    // S lse - sum t x
        tsum[row] = r.s1;
      } else {
        const int64_t y = lab[row];
        const bool valid = y >= 0 && y < (int64_t)C;
        const float xy = valid ? (float)xr[valid ? y : 0] : 0.f;
        loss = __builtin_fmaf(-w_off, r.s0, __builtin_fmaf(-w_on, xy, r.lse));     // lse - (1 - s) x[y] - (s / C) sum x
        bad = valid ? 0 : 1;
      }
      lse[row] = r.lse;
      ws[row] = loss;
      ((int32_t *)ws)[B + row] = bad;
    }
  }
}

// one workgroup: the B row losses and bad-label flags in row order (reduce_partials, reduce_dev.h)
__global__ __launch_bounds__(256) void softce_finalize_kernel(const float *__restrict__ ws, int B, int32_t *__restrict__ rec) {
  const Totals<1, 1> tot = reduce_partials<1, 1>(ws, B, B);
  if (threadIdx.x != 0) return;
  write_loss_record(rec, (float)(tot.s[0] / (double)B), (float)(1.0 / (double)B), 0.f, B, 0, (int)tot.c[0]);
}

// d x = (softmax(x) S - t) * coef * upstream over the flat [B * C] span, V elements of one row per access (V divides C)
template <typename T, int V, bool DENSE>
__global__ __launch_bounds__(PT_THREADS) void softce_bwd_kernel(const T *__restrict__ x, const float *__restrict__ tgt,
                                                                const int64_t *__restrict__ lab, float w_on, float w_off,
                                                                const float *__restrict__ lse, const float *__restrict__ tsum,
                                                                const float *__restrict__ rec, const float *__restrict__ gout,
                                                                int C, int units, T *__restrict__ dx) {
  const float kf = rec[M3_LOSS_REC_COEF] * *gout;
  for (int u0 = blockIdx.x * PT_THREADS; u0 < units; u0 += gridDim.x * PT_THREADS) {
    const int u = u0 + threadIdx.x;
    const bool on = u < units;
    const uint32_t e = (uint32_t)(on ? u : units - 1) * V, row = e / (uint32_t)C;
    const int c0 = (int)(e - row * (uint32_t)C);
    float v[V], tv[V], d[V];
    Pack<T, V>::load(x + e, v);
    const float ls = lse[row];
    float S = 1.f;
    if (DENSE) {
      Pack<float, V>::load(tgt + e, tv);
      S = tsum[row];
    } else {
      const int64_t y = lab[row];
#pragma unroll
      for (int k = 0; k < V; ++k) tv[k] = w_off + (y == (int64_t)(c0 + k) ? w_on : 0.f);     // a bad label matches no class
    }
#pragma unroll
    for (int k = 0; k < V; ++k) d[k] = __builtin_fmaf(__expf(v[k] - ls), S, -tv[k]) * kf;
    if (on) Pack<T, V>::store(dx + e, d);
  }
}

// ------------------------------------------------------------------------------------------------ distillation loss
// pretrain/models/losses.py:50-68 on the student's distillation logits x and the teacher's logits t, each in a dtype of its
// own.  SOFT: tau^2 / (B C) sum_i [ sum_c q_ic (t_ic - x_ic) / tau - lse(t_i / tau) + lse(x_i / tau) ], q = softmax(t / tau)
// (kl_div(log p, log q, sum, log_target) tau^2 / numel with sum_c q = 1); hard: (1 / B) sum_i [ lse(x_i) - x_i[y_i] ], y_i the
// teacher's argmax, ties to the lowest index.  One workgroup per row; the forward leaves per row the student lse and, in aux,
// the teacher lse (f32) or the argmax (i32), which is all the backward needs of the teacher's side.

// lse of sc * x over one row with a running maximum per thread (row_pass's arithmetic; sc = 1 multiplies exactly)
template <typename T, int V>
__device__ __forceinline__ float row_lse_scaled(const T *__restrict__ xr, int C, float sc, float *sh) {
  const int units = C / V;
  float m = -INFINITY, s = 0.f;
  for (int u0 = 0; u0 < units; u0 += PT_THREADS) {
    const int u = u0 + threadIdx.x;
    const bool on = u < units;
    const int e = (on ? u : units - 1) * V;
    float v[V];
    Pack<T, V>::load(xr + e, v);
    if (on) {
#pragma unroll
      for (int k = 0; k < V; ++k) v[k] *= sc;
      float cm = v[0];
#pragma unroll
      for (int k = 1; k < V; ++k) cm = fmaxf(cm, v[k]);
      const float mn = fmaxf(m, cm);
      float cs = 0.f;
#pragma unroll
      for (int k = 0; k < V; ++k) cs += __expf(v[k] - mn);
      s = __builtin_fmaf(s, __expf(m - mn), cs);
      m = mn;
    }
  }
  const float M = block_max(m, sh);
  s = m == -INFINITY ? 0.f : s * __expf(m - M);
  return M + __logf(block_sum(s, sh));
}

// the larger value wins, of equal values the lower index (m3_cls_eval_update's rule)
__device__ __forceinline__ void argmax_take(float &bv, int &bi, float ov, int oi) {
  if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
}

// argmax over one row; every thread returns the same index in [0, C)
template <typename T, int V>
__device__ __forceinline__ int row_argmax(const T *__restrict__ tr, int C, float *sh, int *shi) {
  const int units = C / V;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int u0 = 0; u0 < units; u0 += PT_THREADS) {
    const int u = u0 + threadIdx.x;
    const bool on = u < units;
    const int e = (on ? u : units - 1) * V;
    float v[V];
    Pack<T, V>::load(tr + e, v);
    if (on) {
#pragma unroll
      for (int k = 0; k < V; ++k) argmax_take(bv, bi, v[k], e + k);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    argmax_take(bv, bi, ov, oi);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = bv; shi[threadIdx.x >> 6] = bi; }
  __syncthreads();
  bv = sh[0]; bi = shi[0];
#pragma unroll
  for (int j = 1; j < 4; ++j) argmax_take(bv, bi, sh[j], shi[j]);
  return bi < C ? bi : 0;                                              // (a row without a finite maximum: not the contract)
}

// ws: f32 [B] row terms
template <typename TX, typename TT, int V, bool SOFT>
__global__ __launch_bounds__(PT_THREADS) void distill_fwd_kernel(const TX *__restrict__ x, const TT *__restrict__ t, float inv_tau,
                                                                 int B, int C, float *__restrict__ lse, void *__restrict__ aux,
                                                                 float *__restrict__ ws) {
  __shared__ float sh[4];
  __shared__ int shi[4];
  for (int row = blockIdx.x; row < B; row += gridDim.x) {
    const TX *xr = x + (int64_t)row * C;
    const TT *tr = t + (int64_t)row * C;
    const float lx = row_lse_scaled<TX, V>(xr, C, SOFT ? inv_tau : 1.f, sh);
    if (SOFT) {
      const float lt = row_lse_scaled<TT, V>(tr, C, inv_tau, sh);
      const int units = C / V;
      float a = 0.f;
      for (int u0 = 0; u0 < units; u0 += PT_THREADS) {                  // the row again (it is in the cache): sum q (t - x) / tau
        const int u = u0 + threadIdx.x;
        const bool on = u < units;
        const int e = (on ? u : units - 1) * V;
        float xv[V], tv[V];
        Pack<TX, V>::load(xr + e, xv);
        Pack<TT, V>::load(tr + e, tv);
        if (on) {
#pragma unroll
          for (int k = 0; k < V; ++k) {
            const float ts = tv[k] * inv_tau, xs = xv[k] * inv_tau;
            a = __builtin_fmaf(__expf(ts - lt), ts - xs, a);
          }
        }
      }
      const float dot = block_sum(a, sh);
      if (threadIdx.x == 0) {
        lse[row] = lx;
        ((float *)aux)[row] = lt;
        ws[row] = dot + (lx - lt);
      }
    } else {
      const int y = row_argmax<TT, V>(tr, C, sh, shi);
      if (threadIdx.x == 0) {
        lse[row] = lx;
        ((int32_t *)aux)[row] = y;
        ws[row] = lx - (float)xr[y];
      }
    }
  }
}

// one workgroup: the B row terms in row order in double (as softce_finalize_kernel); value = sum * num / den
__global__ __launch_bounds__(256) void distill_finalize_kernel(const float *__restrict__ ws, int B, double num, double den,
                                                               float coef, int32_t *__restrict__ rec) {
  const Totals<1, 0> tot = reduce_partials<1, 0>(ws, B, B);
  if (threadIdx.x != 0) return;
  write_loss_record(rec, (float)(tot.s[0] * num / den), coef, 0.f, B, 0, 0);
}

// d x over the flat [B * C] span, V elements of one row per access.  SOFT: (exp(x / tau - lse_x) - exp(t / tau - lse_t)) coef
// upstream; hard: (exp(x - lse_x) - [c == y]) coef upstream (t is not read)
template <typename TX, typename TT, int V, bool SOFT>
__global__ __launch_bounds__(PT_THREADS) void distill_bwd_kernel(const TX *__restrict__ x, const TT *__restrict__ t, float inv_tau,
                                                                 const float *__restrict__ lse, const void *__restrict__ aux,
                                                                 const float *__restrict__ rec, const float *__restrict__ gout,
                                                                 int C, int units, TX *__restrict__ dx) {
  const float kf = rec[M3_LOSS_REC_COEF] * *gout;
  for (int u0 = blockIdx.x * PT_THREADS; u0 < units; u0 += gridDim.x * PT_THREADS) {
    const int u = u0 + threadIdx.x;
    const bool on = u < units;
    const uint32_t e = (uint32_t)(on ? u : units - 1) * V, row = e / (uint32_t)C;
    const int c0 = (int)(e - row * (uint32_t)C);
    float xv[V], d[V];
    Pack<TX, V>::load(x + e, xv);
    const float lx = lse[row];
    if (SOFT) {
      float tv[V];
      Pack<TT, V>::load(t + e, tv);
      const float lt = ((const float *)aux)[row];
#pragma unroll
      for (int k = 0; k < V; ++k) d[k] = (__expf(xv[k] * inv_tau - lx) - __expf(tv[k] * inv_tau - lt)) * kf;
    } else {
      const int y = ((const int32_t *)aux)[row];
#pragma unroll
      for (int k = 0; k < V; ++k) d[k] = (__expf(xv[k] - lx) - (c0 + k == y ? 1.f : 0.f)) * kf;
    }
    if (on) Pack<TX, V>::store(dx + e, d);
  }
}

// ------------------------------------------------------------------------------------------------ evaluation update
// Per row: plain cross-entropy lse - x[y], and the rank of the target logit = #{c : x_c beats x_y}: a larger value beats, an
// equal value at a lower index beats, a NaN beats every number and an earlier NaN beats a later one (meter.hip's argmax rule).
// ws: f32 [B] row losses, then i32 [B] top-1 hits, [B] top-5 hits, [B] bad labels.
template <typename T>
__global__ __launch_bounds__(PT_THREADS) void cls_eval_rows_kernel(const T *__restrict__ x, const int64_t *__restrict__ lab,
                                                                   int B, int C, float *__restrict__ ws) {
  __shared__ float sh[4];
  for (int row = blockIdx.x; row < B; row += gridDim.x) {
    const T *xr = x + (int64_t)row * C;
    const int64_t y64 = lab[row];
    const bool valid = y64 >= 0 && y64 < (int64_t)C;
    const int y = valid ? (int)y64 : 0;
    const float xy = (float)xr[y];
    const bool ynan = xy != xy;
    int beat = 0;
    for (int c = threadIdx.x; c < C; c += PT_THREADS) {
      const float xc = (float)xr[c];
      const bool b = xc != xc ? (!ynan || c < y) : (!ynan && (xc > xy || (xc == xy && c < y)));
      beat += b ? 1 : 0;
    }
    const RowStats r = row_pass<T, 1, false>(xr, nullptr, C, sh);
    const int rank = block_sum_i(beat, sh);
    if (threadIdx.x == 0) {
      int32_t *wi = (int32_t *)ws;
      ws[row] = valid ? r.lse - xy : r.lse;
      wi[B + row] = (valid && rank < 1) ? 1 : 0;
      wi[2 * B + row] = (valid && rank < (C < 5 ? C : 5)) ? 1 : 0;
      wi[3 * B + row] = valid ? 0 : 1;
    }
  }
}

// one workgroup ADDS the batch to state: f64 loss_sum, correct1, correct5, count, then i64 n_bad; rows in row order
__global__ __launch_bounds__(256) void cls_eval_finalize_kernel(const float *__restrict__ ws, int B, double *__restrict__ state) {
  const Totals<1, 3> tot = reduce_partials<1, 3>(ws, B, B);            // counts: top-1 hits, top-5 hits, bad labels
  if (threadIdx.x != 0) return;
  state[M3_CLS_EVAL_LOSS_SUM] += tot.s[0];
  state[M3_CLS_EVAL_CORRECT1] += (double)tot.c[0];
  state[M3_CLS_EVAL_CORRECT5] += (double)tot.c[1];
  state[M3_CLS_EVAL_COUNT] += (double)B;
  ((int64_t *)state)[M3_CLS_EVAL_N_BAD] += tot.c[2];
}

// -------------------------------------------------------------------------------------------------------------- EMA
// ema = d ema + (1 - d) p over every tensor of an m3_optim_desc table (p: the shadow, g: the source; m, v, group unused): one
// workgroup per M3_OPTIM_CHUNK elements of one tensor, found by a binary search over chunk_start, four 16-byte pieces per
// thread and stream all loaded before the first use (as m3_optim_step).  d = 0 copies the source's bits.
constexpr int EMA_PIECES = 4;

__device__ __forceinline__ float ema_one(float e, float p, float d, float omd) {
  return d == 0.f ? p : __builtin_fmaf(d, e, omd * p);
}

__global__ __launch_bounds__(256) void ema_kernel(const m3_optim_desc *__restrict__ descs, int n_desc, float d, float omd) {
  const int b = blockIdx.x, t = threadIdx.x;
  int lo = 0, hi = n_desc - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].chunk_start <= b) lo = mid; else hi = mid - 1;
  }
  const m3_optim_desc ds = descs[lo];
  const int64_t base = (int64_t)(b - ds.chunk_start) * M3_OPTIM_CHUNK;
  const int64_t n4 = ds.n & ~(int64_t)3;
  if (ds.vec_ok && n4 > base) {
    const int64_t left = n4 - base;                                   // whole float4s of this chunk hold elements [0, left)
    const int valid = (int)(left < M3_OPTIM_CHUNK ? left : M3_OPTIM_CHUNK);
    float *pe = ds.p + base;
    const float *pp = ds.g + base;
    f32x4 E[EMA_PIECES], P[EMA_PIECES];
    int off[EMA_PIECES];
#pragma unroll
    for (int k = 0; k < EMA_PIECES; ++k) {
      const int e = (k * 256 + t) * 4;
      off[k] = e < valid ? e : valid - 4;                             // clamped, never predicated: all loads issue at once
    }
#pragma unroll
    for (int k = 0; k < EMA_PIECES; ++k) P[k] = *(const f32x4 *)(pp + off[k]);
#pragma unroll
    for (int k = 0; k < EMA_PIECES; ++k) E[k] = *(const f32x4 *)(pe + off[k]);
#pragma unroll
    for (int k = 0; k < EMA_PIECES; ++k) {
      f32x4 r;
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = ema_one(E[k][j], P[k][j], d, omd);
      if ((k * 256 + t) * 4 < valid) *(f32x4 *)(pe + off[k]) = r;
    }
    const int64_t i = n4 + t;                                         // the up to 3 elements behind the last whole float4
    if (base + M3_OPTIM_CHUNK >= ds.n && i < ds.n) ds.p[i] = ema_one(ds.p[i], ds.g[i], d, omd);
  } else {
#pragma unroll 4
    for (int k = 0; k < EMA_PIECES * 4; ++k) {
      const int64_t i = base + k * 256 + t;
      if (i < ds.n) ds.p[i] = ema_one(ds.p[i], ds.g[i], d, omd);
    }
  }
}

static int softce_args_ok(const void *logits, int dtype, const float *target, const int64_t *label, double smoothing, int B,
                          int C, const char *who) {
  M3_REQUIRE(B >= 1 && C >= 1 && C <= M3_SOFTCE_MAX_C, "%s: B = %d, C = %d: B >= 1 and 1 <= C <= %d", who, B, C, M3_SOFTCE_MAX_C);
  M3_REQUIRE(dtype_ok(dtype), "%s: bad dtype code %d", who, dtype);
  M3_REQUIRE((int64_t)B * C < ((int64_t)1 << 31) - ((int64_t)1 << 20), "%s: %lld elements: the kernels index with 32 bits", who,
             (long long)B * C);
  M3_REQUIRE(logits && ((target != nullptr) != (label != nullptr)), "%s: logits and exactly one of target / label", who);
  M3_REQUIRE(smoothing >= 0.0 && smoothing <= 1.0, "%s: smoothing %g outside [0, 1]", who, smoothing);
  return 0;
}

// f(IntTag<V>{}, IntTag<DENSE>{})
template <typename F> static inline void by_vec_form(bool vec, bool dense, F &&f) {
  if (vec) { if (dense) f(IntTag<4>{}, IntTag<1>{}); else f(IntTag<4>{}, IntTag<0>{}); }
  else { if (dense) f(IntTag<1>{}, IntTag<1>{}); else f(IntTag<1>{}, IntTag<0>{}); }
}

static int distill_args_ok(const void *x, int x_dtype, int t_dtype, int kind, double tau, int B, int C, const char *who) {
  M3_REQUIRE(B >= 1 && C >= 1 && C <= M3_SOFTCE_MAX_C, "%s: B = %d, C = %d: B >= 1 and 1 <= C <= %d", who, B, C, M3_SOFTCE_MAX_C);
  M3_REQUIRE(dtype_ok(x_dtype) && dtype_ok(t_dtype), "%s: bad dtype code %d / %d", who, x_dtype, t_dtype);
  M3_REQUIRE((int64_t)B * C < ((int64_t)1 << 31) - ((int64_t)1 << 20), "%s: %lld elements: the kernels index with 32 bits", who,
             (long long)B * C);
  M3_REQUIRE(kind == M3_DISTILL_SOFT || kind == M3_DISTILL_HARD, "%s: bad kind %d", who, kind);
  M3_REQUIRE(kind == M3_DISTILL_HARD || (tau > 0.0 && tau <= 3.0e38), "%s: tau %g must be positive and finite", who, tau);
  M3_REQUIRE(x != nullptr, "%s: null logits", who);
  return 0;
}

// f(DtypeTag<TX>{}, DtypeTag<TT>{}, IntTag<V>{}): V = 1, or the 16-byte width of the pair - 4 elements when both are fp32, 8 as
// soon as one of them has 16 bits (C % V == 0 keeps every row of either on a 16-byte boundary)
template <typename F> static inline void by_distill_form(int x_dtype, int t_dtype, bool vec, F &&f) {
  by_dtype(x_dtype, [&](auto tx) {
    by_dtype(t_dtype, [&](auto tt) {
      constexpr int W = (sizeof(typename decltype(tx)::type) == 4 && sizeof(typename decltype(tt)::type) == 4) ? 4 : 8;
      if (vec) f(tx, tt, IntTag<W>{}); else f(tx, tt, IntTag<1>{});
    });
  });
}
static inline int distill_width(int x_dtype, int t_dtype) { return (x_dtype == M3_F32 && t_dtype == M3_F32) ? 4 : 8; }

}  // namespace m3

using namespace m3;

extern "C" int m3_mix_batch(const float *x, int B, int C, int H, int W, const float *lam, const int32_t *box, void *out,
                            int out_dtype, void *stream) {
  M3_REQUIRE(B >= 2 && B % 2 == 0 && B / 2 <= 65535, "m3_mix_batch: B = %d must be even, in [2, 131070]", B);
  M3_REQUIRE(C >= 1 && H >= 1 && W >= 1, "m3_mix_batch: C, H, W must be positive (got %d, %d, %d)", C, H, W);
  const int64_t N = (int64_t)C * H * W;
  M3_REQUIRE(N < ((int64_t)1 << 31) - ((int64_t)1 << 20), "m3_mix_batch: %lld elements per sample: the kernel indexes with 32 bits", (long long)N);
  M3_REQUIRE(dtype_ok(out_dtype), "m3_mix_batch: bad dtype code %d", out_dtype);
  M3_REQUIRE(x && lam && box && out, "m3_mix_batch: null pointer");
  M3_REQUIRE(out_dtype == M3_F32 || out != (const void *)x, "m3_mix_batch: in place only with an fp32 output");
  const bool vec = aligned16(x) && aligned16(out) && W % 4 == 0;
  const int units = (int)(vec ? N / 4 : N);
  const dim3 grid(blocks_for(units, PT_THREADS), B / 2);
  by_dtype(out_dtype, [&](auto tt) {
    typedef typename decltype(tt)::type TO;
    auto go = [&](auto v) {
      hipLaunchKernelGGL((mix_batch_kernel<TO, decltype(v)::value>), grid, dim3(PT_THREADS), 0, (hipStream_t)stream, x, lam, box,
                         B, (int)N, H * W, W, (TO *)out);
    };
    if (vec) go(IntTag<4>{}); else go(IntTag<1>{});
  });
  return check_launch("m3_mix_batch");
}

extern "C" int m3_mix_target(const int64_t *label, const float *lam, int B, int C, double smoothing, float *target,
                             int32_t *n_bad, void *stream) {
  M3_REQUIRE(B >= 2 && B % 2 == 0, "m3_mix_target: B = %d must be even and positive", B);
  M3_REQUIRE(C >= 1 && (int64_t)B * C < ((int64_t)1 << 31) - ((int64_t)1 << 20), "m3_mix_target: bad C = %d (B = %d)", C, B);
  M3_REQUIRE(smoothing >= 0.0 && smoothing <= 1.0, "m3_mix_target: smoothing %g outside [0, 1]", smoothing);
  M3_REQUIRE(label && lam && target && n_bad, "m3_mix_target: null pointer");
  const double off = smoothing / (double)C, on = 1.0 - smoothing + off;
  hipLaunchKernelGGL(mix_target_kernel, dim3(blocks_for((int64_t)B * C, PT_THREADS)), dim3(PT_THREADS), 0, (hipStream_t)stream,
                     label, lam, B, C, (float)off, (float)on, target, n_bad);
  return check_launch("m3_mix_target");
}

extern "C" int64_t m3_softce_ws_elems(int B) { return B < 1 ? 0 : 2 * (int64_t)B; }

extern "C" int m3_loss_softce_fwd(const void *logits, int dtype, const float *target, const int64_t *label, double smoothing,
                                  int B, int C, float *lse, float *tsum, float *ws, void *record, void *stream) {
  if (int rc = softce_args_ok(logits, dtype, target, label, smoothing, B, C, "m3_loss_softce_fwd")) return rc;
  M3_REQUIRE(lse && ws && record && (tsum || !target), "m3_loss_softce_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const bool dense = target != nullptr;
  const bool vec = C % 4 == 0 && aligned16(logits) && (!dense || aligned16(target));
  const float w_on = (float)(1.0 - smoothing), w_off = (float)(smoothing / (double)C);
  const int nblk = B < LS_MAX_BLOCKS ? B : LS_MAX_BLOCKS;
  by_dtype(dtype, [&](auto tt) {
    typedef typename decltype(tt)::type T;
    by_vec_form(vec, dense, [&](auto v, auto f) {
      hipLaunchKernelGGL((softce_fwd_kernel<T, decltype(v)::value, decltype(f)::value != 0>), dim3(nblk), dim3(PT_THREADS), 0, s,
                         (const T *)logits, target, label, w_on, w_off, B, C, lse, tsum, ws);
    });
  });
  if (int rc = check_launch("m3_loss_softce_fwd (rows)")) return rc;
  hipLaunchKernelGGL(softce_finalize_kernel, dim3(1), dim3(256), 0, s, ws, B, (int32_t *)record);
  return check_launch("m3_loss_softce_fwd (finalize)");
}

extern "C" int m3_loss_softce_bwd(const void *logits, int dtype, const float *target, const int64_t *label, double smoothing,
                                  const float *lse, const float *tsum, const void *record, const float *grad_out, int B, int C,
                                  void *dlogits, void *stream) {
  if (int rc = softce_args_ok(logits, dtype, target, label, smoothing, B, C, "m3_loss_softce_bwd")) return rc;
  M3_REQUIRE(lse && record && grad_out && dlogits && (tsum || !target), "m3_loss_softce_bwd: null pointer");
  const bool dense = target != nullptr;
  const bool vec = C % 4 == 0 && aligned16(logits) && aligned16(dlogits) && (!dense || aligned16(target));
  const float w_on = (float)(1.0 - smoothing), w_off = (float)(smoothing / (double)C);
  const int units = (int)((int64_t)B * C / (vec ? 4 : 1));
  const int nblk = blocks_for(units, PT_THREADS);
  by_dtype(dtype, [&](auto tt) {
    typedef typename decltype(tt)::type T;
    by_vec_form(vec, dense, [&](auto v, auto f) {
      hipLaunchKernelGGL((softce_bwd_kernel<T, decltype(v)::value, decltype(f)::value != 0>), dim3(nblk), dim3(PT_THREADS), 0,
                         (hipStream_t)stream, (const T *)logits, target, label, w_on, w_off, lse, tsum, (const float *)record,
                         grad_out, C, units, (T *)dlogits);
    });
  });
  return check_launch("m3_loss_softce_bwd");
}

extern "C" int64_t m3_distill_ws_elems(int B) { return B < 1 ? 0 : (int64_t)B; }

extern "C" int m3_loss_distill_fwd(const void *logits, int dtype, const void *teacher, int teacher_dtype, int kind, double tau,
                                   int B, int C, float *lse, void *aux, float *ws, void *record, void *stream) {
  if (int rc = distill_args_ok(logits, dtype, teacher_dtype, kind, tau, B, C, "m3_loss_distill_fwd")) return rc;
  M3_REQUIRE(teacher && lse && aux && ws && record, "m3_loss_distill_fwd: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const bool soft = kind == M3_DISTILL_SOFT;
  const bool vec = C % distill_width(dtype, teacher_dtype) == 0 && aligned16(logits) && aligned16(teacher);
  const float inv_tau = soft ? (float)(1.0 / tau) : 1.f;
  const int nblk = B < LS_MAX_BLOCKS ? B : LS_MAX_BLOCKS;
  by_distill_form(dtype, teacher_dtype, vec, [&](auto tx, auto tt, auto v) {
    typedef typename decltype(tx)::type TX;
    typedef typename decltype(tt)::type TT;
    auto go = [&](auto f) {
      hipLaunchKernelGGL((distill_fwd_kernel<TX, TT, decltype(v)::value, decltype(f)::value != 0>), dim3(nblk), dim3(PT_THREADS), 0,
                         s, (const TX *)logits, (const TT *)teacher, inv_tau, B, C, lse, aux, ws);
    };
    if (soft) go(IntTag<1>{}); else go(IntTag<0>{});
  });
  if (int rc = check_launch("m3_loss_distill_fwd (rows)")) return rc;
  const double den = soft ? (double)B * (double)C : (double)B;
  hipLaunchKernelGGL(distill_finalize_kernel, dim3(1), dim3(256), 0, s, ws, B, soft ? tau * tau : 1.0, den,
                     (float)((soft ? tau : 1.0) / den), (int32_t *)record);
  return check_launch("m3_loss_distill_fwd (finalize)");
}

extern "C" int m3_loss_distill_bwd(const void *logits, int dtype, const void *teacher, int teacher_dtype, int kind, double tau,
                                   const float *lse, const void *aux, const void *record, const float *grad_out, int B, int C,
                                   void *dlogits, void *stream) {
  if (int rc = distill_args_ok(logits, dtype, teacher_dtype, kind, tau, B, C, "m3_loss_distill_bwd")) return rc;
  const bool soft = kind == M3_DISTILL_SOFT;
  M3_REQUIRE(lse && aux && record && grad_out && dlogits && (teacher || !soft), "m3_loss_distill_bwd: null pointer");
  if (!soft) teacher_dtype = dtype;                                     // the teacher's logits are not read: one instance per TX
  const int W = distill_width(dtype, teacher_dtype);
  const bool vec = C % W == 0 && aligned16(logits) && aligned16(dlogits) && (!soft || aligned16(teacher));
  const float inv_tau = soft ? (float)(1.0 / tau) : 1.f;
  const int units = (int)((int64_t)B * C / (vec ? W : 1));
  const int nblk = blocks_for(units, PT_THREADS);
  by_distill_form(dtype, teacher_dtype, vec, [&](auto tx, auto tt, auto v) {
    typedef typename decltype(tx)::type TX;
    typedef typename decltype(tt)::type TT;
    auto go = [&](auto f) {
      hipLaunchKernelGGL((distill_bwd_kernel<TX, TT, decltype(v)::value, decltype(f)::value != 0>), dim3(nblk), dim3(PT_THREADS), 0,
                         (hipStream_t)stream, (const TX *)logits, (const TT *)teacher, inv_tau, lse, aux, (const float *)record,
                         grad_out, C, units, (TX *)dlogits);
    };
    if (soft) go(IntTag<1>{}); else go(IntTag<0>{});
  });
  return check_launch("m3_loss_distill_bwd");
}

extern "C" int64_t m3_cls_eval_ws_elems(int B) { return B < 1 ? 0 : 4 * (int64_t)B; }

extern "C" int m3_cls_eval_update(const void *logits, int dtype, const int64_t *label, int B, int C, void *ws, void *state,
                                  void *stream) {
  if (int rc = softce_args_ok(logits, dtype, nullptr, label, 0.0, B, C, "m3_cls_eval_update")) return rc;
  M3_REQUIRE(ws && state, "m3_cls_eval_update: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int nblk = B < LS_MAX_BLOCKS ? B : LS_MAX_BLOCKS;
  by_dtype(dtype, [&](auto tt) {
    typedef typename decltype(tt)::type T;
    hipLaunchKernelGGL(cls_eval_rows_kernel<T>, dim3(nblk), dim3(PT_THREADS), 0, s, (const T *)logits, label, B, C, (float *)ws);
  });
  if (int rc = check_launch("m3_cls_eval_update (rows)")) return rc;
  hipLaunchKernelGGL(cls_eval_finalize_kernel, dim3(1), dim3(256), 0, s, (const float *)ws, B, (double *)state);
  return check_launch("m3_cls_eval_update (finalize)");
}

extern "C" int m3_ema_update(const m3_optim_desc *descs_dev, int n_desc, int total_chunks, float decay, float one_minus_decay,
                             void *stream) {
  M3_REQUIRE(descs_dev && n_desc >= 1 && total_chunks >= 1, "m3_ema_update: bad args");
  M3_REQUIRE(decay >= 0.f && decay <= 1.f && one_minus_decay >= 0.f && one_minus_decay <= 1.f,
             "m3_ema_update: decay %g / 1 - decay %g outside [0, 1]", (double)decay, (double)one_minus_decay);
  if (decay == 1.f) return 0;                      // ema = 1 * ema + 0 * p: nothing to write, the shadow keeps its bits
  hipLaunchKernelGGL(ema_kernel, dim3(total_chunks), dim3(256), 0, (hipStream_t)stream, descs_dev, n_desc, decay, one_minus_decay);
  return check_launch("m3_ema_update");
}
