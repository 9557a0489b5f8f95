// The criterion of a dense-prediction training step for gfx950: pixel-wise softmax cross-entropy, masked L1, the normalised
// normals loss and the balanced binary cross-entropy (the four losses losses/loss_functions.py hands to get_loss), each as a
// forward pair and one backward launch.  Forward, launch one: one pass over pred and label leaves four partials per workgroup
// (two fp32 sums, two integer counts) in the caller's workspace - no atomics.  Forward, launch two: one workgroup adds the
// partials in block order in double and writes the device-resident record (loss, counts, the backward's coefficients, the
// bad-label count).  Backward: one pass over pred, label, the record and the upstream gradient - read through a device
// pointer - writes d pred in pred's dtype and layout.  Nothing is read back to the host; every sum has a fixed order, so two
// runs on the same inputs give the same bits.  Every load of a thread's pieces is issued before the first use; tails clamp
// their offsets and mask the stores ("Predicated loads are basic blocks too").
//
// Layouts: NCHW-contiguous (lanes run along the pixels of a plane, a loop over C) and channels-last (a pixel's C values are
// contiguous: a group of G = 2^k lanes reads one pixel as one span, 64 / G pixels of a wave are one contiguous span, and the
// group reduces with shuffles).  V = 4 elements per access where the host found 16-byte alignment and whole vectors, else V = 1.
#include "loss_dev.h"

namespace m3 {

constexpr int LS_NP = 4;                            // partial rows: sum0, sum1, count0, count1 - each [nblk]
constexpr int LS_CCHUNK = 8;                        // channels of a planar pixel in flight together

enum { K_CE = 0, K_L1 = 1, K_NORMALS = 2, K_BCE = 3 };

// the class of pixel i as the reference's `label[:, 0].long()` sees it (truncation), or -1 for a value that is no class
// index at all.  Returns [0, 255] or -1: 255 is "ignore", [0, C) a class, everything else a bad label.  L, the label dtype, is
// a template constant of every cross-entropy kernel: a run-time switch would put each label load into a basic block of its own,
// with a wait for ALL outstanding loads behind it ("Predicated loads are basic blocks too").
template <int L>
__device__ __forceinline__ int class_label(const void *__restrict__ lab, int i) {
  if constexpr (L == M3_LABEL_I64) {
    const int64_t v = ((const int64_t *)lab)[i];
    return (v >= 0 && v < 256) ? (int)v : -1;
  } else if constexpr (L == M3_LABEL_U8) {
    return (int)((const uint8_t *)lab)[i];
  } else {
    const float f = ((const float *)lab)[i];
    return (f > -1.f && f < 256.f) ? (int)f : -1;
  }
}

// -------------------------------------------------------------------------------------------------------- finalize
__global__ __launch_bounds__(256) void loss_finalize_kernel(const float *__restrict__ ws, int nblk, int kind, double numel,
                                                            int has_pw, double pos_weight, int32_t *__restrict__ rec) {
  const Totals<2, 2> tot = reduce_partials<2, 2>(ws, nblk, nblk);
  if (threadIdx.x != 0) return;
  const double s0 = tot.s[0], s1 = tot.s[1];
  const long long c0 = tot.c[0], c1 = tot.c[1];
  float loss, coef, coef2 = 0.f;
  int n0 = (int)c0, n1 = 0, bad = 0;
  if (kind == K_CE || kind == K_L1) {                // mean over the valid: 0 / 0 = NaN as the reference, and a zero gradient
    loss = (float)(s0 / (double)c0);
    coef = c0 > 0 ? (float)(1.0 / (double)c0) : 0.f;
    bad = (int)c1;
  } else if (kind == K_NORMALS) {                    // sum / max(n_valid, 1e-6): 0 when nothing is valid
    const double d = c0 > 0 ? (double)c0 : 1e-6;
    loss = (float)(s0 / d);
    coef = (float)(1.0 / d);
  } else {                                           // balanced BCE: c0 = n_pos, the rest of numel is negative
    const double n_pos = (double)c0, n_neg = numel - n_pos;
    // the reference forms w from `labels.float()` sums: an fp32 quotient (exact counts below 2^24), then used as a double
    const double w = has_pw ? pos_weight : (double)((float)n_neg / (float)(n_pos + n_neg));
    loss = (float)((w * s0 + (1.0 - w) * s1) / numel);
    coef = (float)(w / numel);
    coef2 = (float)((1.0 - w) / numel);
    n1 = (int)n_neg;
  }
  write_loss_record(rec, loss, coef, coef2, n0, n1, bad);
}

// ------------------------------------------------------------------------------------------ cross-entropy, planar
// A thread owns V consecutive pixels of one plane and walks the C planes LS_CCHUNK at a time with a running maximum: the
// chunk's loads are issued together, then m and s = sum exp(x - m) are updated once per chunk (one rescale per 8 channels).
// units = B * HW / V; upp = HW / V units per image.
template <typename T, int V, int L>
__global__ __launch_bounds__(LS_THREADS) void ce_fwd_planar_kernel(const T *__restrict__ x, const void *__restrict__ lab,
                                                                   int C, int HW, int units, float *__restrict__ lse,
                                                                   float *__restrict__ ws) {
  const int upp = HW / V;
  float acc = 0.f;
  int nv = 0, nb = 0;
  for (int u0 = blockIdx.x * LS_THREADS; u0 < units; u0 += gridDim.x * LS_THREADS) {
    const int u = u0 + threadIdx.x;
    const bool on = u < units;
    const int uc = on ? u : units - 1;
    const int b = uc / upp, r = uc - b * upp;
    const int pix = b * HW + r * V;
    const T *px = x + (int64_t)b * C * HW + r * V;
    int li[V];
#pragma unroll
    for (int j = 0; j < V; ++j) li[j] = class_label<L>(lab, pix + j);
    float m[V], s[V], xl[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { m[j] = -INFINITY; s[j] = 0.f; xl[j] = 0.f; }
    for (int c0 = 0; c0 < C; c0 += LS_CCHUNK) {
      float v[LS_CCHUNK][V];
#pragma unroll
      for (int k = 0; k < LS_CCHUNK; ++k) {
        const int c = c0 + k < C ? c0 + k : C - 1;                    // clamped: the planes past C re-read the last one
        Pack<T, V>::load(px + (int64_t)c * HW, v[k]);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float cm = -INFINITY;
#pragma unroll
        for (int k = 0; k < LS_CCHUNK; ++k) cm = fmaxf(cm, c0 + k < C ? v[k][j] : -INFINITY);
        const float mn = fmaxf(m[j], cm);
        float cs = 0.f;
#pragma unroll
        for (int k = 0; k < LS_CCHUNK; ++k) {
          const bool in = c0 + k < C;
          cs += in ? __expf(v[k][j] - mn) : 0.f;
          xl[j] += (in && c0 + k == li[j]) ? v[k][j] : 0.f;
        }
        s[j] = __builtin_fmaf(s[j], __expf(m[j] - mn), cs);
        m[j] = mn;
      }
    }
    float out[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      out[j] = m[j] + __logf(s[j]);
      const bool valid = li[j] >= 0 && li[j] < C;
      if (on && valid) { acc += out[j] - xl[j]; ++nv; }
      if (on && !valid && li[j] != 255) ++nb;
    }
    if (on) Pack<float, V>::store(lse + pix, out);
  }
  block_partials<2, 2>({acc, 0.f}, {nv, nb}, ws);
}

template <typename T, int V, int L>
__global__ __launch_bounds__(LS_THREADS) void ce_bwd_planar_kernel(const T *__restrict__ x, const void *__restrict__ lab,
                                                                   const float *__restrict__ lse, const float *__restrict__ rec,
                                                                   const float *__restrict__ gout, int C, int HW, int units,
                                                                   T *__restrict__ dx) {
  const int upp = HW / V;
  const float kf = rec[M3_LOSS_REC_COEF] * *gout;
  for (int u0 = blockIdx.x * LS_THREADS; u0 < units; u0 += gridDim.x * LS_THREADS) {
    const int u = u0 + threadIdx.x;
    const bool on = u < units;
    const int uc = on ? u : units - 1;
    const int b = uc / upp, r = uc - b * upp;
    const int pix = b * HW + r * V;
    const int64_t off = (int64_t)b * C * HW + r * V;
    int li[V];
    float ls[V];
#pragma unroll
    for (int j = 0; j < V; ++j) li[j] = class_label<L>(lab, pix + j);
    Pack<float, V>::load(lse + pix, ls);
    for (int c0 = 0; c0 < C; c0 += LS_CCHUNK) {
      float v[LS_CCHUNK][V];
#pragma unroll
      for (int k = 0; k < LS_CCHUNK; ++k) {
        const int c = c0 + k < C ? c0 + k : C - 1;
        Pack<T, V>::load(x + off + (int64_t)c * HW, v[k]);
      }
#pragma unroll
      for (int k = 0; k < LS_CCHUNK; ++k) {
        float d[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const bool valid = li[j] >= 0 && li[j] < C;
          const float p = __expf(v[k][j] - ls[j]);
          d[j] = valid ? (p - (c0 + k == li[j] ? 1.f : 0.f)) * kf : 0.f;
        }
        if (on && c0 + k < C) Pack<T, V>::store(dx + off + (int64_t)(c0 + k) * HW, d);
      }
    }
  }
}

// ----------------------------------------------------------------------------------- cross-entropy, channels-last
// G = 2^gsh lanes read one pixel, so the 64 / G pixels of a wave step are one contiguous span of memory.  The scalar path
// (any C, any alignment): lane j of the group holds channels j, j + G, j + 2G, j + 3G (C <= 255 <= 4 * 64), all four loaded
// before the first is used, and the group reduces with shuffles.
template <typename T, int L>
__global__ __launch_bounds__(LS_THREADS) void ce_fwd_cl1_kernel(const T *__restrict__ x, const void *__restrict__ lab, int C,
                                                                int npix, int gsh, float *__restrict__ lse, float *__restrict__ ws) {
  constexpr int R = 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int G = 1 << gsh, j = lane & (G - 1), pl = lane >> gsh, ppw = 64 >> gsh;
  const int nsteps = (npix + ppw - 1) / ppw;
  float acc = 0.f;
  int nv = 0, nb = 0;
  for (int s0 = blockIdx.x * 4 + wave; s0 < nsteps; s0 += gridDim.x * 4) {                 // wave-uniform
    const int p = s0 * ppw + pl;
    const bool on = p < npix;
    const int pc = on ? p : npix - 1;
    float v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int c = j + r * G;
      v[r] = (float)x[(int64_t)pc * C + (c < C ? c : C - 1)];
    }
    const int li = class_label<L>(lab, pc);
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < R; ++r) m = fmaxf(m, j + r * G < C ? v[r] : -INFINITY);
    for (int o = G >> 1; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float s = 0.f, xl = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int c = j + r * G;
      s += c < C ? __expf(v[r] - m) : 0.f;
      xl += (c < C && c == li) ? v[r] : 0.f;
    }
    for (int o = G >> 1; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); xl += __shfl_xor(xl, o, 64); }
    const float out = m + __logf(s);
    const bool valid = li >= 0 && li < C;
    if (j == 0 && on) {
      lse[pc] = out;
      if (valid) { acc += out - xl; ++nv; }
      else if (li != 255) ++nb;
    }
  }
  block_partials<2, 2>({acc, 0.f}, {nv, nb}, ws);
}

// The vector path of the same reduction (C a multiple of 4: lane j holds channels 4j .. 4j + 3, at most 64 lanes).  What paces
// the shuffle form above is not memory: its shuffles are LDS round trips (ds_bpermute) in dependent chains inside run-time
// loops - measured with 4 channels per lane at 8 x 40 x 480 x 640 fp32: 226 us, 1.7 TB/s, 0.29 of m3_add_f32's rate.  Here the first four levels of a group's reduction are DPP row operations
// (group_allreduce, reduce_dev.h), only groups of
// 32 and 64 lanes fall back to a shuffle; x[label] is not reduced at all - the lane that holds the label's chunk adds the
// pixel's term; every level runs over the U steps together; and the next pass's loads are issued before this one is reduced.
template <typename T, int L>
__global__ __launch_bounds__(LS_THREADS) void ce_fwd_cl4_kernel(const T *__restrict__ x, const void *__restrict__ lab, int C,
                                                                int npix, int gsh, float *__restrict__ lse, float *__restrict__ ws) {
  constexpr int U = 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int G = 1 << gsh, j = lane & (G - 1), pl = lane >> gsh, ppw = 64 >> gsh;
  const int nch = C >> 2;
  const bool in = j < nch;                                       // lanes past the pixel's chunks re-read the last one
  const int joff = (in ? j : nch - 1) * 4;
  const int nsteps = (npix + ppw - 1) / ppw;
  const int stride = gridDim.x * 4 * U;
  float acc = 0.f;
  int nv = 0, nb = 0;
  float v[U][4], vn[U][4];
  int li[U], pc[U], lin[U], pcn[U];
  bool on[U], onn[U];
  int s0 = (blockIdx.x * 4 + wave) * U;                          // wave-uniform
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int p = (s0 + u) * ppw + pl;
    on[u] = p < npix;
    pc[u] = on[u] ? p : npix - 1;
    Pack<T, 4>::load(x + (int64_t)pc[u] * C + joff, v[u]);
    li[u] = class_label<L>(lab, pc[u]);
  }
  for (; s0 < nsteps; s0 += stride) {
#pragma unroll
    for (int u = 0; u < U; ++u) {                                // the next pass (past the end: clamped, never used)
      const int p = (s0 + stride + u) * ppw + pl;
      onn[u] = p < npix;
      pcn[u] = onn[u] ? p : npix - 1;
      Pack<T, 4>::load(x + (int64_t)pcn[u] * C + joff, vn[u]);
      lin[u] = class_label<L>(lab, pcn[u]);
    }
    float m[U], s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) m[u] = in ? fmaxf(fmaxf(v[u][0], v[u][1]), fmaxf(v[u][2], v[u][3])) : -INFINITY;
    group_allreduce<OpMax>(m, gsh);
#pragma unroll
    for (int u = 0; u < U; ++u)
      s[u] = in ? (__expf(v[u][0] - m[u]) + __expf(v[u][1] - m[u])) + (__expf(v[u][2] - m[u]) + __expf(v[u][3] - m[u])) : 0.f;
    group_allreduce<OpSum>(s, gsh);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float out = m[u] + __logf(s[u]);
      const bool valid = li[u] >= 0 && li[u] < C;
      const int e = li[u] - j * 4;                               // the label's channel inside this lane's chunk, if it is here
      if (on[u] && valid && e >= 0 && e < 4) {
        const float xl = e == 0 ? v[u][0] : (e == 1 ? v[u][1] : (e == 2 ? v[u][2] : v[u][3]));
        acc += out - xl;
        ++nv;
      }
      if (j == 0 && on[u]) {
        lse[pc[u]] = out;
        if (!valid && li[u] != 255) ++nb;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) v[u][k] = vn[u][k];
      li[u] = lin[u]; pc[u] = pcn[u]; on[u] = onn[u];
    }
  }
  block_partials<2, 2>({acc, 0.f}, {nv, nb}, ws);
}

// one pass over the flat [npix * C] span, V elements (of one pixel: V divides C) per access, two pieces per thread
template <typename T, int V, int L>
__global__ __launch_bounds__(LS_THREADS) void ce_bwd_cl_kernel(const T *__restrict__ x, const void *__restrict__ lab,
                                                               const float *__restrict__ lse, const float *__restrict__ rec,
                                                               const float *__restrict__ gout, int C, int units, T *__restrict__ dx) {
  constexpr int P = 2;
  const float kf = rec[M3_LOSS_REC_COEF] * *gout;
  for (int u0 = blockIdx.x * (LS_THREADS * P); u0 < units; u0 += gridDim.x * (LS_THREADS * P)) {
    float v[P][V], ls[P];
    int li[P], c0[P], uc[P];
    bool on[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const int u = u0 + k * LS_THREADS + threadIdx.x;
      on[k] = u < units;
      uc[k] = on[k] ? u : units - 1;
      const uint32_t e = (uint32_t)uc[k] * V, pix = e / (uint32_t)C;
      c0[k] = (int)(e - pix * C);
      Pack<T, V>::load(x + (int64_t)uc[k] * V, v[k]);
      ls[k] = lse[pix];
      li[k] = class_label<L>(lab, (int)pix);
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const bool valid = li[k] >= 0 && li[k] < C;
      float d[V];
#pragma unroll
      for (int e = 0; e < V; ++e) d[e] = valid ? (__expf(v[k][e] - ls[k]) - (c0[k] + e == li[k] ? 1.f : 0.f)) * kf : 0.f;
      if (on[k]) Pack<T, V>::store(dx + (int64_t)uc[k] * V, d);
    }
  }
}

// ---------------------------------------------------------------------------------- flat losses: masked L1, balanced BCE
// pred and label share one layout, so both are flat spans of n elements: units = n / V, two pieces per thread.
__device__ __forceinline__ float sign_f(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }   // torch.sign: 0 at 0

// the reference's stable form: -(x (y - [x >= 0]) - log(1 + exp(x - 2 x [x >= 0]))) = x ([x >= 0] - y) + log1p(exp(-|x|))
__device__ __forceinline__ float bce_term(float x, bool y) {
  return x * ((x >= 0.f ? 1.f : 0.f) - (y ? 1.f : 0.f)) + log1pf(__expf(-fabsf(x)));
}

template <typename T, int V, int KIND, bool BWD>
__global__ __launch_bounds__(LS_THREADS) void flat_kernel(const T *__restrict__ x, const float *__restrict__ lab,
                                                          const float *__restrict__ rec, const float *__restrict__ gout,
                                                          int units, T *__restrict__ dx, float *__restrict__ ws) {
  constexpr int P = 2;
  float k0 = 0.f, k1 = 0.f;
  if (BWD) { const float g = *gout; k0 = rec[M3_LOSS_REC_COEF] * g; k1 = rec[M3_LOSS_REC_COEF2] * g; }
  float s0 = 0.f, s1 = 0.f;
  int n0 = 0;
  for (int u0 = blockIdx.x * (LS_THREADS * P); u0 < units; u0 += gridDim.x * (LS_THREADS * P)) {
    float v[P][V], l[P][V];
    int uc[P];
    bool on[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const int u = u0 + k * LS_THREADS + threadIdx.x;
      on[k] = u < units;
      uc[k] = on[k] ? u : units - 1;
      Pack<T, V>::load(x + (int64_t)uc[k] * V, v[k]);
      Pack<float, V>::load(lab + (int64_t)uc[k] * V, l[k]);
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
      float d[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float xv = v[k][e], lv = l[k][e];
        if (KIND == K_L1) {
          const bool valid = lv != 255.f;
          if (BWD) d[e] = valid ? sign_f(xv - lv) * k0 : 0.f;
          else if (on[k] && valid) { s0 += fabsf(xv - lv); ++n0; }
        } else {
          const bool y = lv >= 0.5f;
          if (BWD) {
            const float ex = __expf(-fabsf(xv)), q = 1.f / (1.f + ex);
            const float sg = xv >= 0.f ? q : ex * q;                   // sigmoid(x) without overflow
            d[e] = (sg - (y ? 1.f : 0.f)) * (y ? k0 : k1);
          } else if (on[k]) {
            const float tv = bce_term(xv, y);
            if (y) { s0 += tv; ++n0; } else s1 += tv;
          }
        }
      }
      if (BWD && on[k]) Pack<T, V>::store(dx + (int64_t)uc[k] * V, d);
    }
  }
  if (!BWD) block_partials<2, 2>({s0, s1}, {n0, 0}, ws);
}

// ------------------------------------------------------------------------------------------------------- normals
// One thread per pixel; pred and label each in their own layout: element (b, c, hw) at b * C * HW + hw * sp + c * sc with
// (sp, sc) = (1, HW) planar or (C, 1) channels-last.  Planar: a wave's loads of one channel are one span; channels-last: a
// wave's pixels are one span of 64 * C elements that the C loads of a lane walk together.  CT: C as a constant (3), 0 = run
// time (at most 8; channels past C re-read the last and count for nothing).
template <typename T, int CT, bool BWD>
__global__ __launch_bounds__(LS_THREADS) void normals_kernel(const T *__restrict__ x, const float *__restrict__ lab,
                                                             const float *__restrict__ rec, const float *__restrict__ gout,
                                                             int C_rt, int HW, int npix, int xsp, int xsc, int lsp, int lsc,
                                                             int norm, T *__restrict__ dx, float *__restrict__ ws) {
  constexpr int CM = CT ? CT : M3_LOSS_NORMALS_MAX_C;
  const int C = CT ? CT : C_rt;
  float kf = 0.f;
  if (BWD) kf = rec[M3_LOSS_REC_COEF] * *gout;
  float acc = 0.f;
  int nv = 0;
  for (int p0 = blockIdx.x * LS_THREADS; p0 < npix; p0 += gridDim.x * LS_THREADS) {
    const int p = p0 + threadIdx.x;
    const bool on = p < npix;
    const int pc = on ? p : npix - 1;
    const int b = pc / HW, hw = pc - b * HW;
    const int64_t xo = (int64_t)b * C * HW + (int64_t)hw * xsp, lo = (int64_t)b * C * HW + (int64_t)hw * lsp;
    float xv[CM], lv[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      const int cc = c < C ? c : C - 1;
      xv[c] = (float)x[xo + (int64_t)cc * xsc];
      lv[c] = lab[lo + (int64_t)cc * lsc];
    }
    float n2 = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) n2 = __builtin_fmaf(c < C ? xv[c] : 0.f, xv[c], n2);
    const float n = sqrtf(n2), q = n + 1e-12f;
    float g[CM], gt = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      const bool valid = c < C && lv[c] != 255.f;
      const float t = xv[c] / q, d = t - lv[c];
      if (BWD) {
        g[c] = valid ? (norm == 1 ? sign_f(d) : 2.f * d) : 0.f;
        gt = __builtin_fmaf(g[c], t, gt);
      } else if (on && valid) {
        acc += norm == 1 ? fabsf(d) : d * d;
        ++nv;
      }
    }
    if (BWD) {
      // t = x / q, q = |x| + 1e-12: d t_c / d x_k = ([c == k] - t_c x_k / |x|) / q, and 0 for the norm's own derivative at x = 0
      const float rn = n > 0.f ? 1.f / n : 0.f;
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        const float d = (g[c] - gt * (xv[c] * rn)) / q * kf;
        if (on && c < C) dx[xo + (int64_t)c * xsc] = (T)d;
      }
    }
  }
  if (!BWD) block_partials<2, 2>({acc, 0.f}, {nv, 0}, ws);
}

static int finalize(const float *ws, int nblk, int kind, double numel, int has_pw, double pw, void *rec, hipStream_t s,
                    const char *who) {
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, s, ws, nblk, kind, numel, has_pw, pw, (int32_t *)rec);
  return check_launch(who);
}

}  // namespace m3

using namespace m3;

extern "C" int64_t m3_loss_ws_elems(int64_t n) {
  if (n < 1) return 0;
  return (int64_t)LS_NP * blocks_for(n, LS_THREADS);
}

extern "C" int m3_loss_ce_fwd(const void *pred, int dtype, const void *label, int label_dtype, int B, int C, int H, int W,
                              int layout, float *lse, float *ws, void *record, void *stream) {
  LossShape sh;
  if (int rc = shape_ok(B, C, H, W, 2, 255, layout, dtype, "m3_loss_ce_fwd", &sh)) return rc;
  M3_REQUIRE(pred && label && lse && ws && record, "m3_loss_ce_fwd: null pointer");
  M3_REQUIRE(label_dtype_ok(label_dtype), "m3_loss_ce_fwd: bad label dtype code %d", label_dtype);
  hipStream_t s = (hipStream_t)stream;
  int nblk;
  if (layout == M3_LAYOUT_NCHW) {
    const bool vec = aligned16(pred) && aligned16(lse) && sh.HW % 4 == 0;
    const int units = vec ? sh.npix / 4 : sh.npix;
    nblk = blocks_for(units, LS_THREADS);
    by_dtype(dtype, [&](auto tt) {
      typedef typename decltype(tt)::type T;
      by_label(label_dtype, [&](auto lt) {
        auto go = [&](auto v) {
          hipLaunchKernelGGL((ce_fwd_planar_kernel<T, decltype(v)::value, decltype(lt)::value>), dim3(nblk), dim3(LS_THREADS), 0,
                             s, (const T *)pred, label, C, sh.HW, units, lse, ws);
        };
        if (vec) go(IntTag<4>{}); else go(IntTag<1>{});
      });
    });
  } else {
    const bool vec = aligned16(pred) && C % 4 == 0;
    const int gsh = group_shift(vec ? C / 4 : C), ppw = 64 >> gsh;
    const int64_t steps = ((int64_t)sh.npix + ppw - 1) / ppw;
    // a workgroup's four waves take U steps each per pass; G may exceed the chunks of a pixel (the power of two above them), so
    // the grid is held to the blocks the workspace was sized for (m3_loss_ws_elems) and the kernel's loop takes the rest
    nblk = blocks_for(steps, vec ? 16 : 4);
    if (nblk > blocks_for(sh.n, LS_THREADS)) nblk = blocks_for(sh.n, LS_THREADS);
    by_dtype(dtype, [&](auto tt) {
      typedef typename decltype(tt)::type T;
      by_label(label_dtype, [&](auto lt) {
        constexpr int L = decltype(lt)::value;
        // (the 16-byte and the scalar form are two kernels that differ by NAME, not by a template argument a tag could carry:
        // both have one signature, so the choice is a pointer and the launch is still written once)
        auto *kern = vec ? ce_fwd_cl4_kernel<T, L> : ce_fwd_cl1_kernel<T, L>;
        hipLaunchKernelGGL(kern, dim3(nblk), dim3(LS_THREADS), 0, s, (const T *)pred, label, C, sh.npix, gsh, lse, ws);
      });
    });
  }
  if (int rc = check_launch("m3_loss_ce_fwd (partials)")) return rc;
  return finalize(ws, nblk, K_CE, (double)sh.n, 0, 0.0, record, s, "m3_loss_ce_fwd (finalize)");
}

extern "C" int m3_loss_ce_bwd(const void *pred, int dtype, const void *label, int label_dtype, const float *lse,
                              const void *record, const float *grad_out, int B, int C, int H, int W, int layout, void *dpred,
                              void *stream) {
  LossShape sh;
  if (int rc = shape_ok(B, C, H, W, 2, 255, layout, dtype, "m3_loss_ce_bwd", &sh)) return rc;
  M3_REQUIRE(pred && label && lse && record && grad_out && dpred, "m3_loss_ce_bwd: null pointer");
  M3_REQUIRE(label_dtype_ok(label_dtype), "m3_loss_ce_bwd: bad label dtype code %d", label_dtype);
  hipStream_t s = (hipStream_t)stream;
  const float *rec = (const float *)record;
  if (layout == M3_LAYOUT_NCHW) {
    const bool vec = aligned16(pred) && aligned16(dpred) && aligned16(lse) && sh.HW % 4 == 0;
    const int units = vec ? sh.npix / 4 : sh.npix;
    const int nblk = blocks_for(units, LS_THREADS);
    by_dtype(dtype, [&](auto tt) {
      typedef typename decltype(tt)::type T;
      by_label(label_dtype, [&](auto lt) {
        auto go = [&](auto v) {
          hipLaunchKernelGGL((ce_bwd_planar_kernel<T, decltype(v)::value, decltype(lt)::value>), dim3(nblk), dim3(LS_THREADS), 0,
                             s, (const T *)pred, label, lse, rec, grad_out, C, sh.HW, units, (T *)dpred);
        };
        if (vec) go(IntTag<4>{}); else go(IntTag<1>{});
      });
    });
  } else {
    const bool vec = aligned16(pred) && aligned16(dpred) && C % 4 == 0;
    const int units = (int)(vec ? sh.n / 4 : sh.n);
    const int nblk = blocks_for(units, LS_THREADS * 2);
    by_dtype(dtype, [&](auto tt) {
      typedef typename decltype(tt)::type T;
      by_label(label_dtype, [&](auto lt) {
        auto go = [&](auto v) {
          hipLaunchKernelGGL((ce_bwd_cl_kernel<T, decltype(v)::value, decltype(lt)::value>), dim3(nblk), dim3(LS_THREADS), 0, s,
                             (const T *)pred, label, lse, rec, grad_out, C, units, (T *)dpred);
        };
        if (vec) go(IntTag<4>{}); else go(IntTag<1>{});
      });
    });
  }
  return check_launch("m3_loss_ce_bwd");
}

// the two flat losses: forward (dx == NULL) or backward
template <int KIND>
static int flat_launch(const void *pred, int dtype, const float *label, const void *record, const float *grad_out,
                       const LossShape &sh, void *dpred, float *ws, int *nblk_out, hipStream_t s) {
  const bool bwd = dpred != nullptr;
  const bool vec = aligned16(pred) && aligned16(label) && (!bwd || aligned16(dpred)) && sh.n % 4 == 0;
  const int units = (int)(vec ? sh.n / 4 : sh.n);
  const int nblk = blocks_for(units, LS_THREADS * 2);
  const float *rec = (const float *)record;
  by_dtype(dtype, [&](auto tt) {
    typedef typename decltype(tt)::type T;
    auto go = [&](auto v, auto b) {
      hipLaunchKernelGGL((flat_kernel<T, decltype(v)::value, KIND, decltype(b)::value != 0>), dim3(nblk), dim3(LS_THREADS), 0, s,
                         (const T *)pred, label, rec, grad_out, units, (T *)dpred, ws);
    };
    auto with_v = [&](auto v) { if (bwd) go(v, IntTag<1>{}); else go(v, IntTag<0>{}); };
    if (vec) with_v(IntTag<4>{}); else with_v(IntTag<1>{});
  });
  *nblk_out = nblk;
  return 0;
}

extern "C" int m3_loss_l1_fwd(const void *pred, int dtype, const float *label, int B, int C, int H, int W, int layout,
                              float *ws, void *record, void *stream) {
  LossShape sh;
  if (int rc = shape_ok(B, C, H, W, 1, 1 << 30, layout, dtype, "m3_loss_l1_fwd", &sh)) return rc;
  M3_REQUIRE(pred && label && ws && record, "m3_loss_l1_fwd: null pointer");
  int nblk;
  flat_launch<K_L1>(pred, dtype, label, nullptr, nullptr, sh, nullptr, ws, &nblk, (hipStream_t)stream);
  if (int rc = check_launch("m3_loss_l1_fwd (partials)")) return rc;
  return finalize(ws, nblk, K_L1, (double)sh.n, 0, 0.0, record, (hipStream_t)stream, "m3_loss_l1_fwd (finalize)");
}

extern "C" int m3_loss_l1_bwd(const void *pred, int dtype, const float *label, const void *record, const float *grad_out,
                              int B, int C, int H, int W, int layout, void *dpred, void *stream) {
  LossShape sh;
  if (int rc = shape_ok(B, C, H, W, 1, 1 << 30, layout, dtype, "m3_loss_l1_bwd", &sh)) return rc;
  M3_REQUIRE(pred && label && record && grad_out && dpred, "m3_loss_l1_bwd: null pointer");
  int nblk;
  flat_launch<K_L1>(pred, dtype, label, record, grad_out, sh, dpred, nullptr, &nblk, (hipStream_t)stream);
  return check_launch("m3_loss_l1_bwd");
}

extern "C" int m3_loss_bce_fwd(const void *pred, int dtype, const float *label, int B, int C, int H, int W, int layout,
                               int has_pos_weight, double pos_weight, float *ws, void *record, void *stream) {
  LossShape sh;
  if (int rc = shape_ok(B, C, H, W, 1, 1 << 30, layout, dtype, "m3_loss_bce_fwd", &sh)) return rc;
  M3_REQUIRE(pred && label && ws && record, "m3_loss_bce_fwd: null pointer");
  int nblk;
  flat_launch<K_BCE>(pred, dtype, label, nullptr, nullptr, sh, nullptr, ws, &nblk, (hipStream_t)stream);
  if (int rc = check_launch("m3_loss_bce_fwd (partials)")) return rc;
  return finalize(ws, nblk, K_BCE, (double)sh.n, has_pos_weight ? 1 : 0, pos_weight, record, (hipStream_t)stream,
                  "m3_loss_bce_fwd (finalize)");
}

extern "C" int m3_loss_bce_bwd(const void *pred, int dtype, const float *label, const void *record, const float *grad_out,
                               int B, int C, int H, int W, int layout, void *dpred, void *stream) {
  LossShape sh;
  if (int rc = shape_ok(B, C, H, W, 1, 1 << 30, layout, dtype, "m3_loss_bce_bwd", &sh)) return rc;
  M3_REQUIRE(pred && label && record && grad_out && dpred, "m3_loss_bce_bwd: null pointer");
  int nblk;
  flat_launch<K_BCE>(pred, dtype, label, record, grad_out, sh, dpred, nullptr, &nblk, (hipStream_t)stream);
  return check_launch("m3_loss_bce_bwd");
}

static int normals_launch(const void *pred, int dtype, const float *label, const void *record, const float *grad_out,
                          const LossShape &sh, int layout, int label_layout, int norm, void *dpred, float *ws, hipStream_t s) {
  const bool bwd = dpred != nullptr;
  const int C = sh.C, HW = sh.HW;
  const int xsp = layout == M3_LAYOUT_NCHW ? 1 : C, xsc = layout == M3_LAYOUT_NCHW ? HW : 1;
  const int lsp = label_layout == M3_LAYOUT_NCHW ? 1 : C, lsc = label_layout == M3_LAYOUT_NCHW ? HW : 1;
  const int nblk = blocks_for(sh.npix, LS_THREADS);
  const float *rec = (const float *)record;
  by_dtype(dtype, [&](auto tt) {
    typedef typename decltype(tt)::type T;
    auto go = [&](auto ct, auto b) {
      hipLaunchKernelGGL((normals_kernel<T, decltype(ct)::value, decltype(b)::value != 0>), dim3(nblk), dim3(LS_THREADS), 0, s,
                         (const T *)pred, label, rec, grad_out, C, HW, sh.npix, xsp, xsc, lsp, lsc, norm, (T *)dpred, ws);
    };
    auto with_c = [&](auto ct) { if (bwd) go(ct, IntTag<1>{}); else go(ct, IntTag<0>{}); };
    if (!by_int<3>(C, with_c)) with_c(IntTag<0>{});
  });
  return nblk;
}

extern "C" int m3_loss_normals_fwd(const void *pred, int dtype, const float *label, int B, int C, int H, int W, int layout,
                                   int label_layout, int norm, float *ws, void *record, void *stream) {
  LossShape sh;
  if (int rc = shape_ok(B, C, H, W, 1, M3_LOSS_NORMALS_MAX_C, layout, dtype, "m3_loss_normals_fwd", &sh)) return rc;
  M3_REQUIRE(label_layout == M3_LAYOUT_NCHW || label_layout == M3_LAYOUT_NHWC, "m3_loss_normals_fwd: bad label layout %d", label_layout);
  M3_REQUIRE(norm == 1 || norm == 2, "m3_loss_normals_fwd: norm must be 1 or 2, got %d", norm);
  M3_REQUIRE(pred && label && ws && record, "m3_loss_normals_fwd: null pointer");
  const int nblk = normals_launch(pred, dtype, label, nullptr, nullptr, sh, layout, label_layout, norm, nullptr, ws, (hipStream_t)stream);
  if (int rc = check_launch("m3_loss_normals_fwd (partials)")) return rc;
  return finalize(ws, nblk, K_NORMALS, (double)sh.n, 0, 0.0, record, (hipStream_t)stream, "m3_loss_normals_fwd (finalize)");
}

extern "C" int m3_loss_normals_bwd(const void *pred, int dtype, const float *label, const void *record, const float *grad_out,
                                   int B, int C, int H, int W, int layout, int label_layout, int norm, void *dpred, void *stream) {
  LossShape sh;
  if (int rc = shape_ok(B, C, H, W, 1, M3_LOSS_NORMALS_MAX_C, layout, dtype, "m3_loss_normals_bwd", &sh)) return rc;
  M3_REQUIRE(label_layout == M3_LAYOUT_NCHW || label_layout == M3_LAYOUT_NHWC, "m3_loss_normals_bwd: bad label layout %d", label_layout);
  M3_REQUIRE(norm == 1 || norm == 2, "m3_loss_normals_bwd: norm must be 1 or 2, got %d", norm);
  M3_REQUIRE(pred && label && record && grad_out && dpred, "m3_loss_normals_bwd: null pointer");
  normals_launch(pred, dtype, label, record, grad_out, sh, layout, label_layout, norm, dpred, nullptr, (hipStream_t)stream);
  return check_launch("m3_loss_normals_bwd");
}
