// The task metrics of a dense-prediction training or evaluation step for gfx950: what the reference's PerformanceMeter
// accumulates (evaluation/eval_semseg.py, eval_human_parts.py, eval_depth.py, eval_normals.py, eval_sal.py), computed from the
// RAW head output [B,C,H,W] and the label with get_output's transform (argmax, clamp, normalise, sigmoid) fused in - nothing of
// the prediction's size is written.  An update is two launches.  Launch one: one pass over pred and label leaves per-workgroup
// partials (fp32 sums, int32 counts) in the caller's workspace - no global atomics; a workgroup's class histogram is built with
// integer LDS atomics, whose result does not depend on their order.  Launch two: one workgroup adds the partials in block order
// (float sums in double) INTO the device-resident state of 8-byte words (int64 counts, double sums), which persists across
// updates.  Nothing is read back to the host; two runs over the same sequence of updates give the same bits.
//
// Layouts, vector width, load issue and tails are those of loss.hip: NCHW-contiguous or channels-last, V = 4 where the host
// found 16-byte alignment and whole vectors else V = 1, every load of a thread's pieces before the first use, clamped offsets.
#include "loss_dev.h"

namespace m3 {

constexpr int MT_BINS = M3_METER_IOU_BINS;
constexpr int MT_CCHUNK = 8;                        // channels of a planar pixel in flight together

// ------------------------------------------------------------------------------------------------------------ class IoU
// torch.max's choice as the maximum of an integer key: keys order as the values do, -0 and +0 share one key (they compare
// equal), every NaN has the largest key (a NaN beats everything).  Walking the channels upwards and replacing only on a
// strictly larger key keeps the lowest index of a tie and the first NaN.  0 is below every key: the "no channel" value.
__device__ __forceinline__ uint32_t max_key(float v) {
  if (v != v) return 0xFFFFFFFFu;
  const uint32_t b = v == 0.f ? 0u : __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// the class of pixel i as the reference's `gt == i_part` sees it: [0, 255] where the label EQUALS that integer (no
// truncation: 2.5 is no class), -1 for every other value.  255 is "ignore"; -1 is a valid pixel that matches no class.
template <int L>
__device__ __forceinline__ int meter_label(const void *__restrict__ lab, int i) {
  if constexpr (L == M3_LABEL_I64) {
    const int64_t v = ((const int64_t *)lab)[i];
    return (v >= 0 && v < 256) ? (int)v : -1;
  } else if constexpr (L == M3_LABEL_U8) {
    return (int)((const uint8_t *)lab)[i];
  } else {
    const float f = ((const float *)lab)[i];
    const int k = (f >= 0.f && f < 256.f) ? (int)f : -1;
    return (k >= 0 && (float)k == f) ? k : -1;
  }
}

// a workgroup's histogram: [0] true positives, [1] predictions, [2] labels - each [MT_BINS], over the pixels with label != 255
__device__ __forceinline__ void iou_zero(int *hist) {
  for (int i = threadIdx.x; i < 3 * MT_BINS; i += LS_THREADS) hist[i] = 0;
  __syncthreads();
}
__device__ __forceinline__ void iou_count(int *hist, int pred, int cls) {      // pred in [0, C), C <= 255
  if (cls == 255 || (unsigned)pred >= (unsigned)MT_BINS) return;
  atomicAdd(&hist[MT_BINS + pred], 1);
  if (cls >= 0) {
    atomicAdd(&hist[2 * MT_BINS + cls], 1);
    if (cls == pred) atomicAdd(&hist[pred], 1);
  }
}
__device__ __forceinline__ void iou_flush(const int *hist, int ncls, int32_t *__restrict__ ws) {   // ws: [nblk][3][ncls]
  __syncthreads();
  int32_t *o = ws + (int64_t)blockIdx.x * 3 * ncls;
  for (int i = threadIdx.x; i < 3 * ncls; i += LS_THREADS) {
    const int k = i / ncls;
    o[i] = hist[k * MT_BINS + (i - k * ncls)];
  }
}

// planar: a thread owns V consecutive pixels of one plane and walks the C planes MT_CCHUNK at a time
template <typename T, int V, int L>
__global__ __launch_bounds__(LS_THREADS) void iou_planar_kernel(const T *__restrict__ x, const void *__restrict__ lab, int C,
                                                                int HW, int units, int ncls, int32_t *__restrict__ ws) {
  __shared__ int hist[3 * MT_BINS];
  iou_zero(hist);
  const int upp = HW / V;
  for (int u0 = blockIdx.x * LS_THREADS; u0 < units; u0 += gridDim.x * LS_THREADS) {
    const int u = u0 + threadIdx.x;
    const bool on = u < units;
    const int uc = on ? u : units - 1;
    const int b = uc / upp, r = uc - b * upp;
    const int pix = b * HW + r * V;
    const T *px = x + (int64_t)b * C * HW + r * V;
    int li[V], bi[V];
    uint32_t bk[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { li[j] = meter_label<L>(lab, pix + j); bk[j] = 0u; bi[j] = 0; }
    for (int c0 = 0; c0 < C; c0 += MT_CCHUNK) {
      float v[MT_CCHUNK][V];
#pragma unroll
      for (int k = 0; k < MT_CCHUNK; ++k) {
        const int c = c0 + k < C ? c0 + k : C - 1;                    // clamped: the planes past C re-read the last one
        Pack<T, V>::load(px + (int64_t)c * HW, v[k]);
      }
#pragma unroll
      for (int k = 0; k < MT_CCHUNK; ++k) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const uint32_t key = c0 + k < C ? max_key(v[k][j]) : 0u;
          if (key > bk[j]) { bk[j] = key; bi[j] = c0 + k; }
        }
      }
    }
    if (on) {
#pragma unroll
      for (int j = 0; j < V; ++j) iou_count(hist, bi[j], li[j]);
    }
  }
  iou_flush(hist, ncls, ws);
}

// channels-last: G = 2^gsh lanes read one pixel (loss.hip's geometry).  The group's argmax is two integer reductions - the
// maximum of the keys, then the minimum of the channels that hold it (group_allreduce, reduce_dev.h).
constexpr uint32_t NO_CHANNEL = 0xFFFFu;

// the scalar path (any C, any alignment): lane j of the group holds channels j, j + G, j + 2G, j + 3G (C <= 255 <= 4 * 64)
template <typename T, int L>
__global__ __launch_bounds__(LS_THREADS) void iou_cl1_kernel(const T *__restrict__ x, const void *__restrict__ lab, int C,
                                                             int npix, int gsh, int ncls, int32_t *__restrict__ ws) {
  constexpr int R = 4;
  __shared__ int hist[3 * MT_BINS];
  iou_zero(hist);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int G = 1 << gsh, j = lane & (G - 1), pl = lane >> gsh, ppw = 64 >> gsh;
  const int nsteps = (npix + ppw - 1) / ppw;
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
    const int li = meter_label<L>(lab, pc);
    uint32_t key[R], km[1] = {0u}, cand[1] = {NO_CHANNEL};
#pragma unroll
    for (int r = 0; r < R; ++r) {
      key[r] = j + r * G < C ? max_key(v[r]) : 0u;
      km[0] = OpMax::of(km[0], key[r]);
    }
    group_allreduce<OpMax>(km, gsh);
#pragma unroll
    for (int r = R - 1; r >= 0; --r)                                   // downwards: the lowest channel that holds the maximum stays
      if (key[r] == km[0]) cand[0] = (uint32_t)(j + r * G);
    group_allreduce<OpMin>(cand, gsh);
    if (j == 0 && on) iou_count(hist, (int)cand[0], li);
  }
  iou_flush(hist, ncls, ws);
}

// the vector path (C a multiple of 4: lane j holds channels 4j .. 4j + 3): U steps per pass reduced together, and the next
// pass's loads issued before this one is reduced - ce_fwd_cl4_kernel's schedule
template <typename T, int L>
__global__ __launch_bounds__(LS_THREADS) void iou_cl4_kernel(const T *__restrict__ x, const void *__restrict__ lab, int C,
                                                             int npix, int gsh, int ncls, int32_t *__restrict__ ws) {
  constexpr int U = 4;
  __shared__ int hist[3 * MT_BINS];
  iou_zero(hist);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int G = 1 << gsh, j = lane & (G - 1), pl = lane >> gsh, ppw = 64 >> gsh;
  const int nch = C >> 2;
  const bool in = j < nch;                                       // lanes past the pixel's chunks re-read the last one
  const int joff = (in ? j : nch - 1) * 4;
  const int nsteps = (npix + ppw - 1) / ppw;
  const int stride = gridDim.x * 4 * U;
  float v[U][4], vn[U][4];
  int li[U], lin[U];
  bool on[U], onn[U];
  int s0 = (blockIdx.x * 4 + wave) * U;                          // wave-uniform
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int p = (s0 + u) * ppw + pl;
    on[u] = p < npix;
    const int pc = on[u] ? p : npix - 1;
    Pack<T, 4>::load(x + (int64_t)pc * C + joff, v[u]);
    li[u] = meter_label<L>(lab, pc);
  }
  for (; s0 < nsteps; s0 += stride) {
#pragma unroll
    for (int u = 0; u < U; ++u) {                                // the next pass (past the end: clamped, never used)
      const int p = (s0 + stride + u) * ppw + pl;
      onn[u] = p < npix;
      const int pc = onn[u] ? p : npix - 1;
      Pack<T, 4>::load(x + (int64_t)pc * C + joff, vn[u]);
      lin[u] = meter_label<L>(lab, pc);
    }
    uint32_t key[U][4], km[U], cand[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int k = 0; k < 4; ++k) key[u][k] = in ? max_key(v[u][k]) : 0u;
      km[u] = OpMax::of(OpMax::of(key[u][0], key[u][1]), OpMax::of(key[u][2], key[u][3]));
    }
    group_allreduce<OpMax>(km, gsh);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      cand[u] = NO_CHANNEL;
#pragma unroll
      for (int k = 3; k >= 0; --k)
        if (in && key[u][k] == km[u]) cand[u] = (uint32_t)(j * 4 + k);
    }
    group_allreduce<OpMin>(cand, gsh);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (j == 0 && on[u]) iou_count(hist, (int)cand[u], li[u]);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[u][k] = vn[u][k];
      li[u] = lin[u]; on[u] = onn[u];
    }
  }
  iou_flush(hist, ncls, ws);
}

// one workgroup: the 3 * ncls counts of every block, slices of the blocks side by side, into the state
__global__ __launch_bounds__(1024) void iou_finalize_kernel(const int32_t *__restrict__ ws, int nblk, int ncls,
                                                            int64_t *__restrict__ state) {
  __shared__ long long sh[1024];
  const int items = 3 * ncls, nsl = 1024 / items;                // ncls <= 256: at least one slice
  const int t = threadIdx.x, sl = t / items, i = t - sl * items;
  if (sl < nsl) {
    long long s = 0;
#pragma unroll 8
    for (int b = sl; b < nblk; b += nsl) s += ws[(int64_t)b * items + i];
    sh[t] = s;
  }
  __syncthreads();
  if (t < items) {
    long long a = 0;
    for (int k = 0; k < nsl; ++k) a += sh[k * items + t];
    const int c = t / ncls;
    state[c * MT_BINS + (t - c * ncls)] += a;
  }
}

// ------------------------------------------------------------------------------------- fp32 sums and counts of a workgroup
// state[k] += the sum of row k over the blocks, in block order: double for the NF sums (words 0 .. NF - 1), int64 for the counts
template <int NF, int NI>
__global__ __launch_bounds__(256) void sums_finalize_kernel(const float *__restrict__ ws, int nblk, int64_t *__restrict__ state) {
  const Totals<NF, NI> tot = reduce_partials<NF, NI>(ws, nblk, nblk);
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < NF; ++k)
    if (t == k) ((double *)state)[k] += tot.s[k];
#pragma unroll
  for (int k = 0; k < NI; ++k)
    if (t == NF + k) state[NF + k] += tot.c[k];
}

// ---------------------------------------------------------------------------------------------------------------- depth
// pred and label share one layout, so both are flat spans: units = n / V, two pieces per thread (flat_kernel's shape)
template <typename T, int V>
__global__ __launch_bounds__(LS_THREADS) void depth_kernel(const T *__restrict__ x, const float *__restrict__ lab, int units,
                                                           float *__restrict__ ws) {
  constexpr int P = 2;
  float s[2] = {0.f, 0.f};
  int n[1] = {0};
  for (int u0 = blockIdx.x * (LS_THREADS * P); u0 < units; u0 += gridDim.x * (LS_THREADS * P)) {
    float v[P][V], l[P][V];
    bool on[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const int u = u0 + k * LS_THREADS + threadIdx.x;
      on[k] = u < units;
      const int uc = on[k] ? u : units - 1;
      Pack<T, V>::load(x + (int64_t)uc * V, v[k]);
      Pack<float, V>::load(lab + (int64_t)uc * V, l[k]);
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float g = l[k][e];
        if (on[k] && g != 255.f) {
          const float p = v[k][e] < 1e-9f ? 1e-9f : v[k][e];          // torch.clamp(min=1e-9): a NaN stays a NaN
          const float d = g - p, q = logf(g) - logf(p);
          s[0] += d * d;
          s[1] += q * q;
          ++n[0];
        }
      }
    }
  }
  block_partials<2, 1>(s, n, ws);
}

// -------------------------------------------------------------------------------------------------------------- normals
// One thread per pixel, C = 3; pred and label each in their own layout (normals_kernel's addressing): element (b, c, hw) at
// b * 3 * HW + hw * sp + c * sc.
template <typename T>
__global__ __launch_bounds__(LS_THREADS) void normals_meter_kernel(const T *__restrict__ x, const float *__restrict__ lab,
                                                                   int HW, int npix, int xsp, int xsc, int lsp, int lsc,
                                                                   float *__restrict__ ws) {
  float s[2] = {0.f, 0.f};
  int n[4] = {0, 0, 0, 0};
  for (int p0 = blockIdx.x * LS_THREADS; p0 < npix; p0 += gridDim.x * LS_THREADS) {
    const int p = p0 + threadIdx.x;
    const bool on = p < npix;
    const int pc = on ? p : npix - 1;
    const int b = pc / HW, hw = pc - b * HW;
    const int64_t xo = (int64_t)b * 3 * HW + (int64_t)hw * xsp, lo = (int64_t)b * 3 * HW + (int64_t)hw * lsp;
    float xv[3], lv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      xv[c] = (float)x[xo + (int64_t)c * xsc];
      lv[c] = lab[lo + (int64_t)c * lsc];
    }
    const float nrm = sqrtf(__builtin_fmaf(xv[2], xv[2], __builtin_fmaf(xv[1], xv[1], xv[0] * xv[0])));
    const float q = nrm < 1e-12f ? 1e-12f : nrm;                      // F.normalize: x / max(|x|, eps)
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const bool valid = lv[c] != 255.f;                              // an ignored element is zeroed on both sides
      dot = __builtin_fmaf(valid ? xv[c] / q : 0.f, valid ? lv[c] : 0.f, dot);
    }
    dot = dot < -1.f ? -1.f : (dot > 1.f ? 1.f : dot);                // torch.clamp: a NaN stays a NaN
    const float a = 57.29577951308232f * acosf(dot);
    if (on && lv[0] != 255.f) {
      s[0] += a;
      s[1] += a * a;
      n[0] += a < 11.25f;
      n[1] += a < 22.5f;
      n[2] += a < 30.f;
      ++n[3];
    }
  }
  block_partials<2, 4>(s, n, ws);
}

// ------------------------------------------------------------------------------------------------------------- saliency
// The 15 thresholds are monotone, so a pixel is described by how many lie below p = sigmoid(x) and by its label bit; a
// thread keeps the two cumulative forms it needs per threshold j - pixels with p > t_j, and those of them with a non-zero
// label - in registers, plus the count of non-zero labels: 31 counts from one pass, no histogram in memory.
// A workgroup works on ONE image: block k of the image's bpi blocks; ws: [B * bpi][32] int32.
struct SalThresholds { float t[M3_METER_SAL_THRESHOLDS]; };

template <typename T, int V>
__global__ __launch_bounds__(LS_THREADS) void sal_kernel(const T *__restrict__ x, const float *__restrict__ lab, int HW, int bpi,
                                                         SalThresholds thr, int32_t *__restrict__ ws) {
  constexpr int P = 2, NT = M3_METER_SAL_THRESHOLDS;
  __shared__ int sh[4][32];
  const int img = blockIdx.x / bpi, kb = blockIdx.x - img * bpi;
  const int units = HW / V;
  const T *px = x + (int64_t)img * HW;
  const float *pl = lab + (int64_t)img * HW;
  int np[NT], ntp[NT], ngt = 0;
#pragma unroll
  for (int j = 0; j < NT; ++j) { np[j] = 0; ntp[j] = 0; }
  for (int u0 = kb * (LS_THREADS * P); u0 < units; u0 += bpi * (LS_THREADS * P)) {
    float v[P][V], l[P][V];
    bool on[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const int u = u0 + k * LS_THREADS + threadIdx.x;
      on[k] = u < units;
      const int uc = on[k] ? u : units - 1;
      Pack<T, V>::load(px + (int64_t)uc * V, v[k]);
      Pack<float, V>::load(pl + (int64_t)uc * V, l[k]);
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float p = 1.f / (1.f + expf(-v[k][e]));
        const bool y = on[k] && l[k][e] != 0.f;                       // astype(bool): 255 and NaN count as set
        ngt += y;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const bool g = on[k] && p > thr.t[j];
          np[j] += g;
          ntp[j] += g && y;
        }
      }
    }
  }
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int a = wave_sum_i(np[j]), b = wave_sum_i(ntp[j]);
    if ((t & 63) == 0) { sh[t >> 6][j] = a; sh[t >> 6][NT + j] = b; }
  }
  ngt = wave_sum_i(ngt);
  if ((t & 63) == 0) { sh[t >> 6][2 * NT] = ngt; sh[t >> 6][2 * NT + 1] = 0; }
  __syncthreads();
  if (t < 32) ws[(int64_t)blockIdx.x * 32 + t] = sh[0][t] + sh[1][t] + sh[2][t] + sh[3][t];
}

// one workgroup: per image and threshold the exact counts, jaccard / precision / recall in double, added image by image
__global__ __launch_bounds__(256) void sal_finalize_kernel(const int32_t *__restrict__ ws, int B, int bpi, int64_t *__restrict__ state) {
  constexpr int CH = 16, NT = M3_METER_SAL_THRESHOLDS;                // 16 images x 15 thresholds of a round on 240 threads
  __shared__ double sh[CH][3 * NT];
  const int t = threadIdx.x, bl = t / NT, j = t - bl * NT;
  double acc = 0.0;
  for (int b0 = 0; b0 < B; b0 += CH) {
    const int b = b0 + bl;
    if (bl < CH && b < B) {
      long long tp = 0, npred = 0, ngt = 0;
      for (int q = 0; q < bpi; ++q) {
        const int32_t *w = ws + ((int64_t)b * bpi + q) * 32;
        npred += w[j]; tp += w[NT + j]; ngt += w[2 * NT];
      }
      sh[bl][j] = (ngt == 0 && npred == 0) ? 1.0 : (double)tp / (double)(ngt + npred - tp);
      sh[bl][NT + j] = (double)tp / ((double)npred + 1e-12);
      sh[bl][2 * NT + j] = (double)tp / ((double)ngt + 1e-12);
    }
    __syncthreads();
    if (t < 3 * NT) {
      const int cnt = B - b0 < CH ? B - b0 : CH;
      for (int q = 0; q < cnt; ++q) acc += sh[q][t];
    }
    __syncthreads();
  }
  if (t < 3 * NT) ((double *)state)[t] += acc;
  else if (t == 3 * NT) state[M3_METER_SAL_N_IMAGES] += B;
}

static inline int sal_blocks_per_image(int B, int HW) {
  const int cap = LS_MAX_BLOCKS / B, need = (HW + LS_THREADS * 2 - 1) / (LS_THREADS * 2);
  return need < cap ? need : (cap < 1 ? 1 : cap);
}

}  // namespace m3

using namespace m3;

extern "C" int64_t m3_meter_ws_elems(int kind, int64_t n, int aux) {
  if (n < 1) return 0;
  const int64_t nblk = blocks_for(n, LS_THREADS);
  if (kind == M3_METER_IOU) return (aux >= 1 && aux <= MT_BINS) ? nblk * 3 * aux : 0;
  if (kind == M3_METER_DEPTH) return nblk * 3;
  if (kind == M3_METER_NORMALS) return nblk * 6;
  if (kind == M3_METER_SAL) {
    if (aux < 1 || aux > LS_MAX_BLOCKS || n % aux != 0 || n / aux >= ((int64_t)1 << 31)) return 0;
    return (int64_t)32 * aux * sal_blocks_per_image(aux, (int)(n / aux));
  }
  return 0;
}

extern "C" int m3_meter_iou_update(const void *pred, int dtype, const void *label, int label_dtype, int B, int C, int H, int W,
                                   int layout, int n_classes, void *ws, void *state, void *stream) {
  LossShape sh;
  if (int rc = shape_ok(B, C, H, W, 2, 255, layout, dtype, "m3_meter_iou_update", &sh)) return rc;
  M3_REQUIRE(pred && label && ws && state, "m3_meter_iou_update: null pointer");
  M3_REQUIRE(label_dtype_ok(label_dtype), "m3_meter_iou_update: bad label dtype code %d", label_dtype);
  M3_REQUIRE(n_classes >= 1 && n_classes <= MT_BINS, "m3_meter_iou_update: n_classes = %d outside [1, %d]", n_classes, MT_BINS);
  hipStream_t s = (hipStream_t)stream;
  int32_t *w = (int32_t *)ws;
  int nblk;
  if (layout == M3_LAYOUT_NCHW) {
    const bool vec = aligned16(pred) && sh.HW % 4 == 0;
    const int units = vec ? sh.npix / 4 : sh.npix;
    nblk = blocks_for(units, LS_THREADS);
    by_dtype(dtype, [&](auto tt) {
      typedef typename decltype(tt)::type T;
      by_label(label_dtype, [&](auto lt) {
        auto go = [&](auto v) {
          hipLaunchKernelGGL((iou_planar_kernel<T, decltype(v)::value, decltype(lt)::value>), dim3(nblk), dim3(LS_THREADS), 0, s,
                             (const T *)pred, label, C, sh.HW, units, n_classes, w);
        };
        if (vec) go(IntTag<4>{}); else go(IntTag<1>{});
      });
    });
  } else {
    const bool vec = aligned16(pred) && C % 4 == 0;
    const int gsh = group_shift(vec ? C / 4 : C), ppw = 64 >> gsh;
    const int64_t steps = ((int64_t)sh.npix + ppw - 1) / ppw;
    nblk = blocks_for(steps, vec ? 16 : 4);                      // held to the blocks the workspace was sized for, as m3_loss_ce_fwd
    if (nblk > blocks_for(sh.n, LS_THREADS)) nblk = blocks_for(sh.n, LS_THREADS);
    by_dtype(dtype, [&](auto tt) {
      typedef typename decltype(tt)::type T;
      by_label(label_dtype, [&](auto lt) {
        constexpr int L = decltype(lt)::value;
        auto *kern = vec ? iou_cl4_kernel<T, L> : iou_cl1_kernel<T, L>;
        hipLaunchKernelGGL(kern, dim3(nblk), dim3(LS_THREADS), 0, s, (const T *)pred, label, C, sh.npix, gsh, n_classes, w);
      });
    });
  }
  if (int rc = check_launch("m3_meter_iou_update (partials)")) return rc;
  hipLaunchKernelGGL(iou_finalize_kernel, dim3(1), dim3(1024), 0, s, (const int32_t *)w, nblk, n_classes, (int64_t *)state);
  return check_launch("m3_meter_iou_update (finalize)");
}

extern "C" int m3_meter_depth_update(const void *pred, int dtype, const float *label, int B, int C, int H, int W, int layout,
                                     void *ws, void *state, void *stream) {
  LossShape sh;
  if (int rc = shape_ok(B, C, H, W, 1, 1 << 30, layout, dtype, "m3_meter_depth_update", &sh)) return rc;
  M3_REQUIRE(pred && label && ws && state, "m3_meter_depth_update: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = aligned16(pred) && aligned16(label) && sh.n % 4 == 0;
  const int units = (int)(vec ? sh.n / 4 : sh.n);
  const int nblk = blocks_for(units, LS_THREADS * 2);
  by_dtype(dtype, [&](auto tt) {
    typedef typename decltype(tt)::type T;
    auto go = [&](auto v) {
      hipLaunchKernelGGL((depth_kernel<T, decltype(v)::value>), dim3(nblk), dim3(LS_THREADS), 0, s, (const T *)pred, label, units,
                         (float *)ws);
    };
    if (vec) go(IntTag<4>{}); else go(IntTag<1>{});
  });
  if (int rc = check_launch("m3_meter_depth_update (partials)")) return rc;
  hipLaunchKernelGGL((sums_finalize_kernel<2, 1>), dim3(1), dim3(256), 0, s, (const float *)ws, nblk, (int64_t *)state);
  return check_launch("m3_meter_depth_update (finalize)");
}

extern "C" int m3_meter_normals_update(const void *pred, int dtype, const float *label, int B, int H, int W, int layout,
                                       int label_layout, void *ws, void *state, void *stream) {
  LossShape sh;
  if (int rc = shape_ok(B, 3, H, W, 3, 3, layout, dtype, "m3_meter_normals_update", &sh)) return rc;
  M3_REQUIRE(label_layout == M3_LAYOUT_NCHW || label_layout == M3_LAYOUT_NHWC, "m3_meter_normals_update: bad label layout %d", label_layout);
  M3_REQUIRE(pred && label && ws && state, "m3_meter_normals_update: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int HW = sh.HW;
  const int xsp = layout == M3_LAYOUT_NCHW ? 1 : 3, xsc = layout == M3_LAYOUT_NCHW ? HW : 1;
  const int lsp = label_layout == M3_LAYOUT_NCHW ? 1 : 3, lsc = label_layout == M3_LAYOUT_NCHW ? HW : 1;
  const int nblk = blocks_for(sh.npix, LS_THREADS);
  by_dtype(dtype, [&](auto tt) {
    typedef typename decltype(tt)::type T;
    hipLaunchKernelGGL((normals_meter_kernel<T>), dim3(nblk), dim3(LS_THREADS), 0, s, (const T *)pred, label, HW, sh.npix, xsp, xsc,
                       lsp, lsc, (float *)ws);
  });
  if (int rc = check_launch("m3_meter_normals_update (partials)")) return rc;
  hipLaunchKernelGGL((sums_finalize_kernel<2, 4>), dim3(1), dim3(256), 0, s, (const float *)ws, nblk, (int64_t *)state);
  return check_launch("m3_meter_normals_update (finalize)");
}

extern "C" int m3_meter_sal_update(const void *pred, int dtype, const float *label, int B, int H, int W, void *ws, void *state,
                                   void *stream) {
  LossShape sh;
  if (int rc = shape_ok(B, 1, H, W, 1, 1, M3_LAYOUT_NCHW, dtype, "m3_meter_sal_update", &sh)) return rc;
  M3_REQUIRE(B <= LS_MAX_BLOCKS, "m3_meter_sal_update: B = %d above %d images per update", B, LS_MAX_BLOCKS);
  M3_REQUIRE(pred && label && ws && state, "m3_meter_sal_update: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int HW = sh.HW, bpi = sal_blocks_per_image(B, HW);
  const bool vec = aligned16(pred) && aligned16(label) && HW % 4 == 0;
  SalThresholds thr;                                             // np.linspace(0.2, 0.9, 15), compared in fp32 as torch does
  for (int j = 0; j < M3_METER_SAL_THRESHOLDS; ++j) thr.t[j] = (float)(0.2 + j * ((0.9 - 0.2) / (M3_METER_SAL_THRESHOLDS - 1)));
  thr.t[M3_METER_SAL_THRESHOLDS - 1] = 0.9f;
  by_dtype(dtype, [&](auto tt) {
    typedef typename decltype(tt)::type T;
    auto go = [&](auto v) {
      hipLaunchKernelGGL((sal_kernel<T, decltype(v)::value>), dim3(B * bpi), dim3(LS_THREADS), 0, s, (const T *)pred, label, HW, bpi,
                         thr, (int32_t *)ws);
    };
    if (vec) go(IntTag<4>{}); else go(IntTag<1>{});
  });
  if (int rc = check_launch("m3_meter_sal_update (partials)")) return rc;
  hipLaunchKernelGGL(sal_finalize_kernel, dim3(1), dim3(256), 0, s, (const int32_t *)ws, B, bpi, (int64_t *)state);
  return check_launch("m3_meter_sal_update (finalize)");
}
