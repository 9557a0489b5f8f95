// Weight-gradient GEMM ("TN": contraction over token rows) for gfx950, grouped or dense:
//   dW[g][n,k] = sum_{m in group g} dC[crow(m), n] * A[arow(m), k]
//
// Replaces fastmoe's linear_backward weight/bias part behind FMoELinear
// (models/moe/ckpt/custom_moe_layer.py:32-33) and the nn.Linear weight grads of the
// attention block / dense Mlp (models/moe/ckpt/vision_transformer_moe.py:255-261,295-313);
// the reference's torch-only twin is ParallelLinear.backward
// (models/moe/parallel_experts.py:51-82: d_weight = input^T grad, d_bias = sum grad).
//
// This file: the entry points, the launch plan, the choice of the kernel that takes a call, the slab reductions, the column
// sums and the streaming kernel for the router's weight.  The tile kernels live with their launchers in wgrad_staged.hip
// (register-staged, 128 x 128), wgrad_multi.hip (several dense weights in one launch) and wgrad_dma.hip (LDS-DMA, 128 x 128 and
// 256 x 256), all compiled through wgrad_tiles.hip; wgrad_dev.h holds what they share.
#include "wgrad_dev.h"
#include <algorithm>

namespace m3 {

// ------------------------------------------------------------------------------------------------
// Skinny weight gradient: dW [N, K] with K = 16 or 32 - the router's w_gate (custom_moe_layer.py:213-217:
// dW_gate = h^T d_logits, K = num_experts), no gathers, no bias, one group.  A 128 x 128 MFMA tile pads K to 128: seven of
// eight MFMAs multiply zeros and every A-side DMA piece takes the clamped tail path (25 us fp16 / 112 us fp32 per launch at
// M = 25 216, N = 384 for 0.3 GFLOP).  Here the call is what it is, a stream over dC: lane = two columns n of a 128-wide
// column tile, the 16 k of the wave's slice in registers (32 fp32 accumulators), the A row - the same for every lane - read
// by scalar loads, one fma per (row, n, k).  The four waves of a workgroup take interleaved rows (K = 16) or two k slices x
// two row phases (K = 32) and add up through LDS; a workgroup's [128, K] block goes to its slab exactly like a 128 x 128
// kernel's (same layout, same reduction riding on the next launch).
template <typename T, int KP>
__global__ __launch_bounds__(WG_THREADS) void wgrad_skinny_kernel(const WgradDev p) {
  constexpr int KS = KP / 16, PH = 4 / KS, UNR = 16;
  constexpr int ES = (int)sizeof(T);
  __shared__ float sred[4][64][2][16];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bz, gz;
  if (wgrad_ride_along(p, tid, bz, gz)) return;
  const int ks = wave % KS, ph = wave / KS;
  const int n0 = blockIdx.x * WG_T;
  int n = n0 + 2 * lane;
  if (n > p.N - 2) n = p.N - 2;                       // clamped columns are computed and never stored
  const int64_t per = (p.M + p.splits - 1) / p.splits;
  const int64_t r0 = (int64_t)bz * per, r1 = (r0 + per < p.M) ? r0 + per : p.M;
  typedef T t2 __attribute__((ext_vector_type(2)));
  typedef T t16 __attribute__((ext_vector_type(16)));
  float acc[2][16];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[j][k] = 0.f;
  const char *cb = p.dC + (int64_t)n * ES;
  const char *ab = p.A + (int64_t)ks * 16 * ES;
  // batches of 16 rows (row u of a batch: m + u * PH), every load of a batch issued before its first use.  The A rows - the
  // same for every lane - are loaded by lanes 0..15 (lane u: row u of the batch, converted to fp32 there) and handed out by
  // v_readlane: 16 scalar operands per row.  Addresses: one 64-bit base per batch + 32-bit row offsets; the last, partial
  // batch clamps its rows to the last valid one and zeroes their dC values.
  const uint32_t ldc = (uint32_t)p.lddc_b, lda = (uint32_t)p.lda_b;
  auto batch = [&](const char *cm, const char *am, int cnt, auto full) {
    constexpr bool FULL = decltype(full)::value;
    t2 c[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int uu = FULL ? u : (u < cnt ? u : cnt - 1);
      c[u] = *(const t2 *)(cm + (uint32_t)(uu * PH) * ldc);
    }
    const int ua = FULL ? (lane & 15) : ((lane & 15) < cnt ? (lane & 15) : cnt - 1);
    const t16 ar = *(const t16 *)(am + (uint32_t)(ua * PH) * lda);
    float af[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) af[k] = (float)ar[k];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const bool ok = FULL || u < cnt;                                   // wave-uniform
      const float c0 = ok ? (float)c[u][0] : 0.f, c1 = ok ? (float)c[u][1] : 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const float a = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, af[k]), u));
        acc[0][k] = __builtin_fmaf(c0, a, acc[0][k]);
        acc[1][k] = __builtin_fmaf(c1, a, acc[1][k]);
      }
    }
  };
  int64_t m = r0 + ph;
  const char *cm = cb + m * p.lddc_b, *am = ab + m * p.lda_b;
  for (; m + (int64_t)(UNR - 1) * PH < r1; m += (int64_t)UNR * PH) {
    batch(cm, am, UNR, std::true_type{});
    cm += (int64_t)UNR * PH * p.lddc_b; am += (int64_t)UNR * PH * p.lda_b;
  }
  if (m < r1) batch(cm, am, (int)((r1 - m + PH - 1) / PH), std::false_type{});
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int k = 0; k < 16; ++k) sred[wave][lane][j][k] = acc[j][k];
  __syncthreads();
  float *out = p.ws + (int64_t)bz * p.N * p.K;
  for (int i = tid; i < WG_T * KP; i += WG_THREADS) {
    const int nl = i / KP, k = i - nl * KP;
    if (n0 + nl >= p.N) continue;
    const int sl = k >> 4, kk = k & 15;
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < PH; ++q) v += sred[q * KS + sl][nl >> 1][nl & 1][kk];
    out[(int64_t)(n0 + nl) * p.K + k] = v;
  }
}

// the slab reductions as launches of their own (wgrad_dev.h has the blocks: they also ride in front of the 128-wide kernels)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *ws, int splits, int64_t elems4, float *dW, int beta, int nb_w,
                                                           const float *bias_ws, int64_t belems4, float *db, int beta_db, int cols) {
  wgrad_reduce_block(blockIdx.x, threadIdx.x, ws, splits, elems4, dW, beta, nb_w, bias_ws, belems4, db, beta_db, cols);
}
__global__ __launch_bounds__(256) void wgrad_reduce_grouped_kernel(const float *ws, const int32_t *off, int G, int chunk, int64_t elems4,
                                                                   float *dW, int beta, int nb_w, const float *bias_ws, int64_t belems4,
                                                                   float *db, int beta_db) {
  wgrad_reduce_grouped_block(blockIdx.x, blockIdx.y, threadIdx.x, ws, off, G, chunk, elems4, dW, beta, nb_w, bias_ws, belems4, db, beta_db);
}

// the reductions a batched launch leaves behind (p.rd_n > 1, WgradDev.rd_tab0 ..) as a launch of their own: every block a reduce block
__global__ __launch_bounds__(256) void wgrad_reduce_multi_kernel(const WgradDev p) {
  int bz, gz;
  (void)wgrad_ride_along(p, threadIdx.x, bz, gz);
}

// ------------------------------------------------------------------ column sums
// db[g][n] = sum over rows of group g of dC[crow(m), n].  Stage 1: grid (column blocks,
// strips per group, groups); a workgroup is 64 column chunks (16 B each) x 4 row lanes and
// streams its strip of rows with coalesced 16-byte loads; stage 2 (reduce.hip) adds the strip
// partials in a fixed order.
template <typename T>
__global__ __launch_bounds__(256) void colsum_part_kernel(const char *__restrict__ dC, int64_t lddc_b,
                                                          const int32_t *__restrict__ c_row_idx, int64_t M, int N,
                                                          const int32_t *__restrict__ group_offsets, int spg,
                                                          float *__restrict__ part) {
  constexpr int ES = (int)sizeof(T), EPC = 16 / ES;
  __shared__ float sred[4][64][EPC + 1];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int col = (blockIdx.x * 64 + cl) * EPC;
  const int strip = blockIdx.y, g = blockIdx.z;
  int64_t r0 = 0, r1 = M;
  if (group_offsets) { r0 = group_offsets[g]; r1 = group_offsets[g + 1]; }
  const int64_t per = ((r1 - r0) + spg - 1) / spg;
  const int64_t b0 = r0 + (int64_t)strip * per;
  int64_t b1 = b0 + per;
  if (b1 > r1) b1 = r1;
  float acc[EPC];
#pragma unroll
  for (int j = 0; j < EPC; ++j) acc[j] = 0.f;
  if (col < N) {
#pragma unroll 4
    for (int64_t m = b0 + rl; m < b1; m += 4) {
      const int64_t cr = c_row_idx ? (int64_t)c_row_idx[m] : m;
      const u32x4 raw = *(const u32x4 *)(dC + cr * lddc_b + (int64_t)col * ES);
      const T *e = (const T *)&raw;
#pragma unroll
      for (int j = 0; j < EPC; ++j) acc[j] += (float)e[j];
    }
  }
#pragma unroll
  for (int j = 0; j < EPC; ++j) sred[rl][cl][j] = acc[j];
  __syncthreads();
  if (rl == 0 && col < N) {
    float *o = part + ((int64_t)g * spg + strip) * N + col;
#pragma unroll
    for (int j = 0; j < EPC; ++j) o[j] = sred[0][cl][j] + sred[1][cl][j] + sred[2][cl][j] + sred[3][cl][j];
  }
}

static int colsum_strips_per_group(int64_t M, int G) {
  int64_t per_group = (M + G - 1) / G;
  int64_t s = (per_group + 127) / 128;
  if (s < 1) s = 1;
  if (s > 512) s = 512;
  return (int)s;
}

}  // namespace m3

using namespace m3;

// f(tag) with tag.type = the element type of `dtype`
template <typename T> struct TypeTag { typedef T type; };
template <typename F> static inline void for_dtype(int dtype, F &&f) {
  if (dtype == M3_F16) f(TypeTag<half_t>{});
  else if (dtype == M3_BF16) f(TypeTag<bf16_t>{});
  else f(TypeTag<float>{});
}

static int g_wgrad_dma = -1;
extern "C" int m3_wgrad_set_dma(int on) {
  M3_REQUIRE(on >= -1 && on <= 2, "m3_wgrad_set_dma: %d", on);
  g_wgrad_dma = on;
  return M3_OK;
}
// m3_wgrad_set_dma's rule for a launch of 128 x 128 tiles: 0 never, 2 always, 1 (default) where the LDS-DMA kernel measured
// faster with operands streamed from HBM as inside the training step (tools/wgrad_ab_bench.py,
// profiles/r05_wgrad_ab_streamed.txt): fp32 always (-12..-26 %); 16-bit when the launch has one part per group anyway - tiles x
// groups fill the 1024 workgroup slots: direct accumulation, the ViT-Base experts, -35 % - or the weight is large (N K >= 1.5 M
// elements: ViT-Base qkv / fc1 / fc2, -10..-24 %); at configs[1]'s 384-wide weights the register-staged kernel is level or
// ahead (+-5 %) and keeps them.  m3_wgrad_plan counts workgroup slots by it; m3_wgrad_tn also asks whether the kernel can run
// the call.
static bool wgrad_dma_pays(int N, int K, int G, int dtype) {
  if (g_wgrad_dma < 0) { const char *e = getenv("M3_WGRAD_DMA"); g_wgrad_dma = e ? atoi(e) : 1; }
  if (g_wgrad_dma != 1) return g_wgrad_dma == 2;
  const int64_t tiles = (int64_t)((N + WG_T - 1) / WG_T) * ((K + WG_T - 1) / WG_T) * G;
  return dtype == M3_F32 || (int64_t)N * K >= 1500000 || tiles >= 1024;
}

static int g_wgrad_big = -1;
extern "C" int m3_wgrad_set_big(int on) {
  M3_REQUIRE(on >= -1 && on <= 1, "m3_wgrad_set_big: %d", on);
  g_wgrad_big = on;
  return M3_OK;
}
static bool wgrad_big_shape(int N, int K, int dtype) {
  if (g_wgrad_big < 0) { const char *e = getenv("M3_WGRAD_BIG"); g_wgrad_big = e ? (atoi(e) ? 1 : 0) : 1; }
  return g_wgrad_big && dtype != M3_F32 && N % BG_T == 0 && K % BG_T == 0;
}

extern "C" int m3_wgrad_skinny(int N, int K, int G) { return G == 1 && (K == 16 || K == 32) && N % 2 == 0 && N >= 2; }

// The kernel a shape gets under the current m3_wgrad_set_dma / m3_wgrad_set_big settings: what m3_wgrad_plan sizes the parts
// for, m3_wgrad_tile reports the tile of, and m3_wgrad_tn launches unless the call needs something that kernel has not
// (wgrad_demote).  The streaming and the 256 x 256 shapes are disjoint (K = 16 / 32 against K a multiple of 256).
static WgradKernel wgrad_tile128_kernel(int N, int K, int G, int dtype) { return wgrad_dma_pays(N, K, G, dtype) ? WGRAD_DMA : WGRAD_STAGED; }
static WgradKernel wgrad_kernel_of_shape(int N, int K, int G, int dtype) {
  if (m3_wgrad_skinny(N, K, G)) return WGRAD_SKINNY;
  if (wgrad_big_shape(N, K, dtype)) return WGRAD_BIG;
  return wgrad_tile128_kernel(N, K, G, dtype);
}

// the output tile (n x k) m3_wgrad_tn uses for a shape: 256 x 256 for the 16-bit shapes the big-tile kernel takes, else
// 128 x 128 (m3_wgrad_plan sizes `splits` / `units` for ceil(N / tn) * ceil(K / tk) tiles per group).
extern "C" int m3_wgrad_tile(int N, int K, int dtype, int *tn, int *tk) {
  M3_REQUIRE(tn && tk, "m3_wgrad_tile: null output");
  *tn = *tk = wgrad_kernel_of_shape(N, K, 1, dtype) == WGRAD_BIG ? BG_T : WG_T;      // (the big-tile rule does not look at G)
  return M3_OK;
}

// Row parts of a dense call in whole multiples of the 8 XCDs where that costs at most 1/8 of the parts: the tiles of a part
// read the same rows, and the XCD remap hands every XCD an equal run of consecutive workgroups - with a multiple of 8 parts no
// part straddles two XCDs (its rows then come into one L2, not two).
static int64_t wgrad_whole_xcds(int64_t splits) {
  const int64_t down = splits - splits % 8;
  return splits >= 8 && 8 * down >= 7 * splits ? down : splits;
}

// The row parts the library cuts a call into by itself, for the kernel m3_wgrad_tn will take
static int64_t wgrad_default_splits(int64_t M, int N, int K, int G, int dtype) {
  const WgradKernel kern = wgrad_kernel_of_shape(N, K, G, dtype);
  if (kern == WGRAD_SKINNY) return std::max<int64_t>(1, std::min<int64_t>(256, M / 64));   // a stream over dC, 64+ rows per part (16 per wave)
  const bool big = kern == WGRAD_BIG;
  const int t = big ? BG_T : WG_T;
  const int64_t tiles = (int64_t)((N + t - 1) / t) * ((K + t - 1) / t) * G;
  // at least 16 32-row steps per part, so that short contractions (few tokens) do not pay a 64 KiB slab write + reduce per
  // handful of steps (measured on the 8-image configs; no effect at batch 128)
  const int64_t steps = std::max<int64_t>(1, (M / G + 31) / 32), cap = std::max<int64_t>(1, steps / 16);
  int64_t sp;
  if (!big) {
    // 128 x 128 tiles: fill the resident workgroup slots exactly once (the LDS-DMA kernel runs four workgroups per CU, the
    // register-staged one two) - more parts only add slab traffic and a ragged second wave of workgroups.  fp32 is MFMA-bound
    // (1/16 of the fp16 rate): its slots matter more than its slab bytes, so small weights (proj: 9 tiles) may be cut into as
    // many parts as fill them; 16-bit stays at 32 (slab traffic; 44 / 56 measured level to +0.5 % at configs[1])
    const int64_t slots = kern == WGRAD_DMA ? 1024 : 512, most = dtype == M3_F32 ? 128 : 32;
    sp = std::min(std::min(cap, most), tiles <= slots ? slots / tiles : 1);
  } else {
    // 256 x 256 tiles, one 8-wave workgroup per CU: fill the 256 slots once; with more tiles than slots (grouped experts) one
    // part per group - the kernel then accumulates into dW itself (direct mode), no slabs
    sp = tiles < 256 ? std::min(std::min<int64_t>(cap, 32), 256 / tiles) : 1;
  }
  sp = std::max<int64_t>(1, sp);
  return G == 1 ? wgrad_whole_xcds(sp) : sp;
}

extern "C" int m3_wgrad_plan(const m3_wgrad_shape *s, m3_wgrad_plan_out *p) {
  M3_REQUIRE(s && p, "m3_wgrad_plan: null argument");
  M3_REQUIRE(dtype_ok(s->dtype), "m3_wgrad_plan: bad dtype");
  M3_REQUIRE(s->N > 0 && s->K > 0 && s->M >= 0 && s->M < ((int64_t)1 << 31) && s->G >= 1 && s->splits >= 0, "m3_wgrad_plan: bad shape");
  const int64_t M = s->M, G = s->G;
  const int64_t sp = s->splits ? s->splits : wgrad_default_splits(M, s->N, s->K, s->G, s->dtype);
  // direct mode: with ONE part per group every (group, tile) belongs to one workgroup, which adds its tile into dW itself.  The
  // rule above says 1 exactly when the tiles alone fill the chip (the ViT-Base experts: 2304 tiles, 151 MB of gradient per layer)
  const bool direct = s->direct_ok && sp == 1;
  // grouped calls: work units of equal row counts dealt to the groups by their (device-resident) sizes, so that a hot expert
  // gets more workgroups instead of longer ones; `splits` is the average number of units per group and the chunk sits 1/8
  // above the mean part, so that groups near the mean keep `splits` units
  int64_t chunk = 0, units = sp * G;
  if (s->grouped && !direct && G > 1 && G <= 64 && M > 0) {
    const int64_t part = (M * 9 + 8 * sp * G - 1) / (8 * sp * G);
    chunk = std::max<int64_t>(64, (part + 63) / 64 * 64);
    units = M / chunk + G;
  }
  M3_REQUIRE(units <= INT32_MAX, "m3_wgrad_plan: %lld slab slots", (long long)units);
  p->splits = (int32_t)sp; p->chunk_rows = (int32_t)chunk; p->units = (int32_t)units; p->direct = direct;
  p->ws_elems = direct ? 0 : units * s->N * (s->K + (s->bias ? 1 : 0));
  return M3_OK;
}

// The unit map of a balanced grouped call on the host: the groups walked in order with the two rules the kernels use
// (wgrad_dev.h: wgrad_units_of_group, wgrad_unit_rows)
extern "C" int m3_wgrad_unit_of(const int32_t *group_offsets, int G, int chunk_rows, int unit, int *group, int *row_begin,
                                int *row_end) {
  M3_REQUIRE(group_offsets && group && row_begin && row_end, "m3_wgrad_unit_of: null argument");
  M3_REQUIRE(G >= 1 && G <= 64 && chunk_rows >= WG_ROWS && chunk_rows % WG_ROWS == 0 && unit >= 0,
             "m3_wgrad_unit_of: needs 1 <= G <= 64, chunk_rows a multiple of %d and unit >= 0", WG_ROWS);
  *group = -1; *row_begin = *row_end = 0;
  int first = 0;
  for (int g = 0; g < G; ++g) {
    const int rows = group_offsets[g + 1] - group_offsets[g];
    M3_REQUIRE(rows >= 0, "m3_wgrad_unit_of: group_offsets decrease at group %d", g);
    const int n = wgrad_units_of_group(rows, chunk_rows);
    if (unit < first + n) {
      int b, e;
      wgrad_unit_rows(rows, n, unit - first, b, e);
      *group = g; *row_begin = group_offsets[g] + b; *row_end = group_offsets[g] + e;
      return M3_OK;
    }
    first += n;
  }
  return M3_OK;                                      // a surplus unit: the launch's workgroups of this id have no work
}

// ------------------------------------------------------------------ slab reductions
// 16-byte columns per block of the dense slab reduction: four threads per column from 32 slabs on
static inline int m3_wgrad_reduce_cols(int splits) { return splits >= 32 ? 64 : 256; }

// a slab reduction (plain: chunk_rows == 0, grouped: > 0) as its blocks see it, in a launch of their own or in front of the next one
struct WgradReduceGeom { int64_t e4, b4; int cols, nb_w, nb_b; };
static WgradReduceGeom wgrad_reduce_geom(const m3_wgrad_reduce_desc &r) {
  const int64_t e4 = r.elems / 4, b4 = r.bias_ws ? r.bias_elems / 4 : 0;
  const int cols = r.chunk_rows ? 256 : m3_wgrad_reduce_cols(r.splits);
  return WgradReduceGeom{e4, b4, cols, (int)((e4 + cols - 1) / cols), (int)((b4 + cols - 1) / cols)};
}
static bool wgrad_reduce_desc_ok(const m3_wgrad_reduce_desc &r) {
  return r.ws && r.dW && r.elems >= 0 && r.elems % 4 == 0 &&
         (r.chunk_rows == 0 ? r.splits >= 1 : (r.group_offsets && r.G >= 1 && r.G <= 64));
}
static bool wgrad_reduce_bias_ok(const m3_wgrad_reduce_desc &r) { return !r.bias_ws || (r.db && r.bias_elems > 0 && r.bias_elems % 4 == 0); }
// checks a reduction and launches it, plain or grouped as the descriptor says
static int wgrad_reduce_launch(const m3_wgrad_reduce_desc &r, hipStream_t s) {
  const char *who = r.chunk_rows ? "m3_wgrad_reduce_grouped" : "m3_wgrad_reduce";
  M3_REQUIRE(wgrad_reduce_desc_ok(r) && r.chunk_rows >= 0, "%s: bad args", who);
  M3_REQUIRE(((uintptr_t)r.ws % 16) == 0 && ((uintptr_t)r.dW % 16) == 0, "%s: alignment", who);
  M3_REQUIRE(wgrad_reduce_bias_ok(r) && (!r.bias_ws || (((uintptr_t)r.bias_ws % 16) == 0 && ((uintptr_t)r.db % 16) == 0)),
             "%s: bias slabs need db, 16-byte alignment and a multiple of 4 elements", who);
  if (r.elems == 0) return M3_OK;
  const WgradReduceGeom g = wgrad_reduce_geom(r);
  if (r.chunk_rows)
    hipLaunchKernelGGL(wgrad_reduce_grouped_kernel, dim3((unsigned)(g.nb_w + g.nb_b), (unsigned)r.G), dim3(256), 0, s, r.ws,
                       r.group_offsets, r.G, r.chunk_rows, g.e4, r.dW, r.beta, g.nb_w, r.bias_ws, g.b4, r.db, r.beta_db);
  else
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)(g.nb_w + g.nb_b)), dim3(256), 0, s, r.ws, r.splits, g.e4, r.dW,
                       r.beta, g.nb_w, r.bias_ws, g.b4, r.db, r.beta_db, g.cols);
  return check_launch(who);
}

extern "C" int m3_wgrad_reduce(const float *ws, int splits, int64_t elems, float *dW, int beta, const float *bias_ws,
                               int64_t bias_elems, float *db, int beta_db, void *stream) {
  const m3_wgrad_reduce_desc r = {ws, splits, elems, nullptr, 0, 0, dW, beta, bias_ws, bias_elems, db, beta_db};
  return wgrad_reduce_launch(r, (hipStream_t)stream);
}

extern "C" int m3_wgrad_reduce_grouped(const float *ws, const int32_t *group_offsets, int G, int chunk_rows, int64_t elems,
                                       float *dW, int beta, const float *bias_ws, int64_t bias_elems, float *db,
                                       int beta_db, void *stream) {
  M3_REQUIRE(chunk_rows >= 1, "m3_wgrad_reduce_grouped: bad args");
  const m3_wgrad_reduce_desc r = {ws, 0, elems, group_offsets, G, chunk_rows, dW, beta, bias_ws, bias_elems, db, beta_db};
  return wgrad_reduce_launch(r, (hipStream_t)stream);
}

extern "C" int m3_wgrad_bias_reduce(const float *bias_ws, int splits, int64_t elems, float *db, int beta, void *stream) {
  M3_REQUIRE(bias_ws && db && splits >= 1 && elems > 0 && elems < ((int64_t)1 << 31), "m3_wgrad_bias_reduce: bad args");
  return launch_reduce_rows_f32(bias_ws, splits, (int)elems, 1, 0, db, beta, (hipStream_t)stream);
}

// The reductions of a batched launch (m3_wgrad_multi: n > 1 dense descriptors of the same number of slabs) as the kernels take
// them: WgradDev.rd_tab0 .., the reduce blocks of problem after problem
static int wgrad_fill_rd_multi(WgradDev &d, const m3_wgrad_reduce_desc *r, int n, const char *who) {
  M3_REQUIRE(n >= 2 && n <= WG_MULTI, "%s: %d reductions in one descriptor table (2 .. %d)", who, n, WG_MULTI);
  WgradRdProb *tab = &d.rd_tab0;
  int first = 0;
  for (int j = 0; j < WG_MULTI; ++j) {
    tab[j] = WgradRdProb{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, INT32_MAX, 0};
    if (j >= n) continue;
    M3_REQUIRE(wgrad_reduce_desc_ok(r[j]) && wgrad_reduce_bias_ok(r[j]) && r[j].chunk_rows == 0 && r[j].elems > 0 && r[j].splits == r[0].splits,
               "%s: a table of reductions holds dense ones of the same number of slabs", who);
    M3_REQUIRE(((uintptr_t)r[j].ws % 16) == 0 && ((uintptr_t)r[j].dW % 16) == 0 &&
               (!r[j].bias_ws || (((uintptr_t)r[j].bias_ws % 16) == 0 && ((uintptr_t)r[j].db % 16) == 0)), "%s: reduction alignment", who);
    const WgradReduceGeom g = wgrad_reduce_geom(r[j]);
    tab[j] = WgradRdProb{r[j].ws, r[j].dW, r[j].bias_ws, r[j].db, g.e4, (int32_t)g.b4, g.nb_w, first, (r[j].beta ? 1 : 0) | (r[j].beta_db ? 2 : 0)};
    first += g.nb_w + g.nb_b;
  }
  d.rd_n = n; d.rd_blocks = first; d.rd_nbx = first; d.rd_nbw = 0; d.rd_chunk = 0;
  d.rd_splits = r[0].splits; d.rd_cols = m3_wgrad_reduce_cols(r[0].splits);
  return M3_OK;
}

extern "C" int m3_wgrad_reduce_multi(const m3_wgrad_reduce_desc *descs, int n, void *stream) {
  M3_REQUIRE(descs && n >= 1, "m3_wgrad_reduce_multi: bad args");
  if (n == 1) return wgrad_reduce_launch(descs[0], (hipStream_t)stream);
  WgradDev d = {};
  if (int rc = wgrad_fill_rd_multi(d, descs, n, "m3_wgrad_reduce_multi")) return rc;
  d.rd_zslices = 1;
  hipLaunchKernelGGL(wgrad_reduce_multi_kernel, dim3((unsigned)d.rd_blocks), dim3(256), 0, (hipStream_t)stream, d);
  return check_launch("m3_wgrad_reduce_multi");
}

// The previous call's slab reduction(s) (prev[0 .. n_prev)) for a launch with the argument block d: into d.rd_*, to ride in
// front of that launch - or, where the launch cannot carry them (own_launch), launched here
static int wgrad_take_prev(WgradDev &d, const m3_wgrad_reduce_desc *prev, int n_prev, const float *ws, bool own_launch, hipStream_t s,
                           const char *who) {
  d.rd_blocks = 0; d.rd_zslices = 0; d.rd_cols = 256; d.rd_n = 0;
  if (!prev) return M3_OK;
  const int n = n_prev > 1 ? n_prev : 1;
  M3_REQUIRE(n <= WG_MULTI, "%s: n_prev %d", who, n);
  for (int j = 0; j < n; ++j) {
    M3_REQUIRE(wgrad_reduce_desc_ok(prev[j]), "%s: bad prev reduce descriptor", who);
    M3_REQUIRE(wgrad_reduce_bias_ok(prev[j]), "%s: prev bias slabs need db", who);
    M3_REQUIRE(prev[j].ws != ws, "%s: prev slabs and this call's slabs must be different buffers", who);
  }
  if (n > 1) {
    if (own_launch) return m3_wgrad_reduce_multi(prev, n, s);
    return wgrad_fill_rd_multi(d, prev, n, who);
  }
  const m3_wgrad_reduce_desc *r = prev;
  if (r->elems > 0) {
    if (own_launch) return wgrad_reduce_launch(*r, s);
    const WgradReduceGeom g = wgrad_reduce_geom(*r);
    d.rd_cols = g.cols; d.rd_nbw = g.nb_w; d.rd_nbx = g.nb_w + g.nb_b;
    d.rd_blocks = d.rd_nbx * (r->chunk_rows ? r->G : 1);
    d.rd_ws = r->ws; d.rd_splits = r->splits; d.rd_e4 = g.e4; d.rd_off = r->group_offsets; d.rd_G = r->G; d.rd_chunk = r->chunk_rows;
    d.rd_dW = r->dW; d.rd_beta = r->beta; d.rd_bws = r->bias_ws; d.rd_b4 = g.b4; d.rd_db = r->db; d.rd_beta_db = r->beta_db;
  }
  return M3_OK;
}
// the grid's leading z slices for the reduce blocks d carries
static void wgrad_prev_slices(WgradDev &d, dim3 &grid) {
  if (d.rd_blocks <= 0) return;
  const int per_slice = (int)(grid.x * grid.y);
  d.rd_zslices = (d.rd_blocks + per_slice - 1) / per_slice;
  grid.z += d.rd_zslices;
}

// ------------------------------------------------------------------ the weight-gradient call
// Every operand row within the 32-bit offsets a lane adds to the operand base.  M + 1 rows: a whole row past the last one, so
// that row offset + column offset stays below 2^32; gathered source rows must be < M
static bool wgrad_within_reach(const m3_wgrad_args *a, const WgradDev &d) {
  return (a->M + 1) * d.lddc_b < ((int64_t)1 << 32) && (a->M + 1) * d.lda_b < ((int64_t)1 << 32);
}
// "The LDS-DMA form can run this call" (both wgrad_dma.hip kernels): power-of-two gather divisors (the kernels shift), every
// operand row within reach, and a per-row factor only on gathered rows of a dtype whose instances multiply it in: fp16, and
// fp32 where the family has it (sc_f32: the 128 x 128 kernel)
static bool wgrad_dma_form(const m3_wgrad_args *a, const WgradDev &d, bool sc_f32) {
  const bool sc_ok = !a->c_row_scale || (a->c_row_idx && (a->dtype == M3_F16 || (sc_f32 && a->dtype == M3_F32)));
  return sc_ok && d.a_row_sh >= 0 && d.c_row_sh >= 0 && wgrad_within_reach(a, d);
}
// A call the shape's kernel cannot run steps down: 256 x 256 tiles (the caller sized `splits` / `units` for that tile count;
// any kernel works with them) and the streaming kernel (plain rows only: m3_wgrad_skinny reports the rule to the caller, who
// sizes `splits` for it) to the 128 x 128 kernel m3_wgrad_set_dma's rule names, the LDS-DMA one of those to the register-staged
// kernel, which takes everything.  The streaming kernel adds a 32-bit (row in the batch) x stride product, up to 60 rows, to a
// batch's base: inside the 4 GiB reach a batch's rows are rows of the call and the product cannot wrap; past it, it can
static WgradKernel wgrad_demote(WgradKernel kern, const m3_wgrad_args *a, const WgradDev &d) {
  const bool plain = !a->c_row_idx && !a->a_row_idx && !a->c_row_scale && !a->bias_ws && !a->chunk_rows && !a->direct_dW;
  if ((kern == WGRAD_BIG && !wgrad_dma_form(a, d, false)) || (kern == WGRAD_SKINNY && !(plain && wgrad_within_reach(a, d))))
    kern = wgrad_tile128_kernel(a->N, a->K, a->G, a->dtype);
  if (kern == WGRAD_DMA && !wgrad_dma_form(a, d, true)) kern = WGRAD_STAGED;
  return kern;
}

// What m3_wgrad_tn does with a call before it launches anything: the checks of the call itself, the kernels' argument block
// (pointers are copied, never read) and the kernel after wgrad_demote.  m3_wgrad_tn launches from it, m3_wgrad_kernel reports it.
// (The descriptors behind a->prev do not enter the choice: the launch checks them, wgrad_take_prev.)
static int wgrad_prepare(const m3_wgrad_args *a, const char *who, WgradDev &d, WgradKernel &kern) {
  M3_REQUIRE(a && a->dC && a->A && (a->ws || a->direct_dW), "%s: null operand", who);
  M3_REQUIRE(dtype_ok(a->dtype), "%s: bad dtype", who);
  const int es = dtype_size(a->dtype);
  M3_REQUIRE(a->N > 0 && a->K > 0 && a->M >= 0 && a->G >= 1 && a->splits >= 1, "%s: bad shape", who);
  M3_REQUIRE(a->M < ((int64_t)1 << 31), "%s: M exceeds the 32-bit row indices", who);
  M3_REQUIRE((a->N * es) % 16 == 0 && (a->K * es) % 16 == 0, "%s: N*elem and K*elem must be multiples of 16 bytes", who);
  M3_REQUIRE((a->lddc * es) % 16 == 0 && (a->lda * es) % 16 == 0, "%s: rows must be 16-byte aligned", who);
  M3_REQUIRE(a->lddc >= 0 && a->lda >= 0 && a->lddc * es < ((int64_t)1 << 32) && a->lda * es < ((int64_t)1 << 32),
             "%s: a row stride of 4 GiB or more (the kernels form row offsets from 32-bit rows and strides)", who);
  M3_REQUIRE(((uintptr_t)a->dC % 16) == 0 && ((uintptr_t)a->A % 16) == 0 && ((uintptr_t)a->ws % 16) == 0, "%s: alignment", who);
  M3_REQUIRE(!a->direct_dW || (a->splits == 1 && a->chunk_rows == 0 && ((uintptr_t)a->direct_dW % 16) == 0 && !a->bias_ws),
             "%s: direct mode needs splits == 1, no balanced units, a 16-byte aligned dW and no bias slabs", who);
  M3_REQUIRE(!a->direct_db || a->direct_dW, "%s: direct_db goes with direct_dW", who);
  M3_REQUIRE(a->G == 1 || a->group_offsets, "%s: grouped call needs group_offsets", who);
  M3_REQUIRE(!a->a_row_idx || a->a_row_div >= 1, "%s: a_row_div", who);
  d.dC = (const char *)a->dC; d.lddc_b = a->lddc * es; d.c_row_idx = a->c_row_idx;
  M3_REQUIRE(a->c_row_idx || (!a->c_row_scale && a->c_row_div <= 1), "%s: c_row_div / c_row_scale need c_row_idx", who);
  M3_REQUIRE(a->c_row_div >= 0, "%s: c_row_div", who);
  d.c_row_div = (a->c_row_idx && a->c_row_div >= 1) ? a->c_row_div : 1;
  d.c_row_scale = a->c_row_scale;
  d.c_row_sh = div_shift(d.c_row_div);
  d.A = (const char *)a->A; d.lda_b = a->lda * es; d.a_row_idx = a->a_row_idx; d.a_row_div = a->a_row_idx ? a->a_row_div : 1;
  d.a_row_sh = div_shift(d.a_row_div);
  d.M = a->M; d.N = a->N; d.K = a->K; d.G = a->G; d.group_offsets = a->group_offsets;
  d.splits = a->splits; d.ws = a->ws; d.bias_ws = a->bias_ws;
  d.direct_dW = a->direct_dW; d.direct_db = a->direct_dW ? a->direct_db : nullptr;
  d.direct_beta = a->direct_beta; d.direct_beta_db = a->direct_beta_db;
  M3_REQUIRE(a->chunk_rows >= 0 && (a->chunk_rows == 0 || (a->group_offsets && a->chunk_rows % WG_ROWS == 0 && a->units >= 1 && a->G <= 64)),
             "%s: balanced mode needs group_offsets, G <= 64, chunk_rows a multiple of %d and units >= 1", who, WG_ROWS);
  d.chunk_rows = a->chunk_rows;
  kern = wgrad_demote(wgrad_kernel_of_shape(a->N, a->K, a->G, a->dtype), a, d);
  return M3_OK;
}

extern "C" int m3_wgrad_kernel(const m3_wgrad_args *a, m3_wgrad_kernel_out *out) {
  M3_REQUIRE(out, "m3_wgrad_kernel: null output");
  WgradDev d;
  WgradKernel kern;
  if (int rc = wgrad_prepare(a, "m3_wgrad_kernel", d, kern)) return rc;
  *out = m3_wgrad_kernel_out{};
  out->kernel = kern == WGRAD_BIG ? M3_WGRAD_KERNEL_BIG : kern == WGRAD_SKINNY ? M3_WGRAD_KERNEL_SKINNY : kern == WGRAD_DMA ? M3_WGRAD_KERNEL_DMA : M3_WGRAD_KERNEL_STAGED;
  out->gather_c = a->c_row_idx != nullptr; out->gather_a = a->a_row_idx != nullptr; out->scale_c = a->c_row_scale != nullptr;
  out->tile_n = kern == WGRAD_BIG ? BG_T : WG_T;
  out->tile_k = kern == WGRAD_BIG ? BG_T : kern == WGRAD_SKINNY ? a->K : WG_T;
  return M3_OK;
}

extern "C" int m3_wgrad_tn(const m3_wgrad_args *a, void *stream) {
  WgradDev d;
  WgradKernel kern;
  if (int rc = wgrad_prepare(a, "m3_wgrad_tn", d, kern)) return rc;
  const int es = dtype_size(a->dtype);
  hipStream_t s = (hipStream_t)stream;
  const bool gc = a->c_row_idx != nullptr, ga = a->a_row_idx != nullptr, sc = a->c_row_scale != nullptr;
  const bool big = kern == WGRAD_BIG;
  // the previous call's slab reduction (a->prev): in front of this launch (128-wide kernels), or as its own launch.  In direct
  // mode this launch read-add-writes dW while those blocks run: they must not write the same tensor
  const int n_prev = a->prev ? (a->n_prev > 1 ? a->n_prev : 1) : 0;
  for (int j = 0; j < n_prev && a->direct_dW; ++j)
    M3_REQUIRE(a->prev[j].dW != a->direct_dW && (!a->direct_db || a->prev[j].db != a->direct_db),
               "m3_wgrad_tn: the prev reduction writes the dW / db this direct-mode launch adds into");
  if (int rc = wgrad_take_prev(d, a->prev, a->n_prev, a->ws, big || a->M == 0, s, "m3_wgrad_tn")) return rc;
  static int lpt = -1;
  if (lpt < 0) { const char *e = getenv("M3_WGRAD_LPT"); lpt = e ? (atoi(e) ? 1 : 0) : 1; }
  d.lpt = lpt;
  const int t = big ? BG_T : WG_T;
  d.tiles_k = (a->K + t - 1) / t;
  dim3 grid(((a->N + t - 1) / t) * d.tiles_k, a->chunk_rows ? a->units : a->G, a->chunk_rows ? 1 : a->splits);
  wgrad_prev_slices(d, grid);
  if (big) return launch_wgrad_big(a->dtype, gc, ga, sc, grid, d, s);
  if (kern == WGRAD_SKINNY) {                    // the router's weight (K = 16 / 32, plain rows): the streaming kernel
    for_dtype(a->dtype, [&](auto tag) {
      typedef typename decltype(tag)::type T;
      if (a->K == 16) hipLaunchKernelGGL((wgrad_skinny_kernel<T, 16>), grid, dim3(WG_THREADS), 0, s, d);
      else hipLaunchKernelGGL((wgrad_skinny_kernel<T, 32>), grid, dim3(WG_THREADS), 0, s, d);
    });
    return check_launch("m3_wgrad_tn");
  }
  M3_REQUIRE(a->N * es >= 16 && a->K * es >= 16, "m3_wgrad_tn: N, K too small");
  return kern == WGRAD_DMA ? launch_wgrad_dma(a->dtype, gc, ga, sc, grid, d, s) : launch_wgrad_staged(a->dtype, gc, ga, sc, grid, d, s);
}

// ------------------------------------------------------------------ the batched weight-gradient call
// One launch for several dense weight gradients over the same rows (wgrad_multi.hip).  Allowed where every problem is one the
// register-staged kernel takes by today's rules, in 16 bit: fp32 and the shapes of the LDS-DMA and 256 x 256 kernels (ViT-Base)
// keep their launch per weight.
// Row parts: ONE count P for all problems, the smallest that fills 432 workgroups (what the qkv weight of configs[1] gets by
// itself: 27 tiles x 16 parts; the slot sweep of profiles/r04_levers_measured_and_dropped.txt found 432 about level with all
// 512 resident slots) - unless that spills over the 512 slots, where a few workgroups would run as a second round: then the
// most parts that fit.  At most 16 parts, and at least 16 32-row steps per part, as for a single call.  Measured at M = 25 216,
// 108 tiles (a dense block of configs[1]): P = 4 (432 workgroups) 148 us, P = 5 (540: a second round of 28) 188 us, P = 9 147 us
// with more than twice the slab bytes (profiles/wgrad_multi_premise.txt).
extern "C" int m3_wgrad_multi_plan(const m3_wgrad_multi_shape *s, m3_wgrad_multi_plan_out *p) {
  M3_REQUIRE(s && p, "m3_wgrad_multi_plan: null argument");
  M3_REQUIRE(dtype_ok(s->dtype) && s->n >= 1 && s->n <= M3_WGRAD_MULTI_MAX && s->M >= 0 && s->M < ((int64_t)1 << 31) && s->parts >= 0,
             "m3_wgrad_multi_plan: bad shape");
  *p = m3_wgrad_multi_plan_out{};
  bool ok = s->dtype != M3_F32 && s->M > 0;
  int64_t tiles = 0;
  for (int j = 0; j < s->n; ++j) {
    M3_REQUIRE(s->N[j] > 0 && s->K[j] > 0, "m3_wgrad_multi_plan: bad shape of problem %d", j);
    ok = ok && wgrad_kernel_of_shape(s->N[j], s->K[j], 1, s->dtype) == WGRAD_STAGED;
    tiles += (int64_t)((s->N[j] + WG_T - 1) / WG_T) * ((s->K[j] + WG_T - 1) / WG_T);
  }
  M3_REQUIRE(tiles <= (1 << 20), "m3_wgrad_multi_plan: %lld tiles", (long long)tiles);
  int64_t P = s->parts;
  if (!P) {
    const int64_t steps = std::max<int64_t>(1, (s->M + 31) / 32), cap = std::min<int64_t>(16, std::max<int64_t>(1, steps / 16));
    P = (432 + tiles - 1) / tiles;
    if (P * tiles > 512) P = std::max<int64_t>(1, 512 / tiles);
    P = std::min(P, cap);
  }
  M3_REQUIRE(P <= 4096, "m3_wgrad_multi_plan: %lld parts", (long long)P);
  p->allowed = ok; p->parts = (int32_t)P; p->tiles = (int32_t)tiles; p->workgroups = (int32_t)(P * tiles);
  int64_t off = 0;
  for (int j = 0; j < s->n; ++j) { p->ws_off[j] = off; off += P * s->N[j] * s->K[j]; }
  for (int j = 0; j < s->n; ++j) { p->bias_off[j] = off; off += s->bias[j] ? P * s->N[j] : 0; }
  p->ws_elems = off;
  return M3_OK;
}

extern "C" int m3_wgrad_multi(const m3_wgrad_multi_args *a, void *stream) {
  M3_REQUIRE(a && a->ws && a->reduce_out, "m3_wgrad_multi: null argument");
  M3_REQUIRE(a->n >= 1 && a->n <= M3_WGRAD_MULTI_MAX && a->parts >= 0, "m3_wgrad_multi: %d problems, %d parts", a->n, a->parts);
  M3_REQUIRE(((uintptr_t)a->ws % 16) == 0, "m3_wgrad_multi: alignment");
  m3_wgrad_multi_shape sh = {};
  sh.M = a->M; sh.dtype = a->dtype; sh.n = a->n; sh.parts = a->parts;
  for (int j = 0; j < a->n; ++j) { sh.N[j] = a->prob[j].N; sh.K[j] = a->prob[j].K; sh.bias[j] = a->prob[j].db != nullptr; }
  m3_wgrad_multi_plan_out pl;
  if (int rc = m3_wgrad_multi_plan(&sh, &pl)) return rc;
  M3_REQUIRE(pl.allowed, "m3_wgrad_multi: this batch is not one m3_wgrad_multi_plan allows (16-bit, M > 0, shapes of the register-staged kernel)");
  const int es = dtype_size(a->dtype);
  const int n_prev = a->prev ? (a->n_prev > 1 ? a->n_prev : 1) : 0;
  WgradMultiDev md = {};
  WgradProb *tab = &md.tab0;
  for (int j = 0; j < WG_MULTI; ++j) tab[j].first = INT32_MAX;
  int first = 0;
  for (int j = 0; j < a->n; ++j) {
    const m3_wgrad_problem &q = a->prob[j];
    M3_REQUIRE(q.dC && q.A && q.dW, "m3_wgrad_multi: null operand in problem %d", j);
    M3_REQUIRE((q.N * es) % 16 == 0 && (q.K * es) % 16 == 0 && (q.lddc * es) % 16 == 0 && (q.lda * es) % 16 == 0 && q.lddc >= q.N && q.lda >= q.K,
               "m3_wgrad_multi: problem %d: rows and N*elem, K*elem must be multiples of 16 bytes", j);
    M3_REQUIRE(q.lddc * es < ((int64_t)1 << 32) && q.lda * es < ((int64_t)1 << 32), "m3_wgrad_multi: problem %d: a row stride of 4 GiB or more", j);
    M3_REQUIRE(((uintptr_t)q.dC % 16) == 0 && ((uintptr_t)q.A % 16) == 0 && ((uintptr_t)q.dW % 16) == 0 && ((uintptr_t)q.db % 16) == 0,
               "m3_wgrad_multi: problem %d: alignment", j);
    for (int i = 0; i < j; ++i)
      M3_REQUIRE(a->prob[i].dW != q.dW && (!q.db || a->prob[i].db != q.db), "m3_wgrad_multi: problems %d and %d write the same dW / db", i, j);
    // the prev reductions run inside this launch, this launch's own after it: one that writes the same tensor would be a caller
    // that accumulates into a gradient twice in a row - refused rather than ordered
    for (int i = 0; i < n_prev; ++i)
      M3_REQUIRE(a->prev[i].dW != q.dW && (!q.db || a->prev[i].db != q.db),
                 "m3_wgrad_multi: the prev reduction writes the dW / db of problem %d", j);
    const int tiles_k = (q.K + WG_T - 1) / WG_T;
    float *bws = q.db ? a->ws + pl.bias_off[j] : nullptr;
    tab[j] = WgradProb{(const char *)q.dC, q.lddc * es, (const char *)q.A, q.lda * es, a->ws + pl.ws_off[j], bws, q.N, q.K, tiles_k, first};
    first += ((q.N + WG_T - 1) / WG_T) * tiles_k;
    a->reduce_out[j] = m3_wgrad_reduce_desc{a->ws + pl.ws_off[j], pl.parts, (int64_t)q.N * q.K, nullptr, 1, 0, q.dW, q.beta ? 1 : 0,
                                            bws, q.db ? (int64_t)q.N : 0, q.db, q.beta_db ? 1 : 0};
  }
  WgradDev &d = md.d;
  d.M = a->M; d.G = 1; d.splits = pl.parts; d.a_row_div = 1; d.c_row_div = 1;
  hipStream_t s = (hipStream_t)stream;
  // slabs of the prev reductions: anywhere but in this launch's workspace
  for (int i = 0; i < n_prev; ++i)
    M3_REQUIRE(a->prev[i].ws < a->ws || a->prev[i].ws >= a->ws + pl.ws_elems, "m3_wgrad_multi: prev slabs inside this call's workspace");
  if (int rc = wgrad_take_prev(d, a->prev, a->n_prev, a->ws, false, s, "m3_wgrad_multi")) return rc;
  dim3 grid((unsigned)pl.tiles, 1, (unsigned)pl.parts);
  wgrad_prev_slices(d, grid);
  return launch_wgrad_multi(a->dtype, grid, md, s);
}

// ------------------------------------------------------------------ column sums
extern "C" int64_t m3_colsum_ws_elems(int64_t M, int N, int G) {
  return (int64_t)G * colsum_strips_per_group(M, G) * N;
}

extern "C" int m3_colsum(const void *dC, int dtype, int64_t lddc, const int32_t *c_row_idx, int64_t M, int N, int G,
                         const int32_t *group_offsets, float *ws, float *db, int beta, void *stream) {
  M3_REQUIRE(dC && ws && db, "m3_colsum: null operand");
  M3_REQUIRE(dtype_ok(dtype), "m3_colsum: bad dtype");
  M3_REQUIRE(N % 4 == 0 && lddc % 4 == 0 && G >= 1, "m3_colsum: N, lddc must be multiples of 4");
  M3_REQUIRE(G == 1 || group_offsets, "m3_colsum: grouped call needs group_offsets");
  M3_REQUIRE((N * dtype_size(dtype)) % 16 == 0 && (lddc * dtype_size(dtype)) % 16 == 0 && ((uintptr_t)dC % 16) == 0,
             "m3_colsum: rows must be 16-byte aligned and N*elem a multiple of 16");
  const int spg = colsum_strips_per_group(M, G);
  const int es = dtype_size(dtype);
  hipStream_t s = (hipStream_t)stream;
  const int chunks = N * es / 16;
  const dim3 grid((chunks + 63) / 64, spg, G), block(256);
  for_dtype(dtype, [&](auto tag) {
    hipLaunchKernelGGL(colsum_part_kernel<typename decltype(tag)::type>, grid, block, 0, s, (const char *)dC, lddc * es, c_row_idx, M, N,
                       group_offsets, spg, ws);
  });
  int rc = check_launch("m3_colsum(part)");
  if (rc) return rc;
  return launch_reduce_rows_f32(ws, spg, N, G, (int64_t)spg * N, db, beta, s);
}
