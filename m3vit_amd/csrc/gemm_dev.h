// Definitions shared by the NT GEMM kernels and their host entry m3_gemm_nt (gemm.hip): the device-side argument block, the
// grouped tile -> expert map, the tile order, the epilogue kinds and what each kernel's file exposes to the host.
//   gemm_staged.hip  128 / 160 x 128 tiles, operands staged through registers: fp32 and the shapes the others refuse
//   gemm_dma.hip     128 x 128 tiles, operands by LDS-DMA: the 16-bit launches
//   gemm_big.hip     256 x 256 tiles, LDS-DMA ring: 16-bit launches with a long contraction
#pragma once
#include <type_traits>
#include "common.h"

namespace m3 {

constexpr int BM = 128, BN = 128, ROWB = 128;  // ROWB: bytes of K per row per step
constexpr int GEMM_THREADS = 256;

struct GemmDev {
  const char *A; int64_t lda_b;                 // byte strides
  const int32_t *a_row_idx; int32_t a_row_div; int32_t a_row_sh;   // a_row_sh: log2(a_row_div) if a power of two, else -1
  const char *B; int64_t ldb_b; int64_t b_group_b;
  char *C; int64_t ldc; int32_t c_f32;
  const int32_t *c_row_idx;
  const float *bias;
  char *pre_out; int64_t ld_pre;
  const char *gpre; int64_t ld_gpre;
  const float *residual; int64_t ld_res;
  const float *row_scale; int32_t row_scale_div;   // value *= row_scale[srow / div] in front of the residual add,
  const int32_t *row_scale_idx;                    // srow = row_scale_idx ? row_scale_idx[m] : crow
  int32_t row_scale_sh;                            // log2(row_scale_div) if a power of two, else -1 (as a_row_sh)
  int32_t act;
  int64_t M; int32_t N; int32_t K;
  int32_t G;
  const int32_t *group_offsets;
  const int32_t *tile_starts;
  int32_t n_tiles;
  int32_t m_band;                  // row tiles per band of the tile order (tile_of): 1 = row-tile major
  int32_t m_tiles_max;
  int32_t vec8;                                 // N and all leading dims multiples of 8: staged epilogue
  // gemm_nt_big_kernel's segmented-A instance only (conv.hip; 0 elsewhere): a row of A is three runs of a_seg_tiles 128-byte
  // K tiles, the start of a run a_seg_jump_b bytes behind the end of the run before it
  int32_t a_seg_tiles; int64_t a_seg_jump_b;
};

// Grouped call: which (group, first row, end row) owns row tile mt, and how many workgroups are live.  G <= 64: ONE
// vector load of the tile prefix (lane l holds tile_starts[l + 1]) + a ballot instead of a chain of up to G dependent
// scalar loads in front of every tile (the expert GEMMs run ~800 row tiles x 3 column tiles per launch).
struct TileOwner { int g; int64_t m_begin, m_end; };
__device__ __forceinline__ int grouped_live_tiles(const int32_t *tile_starts, int G, int lane, int &ts_lane) {
  if (G <= 64) {
    ts_lane = lane < G ? tile_starts[lane + 1] : 0x7fffffff;
    return __builtin_amdgcn_readfirstlane(__shfl(ts_lane, G - 1, 64));
  }
  ts_lane = 0;
  return tile_starts[G];
}
// row tile mt of group g, whose first row tile is t0 (tiles of ROWS rows) -> the tile's rows
template <int ROWS>
__device__ __forceinline__ TileOwner grouped_tile_rows(const int32_t *group_offsets, int g, int t0, int mt) {
  TileOwner o;
  // (everything here is wave-uniform: say so, or the compiler carries the tile bounds in vector registers)
  g = __builtin_amdgcn_readfirstlane(g);
  t0 = __builtin_amdgcn_readfirstlane(t0);
  o.g = g;
  o.m_begin = (int64_t)__builtin_amdgcn_readfirstlane(group_offsets[g]) + (int64_t)(mt - t0) * ROWS;
  o.m_end = __builtin_amdgcn_readfirstlane(group_offsets[g + 1]);
  return o;
}
// the group that owns row tile mt and the group's first row tile: no memory access with G <= 64 (ts_lane: grouped_live_tiles)
__device__ __forceinline__ void grouped_tile_group(const int32_t *tile_starts, int G, int mt, int lane, int ts_lane, int &g,
                                                   int &t0) {
  g = 0;
  if (G <= 64) {
    // groups whose END prefix is <= mt lie wholly before the tile (the prefix is monotone; the last group never counts)
    g = __popcll(__ballot(lane < G - 1 && ts_lane <= mt));
    t0 = g ? __shfl(ts_lane, g - 1, 64) : 0;
  } else {
    while (g + 1 < G && tile_starts[g + 1] <= mt) ++g;
    t0 = tile_starts[g];
  }
}
__device__ __forceinline__ TileOwner grouped_tile_owner(const int32_t *tile_starts, const int32_t *group_offsets, int G,
                                                        int mt, int lane, int ts_lane) {
  int g, t0;
  grouped_tile_group(tile_starts, G, mt, lane, ts_lane, g, t0);
  return grouped_tile_rows<128>(group_offsets, g, t0, mt);
}

__device__ __forceinline__ int dma_swz(int row) { return (row >> 1) & 7; }

// EPI: the epilogue's kind as a template constant of the two LDS-DMA kernels.  DMA_EPI_ANY keeps every option behind
// run-time flags: each `if (p.gpre)` / `if (p.residual)` / `if (m >= m_end) break` is then a basic-block boundary, the loads
// of a store pass are issued inside the pass and the passes of a tile run strictly one after the other, every one paying its
// memory latency in front of its stores.  The four kinds below cover every 16-bit launch of the training step with
// straight-line passes: what a thread needs from memory for a half tile - scatter indices, GELU' pre-activations, residual
// rows - is requested BEFORE that half's staging barriers and arrives under the LDS transposition; the per-row factor is
// always applied (1.0 without row_scale); rows past the group's end repeat the group's last row (the operand rows were
// clamped at the load, so the values are that row's own: a duplicate store of identical data) - except with the fp32
// residual, where C may alias the residual and the store stays predicated.
//   PLAIN  C = acc (+ bias), optional scatter                      qkv, every plain input gradient, expert FC2 forward
//   GELU   pre_out = acc + bias ; C = GELU(pre_out)                fc1 / expert FC1 forward
//   GPRE   C = acc * GELU'(gpre)                                   fc2 / expert FC2 input gradient
//   RES    C(fp32) = acc (+ bias) + residual                       proj, fc2 forward
enum { DMA_EPI_ANY = 0, DMA_EPI_GPRE = 1, DMA_EPI_RES = 2, DMA_EPI_PLAIN = 3, DMA_EPI_GELU = 4 };

// run-time kind -> template constant: f is called once, with the kind as a std::integral_constant
template <typename F> inline void with_epi(int epi, F &&f) {
  switch (epi) {
    case DMA_EPI_GPRE: f(std::integral_constant<int, DMA_EPI_GPRE>()); break;
    case DMA_EPI_RES: f(std::integral_constant<int, DMA_EPI_RES>()); break;
    case DMA_EPI_PLAIN: f(std::integral_constant<int, DMA_EPI_PLAIN>()); break;
    case DMA_EPI_GELU: f(std::integral_constant<int, DMA_EPI_GELU>()); break;
    default: f(std::integral_constant<int, DMA_EPI_ANY>()); break;
  }
}

// The run-time-flag epilogue of one output row m, 8 columns from n: v0 | v1 = acc + bias.  It is the staged epilogue of
// gemm_nt_kernel and the DMA_EPI_ANY branch of both LDS-DMA kernels.  row_factor(crow) is the row's row_scale factor, asked
// for only with row_scale set: the register-staged kernel loads it here, the LDS-DMA kernels prefetched it into LDS.
template <typename T, typename RowFactor>
__device__ __forceinline__ void epilogue_row_any(const GemmDev &p, int64_t m, int n, f32x4 v0, f32x4 v1, RowFactor row_factor) {
  const int64_t crow = p.c_row_idx ? (int64_t)p.c_row_idx[m] : m;
  if (p.pre_out) Vec8<T>::store((T *)p.pre_out + crow * p.ld_pre + n, v0, v1);
  if (p.act == M3_ACT_GELU) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { v0[j] = gelu_f(v0[j]); v1[j] = gelu_f(v1[j]); }
  }
  if (p.gpre) {
    f32x4 p0, p1;
    Vec8<T>::load((const T *)p.gpre + crow * p.ld_gpre + n, p0, p1);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v0[j] *= gelu_grad_f(p0[j]); v1[j] *= gelu_grad_f(p1[j]); }
  }
  if (p.row_scale) {
    const float sc = row_factor(crow);
    v0 *= sc; v1 *= sc;
  }
  if (p.residual) {
    v0 += *(const f32x4 *)(p.residual + crow * p.ld_res + n);
    v1 += *(const f32x4 *)(p.residual + crow * p.ld_res + n + 4);
  }
  if (p.c_f32) {
    *(f32x4 *)((float *)p.C + crow * p.ldc + n) = v0;
    *(f32x4 *)((float *)p.C + crow * p.ldc + n + 4) = v1;
  } else {
    Vec8<T>::store((T *)p.C + crow * p.ldc + n, v0, v1);
  }
}

// What each kernel's file exposes.  m3_gemm_nt has validated the call, chosen the kernel and set the tile order for it
// (n_tiles, m_band, m_tiles_max): a launch function runs m_tiles_max * n_tiles workgroups of its kernel.
constexpr int BIG_B = 256;                        // tile edge of gemm_big.hip
int launch_gemm_staged(const GemmDev &d, int dtype, bool tall, hipStream_t s);        // tall: 160-row tiles (fp32, whole K slices)
int launch_gemm_dma(const GemmDev &d, int dtype, int epi, hipStream_t s);             // 16-bit dtypes
bool gemm_big_eligible(const GemmDev &d, int dtype_size_bytes, bool force);           // false: not a call the 256 x 256 kernel takes
int launch_gemm_big(const GemmDev &d, int dtype, int epi, hipStream_t s);             // 16-bit dtypes
int launch_gemm_big_seg(const GemmDev &d, int dtype, hipStream_t s, const char *who);  // segmented A rows, PLAIN epilogue (conv.hip)

// Logical tile id -> (row tile, column tile).  Row-tile major (band 1): the n_tiles column tiles of a row tile are neighbours
// (one XCD, one moment: the A rows come from HBM once).  When a column-tile's weight panel set does not fit the XCD's L2
// (the ViT-Base N = 2304 / 3072 launches: 18-24 panels of 196 KB), that order re-fetches every panel for every row tile; in
// bands of m_band row tiles - column tile major inside a band - the 32 workgroups an XCD runs at a time cover m_band row
// tiles x 32 / m_band panels, so a panel is fetched once per band and the band's A rows stay resident while its column tiles
// go by.  live_m: live row tiles of the launch.
__device__ __forceinline__ void tile_of(int t, int n_tiles, int m_band, int live_m, int &mt, int &nt) {
  if (m_band <= 1) { mt = t / n_tiles; nt = t - mt * n_tiles; return; }
  const int per = m_band * n_tiles;
  const int band = t / per, r = t - band * per;
  const int rows = min(m_band, live_m - band * m_band);
  nt = r / rows;
  mt = band * m_band + (r - nt * rows);
}
}  // namespace m3
