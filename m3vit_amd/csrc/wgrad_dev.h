// Shared by the weight-gradient sources (wgrad.hip: entry points, launch plan, kernel choice, slab reductions, column sums,
// the streaming kernel; wgrad_staged.hip: the register-staged 128 x 128 kernel; wgrad_multi.hip: the same over several weights
// in one launch; wgrad_dma.hip: the LDS-DMA kernels, 128 x 128 and 256 x 256): the kernels' argument block, the work units of a grouped call, the result stores, the slab reduction that
// rides in front of a launch, and the launchers wgrad.hip dispatches to.
#pragma once
#include "common.h"
#include <type_traits>

namespace m3 {

constexpr int WG_T = 128;        // tile edge (n and k)
constexpr int WG_ROWS = 64;      // granule of the row splits (= the largest per-dtype step below)
constexpr int WG_THREADS = 256;
constexpr int BG_T = 256, BG_THREADS = 512, BG_RS = 512;

// The register-staged kernel's gather table (wgrad_staged.hip): pieces of WG_TAB_ROWS rows, one row per thread, two slots;
// three arrays of 4-byte entries behind the operand images - source row of dC, per-row factor, source row of A
constexpr int WG_TAB_ROWS = WG_THREADS;
constexpr int WG_TAB_BYTES = 3 * 2 * WG_TAB_ROWS * 4;

constexpr int WG_MULTI = 8;     // problems of one batched launch (M3_WGRAD_MULTI_MAX)

// one of the dense slab reductions a batched launch leaves behind (WgradDev.rd_tab)
struct WgradRdProb {
  const float *ws; float *dW; const float *bws; float *db;
  int64_t e4; int32_t b4;
  int32_t nbw;                     // reduce blocks of the weight elements (the bias blocks follow them)
  int32_t first;                   // the first reduce block of this problem; INT32_MAX in the unused entries
  int32_t beta;                    // bit 0: dW += , bit 1: db +=
};

struct WgradDev {
  const char *dC; int64_t lddc_b; const int32_t *c_row_idx;
  int32_t c_row_div; const float *c_row_scale;   // dC row of slot m = c_row_scale[c_row_idx[m]] * dC[c_row_idx[m] / c_row_div]
  int32_t a_row_sh, c_row_sh;                    // log2 of the divisors when they are powers of two, else -1
  const char *A; int64_t lda_b; const int32_t *a_row_idx; int32_t a_row_div;
  int64_t M; int32_t N; int32_t K; int32_t G;
  const int32_t *group_offsets;
  int32_t splits;
  float *ws;
  float *bias_ws;                  // optional [splits][G][N]: column sums of dC (bias grads), fused
  int32_t tiles_k;
  int32_t chunk_rows;              // > 0: balanced grouped mode - a work unit is `chunk_rows` rows of ONE group
  // The slab reduction of the PREVIOUS weight-gradient call of the stream, done by this launch's leading blocks
  // (m3_wgrad_args.prev): rd_blocks > 0 switches it on; layouts as m3_wgrad_reduce / m3_wgrad_reduce_grouped take them
  int32_t rd_blocks, rd_zslices;   // reduce blocks (flattened x, group) and the grid z slices they occupy
  int32_t rd_nbx, rd_nbw;          // blocks per group (weight + bias part), of those for the weight elements
  int32_t rd_cols;                 // 16-byte columns per reduce block: 256, or 64 with four threads per column (dense, many slabs)
  const float *rd_ws; int32_t rd_splits; int64_t rd_e4;
  const int32_t *rd_off; int32_t rd_G, rd_chunk;
  float *rd_dW; int32_t rd_beta;
  const float *rd_bws; int64_t rd_b4; float *rd_db; int32_t rd_beta_db;
  // rd_n > 1: the previous call was a batched launch (m3_wgrad_multi) - rd_n dense reductions of rd_splits slabs each, their
  // blocks one problem after the other (rd_tab[j].first); the table replaces rd_ws .. rd_beta_db above
  int32_t rd_n;
  WgradRdProb rd_tab0, rd_tab1, rd_tab2, rd_tab3, rd_tab4, rd_tab5, rd_tab6, rd_tab7;
  // direct mode (splits == 1, no balanced units: every (group, tile) belongs to exactly ONE workgroup): the result tiles are
  // added into dW [G][N][K] (the column sums into db [G][N]) by the kernel itself - no slabs, no reduction
  float *direct_dW; float *direct_db; int32_t direct_beta, direct_beta_db;
  int32_t lpt;                     // grouped, one part per group: the groups are taken longest first (wgrad_lpt_group)
};

// the result of a workgroup: one 128 x 128 fp32 tile (lane holds k = kb + 4 lg + r, n = nb + li) to its slab, or - direct
// mode - read-add-written into dW
__device__ __forceinline__ void wgrad_store_tile(const WgradDev &p, const f32x4 (&acc)[4][4], int64_t slab_id, int g, int n0, int k0,
                                                 int wr, int wc, int li, int lg) {
  float *out = p.direct_dW ? p.direct_dW + (int64_t)g * p.N * p.K : p.ws + slab_id * (int64_t)p.N * p.K;
  const bool add = p.direct_dW && p.direct_beta;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int n = n0 + wc * 64 + ni * 16 + li;
    if (n >= p.N) continue;
    f32x4 old[4];
    if (add) {
#pragma unroll
      for (int ki = 0; ki < 4; ++ki) {
        const int k = k0 + wr * 64 + ki * 16 + 4 * lg;
        old[ki] = k < p.K ? *(const f32x4 *)(out + (int64_t)n * p.K + k) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int ki = 0; ki < 4; ++ki) {
      const int k = k0 + wr * 64 + ki * 16 + 4 * lg;
      if (k >= p.K) continue;
      *(f32x4 *)(out + (int64_t)n * p.K + k) = add ? acc[ki][ni] + old[ki] : acc[ki][ni];
    }
  }
}
__device__ __forceinline__ void wgrad_store_bias(const WgradDev &p, float v, int64_t slab_id, int g, int n) {
  if (p.direct_db) {
    float *d = p.direct_db + (int64_t)g * p.N + n;
    *d = p.direct_beta_db ? *d + v : v;
  } else {
    p.bias_ws[slab_id * p.N + n] = v;
  }
}

// balanced grouped mode: units are dealt to the groups in order, n_g = ceil(rows_g / chunk) each, a group's rows
// divided evenly over its units (a hot expert gets proportionally more units; the slab of unit u is ws[u]).
// The two rules of the map, host and device (the kernels below, m3_wgrad_reduce_grouped and the host query m3_wgrad_unit_of
// all go through them): how many units a group gets, and which of its rows unit j of them covers - equal shares in whole
// WG_ROWS granules, share = round_up(ceil(rows / n), WG_ROWS) <= chunk (chunk is a multiple of WG_ROWS), so (n - 1) * share
// <= (n - 1) * chunk < rows: no unit is empty, none is longer than chunk, all but a group's last are whole granules.
__host__ __device__ __forceinline__ int wgrad_units_of_group(int rows, int chunk) { return (rows + chunk - 1) / chunk; }
__host__ __device__ __forceinline__ void wgrad_unit_rows(int rows, int n, int j, int &begin, int &end) {
  const int per = ((rows + n - 1) / n + WG_ROWS - 1) / WG_ROWS * WG_ROWS;
  begin = j * per;
  end = begin + per < rows ? begin + per : rows;
}

// One lane per group (G <= 64): ONE load of the offsets per wave and a shuffle scan instead of G dependent loads.
// Returns this lane's group's (rows, n, exclusive prefix of n).
__device__ __forceinline__ void wgrad_unit_scan(const int32_t *off, int G, int chunk, int lane, int &rows, int &n, int &first) {
  rows = lane < G ? off[lane + 1] - off[lane] : 0;
  n = wgrad_units_of_group(rows, chunk);
  int incl = n;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  first = incl - n;
}

// logical id (after the XCD remap over the LIVE workgroups only: tiles x sum of n_g - the grid is sized for the upper
// bound, and remapping over the whole grid would park the surplus ids, i.e. no work at all, on the last XCDs)
// -> (tile, unit, group, first row, end row); false: this workgroup is surplus
__device__ __forceinline__ bool wgrad_unit(const int32_t *off, int G, int chunk, int lin, int tiles, int lane, int &tile,
                                           int &u, int &g, int64_t &r0, int64_t &r1) {
  int rows, n, first;
  wgrad_unit_scan(off, G, chunk, lane, rows, n, first);
  const int units = __shfl(first + n, 63, 64);
  if (lin >= units * tiles) return false;
  const int log_id = xcd_remap(lin, units * tiles);
  tile = log_id % tiles;
  u = log_id / tiles;
  const unsigned long long m = __ballot(u >= first && u < first + n);
  g = __ffsll((long long)m) - 1;
  rows = __shfl(rows, g, 64); n = __shfl(n, g, 64); first = __shfl(first, g, 64);
  int b, e;
  wgrad_unit_rows(rows, n, u - first, b, e);
  r0 = (int64_t)off[g] + b;
  r1 = (int64_t)off[g] + e;
  return true;
}

// Groups of unequal size, one part per (group, tile) workgroup (the experts' weight gradients in direct mode): a workgroup's
// life is proportional to its expert's rows, and dealt out in expert order the hot experts' workgroups can all start in the
// last round (configs[3] / [4] with the learned router: +30..40 % over the same launch with uniform routing).  Longest first:
// unit u of the launch (in dispatch order: the XCD remap hands each XCD one contiguous eighth of the units) takes the
// group of size rank 8 * (u mod G/8) + u / (G/8) - every XCD gets every eighth-largest group, largest first.  One lane per
// group (G <= 64, G a multiple of 8; else the identity), ranks by 64 shuffles; which workgroup computes a tile never
// changes the tile's value.
__device__ __forceinline__ int wgrad_lpt_group(const int32_t *off, int G, int u, int lane) {
  if (G > 64 || (G & 7)) return u;
  const int cnt = lane < G ? off[lane + 1] - off[lane] : -1;
  int rank = 0;
  for (int j = 0; j < G; ++j) {
    const int cj = __shfl(cnt, j, 64);
    rank += (cj > cnt || (cj == cnt && j < lane)) ? 1 : 0;
  }
  const int per = G >> 3;
  const int want = 8 * (u % per) + u / per;
  const unsigned long long m = __ballot(lane < G && rank == want);
  return __ffsll((long long)m) - 1;
}

// A batched launch (m3_wgrad_multi, wgrad_multi.hip): up to WG_MULTI dense problems over the same M rows, every one cut into
// the same d.splits row parts.  `d` carries what the problems share (M, splits, the reduction riding in front); a workgroup
// copies its problem's operands, shape and slabs from the table into it.
struct WgradProb {
  const char *dC; int64_t lddc_b; const char *A; int64_t lda_b;
  float *ws; float *bias_ws;       // this problem's slabs [splits][N][K] and (or null) [splits][N]
  int32_t N, K, tiles_k;
  int32_t first;                   // the first tile of this problem among the launch's tiles; INT32_MAX in the unused entries
};
struct WgradMultiDev {
  WgradDev d;
  WgradProb tab0, tab1, tab2, tab3, tab4, tab5, tab6, tab7;
};

typedef __fp16 fp16x4_t __attribute__((__vector_size__(4 * sizeof(__fp16))));

// slabs -> dW (blocks [0, nb_w)) and, in the same launch, bias slabs -> db (blocks [nb_w, ...)); splits in order
__device__ __forceinline__ f32x4 wgrad_sum_slabs(const f32x4 *w, int64_t elems4, int lo, int hi, f32x4 s) {
  // eight slabs' loads in flight before the first add (a thread owns ONE 16-byte column of its slabs: issued one dependent
  // load at a time the reduction was latency-bound); slabs are added in index order
  int sp = lo;
  for (; sp + 8 <= hi; sp += 8) {
    f32x4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w[(int64_t)(sp + j) * elems4];
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[j];
  }
  for (; sp < hi; ++sp) s += w[(int64_t)sp * elems4];
  return s;
}
// cols = 256: a thread per 16-byte column, the slabs one after the other.  cols = 64 (many slabs - m3_wgrad_reduce_cols: a
// column's chain of dependent load batches was the whole duration of a launch with 100+ parts): four threads per column,
// each sums a quarter of the slabs (contiguous ranges), the quarters are added in order by the first; deterministic, another
// association than cols = 256.  Every thread of the block must call (a barrier inside).
__device__ __forceinline__ void wgrad_reduce_block(int64_t blk, int tid, const float *ws, int splits, int64_t elems4, float *dW,
                                                   int beta, int nb_w, const float *bias_ws, int64_t belems4, float *db, int beta_db,
                                                   int cols) {
  if (blk >= nb_w) {
    blk -= nb_w; ws = bias_ws; elems4 = belems4; dW = db; beta = beta_db;
  }
  if (cols == 256) {
    const int64_t i = blk * 256 + tid;
    if (i >= elems4) return;
    f32x4 s = beta ? ((const f32x4 *)dW)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    ((f32x4 *)dW)[i] = wgrad_sum_slabs((const f32x4 *)ws + i, elems4, 0, splits, s);
    return;
  }
  __shared__ f32x4 spart[3][64];
  const int col = tid & 63, part = tid >> 6;
  const int64_t i = blk * 64 + col;
  const bool in = i < elems4;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (in) {
    if (part == 0 && beta) s = ((const f32x4 *)dW)[i];
    s = wgrad_sum_slabs((const f32x4 *)ws + i, elems4, splits * part / 4, splits * (part + 1) / 4, s);
  }
  if (part > 0) spart[part - 1][col] = s;
  __syncthreads();
  if (part == 0 && in) {
    s += spart[0][col]; s += spart[1][col]; s += spart[2][col];
    ((f32x4 *)dW)[i] = s;
  }
}

// balanced grouped mode: dW[g] (+)= sum of the slabs of group g's units, in unit order; g = group,
// blocks [0, nb_w) the weight elements, [nb_w, ..) the bias elements
__device__ __forceinline__ void wgrad_reduce_grouped_block(int64_t blk, int g, int tid, const float *ws, const int32_t *off, int G,
                                                           int chunk, int64_t elems4, float *dW, int beta, int nb_w,
                                                           const float *bias_ws, int64_t belems4, float *db, int beta_db) {
  if (blk >= nb_w) {
    blk -= nb_w; ws = bias_ws; elems4 = belems4; dW = db; beta = beta_db;
  }
  const int64_t i = blk * 256 + tid;
  int rows, n, first;
  wgrad_unit_scan(off, G, chunk, tid & 63, rows, n, first);       // all lanes take part in the scan
  n = __shfl(n, g, 64); first = __shfl(first, g, 64);
  if (i >= elems4) return;
  f32x4 *out = (f32x4 *)dW + (int64_t)g * elems4 + i;
  f32x4 s = beta ? *out : f32x4{0.f, 0.f, 0.f, 0.f};
  // as in wgrad_reduce_block: up to eight slabs' loads in flight before the first add (one dependent load per unit made the
  // reduction riding on a short launch - the router's weight gradient - the longest part of it); same summation order
  const f32x4 *w = (const f32x4 *)ws + (int64_t)first * elems4 + i;
  int u = 0;
  for (; u + 8 <= n; u += 8) {
    f32x4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = w[(int64_t)(u + j) * elems4];
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[j];
  }
  if (u + 4 <= n) {
    f32x4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = w[(int64_t)(u + j) * elems4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s += v[j];
    u += 4;
  }
  if (u + 2 <= n) {
    const f32x4 v0 = w[(int64_t)u * elems4], v1 = w[(int64_t)(u + 1) * elems4];
    s += v0; s += v1;
    u += 2;
  }
  if (u < n) s += w[(int64_t)u * elems4];
  *out = s;
}

// The previous call's slab reduction riding in front of a weight-gradient launch: the grid's first rd_zslices z slices
// are reduce blocks (dispatched first; a few microseconds of streaming), the rest is the launch proper with its z index
// shifted down.  Returns true for a reduce block (which is then done).  What it replaces: one extra launch per
// weight-gradient GEMM (110 per step) whose ~8 us were mostly launch boundary and ramp.
__device__ __forceinline__ bool wgrad_ride_along(const WgradDev &p, int tid, int &bz, int &gz) {
  bz = blockIdx.z; gz = gridDim.z;
  if (p.rd_blocks <= 0) return false;
  if (bz < p.rd_zslices) {
    const int rid = blockIdx.x + (int)gridDim.x * (blockIdx.y + (int)gridDim.y * bz);
    if (rid < p.rd_blocks) {
      const int g = rid / p.rd_nbx, bx = rid - g * p.rd_nbx;
      if (p.rd_n > 1) {
        const float *ws = p.rd_tab0.ws, *bws = p.rd_tab0.bws;
        float *dW = p.rd_tab0.dW, *db = p.rd_tab0.db;
        int64_t e4 = p.rd_tab0.e4;
        int b4 = p.rd_tab0.b4, nbw = p.rd_tab0.nbw, first = p.rd_tab0.first, beta = p.rd_tab0.beta;
        // every entry is read, then chosen by value: reads under the condition come out as a choice between ADDRESSES of
        // table entries, and the table then stays in scratch, written there by every workgroup of every launch
#define M3_RD_FROM(j)                                                                                                   \
  {                                                                                                                     \
    const float *ws_ = p.rd_tab##j.ws, *bws_ = p.rd_tab##j.bws;                                                         \
    float *dW_ = p.rd_tab##j.dW, *db_ = p.rd_tab##j.db;                                                                 \
    const int64_t e4_ = p.rd_tab##j.e4;                                                                                 \
    const int b4_ = p.rd_tab##j.b4, nbw_ = p.rd_tab##j.nbw, first_ = p.rd_tab##j.first, beta_ = p.rd_tab##j.beta;       \
    const bool h_ = rid >= first_;                                                                                      \
    ws = h_ ? ws_ : ws; bws = h_ ? bws_ : bws; dW = h_ ? dW_ : dW; db = h_ ? db_ : db; e4 = h_ ? e4_ : e4;              \
    b4 = h_ ? b4_ : b4; nbw = h_ ? nbw_ : nbw; first = h_ ? first_ : first; beta = h_ ? beta_ : beta;                   \
  }
        static_assert(WG_MULTI == 8, "one M3_RD_FROM per entry");
        M3_RD_FROM(1) M3_RD_FROM(2) M3_RD_FROM(3) M3_RD_FROM(4) M3_RD_FROM(5) M3_RD_FROM(6) M3_RD_FROM(7)
#undef M3_RD_FROM
        wgrad_reduce_block(rid - first, tid, ws, p.rd_splits, e4, dW, beta & 1, nbw, bws, b4, db, beta >> 1, p.rd_cols);
      } else if (p.rd_chunk)
        wgrad_reduce_grouped_block(bx, g, tid, p.rd_ws, p.rd_off, p.rd_G, p.rd_chunk, p.rd_e4, p.rd_dW, p.rd_beta, p.rd_nbw,
                                   p.rd_bws, p.rd_b4, p.rd_db, p.rd_beta_db);
      else
        wgrad_reduce_block(bx, tid, p.rd_ws, p.rd_splits, p.rd_e4, p.rd_dW, p.rd_beta, p.rd_nbw, p.rd_bws, p.rd_b4, p.rd_db,
                           p.rd_beta_db, p.rd_cols);
    }
    return true;
  }
  bz -= p.rd_zslices; gz -= p.rd_zslices;
  return false;
}

// a 16-byte chunk of T times a per-row factor (the gate score of a routed row: the combine's backward d y = score * d out
// applied where the row enters the LDS image, so that the scaled [T*k, D] copy never exists in memory)
template <typename T> __device__ __forceinline__ u32x4 scale_chunk(u32x4 v, float s);
template <> __device__ __forceinline__ u32x4 scale_chunk<half_t>(u32x4 v, float s) {
  // fp32 product, ONE rounding - the value the dgrad GEMM's fp32 epilogue forms for the same row (a fp16 multiply would round
  // the score to 11 bits first: the two consumers of d y = score * d out would then see different rows)
  f16x8 f = __builtin_bit_cast(f16x8, v);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (half_t)((float)f[j] * s);
  return __builtin_bit_cast(u32x4, f);
}
template <> __device__ __forceinline__ u32x4 scale_chunk<bf16_t>(u32x4 v, float s) {
  bf16x8 f = __builtin_bit_cast(bf16x8, v);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (bf16_t)((float)f[j] * s);
  return __builtin_bit_cast(u32x4, f);
}
template <> __device__ __forceinline__ u32x4 scale_chunk<float>(u32x4 v, float s) {
  return __builtin_bit_cast(u32x4, __builtin_bit_cast(f32x4, v) * s);
}

// ---- value helpers of the 16-bit paths
// A 16-bit fragment out of a row-major LDS image: two transposed reads (ds_read_b64_tr_b16: 4 rows x 16 columns per
// 16-lane group), p0 for the lane's rows r .. r + 3 and p1 for r + 16 .. r + 19 -> the lane's 8 contraction slots
__device__ __forceinline__ f16x8 wgrad_tr16_frag(const char *p0, const char *p1) {
  typedef __attribute__((address_space(3))) fp16x4_t lds_h4;
  const fp16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h4 *)p0);
  const fp16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h4 *)p1);
  f16x8 f;
  f[0] = (half_t)lo[0]; f[1] = (half_t)lo[1]; f[2] = (half_t)lo[2]; f[3] = (half_t)lo[3];
  f[4] = (half_t)hi[0]; f[5] = (half_t)hi[1]; f[6] = (half_t)hi[2]; f[7] = (half_t)hi[3];
  return f;
}
// a + the sum of a dC fragment's 8 (fp32: 4) contraction rows - the lane's share of a column sum: four v_dot2 with a pair of
// ones (fp32: three adds)
template <typename T> __device__ __forceinline__ float wgrad_colsum8(const typename Mma<T>::frag &f, float a) {
  typedef T t2 __attribute__((ext_vector_type(2)));
  if constexpr (sizeof(T) == 4) {
    return a + ((f[0] + f[1]) + (f[2] + f[3]));
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const t2 pr = t2{f[2 * j], f[2 * j + 1]};
      if constexpr (std::is_same<T, half_t>::value)
        a = __builtin_amdgcn_fdot2(pr, t2{(T)1, (T)1}, a, false);
      else if constexpr (std::is_same<T, bf16_t>::value)
        a = __builtin_amdgcn_fdot2_f32_bf16(pr, t2{(T)1.f, (T)1.f}, a, false);
    }
    return a;
  }
}
// the per-row factors of a fp16 fragment's 8 contraction slots (rows r .. r + 3 and r + 16 .. r + 19), rounded to fp16
__device__ __forceinline__ f16x8 wgrad_factor_f16x8(f32x4 s0, f32x4 s1) {
  return f16x8{(half_t)s0[0], (half_t)s0[1], (half_t)s0[2], (half_t)s0[3], (half_t)s1[0], (half_t)s1[1], (half_t)s1[2], (half_t)s1[3]};
}

// ------------------------------------------------------------------------------------------------ host side
// the kernel that takes a call (wgrad.hip: wgrad_kernel_of_shape names it, wgrad_demote steps down where it cannot run the call)
enum WgradKernel { WGRAD_STAGED, WGRAD_DMA, WGRAD_BIG, WGRAD_SKINNY };

// A tile-kernel family states its instances ONCE, as a struct with
//   template <typename T, bool GC, bool GA, bool SC> static const void *instance();
// that returns the kernel where the family has the combination and nullptr where it has not (by `if constexpr`: only the
// kernels named there are compiled).  wgrad_each_instance calls f(dtype, gc, ga, sc, kernel) for those that exist; the
// launch and the attribute calls both go through it.
template <typename T> constexpr int wgrad_dtype_of = std::is_same<T, half_t>::value ? M3_F16 : std::is_same<T, bf16_t>::value ? M3_BF16 : M3_F32;
template <typename Fam, typename T, int I = 0, typename F> static inline void wgrad_each_flags(F &f) {
  if constexpr (I < 8) {
    constexpr bool GC = (I & 1) != 0, GA = (I & 2) != 0, SC = (I & 4) != 0;
    if (const void *k = Fam::template instance<T, GC, GA, SC>()) f(wgrad_dtype_of<T>, GC, GA, SC, k);
    wgrad_each_flags<Fam, T, I + 1>(f);
  }
}
template <typename Fam, typename F> static inline void wgrad_each_instance(F f) {
  wgrad_each_flags<Fam, half_t>(f); wgrad_each_flags<Fam, bf16_t>(f); wgrad_each_flags<Fam, float>(f);
}
// launches the family's instance for (dtype, gc, ga, sc); a call without one is an error
template <typename Fam>
static inline int wgrad_launch_instance(int dtype, bool gc, bool ga, bool sc, dim3 grid, dim3 block, size_t lds, WgradDev d, hipStream_t s) {
  const void *kernel = nullptr;
  wgrad_each_instance<Fam>([&](int dt, bool c, bool a, bool f, const void *k) { if (dt == dtype && c == gc && a == ga && f == sc) kernel = k; });
  M3_REQUIRE(kernel, "m3_wgrad_tn: no kernel instance for dtype %d, gathers (%d, %d), per-row factor %d", dtype, gc, ga, sc);
  void *args[] = {&d};
  (void)hipLaunchKernel(kernel, grid, block, args, lds, s);
  return check_launch("m3_wgrad_tn");
}

// The launchers: `grid` as m3_wgrad_tn sizes it for the family's tile; gc / ga: gathered dC / A rows, sc: per-row factor
int launch_wgrad_staged(int dtype, bool gc, bool ga, bool sc, dim3 grid, const WgradDev &d, hipStream_t s);   // wgrad_staged.hip
int launch_wgrad_dma(int dtype, bool gc, bool ga, bool sc, dim3 grid, const WgradDev &d, hipStream_t s);      // wgrad_dma.hip
int launch_wgrad_big(int dtype, bool gc, bool ga, bool sc, dim3 grid, const WgradDev &d, hipStream_t s);
int launch_wgrad_multi(int dtype, dim3 grid, const WgradMultiDev &d, hipStream_t s);                          // wgrad_multi.hip

}  // namespace m3
