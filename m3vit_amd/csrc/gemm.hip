// Grouped / dense "NT" GEMM for gfx950:  C[m,n] = epi( sum_k A[arow(m),k] * B[g][n,k] ) - the host entry m3_gemm_nt.
//
// Replaces the per-expert cuBLAS loop behind FMoELinear (reference call sites
// models/moe/ckpt/custom_moe_layer.py:32-33,41,43), the row gather/scatter of
// MOEScatter/MOEGather (custom_moe_layer.py:263-265) which is fused into the operand
// load / the store, and the nn.Linear GEMMs of the attention block and the dense Mlp
// (models/moe/ckpt/vision_transformer_moe.py:255-261,295-313).
//
// This file validates a call, fills the kernels' argument block and decides the epilogue kind, the kernel and the tile
// order; the kernels and their launch functions are in gemm_staged.hip, gemm_dma.hip and gemm_big.hip (gemm_dev.h).
#include <stdlib.h>
#include "gemm_dev.h"

using namespace m3;

// Environment switches, read once (diagnostics; the default is what is measured and shipped)
struct GemmEnv {
  int band;        // M3_GEMM_BAND=n: n row tiles per band of the tile order everywhere (1 = row-tile major); unset: by weight size
  bool dma;        // M3_GEMM_DMA=0: no LDS-DMA kernel, the register-staged one takes the 16-bit launches too
  bool tall;       // M3_GEMM_F32_TALL=0: no 160-row fp32 tiles
};
static int env_int(const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; }
static const GemmEnv &gemm_env() {
  static const GemmEnv env = {env_int("M3_GEMM_BAND", 0), env_int("M3_GEMM_DMA", 1) != 0, env_int("M3_GEMM_F32_TALL", 1) != 0};
  return env;
}

// The 256 x 256 kernel: 0 never, 1 whenever it can run the shape, 2 (default) when the shape also has enough tiles to fill
// the chip twice.  Not part of GemmEnv: m3_gemm_set_big(-1) has the next call read M3_GEMM_BIG again
static int g_big_mode = -1;
extern "C" int m3_gemm_set_big(int mode) {
  M3_REQUIRE(mode >= -1 && mode <= 2, "m3_gemm_set_big: mode %d out of range", mode);
  g_big_mode = mode;
  return M3_OK;
}

// The epilogue kind of a 16-bit call (gemm_dev.h); anything else takes the run-time-flag epilogue
static int epilogue_kind(const m3_gemm_args *a) {
  if (dtype_size(a->dtype) != 2) return DMA_EPI_ANY;
  const bool c_f32 = a->c_dtype == M3_F32, none = a->act == M3_ACT_NONE && !a->pre_out;
  if (none && a->gelu_grad_pre && !a->residual && !c_f32 && !a->bias) return DMA_EPI_GPRE;
  if (none && a->residual && !a->gelu_grad_pre && c_f32) return DMA_EPI_RES;
  if (none && !a->gelu_grad_pre && !a->residual && !c_f32) return DMA_EPI_PLAIN;
  if (a->act == M3_ACT_GELU && a->pre_out && !a->gelu_grad_pre && !a->residual && !c_f32) return DMA_EPI_GELU;
  return DMA_EPI_ANY;
}

enum GemmKernel { GEMM_BIG, GEMM_DMA, GEMM_STAGED, GEMM_STAGED_TALL };

// Which kernel takes the call (d: everything but the tile order)
static GemmKernel choose_kernel(const GemmDev &d, int dtype) {
  const GemmEnv &env = gemm_env();
  const int es = dtype_size(dtype);
  // long contractions (the ViT-Base shapes): 256 x 256 tiles
  if (g_big_mode < 0) g_big_mode = env_int("M3_GEMM_BIG", 2);
  if (g_big_mode && gemm_big_eligible(d, es, g_big_mode == 1)) return GEMM_BIG;
  // 16-bit -> LDS-DMA kernel; fp32 (MFMA-bound, measured 2 % slower there) and odd shapes -> register-staged kernel
  if (env.dma && es == 2 && d.vec8 && (d.K * es) % ROWB == 0) return GEMM_DMA;
  // fp32, dense, whole K slices: 160-row tiles where they even out the last round.  The busiest CU's share of the rows -
  // ceil(tiles / 256 CUs) x tile rows - decides an MFMA-bound launch
  if (env.tall && dtype == M3_F32 && (d.K * es) % ROWB == 0 && !d.group_offsets) {
    const int64_t nt = (d.N + BN - 1) / BN, t128 = (d.M + 127) / 128 * nt, t160 = (d.M + 159) / 160 * nt;
    if ((t160 + 255) / 256 * 160 < (t128 + 255) / 256 * 128) return GEMM_STAGED_TALL;
  }
  return GEMM_STAGED;
}

// What m3_gemm_nt does with a call, short of launching it: the checks, the kernels' argument block (pointers are copied,
// never read), the kernel, the epilogue kind it is launched with and the tile order.  m3_gemm_nt launches from it,
// m3_gemm_plan reports it
struct GemmLaunch { GemmDev d; GemmKernel kernel; int epi, tile_m, tile_n; bool empty; };
static int gemm_prepare(const m3_gemm_args *a, const char *who, GemmLaunch &L) {
  M3_REQUIRE(a && a->A && a->B && a->C, "%s: null operand", who);
  M3_REQUIRE(dtype_ok(a->dtype), "%s: bad dtype %d", who, a->dtype);
  const int es = dtype_size(a->dtype);
  M3_REQUIRE(a->M >= 0 && a->N > 0 && a->K > 0, "%s: bad shape M=%lld N=%d K=%d", who, (long long)a->M, a->N, a->K);
  M3_REQUIRE((a->K * es) % 16 == 0, "%s: K*elem (%d) must be a multiple of 16 bytes", who, a->K * es);
  M3_REQUIRE((a->lda * es) % 16 == 0 && (a->ldb * es) % 16 == 0, "%s: lda/ldb rows must be 16-byte aligned", who);
  M3_REQUIRE(((uintptr_t)a->A % 16) == 0 && ((uintptr_t)a->B % 16) == 0 && ((uintptr_t)a->C % 16) == 0,
             "%s: operands must be 16-byte aligned", who);
  M3_REQUIRE(a->N % 4 == 0 && a->ldc % 4 == 0, "%s: N and ldc must be multiples of 4", who);
  M3_REQUIRE(a->lda >= a->K && a->ldb >= a->K && a->ldc >= a->N, "%s: leading dimension too small", who);
  M3_REQUIRE(a->c_dtype == M3_F32 || a->c_dtype == a->dtype, "%s: c_dtype must be f32 or the operand dtype", who);
  M3_REQUIRE(a->G >= 1, "%s: G must be >= 1", who);
  M3_REQUIRE((a->group_offsets == nullptr) == (a->tile_starts == nullptr), "%s: group_offsets/tile_starts go together", who);
  M3_REQUIRE(a->G == 1 || a->group_offsets, "%s: grouped call needs group_offsets", who);
  M3_REQUIRE(!a->a_row_idx || a->a_row_div >= 1, "%s: a_row_div must be >= 1", who);
  M3_REQUIRE(!a->pre_out || a->ld_pre % 4 == 0, "%s: ld_pre %% 4", who);
  M3_REQUIRE(!a->gelu_grad_pre || a->ld_gpre % 4 == 0, "%s: ld_gpre %% 4", who);
  M3_REQUIRE(!a->residual || a->ld_res % 4 == 0, "%s: ld_res %% 4", who);
  M3_REQUIRE(!a->row_scale || a->row_scale_div >= 1, "%s: row_scale_div must be >= 1", who);
  L.empty = a->M == 0;
  if (L.empty) return M3_OK;

  GemmDev &d = L.d;
  d.A = (const char *)a->A; d.lda_b = a->lda * es;
  d.a_row_idx = a->a_row_idx; d.a_row_div = a->a_row_idx ? a->a_row_div : 1;
  d.a_row_sh = div_shift(d.a_row_div);
  d.B = (const char *)a->B; d.ldb_b = a->ldb * es; d.b_group_b = (int64_t)a->N * a->ldb * es;
  d.C = (char *)a->C; d.ldc = a->ldc; d.c_f32 = (a->c_dtype == M3_F32) ? 1 : 0;
  d.c_row_idx = a->c_row_idx;
  d.bias = a->bias;
  d.pre_out = (char *)a->pre_out; d.ld_pre = a->ld_pre;
  d.gpre = (const char *)a->gelu_grad_pre; d.ld_gpre = a->ld_gpre;
  d.residual = a->residual; d.ld_res = a->ld_res;
  d.row_scale = a->row_scale; d.row_scale_div = a->row_scale ? a->row_scale_div : 1;
  d.row_scale_idx = a->row_scale ? a->row_scale_idx : nullptr;
  d.row_scale_sh = div_shift(d.row_scale_div);
  d.act = a->act;
  d.M = a->M; d.N = a->N; d.K = a->K; d.G = a->G;
  d.group_offsets = a->group_offsets; d.tile_starts = a->tile_starts;
  d.a_seg_tiles = 0; d.a_seg_jump_b = 0;
  d.vec8 = (a->N % 8 == 0 && a->ldc % 8 == 0 && (!a->pre_out || a->ld_pre % 8 == 0) &&
            (!a->gelu_grad_pre || a->ld_gpre % 8 == 0) && (!a->residual || a->ld_res % 8 == 0)) ? 1 : 0;
  // 32-bit per-lane byte offsets: A rows (gathered source rows must be < M) and one B group must fit 4 GiB
  M3_REQUIRE((a->M + 1) * a->lda * es < ((int64_t)1 << 32) && (int64_t)a->N * a->ldb * es < ((int64_t)1 << 32),
             "%s: operand panel exceeds the 4 GiB reach of the 32-bit lane offsets", who);
  // 32-bit rows in the kernels' prologues (row clamps, the row of the per-row factor)
  M3_REQUIRE(a->M < ((int64_t)1 << 31), "%s: M %lld does not fit 32 bits", who, (long long)a->M);

  const GemmKernel kernel = L.kernel = choose_kernel(d, a->dtype);
  // the register-staged kernels have the run-time-flag epilogue only
  L.epi = kernel == GEMM_BIG || kernel == GEMM_DMA ? epilogue_kind(a) : DMA_EPI_ANY;
  // tile order (gemm_dev.h: tile_of) of the kernel chosen.  128-row tiles: bands of four row tiles when a group's weight
  // does not fit an XCD's L2 beside the rows (> 2 MB: the ViT-Base N = 2304 / 3072 launches and K = 3072).  256-row tiles:
  // row-tile major always - a tile's A rows at K >= 2048 are 1 MB and more, four of them do not sit in an L2 (counters:
  // banded +13 % fetch).  A grouped call's grid is sized for the upper bound of row tiles: one partial tile per group
  const int tile_m = L.tile_m = kernel == GEMM_BIG ? BIG_B : kernel == GEMM_STAGED_TALL ? 160 : BM;
  const int tile_n = L.tile_n = kernel == GEMM_BIG ? BIG_B : BN;
  const int band = gemm_env().band > 0 ? gemm_env().band : ((int64_t)a->N * a->K * es > ((int64_t)2 << 20) ? 4 : 1);
  const int64_t mt = (a->M + tile_m - 1) / tile_m + (a->group_offsets ? a->G : 0);
  d.n_tiles = (a->N + tile_n - 1) / tile_n;
  d.m_band = kernel == GEMM_BIG ? 1 : band;
  M3_REQUIRE(mt * d.n_tiles < (int64_t)1 << 30, "%s: grid too large", who);
  d.m_tiles_max = (int)mt;
  return M3_OK;
}

extern "C" int m3_gemm_nt(const m3_gemm_args *a, void *stream) {
  GemmLaunch L;
  if (int rc = gemm_prepare(a, "m3_gemm_nt", L)) return rc;
  if (L.empty) return M3_OK;
  hipStream_t s = (hipStream_t)stream;
  switch (L.kernel) {
    case GEMM_BIG: return launch_gemm_big(L.d, a->dtype, L.epi, s);
    case GEMM_DMA: return launch_gemm_dma(L.d, a->dtype, L.epi, s);
    default: return launch_gemm_staged(L.d, a->dtype, L.kernel == GEMM_STAGED_TALL, s);
  }
}

extern "C" int m3_gemm_plan(const m3_gemm_args *a, m3_gemm_plan_out *p) {
  M3_REQUIRE(p, "m3_gemm_plan: null output");
  GemmLaunch L;
  if (int rc = gemm_prepare(a, "m3_gemm_plan", L)) return rc;
  *p = m3_gemm_plan_out{};
  p->kernel = M3_GEMM_NONE;
  if (L.empty) return M3_OK;
  p->kernel = L.kernel == GEMM_BIG ? M3_GEMM_BIG : L.kernel == GEMM_DMA ? M3_GEMM_DMA : L.kernel == GEMM_STAGED_TALL ? M3_GEMM_STAGED_TALL : M3_GEMM_STAGED;
  p->epilogue = L.epi; p->tile_m = L.tile_m; p->tile_n = L.tile_n; p->m_band = L.d.m_band; p->vec8 = L.d.vec8;
  p->n_tiles = L.d.n_tiles; p->m_tiles_max = L.d.m_tiles_max;
  return M3_OK;
}
