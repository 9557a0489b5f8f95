// 3 x 3, stride 1, padding 1 convolutions of the decoder heads (reference: models/heads/vit_up_head.py:181-214, conv_0..3;
// TamModule, models/models.py:11-134, layers0..3) on the project's own GEMM and weight-gradient kernels.
//
// Layout.  An activation that feeds a convolution is a ZERO-BORDERED channels-last image [N, H+2, W+2, C] (16-bit).  The
// window of output pixel (n, y, x) is then three contiguous runs of 3 C elements, one per kernel row dy, run dy starting at
// bordered pixel (n, y + dy, x); the starts of consecutive runs are one bordered image row apart.  With K ordered (dy, dx, c)
// the convolution is an NT GEMM  Y[m, co] = sum_k window(m)[k] * Wk[co, k],  M = N H W, K = 9 C, whose A rows are addressed
// through the row gather every GEMM kernel here has (a_row_idx: pixel m -> index of bordered pixel (n, y, x), leading
// dimension C) plus ONE addressing option of gemm_nt_big_kernel, the segmented A row (gemm_big.hip, SEG): the source of K
// tile kt moves by (kt / seg_tiles) * seg_jump bytes, seg_tiles = 3 C * 2 / 128, seg_jump = the bordered row pitch minus 3 C
// elements.  The border makes padding and image boundaries free: no masks, no bleed between images.
//   forward   A = bordered x,  B = weight.permute(0, 2, 3, 1) as [Cout, 9 C],  epilogue PLAIN (+ fp32 bias), Y dense [M, Cout]
//   dgrad     the same entry: A = bordered dY, B = the weight flipped in both spatial directions as [C, 9 Cout], dX dense [M, C]
//   wgrad     dW[co, (dy, dx, c)] = sum_m dY[m, co] * window(m): three m3_wgrad_tn problems, one per dy (N = Cout, K = 3 C, A
//             offset by dy bordered rows, the same pixel table, leading dimension C), the bias gradient riding on the first;
//             their slabs are summed by one m3_wgrad_reduce_multi launch.  The weight-gradient kernels only READ A through
//             (row, column) addresses, so rows that overlap in memory are no concern of theirs.
// Also here: the pixel table and the dense -> bordered copy.  The bordered form of the ReLU + x2 stage is in resize.hip.
#include "gemm_dev.h"

namespace m3 {

// idx[m] = bordered pixel index of output pixel m = (n, y, x): the top-left tap of its window
__global__ __launch_bounds__(256) void conv_pixel_index_kernel(int64_t M, int H, int W, int32_t *__restrict__ idx) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const int x = (int)(m % W);
  const int64_t r = m / W;
  const int y = (int)(r % H);
  const int64_t n = r / H;
  idx[m] = (int32_t)((n * (H + 2) + y) * (W + 2) + x);
}

// dense [N, H, W, C] -> zero-bordered [N, H+2, W+2, C]: a thread per 16-byte vector of the OUTPUT (the border is written here)
__global__ __launch_bounds__(256) void pad_border_kernel(const u32x4 *__restrict__ x, int64_t total, int H, int W, int CV,
                                                         u32x4 *__restrict__ xb) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int cv = (int)(t % CV);
  int64_t r = t / CV;
  const int bx = (int)(r % (W + 2)); r /= (W + 2);
  const int by = (int)(r % (H + 2));
  const int64_t n = r / (H + 2);
  u32x4 v = u32x4{0u, 0u, 0u, 0u};
  if (bx >= 1 && bx <= W && by >= 1 && by <= H) v = x[((n * H + (by - 1)) * (int64_t)W + (bx - 1)) * CV + cv];
  xb[t] = v;
}

}  // namespace m3

using namespace m3;

static const int64_t REACH = (int64_t)1 << 32;      // the 32-bit lane offsets of the LDS-DMA kernels

// Does a [N, H, W, C] -> Cout convolution take the GEMM path (as a forward: the input gradient is the same question with C
// and Cout swapped)?  M3_CONV_OK or the reason why not
static int conv_refusal(int dtype, int64_t N, int H, int W, int C, int Cout) {
  if (dtype != M3_F16 && dtype != M3_BF16) return M3_CONV_REFUSE_DTYPE;
  if (C < 128 || C % 128 != 0) return M3_CONV_REFUSE_CIN;              // whole, even-numbered K tiles per run
  if (Cout < 8 || Cout % 8 != 0) return M3_CONV_REFUSE_COUT;           // 16-byte output vectors
  const int64_t M = N * H * W, PB = N * (H + 2) * (int64_t)(W + 2);
  if (M >= ((int64_t)1 << 31) || PB >= ((int64_t)1 << 31) || PB * C * 2 >= REACH || (int64_t)Cout * 9 * C * 2 >= REACH ||
      (M + 255) / 256 * ((Cout + 255) / 256) >= ((int64_t)1 << 30))
    return M3_CONV_REFUSE_REACH;
  return M3_CONV_OK;
}

static int conv_shape_ok(const char *who, int64_t N, int H, int W, int C, int Cout) {
  M3_REQUIRE(N >= 0 && H >= 1 && W >= 1 && C >= 1 && Cout >= 1 && N < (1 << 20) && H < (1 << 16) && W < (1 << 16) && C < (1 << 20) &&
             Cout < (1 << 20), "%s: bad shape N=%lld H=%d W=%d C=%d Cout=%d", who, (long long)N, H, W, C, Cout);
  // (the pixel table is int32; with this bound no product below overflows 64 bits)
  M3_REQUIRE(N * (H + 2) * (int64_t)(W + 2) < ((int64_t)1 << 31), "%s: more than 2^31 bordered pixels", who);
  return M3_OK;
}

static const char *conv_reason_text(int r) {
  switch (r) {
    case M3_CONV_REFUSE_DTYPE: return "16-bit activations only";
    case M3_CONV_REFUSE_CIN: return "input channels must be a multiple of 128";
    case M3_CONV_REFUSE_COUT: return "output channels must be a multiple of 8";
    case M3_CONV_REFUSE_REACH: return "operand past the 4 GiB reach of the 32-bit lane offsets";
    default: return "ok";
  }
}

extern "C" int m3_conv3x3_plan(int dtype, int64_t N, int H, int W, int C, int Cout, m3_conv3x3_plan_out *p) {
  M3_REQUIRE(p, "m3_conv3x3_plan: null output");
  M3_REQUIRE(dtype_ok(dtype), "m3_conv3x3_plan: bad dtype %d", dtype);
  if (int rc = conv_shape_ok("m3_conv3x3_plan", N, H, W, C, Cout)) return rc;
  *p = m3_conv3x3_plan_out{};
  p->kernel = M3_GEMM_NONE;
  p->reason = conv_refusal(dtype, N, H, W, C, Cout);
  p->ok = p->reason == M3_CONV_OK;
  if (!p->ok) return M3_OK;
  p->dgrad_ok = conv_refusal(dtype, N, H, W, Cout, C) == M3_CONV_OK;
  p->M = N * H * W;
  p->bordered_pixels = N * (H + 2) * (int64_t)(W + 2);
  p->kernel = p->M ? M3_GEMM_BIG : M3_GEMM_NONE;
  p->epilogue = M3_GEMM_EPI_PLAIN;
  p->tile_m = p->tile_n = BIG_B;
  p->m_tiles = (int32_t)((p->M + BIG_B - 1) / BIG_B);
  p->n_tiles = (Cout + BIG_B - 1) / BIG_B;
  p->seg_tiles = 3 * C * 2 / 128;
  p->k_tiles = 3 * p->seg_tiles;
  p->seg_jump_bytes = (int64_t)(W - 1) * C * 2;
  // the three weight-gradient problems: N = Cout, K = 3 C over the M pixels, each cut as m3_wgrad_plan cuts it
  int tn = 0, tk = 0;
  if (int rc = m3_wgrad_tile(Cout, 3 * C, dtype, &tn, &tk)) return rc;
  p->wgrad_tile = tn;
  m3_wgrad_shape s = {};
  s.M = p->M; s.N = Cout; s.K = 3 * C; s.G = 1; s.dtype = dtype; s.bias = 1;
  m3_wgrad_plan_out wp;
  if (int rc = m3_wgrad_plan(&s, &wp)) return rc;
  p->wgrad_splits = wp.splits;
  p->wgrad_ws_elems = (int64_t)wp.splits * Cout * (3 * (int64_t)3 * C + 1);
  return M3_OK;
}

extern "C" int m3_conv3x3_index(int64_t N, int H, int W, int32_t *idx, void *stream) {
  if (int rc = conv_shape_ok("m3_conv3x3_index", N, H, W, 1, 1)) return rc;
  const int64_t M = N * H * W;
  M3_REQUIRE(idx && N * (H + 2) * (int64_t)(W + 2) < ((int64_t)1 << 31), "m3_conv3x3_index: null table or more than 2^31 bordered pixels");
  if (M == 0) return M3_OK;
  hipLaunchKernelGGL(conv_pixel_index_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, M, H, W, idx);
  return check_launch("m3_conv3x3_index");
}

extern "C" int m3_pad_border_nhwc(const void *x, int dtype, int64_t N, int H, int W, int C, void *xb, void *stream) {
  M3_REQUIRE(x && xb, "m3_pad_border_nhwc: null operand");
  M3_REQUIRE(dtype == M3_F16 || dtype == M3_BF16, "m3_pad_border_nhwc: 16-bit activations only");
  if (int rc = conv_shape_ok("m3_pad_border_nhwc", N, H, W, C, 1)) return rc;
  M3_REQUIRE(C % 8 == 0, "m3_pad_border_nhwc: C must be a multiple of 8");
  M3_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)xb % 16) == 0, "m3_pad_border_nhwc: 16-byte aligned tensors");
  const int64_t total = N * (H + 2) * (int64_t)(W + 2) * (C / 8);
  M3_REQUIRE(total < ((int64_t)1 << 39), "m3_pad_border_nhwc: tensor too large");
  if (total == 0) return M3_OK;
  hipLaunchKernelGGL(pad_border_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const u32x4 *)x, total,
                     H, W, C / 8, (u32x4 *)xb);
  return check_launch("m3_pad_border_nhwc");
}

// forward and input gradient: one segmented-A launch of the 256 x 256 kernel
static int conv_gemm(const char *who, const void *xb, int dtype, int64_t N, int H, int W, int C, const void *w, int Cout,
                     const float *bias, const int32_t *pix_idx, void *y, void *stream) {
  M3_REQUIRE(xb && w && y && pix_idx, "%s: null operand", who);
  M3_REQUIRE(dtype_ok(dtype), "%s: bad dtype %d", who, dtype);
  if (int rc = conv_shape_ok(who, N, H, W, C, Cout)) return rc;
  const int why = conv_refusal(dtype, N, H, W, C, Cout);
  M3_REQUIRE(why == M3_CONV_OK, "%s: %s (C=%d, Cout=%d, dtype %d)", who, conv_reason_text(why), C, Cout, dtype);
  M3_REQUIRE(((uintptr_t)xb % 16) == 0 && ((uintptr_t)w % 16) == 0 && ((uintptr_t)y % 16) == 0 && ((uintptr_t)bias % 16) == 0 &&
             ((uintptr_t)pix_idx % 4) == 0, "%s: operands must be 16-byte aligned", who);
  const int64_t M = N * H * W;
  if (M == 0) return M3_OK;
  GemmDev d = {};
  d.A = (const char *)xb; d.lda_b = (int64_t)C * 2;
  d.a_row_idx = pix_idx; d.a_row_div = 1; d.a_row_sh = 0;
  d.B = (const char *)w; d.ldb_b = (int64_t)9 * C * 2; d.b_group_b = (int64_t)Cout * d.ldb_b;
  d.C = (char *)y; d.ldc = Cout; d.c_f32 = 0;
  d.bias = bias;
  d.row_scale_div = 1;
  d.act = M3_ACT_NONE;
  d.M = M; d.N = Cout; d.K = 9 * C; d.G = 1;
  d.n_tiles = (Cout + BIG_B - 1) / BIG_B;
  d.m_band = 1;
  d.m_tiles_max = (int32_t)((M + BIG_B - 1) / BIG_B);
  d.vec8 = 1;
  d.a_seg_tiles = 3 * C * 2 / 128;                       // C % 128 == 0: an even number, run boundaries on even K tiles
  d.a_seg_jump_b = (int64_t)(W - 1) * C * 2;             // bordered row pitch (W + 2) C minus the run's 3 C elements
  return launch_gemm_big_seg(d, dtype, (hipStream_t)stream, who);
}

extern "C" int m3_conv3x3_fwd(const void *xb, int dtype, int64_t N, int H, int W, int C, const void *w, int Cout, const float *bias,
                              const int32_t *pix_idx, void *y, void *stream) {
  return conv_gemm("m3_conv3x3_fwd", xb, dtype, N, H, W, C, w, Cout, bias, pix_idx, y, stream);
}

extern "C" int m3_conv3x3_dgrad(const void *dyb, int dtype, int64_t N, int H, int W, int C, const void *w_flip, int Cout,
                                const int32_t *pix_idx, void *dx, void *stream) {
  return conv_gemm("m3_conv3x3_dgrad", dyb, dtype, N, H, W, Cout, w_flip, C, nullptr, pix_idx, dx, stream);
}

extern "C" int m3_conv3x3_wgrad(const void *xb, const void *dy, int dtype, int64_t N, int H, int W, int C, int Cout,
                                const int32_t *pix_idx, float *ws, int64_t ws_elems, float *dw3, float *db, void *stream) {
  const char *who = "m3_conv3x3_wgrad";
  M3_REQUIRE(xb && dy && pix_idx && ws && dw3, "%s: null operand", who);
  m3_conv3x3_plan_out pl;
  if (int rc = m3_conv3x3_plan(dtype, N, H, W, C, Cout, &pl)) return rc;
  M3_REQUIRE(pl.ok, "%s: %s (C=%d, Cout=%d, dtype %d)", who, conv_reason_text(pl.reason), C, Cout, dtype);
  M3_REQUIRE(ws_elems >= pl.wgrad_ws_elems, "%s: workspace of %lld floats, m3_conv3x3_plan asks for %lld", who, (long long)ws_elems,
             (long long)pl.wgrad_ws_elems);
  M3_REQUIRE(((uintptr_t)xb % 16) == 0 && ((uintptr_t)dy % 16) == 0 && ((uintptr_t)ws % 16) == 0 && ((uintptr_t)dw3 % 16) == 0 &&
             ((uintptr_t)db % 16) == 0, "%s: operands must be 16-byte aligned", who);
  const int64_t slab = (int64_t)Cout * 3 * C;            // one [Cout, 3 C] result
  if (pl.M == 0) {
    (void)hipMemsetAsync(dw3, 0, 3 * slab * sizeof(float), (hipStream_t)stream);
    if (db) (void)hipMemsetAsync(db, 0, Cout * sizeof(float), (hipStream_t)stream);
    return check_launch(who);
  }
  float *bias_ws = db ? ws + 3 * pl.wgrad_splits * slab : nullptr;
  m3_wgrad_reduce_desc rd[3];
  for (int dy_ = 0; dy_ < 3; ++dy_) {
    m3_wgrad_args a = {};
    a.dC = dy; a.lddc = Cout;
    a.A = (const char *)xb + (int64_t)dy_ * (W + 2) * C * 2; a.lda = C;
    a.a_row_idx = pix_idx; a.a_row_div = 1;
    a.M = pl.M; a.N = Cout; a.K = 3 * C; a.G = 1;
    a.splits = pl.wgrad_splits;
    a.ws = ws + dy_ * pl.wgrad_splits * slab;
    a.dtype = dtype;
    a.bias_ws = dy_ == 0 ? bias_ws : nullptr;
    if (int rc = m3_wgrad_tn(&a, stream)) return rc;
    rd[dy_] = m3_wgrad_reduce_desc{a.ws, pl.wgrad_splits, slab, nullptr, 1, 0, dw3 + dy_ * slab, 0,
                                   a.bias_ws, a.bias_ws ? (int64_t)Cout : 0, a.bias_ws ? db : nullptr, 0};
  }
  return m3_wgrad_reduce_multi(rd, 3, stream);
}
