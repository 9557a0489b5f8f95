// ReLU + bilinear x2 up-sampling (align_corners = False) in ONE pass, and its backward, for channels-last activations:
// the element-wise half of a decoder-head stage of the reference, models/heads/vit_up_head.py:181-214
//     x = F.relu(syncbn_fc_i(conv_i(x)), inplace=True) ; x = F.interpolate(x, size=x.shape[-1]*2, mode='bilinear')
// ("MIOpen first, custom later").  Under fp16 autocast torch runs the resize in fp32 (its output
// and the gradient that comes back are fp32 tensors 4x the stage's input, with a cast kernel each way) and its backward as a
// generic scatter: at 8 x 480 x 640 the resizes and the casts around them are ~6.5 of the head's 13.7 ms forward + backward.
// Here the 16-bit activations go in and come out (fp32 output optional, for the classifier stage), HBM-bound by design:
//
//   forward : thread = 8 (16-bit) / 4 (fp32) channels of one INPUT pixel: 3 x 3 neighbourhood (replicate-clamped: the
//             align_corners=False source coordinate (o + 0.5) / 2 - 0.5 clamped at 0 is exactly "weights 0.25 / 0.75 on the
//             clamped neighbours"), ReLU on the way in, the 2 x 2 output pixels it owns written as 16-byte vectors;
//   backward: thread = the same channels of one input pixel: the 4 x 4 window of output gradients it fed (rows 2i-1 .. 2i+2
//             with weights .25 .75 .75 .25, indices clamped - the clamped neighbours' share comes back to the border pixel),
//             times the ReLU mask recomputed from x.  A gather: deterministic, no atomics.
// Channels-last ([N, H, W, C], C a multiple of the vector width): consecutive lanes walk C, so every access of a wave is a
// run of whole cache lines.
#include "common.h"

namespace m3 {

constexpr int RZ_BYTES = 16;           // a thread's channels are one 16-byte vector of the INPUT dtype: Pack<T, RZ_BYTES / sizeof(T)>;
                                       // an fp32 output or gradient of a 16-bit input is the same count, two 16-byte accesses

// BORD: y is a zero-bordered image [N, 2H+2, 2W+2, C] whose interior is written (the operand layout of conv.hip; the border is
// the caller's and is not touched)
template <typename T, typename TO, bool RELU, bool BORD = false>
__global__ __launch_bounds__(256) void relu_up2x_fwd_kernel(const T *__restrict__ x, int64_t total, int H, int W, int C,
                                                            TO *__restrict__ y) {
  constexpr int NV = RZ_BYTES / (int)sizeof(T);
  const int CV = C / NV;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int cv = (int)(t % CV);
  int64_t r = t / CV;
  const int ix = (int)(r % W); r /= W;
  const int iy = (int)(r % H);
  const int64_t n = r / H;
  const int ym = iy > 0 ? iy - 1 : 0, yp = iy + 1 < H ? iy + 1 : H - 1;
  const int xm = ix > 0 ? ix - 1 : 0, xp = ix + 1 < W ? ix + 1 : W - 1;
  const T *base = x + (n * H * (int64_t)W) * C + cv * NV;
  const int rows[3] = {ym, iy, yp}, cols[3] = {xm, ix, xp};
  float z[3][3][NV];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      Pack<T, NV>::load(base + ((int64_t)rows[a] * W + cols[b]) * C, z[a][b]);
      if (RELU) {
#pragma unroll
        for (int j = 0; j < NV; ++j) z[a][b][j] = z[a][b][j] <= 0.f ? 0.f : z[a][b][j];      // F.relu: a NaN stays a NaN
      }
    }
  // horizontal blends of every row: h[a][0] -> output column 2*ix, h[a][1] -> 2*ix + 1
  float h[3][2][NV];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      h[a][0][j] = 0.25f * z[a][0][j] + 0.75f * z[a][1][j];
      h[a][1][j] = 0.75f * z[a][1][j] + 0.25f * z[a][2][j];
    }
  constexpr int PAD = BORD ? 1 : 0;
  TO *out = y + ((n * (2 * H + 2 * PAD) + 2 * iy + PAD) * (2 * (int64_t)W + 2 * PAD) + 2 * ix + PAD) * C + cv * NV;
  const int64_t orow = (2 * (int64_t)W + 2 * PAD) * C;
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    float o0[NV], o1[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      o0[j] = 0.25f * h[0][b][j] + 0.75f * h[1][b][j];
      o1[j] = 0.75f * h[1][b][j] + 0.25f * h[2][b][j];
    }
    Pack<TO, NV>::store(out + b * C, o0);
    Pack<TO, NV>::store(out + orow + b * C, o1);
  }
}

template <typename T, typename TG, bool RELU>
__global__ __launch_bounds__(256) void relu_up2x_bwd_kernel(const TG *__restrict__ dy, const T *__restrict__ x, int64_t total,
                                                            int H, int W, int C, T *__restrict__ dx) {
  constexpr int NV = RZ_BYTES / (int)sizeof(T);
  const int CV = C / NV;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int cv = (int)(t % CV);
  int64_t r = t / CV;
  const int ix = (int)(r % W); r /= W;
  const int iy = (int)(r % H);
  const int64_t n = r / H;
  const int H2 = 2 * H, W2 = 2 * W;
  const float wgt[4] = {0.25f, 0.75f, 0.75f, 0.25f};
  int oy[4], ox[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    int v = 2 * iy - 1 + a;
    oy[a] = v < 0 ? 0 : (v >= H2 ? H2 - 1 : v);
    v = 2 * ix - 1 + a;
    ox[a] = v < 0 ? 0 : (v >= W2 ? W2 - 1 : v);
  }
  const TG *gbase = dy + (n * H2 * (int64_t)W2) * C + cv * NV;
  float acc[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    float rowacc[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) rowacc[j] = 0.f;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      float g[NV];
      Pack<TG, NV>::load(gbase + ((int64_t)oy[a] * W2 + ox[b]) * C, g);
#pragma unroll
      for (int j = 0; j < NV; ++j) rowacc[j] += wgt[b] * g[j];
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] += wgt[a] * rowacc[j];
  }
  const int64_t off = ((n * H + iy) * (int64_t)W + ix) * C + cv * NV;
  if (RELU) {
    float xv[NV];
    Pack<T, NV>::load(x + off, xv);
#pragma unroll
    for (int j = 0; j < NV; ++j) acc[j] = xv[j] <= 0.f ? 0.f : acc[j];      // torch's threshold_backward: the gradient passes where x is NaN
  }
  Pack<T, NV>::store(dx + off, acc);
}

}  // namespace m3

using namespace m3;

static bool rz_shape_ok(int dtype, int64_t N, int H, int W, int C) {
  const int nv = dtype == M3_F32 ? 4 : 8;
  return N >= 0 && H >= 1 && W >= 1 && C >= nv && C % nv == 0 && N * H * (int64_t)W * C < ((int64_t)1 << 40);
}

extern "C" int m3_relu_up2x_fwd(const void *x, int x_dtype, int64_t N, int H, int W, int C, int relu, void *y, int y_dtype,
                                void *stream) {
  M3_REQUIRE(x && y, "m3_relu_up2x_fwd: null operand");
  M3_REQUIRE(dtype_ok(x_dtype) && (y_dtype == x_dtype || y_dtype == M3_F32), "m3_relu_up2x_fwd: output dtype is the input's or fp32");
  M3_REQUIRE(rz_shape_ok(x_dtype, N, H, W, C), "m3_relu_up2x_fwd: C must be a multiple of 8 (16-bit) / 4 (fp32)");
  M3_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0, "m3_relu_up2x_fwd: 16-byte aligned tensors");
  if (N == 0) return M3_OK;
  hipStream_t s = (hipStream_t)stream;
  by_dtype(x_dtype, [&](auto tt) {
    typedef typename decltype(tt)::type T;
    const int64_t total = N * H * (int64_t)W * (C / (RZ_BYTES / (int)sizeof(T)));
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    auto go = [&](auto to, auto r) {
      typedef typename decltype(to)::type TO;
      hipLaunchKernelGGL((relu_up2x_fwd_kernel<T, TO, decltype(r)::value != 0>), grid, block, 0, s, (const T *)x, total, H, W, C,
                         (TO *)y);
    };
    auto with_out = [&](auto to) { if (relu) go(to, IntTag<1>{}); else go(to, IntTag<0>{}); };
    if (y_dtype == M3_F32) with_out(DtypeTag<float>{}); else with_out(tt);
  });
  return check_launch("m3_relu_up2x_fwd");
}

extern "C" int m3_relu_up2x_fwd_bordered(const void *x, int dtype, int64_t N, int H, int W, int C, int relu, void *yb, void *stream) {
  M3_REQUIRE(x && yb, "m3_relu_up2x_fwd_bordered: null operand");
  M3_REQUIRE(dtype == M3_F16 || dtype == M3_BF16, "m3_relu_up2x_fwd_bordered: 16-bit activations only");
  M3_REQUIRE(rz_shape_ok(dtype, N, H, W, C) && N * (2 * H + 2) * (2 * (int64_t)W + 2) * C < ((int64_t)1 << 40),
             "m3_relu_up2x_fwd_bordered: C must be a multiple of 8");
  M3_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)yb % 16) == 0, "m3_relu_up2x_fwd_bordered: 16-byte aligned tensors");
  if (N == 0) return M3_OK;
  hipStream_t s = (hipStream_t)stream;
  by_dtype(dtype, [&](auto tt) {
    typedef typename decltype(tt)::type T;
    if constexpr (sizeof(T) == 2) {
      const int64_t total = N * H * (int64_t)W * (C / (RZ_BYTES / (int)sizeof(T)));
      const dim3 grid((unsigned)((total + 255) / 256)), block(256);
      if (relu) hipLaunchKernelGGL((relu_up2x_fwd_kernel<T, T, true, true>), grid, block, 0, s, (const T *)x, total, H, W, C, (T *)yb);
      else hipLaunchKernelGGL((relu_up2x_fwd_kernel<T, T, false, true>), grid, block, 0, s, (const T *)x, total, H, W, C, (T *)yb);
    }
  });
  return check_launch("m3_relu_up2x_fwd_bordered");
}

extern "C" int m3_relu_up2x_bwd(const void *dy, int dy_dtype, const void *x, int x_dtype, int64_t N, int H, int W, int C,
                                int relu, void *dx, void *stream) {
  M3_REQUIRE(dy && dx && (x || !relu), "m3_relu_up2x_bwd: null operand");
  M3_REQUIRE(dtype_ok(x_dtype) && (dy_dtype == x_dtype || dy_dtype == M3_F32), "m3_relu_up2x_bwd: gradient dtype is the input's or fp32");
  M3_REQUIRE(rz_shape_ok(x_dtype, N, H, W, C), "m3_relu_up2x_bwd: C must be a multiple of 8 (16-bit) / 4 (fp32)");
  M3_REQUIRE(((uintptr_t)dy % 16) == 0 && ((uintptr_t)dx % 16) == 0 && ((uintptr_t)x % 16) == 0, "m3_relu_up2x_bwd: 16-byte aligned tensors");
  if (N == 0) return M3_OK;
  hipStream_t s = (hipStream_t)stream;
  by_dtype(x_dtype, [&](auto tt) {
    typedef typename decltype(tt)::type T;
    const int64_t total = N * H * (int64_t)W * (C / (RZ_BYTES / (int)sizeof(T)));
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    auto go = [&](auto tg, auto r) {
      typedef typename decltype(tg)::type TG;
      hipLaunchKernelGGL((relu_up2x_bwd_kernel<T, TG, decltype(r)::value != 0>), grid, block, 0, s, (const TG *)dy, (const T *)x,
                         total, H, W, C, (T *)dx);
    };
    auto with_grad = [&](auto tg) { if (relu) go(tg, IntTag<1>{}); else go(tg, IntTag<0>{}); };
    if (dy_dtype == M3_F32) with_grad(DtypeTag<float>{}); else with_grad(tt);
  });
  return check_launch("m3_relu_up2x_bwd");
}
