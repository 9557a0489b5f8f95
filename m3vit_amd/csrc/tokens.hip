// Patch and token plumbing of the ViT front end for gfx950: image -> patch rows for the embedding GEMM, patch rows + cls +
// pos -> the token stream, and the backward of that assembly.  HBM-bound, 16-byte accesses along the contiguous axis.
//
//   im2row / assemble_tokens: PatchEmbed + cls/pos, models/moe/ckpt/vision_transformer_moe.py:330-341,782-791
//   the two-prefix forms (cls, dist in front of the patches: a distilled model): vision_transformer_moe.py:784-790
#include "common.h"

namespace m3 {

// rows[(b*hp + py)*wp + px][c*P*P + iy*P + ix] = img[b][c][py*P+iy][px*P+ix]
template <typename T>
__global__ void im2row_kernel(const float *__restrict__ img, int B, int Cin, int H, int W, int P, T *__restrict__ rows) {
  const int hp = H / P, wp = W / P;
  const int K = Cin * P * P;
  const int64_t total4 = (int64_t)B * hp * wp * K / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = i * 4;
    const int64_t row = e / K;
    const int kk = (int)(e - row * K);
    const int c = kk / (P * P), rem = kk - c * P * P, iy = rem / P, ix = rem - iy * P;   // ix % 4 == 0 (P % 4 == 0)
    const int px = (int)(row % wp), py = (int)((row / wp) % hp), b = (int)(row / ((int64_t)wp * hp));
    const float *s = img + (((int64_t)b * Cin + c) * H + (py * P + iy)) * W + px * P + ix;
    Vec4<T>::store(rows + e, *(const f32x4 *)s);
  }
}

// NP prefix tokens in front of the patches: token 0 = cls, token 1 = dist (NP = 2; dist is not read with NP = 1)
template <int NP>
__global__ void assemble_tokens_kernel(const float *__restrict__ patch, const float *__restrict__ cls,
                                       const float *__restrict__ dist, const float *__restrict__ pos, int B, int np_, int D,
                                       float *__restrict__ tok) {
  const int N = np_ + NP;
  const int64_t total4 = (int64_t)B * N * D / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = i * 4;
    const int d = (int)(e % D);
    const int64_t r = e / D;
    const int n = (int)(r % N), b = (int)(r / N);
    const f32x4 p = *(const f32x4 *)(pos + (int64_t)n * D + d);
    const f32x4 v = (n < NP) ? *(const f32x4 *)((NP == 2 && n == 1 ? dist : cls) + d)
                             : *(const f32x4 *)(patch + ((int64_t)b * np_ + (n - NP)) * D + d);
    *(f32x4 *)(tok + e) = v + p;
  }
}

// ---- backward of assemble_tokens: dpatch (act dtype) = dtok[:,NP:,:] ; dpos (+)= sum_b dtok ;
// dcls (+)= sum_b dtok[:,0,:] ; NP = 2: ddist (+)= sum_b dtok[:,1,:]
// thread (e, bl): 16-byte element e of a [N, D] token image, batch lane bl of TB_BL: images bl, bl + TB_BL, ... summed in that
// order, then the lanes' sums added in lane order through LDS (fixed order: deterministic).  (One thread per element
// walking all B images by itself - 74 workgroups for ViT-S - ran at 1 TB/s.)
constexpr int TB_BL = 8, TB_EL = 32;                 // batch lanes x elements per 256-thread workgroup
template <typename T, int NP>
__global__ __launch_bounds__(TB_BL * TB_EL) void tokens_bwd_kernel(const float *__restrict__ dtok, int B, int np_, int D, T *__restrict__ dpatch,
                                  float *__restrict__ dpos, float *__restrict__ dcls, float *__restrict__ ddist, int beta) {
  __shared__ f32x4 part[TB_BL][TB_EL];
  const int N = np_ + NP;
  const int64_t total4 = (int64_t)N * D / 4;
  const int el = threadIdx.x % TB_EL, bl = threadIdx.x / TB_EL;
  const int64_t i = (int64_t)blockIdx.x * TB_EL + el;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  int n = 0, d = 0;
  if (i < total4) {
    const int64_t e = i * 4;
    n = (int)(e / D); d = (int)(e - (int64_t)n * D);
    for (int b = bl; b < B; b += TB_BL) {
      const f32x4 g = *(const f32x4 *)(dtok + ((int64_t)b * N + n) * D + d);
      s += g;
      if (n >= NP && dpatch) Vec4<T>::store(dpatch + ((int64_t)b * np_ + (n - NP)) * D + d, g);
    }
  }
  part[bl][el] = s;
  __syncthreads();
  if (bl == 0 && i < total4) {
#pragma unroll
    for (int j = 1; j < TB_BL; ++j) s += part[j][el];
    f32x4 *pp = (f32x4 *)(dpos + i * 4);
    *pp = beta ? (*pp + s) : s;
    if (n < NP) {
      f32x4 *pc = (f32x4 *)((NP == 2 && n == 1 ? ddist : dcls) + d);
      *pc = beta ? (*pc + s) : s;
    }
  }
}

}  // namespace m3

using namespace m3;

extern "C" int m3_im2row(const float *img, int B, int Cin, int H, int W, int P, void *rows, int dtype, void *stream) {
  M3_REQUIRE(img && rows, "m3_im2row: null operand");
  M3_REQUIRE(dtype_ok(dtype), "m3_im2row: bad dtype");
  M3_REQUIRE(P % 4 == 0 && H % P == 0 && W % P == 0 && W % 4 == 0, "m3_im2row: P, W must be multiples of 4; H, W multiples of P");
  hipStream_t s = (hipStream_t)stream;
  by_dtype(dtype, [&](auto tt) {
    typedef typename decltype(tt)::type T;
    hipLaunchKernelGGL(im2row_kernel<T>, dim3(2048), dim3(256), 0, s, img, B, Cin, H, W, P, (T *)rows);
  });
  return check_launch("m3_im2row");
}

extern "C" int m3_assemble_tokens(const float *patch, const float *cls, const float *pos, int B, int np_, int D,
                                  float *tokens, void *stream) {
  M3_REQUIRE(patch && cls && pos && tokens && D % 4 == 0, "m3_assemble_tokens: bad args");
  hipLaunchKernelGGL(assemble_tokens_kernel<1>, dim3(2048), dim3(256), 0, (hipStream_t)stream, patch, cls,
                     (const float *)nullptr, pos, B, np_, D, tokens);
  return check_launch("m3_assemble_tokens");
}

extern "C" int m3_assemble_tokens2(const float *patch, const float *cls, const float *dist, const float *pos, int B, int np_,
                                   int D, float *tokens, void *stream) {
  M3_REQUIRE(patch && cls && dist && pos && tokens && D % 4 == 0, "m3_assemble_tokens2: bad args");
  hipLaunchKernelGGL(assemble_tokens_kernel<2>, dim3(2048), dim3(256), 0, (hipStream_t)stream, patch, cls, dist, pos, B, np_, D,
                     tokens);
  return check_launch("m3_assemble_tokens2");
}

extern "C" int m3_tokens_bwd(const float *dtok, int B, int np_, int D, void *dpatch, int dtype, float *dpos,
                             float *dcls, int beta, void *stream) {
  M3_REQUIRE(dtok && dpos && dcls && D % 4 == 0, "m3_tokens_bwd: bad args");
  M3_REQUIRE(dtype_ok(dtype), "m3_tokens_bwd: bad dtype");
  const int64_t total4 = (int64_t)(np_ + 1) * D / 4;
  const dim3 grid((unsigned)((total4 + TB_EL - 1) / TB_EL)), block(TB_BL * TB_EL);
  hipStream_t s = (hipStream_t)stream;
  by_dtype(dtype, [&](auto tt) {
    typedef typename decltype(tt)::type T;
    hipLaunchKernelGGL((tokens_bwd_kernel<T, 1>), grid, block, 0, s, dtok, B, np_, D, (T *)dpatch, dpos, dcls, (float *)nullptr,
                       beta);
  });
  return check_launch("m3_tokens_bwd");
}

extern "C" int m3_tokens_bwd2(const float *dtok, int B, int np_, int D, void *dpatch, int dtype, float *dpos, float *dcls,
                              float *ddist, int beta, void *stream) {
  M3_REQUIRE(dtok && dpos && dcls && ddist && D % 4 == 0, "m3_tokens_bwd2: bad args");
  M3_REQUIRE(dtype_ok(dtype), "m3_tokens_bwd2: bad dtype");
  const int64_t total4 = (int64_t)(np_ + 2) * D / 4;
  const dim3 grid((unsigned)((total4 + TB_EL - 1) / TB_EL)), block(TB_BL * TB_EL);
  hipStream_t s = (hipStream_t)stream;
  by_dtype(dtype, [&](auto tt) {
    typedef typename decltype(tt)::type T;
    hipLaunchKernelGGL((tokens_bwd_kernel<T, 2>), grid, block, 0, s, dtok, B, np_, D, (T *)dpatch, dpos, dcls, ddist, beta);
  });
  return check_launch("m3_tokens_bwd2");
}
