// The cast and add helpers of gfx950: fp32 masters -> activation-dtype copies (plain, transposed, many matrices in one
// launch), fp32 spans -> the activation dtype with or without a per-row scale, and the fp32 accumulate.  All HBM-bound:
// 16-byte loads, 8- or 16-byte stores, transposes through a padded 32 x 32 LDS tile.
#include "common.h"

namespace m3 {

template <typename T>
__global__ void cast_matrix_kernel(const float *__restrict__ src, int rows, int cols, int transpose, T *__restrict__ dst) {
  // grid.z = group; tile 32x32 through LDS when transposing
  __shared__ float tile[32][33];
  const int64_t goff = (int64_t)blockIdx.z * rows * cols;
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  if (!transpose) {
    for (int i = ty; i < 32; i += 8) {
      const int r = r0 + i, c = c0 + tx;
      if (r < rows && c < cols) dst[goff + (int64_t)r * cols + c] = (T)src[goff + (int64_t)r * cols + c];
    }
    return;
  }
  for (int i = ty; i < 32; i += 8) {
    const int r = r0 + i, c = c0 + tx;
    tile[i][tx] = (r < rows && c < cols) ? src[goff + (int64_t)r * cols + c] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, r = r0 + tx;   // dst[c][r]
    if (r < rows && c < cols) dst[goff + (int64_t)c * rows + r] = (T)tile[tx][i];
  }
}

// many matrices in one launch: block -> descriptor by binary search over the tile prefix; a job may ask for the
// plain copy, the transposed copy, or both from ONE read of the fp32 tile
struct CastDesc {            // = m3_cast_desc
  const float *src; void *dst; void *dst_t;
  int32_t G, rows, cols;
  int32_t tile_start;
};

template <typename T>
__global__ __launch_bounds__(256) void cast_batch_kernel(const CastDesc *__restrict__ descs, int n_desc) {
  __shared__ float tile[32][33];
  int lo = 0, hi = n_desc - 1;
  const int b = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].tile_start <= b) lo = mid; else hi = mid - 1;
  }
  const CastDesc d = descs[lo];
  const int tcols = (d.cols + 31) / 32, trows = (d.rows + 31) / 32;
  int rest = b - d.tile_start;
  const int g = rest / (tcols * trows);
  rest -= g * tcols * trows;
  const int r0 = (rest / tcols) * 32, c0 = (rest % tcols) * 32;
  const int64_t goff = (int64_t)g * d.rows * d.cols;
  const float *src = d.src + goff;
  if (((d.rows | d.cols) & 3) == 0) {
    // rows and columns multiples of 4 (every weight of the model): one 16-byte load per thread (8 threads x 32 rows), 8-byte
    // stores for the plain copy and - through the LDS tile - for the transposed one
    const int tr = threadIdx.x >> 3, tg = threadIdx.x & 7;
    const int r = r0 + tr, c = c0 + 4 * tg;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (r < d.rows && c < d.cols) v = *(const f32x4 *)(src + (int64_t)r * d.cols + c);
    if (d.dst && r < d.rows && c < d.cols)
      Vec4<T>::store((T *)d.dst + goff + (int64_t)r * d.cols + c, v);
    tile[tr][4 * tg + 0] = v[0]; tile[tr][4 * tg + 1] = v[1]; tile[tr][4 * tg + 2] = v[2]; tile[tr][4 * tg + 3] = v[3];
    if (!d.dst_t) return;
    __syncthreads();
    const int cc = c0 + tr, rg = r0 + 4 * tg;                        // dst_t[cc][rg .. rg + 3] = src[rg .. rg + 3][cc]
    if (cc < d.cols && rg < d.rows) {
      const f32x4 w = f32x4{tile[4 * tg + 0][tr], tile[4 * tg + 1][tr], tile[4 * tg + 2][tr], tile[4 * tg + 3][tr]};
      Vec4<T>::store((T *)d.dst_t + goff + (int64_t)cc * d.rows + rg, w);
    }
    return;
  }
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  for (int i = ty; i < 32; i += 8) {
    const int r = r0 + i, c = c0 + tx;
    const float v = (r < d.rows && c < d.cols) ? src[(int64_t)r * d.cols + c] : 0.f;
    if (d.dst && r < d.rows && c < d.cols) ((T *)d.dst + goff)[(int64_t)r * d.cols + c] = (T)v;
    tile[i][tx] = v;
  }
  if (!d.dst_t) return;
  __syncthreads();
  T *dst_t = (T *)d.dst_t + goff;
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, r = r0 + tx;   // dst_t[c][r]
    if (r < d.rows && c < d.cols) dst_t[(int64_t)c * d.rows + r] = (T)tile[tx][i];
  }
}

__global__ void add_f32_kernel(float *__restrict__ dst, const float *__restrict__ src, int64_t n4, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n4) {
    ((f32x4 *)dst)[i] += ((const f32x4 *)src)[i];
  } else if (i == n4) {
    for (int64_t j = n4 * 4; j < n; ++j) dst[j] += src[j];
  }
}

template <typename T>
__global__ void cast_f32_kernel(const float *__restrict__ src, int64_t n4, T *__restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  Vec4<T>::store(dst + i * 4, *(const f32x4 *)(src + i * 4));
}

template <typename T>
__global__ void scale_rows_cast_kernel(const float *__restrict__ src, int64_t n4, int cols4, const float *__restrict__ scale,
                                       int div, T *__restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const float sc = scale[(i / cols4) / div];
  Vec4<T>::store(dst + i * 4, *(const f32x4 *)(src + i * 4) * sc);
}

}  // namespace m3

using namespace m3;

extern "C" int m3_cast_matrix(const float *src, int G, int rows, int cols, int transpose, void *dst, int dst_dtype,
                              void *stream) {
  M3_REQUIRE(src && dst && G >= 1 && rows > 0 && cols > 0, "m3_cast_matrix: bad args");
  M3_REQUIRE(dtype_ok(dst_dtype), "m3_cast_matrix: bad dtype");
  const dim3 grid((cols + 31) / 32, (rows + 31) / 32, G), block(256);
  hipStream_t s = (hipStream_t)stream;
  by_dtype(dst_dtype, [&](auto tt) {
    typedef typename decltype(tt)::type T;
    hipLaunchKernelGGL(cast_matrix_kernel<T>, grid, block, 0, s, src, rows, cols, transpose, (T *)dst);
  });
  return check_launch("m3_cast_matrix");
}

extern "C" int m3_cast_batch(const m3_cast_desc *descs_dev, int n_desc, int total_tiles, int dst_dtype, void *stream) {
  static_assert(sizeof(m3_cast_desc) == sizeof(CastDesc), "descriptor layout");
  M3_REQUIRE(descs_dev && n_desc >= 1 && total_tiles >= 1, "m3_cast_batch: bad args");
  M3_REQUIRE(dtype_ok(dst_dtype), "m3_cast_batch: bad dtype");
  hipStream_t s = (hipStream_t)stream;
  const CastDesc *d = (const CastDesc *)descs_dev;
  by_dtype(dst_dtype, [&](auto tt) {
    typedef typename decltype(tt)::type T;
    hipLaunchKernelGGL(cast_batch_kernel<T>, dim3(total_tiles), dim3(256), 0, s, d, n_desc);
  });
  return check_launch("m3_cast_batch");
}

extern "C" int m3_add_f32(float *dst, const float *src, int64_t n, void *stream) {
  M3_REQUIRE(dst && src && n >= 0, "m3_add_f32: bad args");
  M3_REQUIRE(((uintptr_t)dst % 16) == 0 && ((uintptr_t)src % 16) == 0, "m3_add_f32: 16-byte alignment");
  if (n == 0) return M3_OK;
  const int64_t n4 = n / 4;
  hipLaunchKernelGGL(add_f32_kernel, dim3((unsigned)((n4 + 1 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dst, src,
                     n4, n);
  return check_launch("m3_add_f32");
}

extern "C" int m3_cast_f32(const float *src, int64_t n, void *dst, int dst_dtype, void *stream) {
  M3_REQUIRE(src && dst && n >= 0 && n % 4 == 0, "m3_cast_f32: n must be a multiple of 4");
  M3_REQUIRE(dtype_ok(dst_dtype), "m3_cast_f32: bad dtype");
  if (n == 0) return M3_OK;
  const int64_t n4 = n / 4;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((n4 + 255) / 256)), block(256);
  by_dtype(dst_dtype, [&](auto tt) {
    typedef typename decltype(tt)::type T;
    hipLaunchKernelGGL(cast_f32_kernel<T>, grid, block, 0, s, src, n4, (T *)dst);
  });
  return check_launch("m3_cast_f32");
}

extern "C" int m3_scale_rows_cast(const float *src, int64_t rows, int cols, const float *row_scale, int div, void *dst,
                                  int dst_dtype, void *stream) {
  M3_REQUIRE(src && dst && row_scale && rows >= 0 && cols > 0 && cols % 4 == 0 && div >= 1, "m3_scale_rows_cast: bad args");
  M3_REQUIRE(dtype_ok(dst_dtype), "m3_scale_rows_cast: bad dtype");
  if (rows == 0) return M3_OK;
  const int64_t n4 = rows * cols / 4;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((n4 + 255) / 256)), block(256);
  by_dtype(dst_dtype, [&](auto tt) {
    typedef typename decltype(tt)::type T;
    hipLaunchKernelGGL(scale_rows_cast_kernel<T>, grid, block, 0, s, src, n4, cols / 4, row_scale, div, (T *)dst);
  });
  return check_launch("m3_scale_rows_cast");
}
