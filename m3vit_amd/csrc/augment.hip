// The transform chain in front of a multi-task training step for gfx950 (utils/common_config.py:583-632 over
// data/custom_transforms.py): RandomHorizontalFlip, ScaleNRotate, FixedResize, AddIgnoreRegions, ToTensor and Normalize of every
// map of a raw batch in one launch.  Flip, warp and resize arrive composed in one 2 x 3 double matrix per sample (output pixel ->
// source coordinates); a thread resamples four neighbouring output pixels of one row (eight of a 16-bit image), all channels,
// applies the map kind's post-operation and stores NCHW rows with 16-byte stores.  The source taps (1, 4 or 16 per pixel) are
// read through L1 / L2: under a rotation the footprint of an output tile is no rectangle of source rows, and neighbouring
// pixels share their taps.  Every tap index is clamped or tested before the read, every store is tested against Wo and Ho.
// No atomics, no reductions: an output element depends on its own pixel only, so the bits repeat from run to run.
#include "loss_dev.h"

namespace m3 {

constexpr int AUG_TX = 32, AUG_TY = 8;             // threads of a workgroup; a wave covers 2 output rows (measured: DESIGN section 4)
constexpr int AUG_THREADS = AUG_TX * AUG_TY;
constexpr float AUG_EPS32 = 1.1920928955078125e-07f;   // np.finfo(np.float32).eps

struct AugTable { m3_augment_desc d[M3_AUG_MAX_MAPS]; };

// u = (a * x + b * y) + c with the two products and the two sums each rounded to double: a float64 restatement on the host
// gets the same bits, so nearest taps and the uint8 truncation agree exactly
__device__ __forceinline__ double aug_coord(double a, double b, double c, double x, double y) {
#pragma clang fp contract(off)
  const double p = a * x;
  const double q = b * y;
  const double s = p + q;
  return s + c;
}

// the taps of one axis: indices i0 .. i0 + n - 1 with weights w[0 .. n)
struct AugAxis { int i0, n; float w[4]; };

// a double that may be anything (NaN, 1e300) -> an int near [lo, hi]: what lies outside is outside the source either way
__device__ __forceinline__ int aug_int(double f, int size) { return (int)fmin(fmax(f, -4.0), (double)size + 4.0); }

__device__ __forceinline__ AugAxis aug_axis(double u, int mode, int size) {
  AugAxis a;
  a.w[0] = 1.f; a.w[1] = a.w[2] = a.w[3] = 0.f;
  if (mode == M3_AUG_NEAREST) {
    a.i0 = aug_int(floor(u + 0.5), size);
    a.n = 1;
    return a;
  }
  const double f = floor(u);
  const float t = (float)(u - f);
  const int x0 = aug_int(f, size);
  if (mode == M3_AUG_LINEAR) {
    a.i0 = x0; a.n = 2;
    if (t != 0.f) { a.w[0] = 1.f - t; a.w[1] = t; }
    return a;
  }
  a.i0 = x0 - 1; a.n = 4;
  a.w[0] = 0.f; a.w[1] = 1.f;
  if (t != 0.f) {
    // Keys, a = -0.75: W(1 + t) = a t (1 - t)^2, W(t) = 1 - t^2 ((a + 3) - (a + 2) t), and the mirror images in 1 - t
    const float s = 1.f - t;
    a.w[0] = -0.75f * t * (s * s);
    a.w[1] = 1.f - (t * t) * (2.25f - 1.25f * t);
    a.w[2] = 1.f - (s * s) * (2.25f - 1.25f * s);
    a.w[3] = -0.75f * s * (t * t);
  }
  return a;
}

__device__ __forceinline__ float aug_load(const uint8_t *p) { return (float)*p; }
__device__ __forceinline__ float aug_load(const float *p) { return *p; }

// out[c] = sum over the taps of wx wy src[b, y, x, c]; the first contributing tap sets the accumulator (a single tap of
// weight 1 is a bit copy, -0 included), a zero weight or a tap outside a zero border contributes nothing and is not read
template <typename TS, int C>
__device__ __forceinline__ void aug_sample(const TS *__restrict__ img, int H, int W, const AugAxis &ax, const AugAxis &ay,
                                           int border, float (&out)[C]) {
  bool first = true;
#pragma unroll
  for (int c = 0; c < C; ++c) out[c] = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j >= ay.n || ay.w[j] == 0.f) continue;
    int yy = ay.i0 + j;
    if (border == M3_AUG_BORDER_ZERO) { if (yy < 0 || yy >= H) continue; }
    else yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i >= ax.n || ax.w[i] == 0.f) continue;
      int xx = ax.i0 + i;
      if (border == M3_AUG_BORDER_ZERO) { if (xx < 0 || xx >= W) continue; }
      else xx = xx < 0 ? 0 : (xx > W - 1 ? W - 1 : xx);
      const float w = ax.w[i] * ay.w[j];
      const TS *p = img + ((int64_t)yy * W + xx) * C;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float tap = aug_load(p + c);
        out[c] = first ? w * tap : __builtin_fmaf(w, tap, out[c]);
      }
      first = false;
    }
  }
}

// PX values of one output row: one 16-byte store where the address allows it (PX * sizeof(TO) == 16), else element by element
template <typename TO, int PX>
__device__ __forceinline__ void aug_store(TO *row, int x0, int Wo, const float (&v)[PX]) {
  TO *p = row + x0;
  if (x0 + PX <= Wo && ((uintptr_t)p & 15) == 0) {
    Pack<TO, PX>::store(p, v);
  } else {
#pragma unroll
    for (int k = 0; k < PX; ++k)
      if (x0 + k < Wo) p[k] = (TO)v[k];
  }
}

// one map, one sample, one tile of AUG_TX PX x AUG_TY output pixels
template <typename TS, typename TO, int C, int PX>
__device__ __forceinline__ void aug_tile(const m3_augment_desc &d, int b, int tile, int H, int W, int Ho, int Wo, int border,
                                         const double *__restrict__ mats, const float *__restrict__ aux) {
  const int tiles_x = (Wo + AUG_TX * PX - 1) / (AUG_TX * PX);
  const int tiles_y = (Ho + AUG_TY - 1) / AUG_TY;
  if (tile >= tiles_x * tiles_y) return;                   // the grid is sized for the narrowest tile of the call
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int x0 = (tx * AUG_TX + (threadIdx.x & (AUG_TX - 1))) * PX;
  const int y = ty * AUG_TY + (threadIdx.x / AUG_TX);
  if (y >= Ho || x0 >= Wo) return;
  const double a00 = mats[6 * b], a01 = mats[6 * b + 1], a02 = mats[6 * b + 2];
  const double a10 = mats[6 * b + 3], a11 = mats[6 * b + 4], a12 = mats[6 * b + 5];
  const float sc = aux[4 * b], cs = aux[4 * b + 1], sn = aux[4 * b + 2];
  const bool flip = aux[4 * b + 3] != 0.f;
  const TS *img = (const TS *)d.src + (int64_t)b * H * W * C;
  float res[C][PX];
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    const int x = x0 + k < Wo ? x0 + k : Wo - 1;             // a lane past the row repeats its last pixel; never stored
    const double u = aug_coord(a00, a01, a02, (double)x, (double)y);
    const double v = aug_coord(a10, a11, a12, (double)x, (double)y);
    const AugAxis ax = aug_axis(u, d.mode, W), ay = aug_axis(v, d.mode, H);
    float val[C];
    aug_sample<TS, C>(img, H, W, ax, ay, border, val);
    if (d.kind == M3_AUG_IMAGE) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        float q = val[c];
        if (d.quantize) q = truncf(fminf(fmaxf(q, 0.f), 255.f));      // a NaN becomes 0
        val[c] = (q / 255.f - d.mean[c]) / d.std[c];
      }
    } else if (d.kind == M3_AUG_DEPTH) {
      const float z = val[0] / sc;
      val[0] = z == 0.f ? 255.f : z;
    }
    if constexpr (C == 3) {
      if (d.kind == M3_AUG_NORMALS) {
        const float n0 = flip ? -val[0] : val[0], n1 = val[1], n2 = val[2];
        const float r0 = __builtin_fmaf(n1, sn, n0 * cs), r1 = __builtin_fmaf(-n0, sn, n1 * cs);
        const float nn = sqrtf(__builtin_fmaf(n2, n2, __builtin_fmaf(r1, r1, r0 * r0)));
        const float den = nn + AUG_EPS32;
        const bool dead = nn == 0.f;
        val[0] = dead ? 255.f : r0 / den;
        val[1] = dead ? 255.f : r1 / den;
        val[2] = dead ? 255.f : n2 / den;
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) res[c][k] = val[c];
  }
  TO *dst = (TO *)d.dst + (int64_t)b * C * Ho * Wo;
#pragma unroll
  for (int c = 0; c < C; ++c) aug_store<TO, PX>(dst + ((int64_t)c * Ho + y) * Wo, x0, Wo, res[c]);
}

// grid (tile, sample, map)
__global__ __launch_bounds__(AUG_THREADS) void augment_kernel(const AugTable tab, int H, int W, int Ho, int Wo, int border,
                                                              const double *__restrict__ mats, const float *__restrict__ aux) {
  const m3_augment_desc &d = tab.d[blockIdx.z];
  const int b = blockIdx.y, tile = blockIdx.x;
  const bool u8 = d.src_dtype == M3_AUG_U8;
  if (d.C == 1) {                                            // label, depth: fp32 out
    if (u8) aug_tile<uint8_t, float, 1, 4>(d, b, tile, H, W, Ho, Wo, border, mats, aux);
    else aug_tile<float, float, 1, 4>(d, b, tile, H, W, Ho, Wo, border, mats, aux);
  } else if (d.dst_dtype == M3_F32) {                        // image, normals
    if (u8) aug_tile<uint8_t, float, 3, 4>(d, b, tile, H, W, Ho, Wo, border, mats, aux);
    else aug_tile<float, float, 3, 4>(d, b, tile, H, W, Ho, Wo, border, mats, aux);
  } else if (d.dst_dtype == M3_F16) {                        // image, 16 bit: 8 pixels make 16 bytes
    if (u8) aug_tile<uint8_t, half_t, 3, 8>(d, b, tile, H, W, Ho, Wo, border, mats, aux);
    else aug_tile<float, half_t, 3, 8>(d, b, tile, H, W, Ho, Wo, border, mats, aux);
  } else {
    if (u8) aug_tile<uint8_t, bf16_t, 3, 8>(d, b, tile, H, W, Ho, Wo, border, mats, aux);
    else aug_tile<float, bf16_t, 3, 8>(d, b, tile, H, W, Ho, Wo, border, mats, aux);
  }
}

}  // namespace m3

using namespace m3;

extern "C" int m3_augment_batch(const m3_augment_desc *descs, int n_maps, int B, int H, int W, int Ho, int Wo, int border,
                                const double *mats, const float *aux, void *stream) {
  M3_REQUIRE(descs && n_maps >= 1 && n_maps <= M3_AUG_MAX_MAPS, "m3_augment_batch: %d maps: 1 to %d per call", n_maps,
             M3_AUG_MAX_MAPS);
  M3_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1,
             "m3_augment_batch: B = %d (1 .. 65535), H, W = %d, %d, Ho, Wo = %d, %d must be positive", B, H, W, Ho, Wo);
  M3_REQUIRE(border == M3_AUG_BORDER_ZERO || border == M3_AUG_BORDER_REPLICATE, "m3_augment_batch: bad border code %d", border);
  M3_REQUIRE(mats && aux, "m3_augment_batch: null parameter pointer");
  const int64_t lim = ((int64_t)1 << 31) - ((int64_t)1 << 20);
  AugTable tab;
  memset(&tab, 0, sizeof(tab));
  for (int i = 0; i < n_maps; ++i) {
    const m3_augment_desc &d = descs[i];
    M3_REQUIRE(d.src && d.dst, "m3_augment_batch: map %d: null pointer", i);
    M3_REQUIRE(d.kind == M3_AUG_IMAGE || d.kind == M3_AUG_LABEL || d.kind == M3_AUG_DEPTH || d.kind == M3_AUG_NORMALS,
               "m3_augment_batch: map %d: bad kind code %d", i, d.kind);
    M3_REQUIRE(d.mode == M3_AUG_NEAREST || d.mode == M3_AUG_LINEAR || d.mode == M3_AUG_CUBIC,
               "m3_augment_batch: map %d: bad mode code %d", i, d.mode);
    const int want_c = (d.kind == M3_AUG_IMAGE || d.kind == M3_AUG_NORMALS) ? 3 : 1;
    M3_REQUIRE(d.C == want_c, "m3_augment_batch: map %d: C = %d, its kind takes %d", i, d.C, want_c);
    M3_REQUIRE(d.src_dtype == M3_F32 || d.src_dtype == M3_AUG_U8, "m3_augment_batch: map %d: source must be fp32 or uint8", i);
    M3_REQUIRE(d.src_dtype == M3_F32 || d.kind == M3_AUG_IMAGE || d.mode == M3_AUG_NEAREST,
               "m3_augment_batch: map %d: a uint8 map that is no image is a class map: nearest only", i);
    M3_REQUIRE(d.kind == M3_AUG_IMAGE ? dtype_ok(d.dst_dtype) : d.dst_dtype == M3_F32,
               "m3_augment_batch: map %d: bad output dtype code %d for its kind", i, d.dst_dtype);
    if (d.kind == M3_AUG_IMAGE)
      M3_REQUIRE(d.std[0] > 0.f && d.std[1] > 0.f && d.std[2] > 0.f, "m3_augment_batch: map %d: std must be positive", i);
    M3_REQUIRE((int64_t)B * H * W * d.C < lim && (int64_t)B * d.C * Ho * Wo < lim,
               "m3_augment_batch: map %d: 2^31 - 2^20 elements or more", i);
    tab.d[i] = d;
  }
  const int tiles = ((Wo + AUG_TX * 4 - 1) / (AUG_TX * 4)) * ((Ho + AUG_TY - 1) / AUG_TY);
  hipLaunchKernelGGL(augment_kernel, dim3(tiles, B, n_maps), dim3(AUG_THREADS), 0, (hipStream_t)stream, tab, H, W, Ho, Wo,
                     border, mats, aux);
  return check_launch("m3_augment_batch");
}
