// The batched weight-gradient kernel (wgrad_multi_kernel) and its launcher; m3_wgrad_multi in wgrad.hip describes the call.
// Compiled as part of wgrad_tiles.hip, after wgrad_staged.hip: the tile loop is that kernel's (wgrad_tile_loop, plain rows),
// only the way a workgroup finds its work is new.
//
// Up to WG_MULTI dense problems dW_j [N_j, K_j] = dC_j^T A_j over the same M rows (the dense weights of one transformer
// block's backward: their operands are all there once the attention backward has run, and nothing in the block waits for
// them) in ONE launch, every problem cut into the same P row parts.  A launch per weight sizes its parts to fill the chip by
// itself - 9 tiles x 32 parts for the 384 x 384 projection - and pays a 64 KiB fp32 slab per part and tile, written once and
// read once; 108 tiles fill it with P = 4.
// Work order: part-major, inside a part problem after problem, tile after tile.  The XCD remap hands each XCD one contiguous
// run of logical ids, so the workgroups of a part - which all read the same rows, many of them the same operand - share an L2.
#include "wgrad_dev.h"

namespace m3 {

template <typename T>
__global__ __launch_bounds__(WG_THREADS, 2) void wgrad_multi_kernel(const WgradMultiDev mp) {
  constexpr int ROWS = WgLds<T>::ROWS;
  const int tiles = gridDim.x;                   // of all problems together
  int bz, gz;
  if (wgrad_ride_along(mp.d, threadIdx.x, bz, gz)) return;
  const int log_id = xcd_remap(blockIdx.x + tiles * bz, tiles * gz);
  const int t = log_id % tiles, sp = log_id / tiles;
  // the problem of tile t.  Every entry of the table is read, then chosen by value (see wgrad_ride_along)
  WgradDev p = mp.d;
  p.dC = mp.tab0.dC; p.lddc_b = mp.tab0.lddc_b; p.A = mp.tab0.A; p.lda_b = mp.tab0.lda_b;
  p.ws = mp.tab0.ws; p.bias_ws = mp.tab0.bias_ws;
  p.N = mp.tab0.N; p.K = mp.tab0.K; p.tiles_k = mp.tab0.tiles_k;
  int first = 0;
#define M3_FROM(j)                                                                                                      \
  {                                                                                                                     \
    const char *dC_ = mp.tab##j.dC, *A_ = mp.tab##j.A;                                                                  \
    const int64_t lddc_ = mp.tab##j.lddc_b, lda_ = mp.tab##j.lda_b;                                                     \
    float *ws_ = mp.tab##j.ws, *bws_ = mp.tab##j.bias_ws;                                                               \
    const int N_ = mp.tab##j.N, K_ = mp.tab##j.K, tk_ = mp.tab##j.tiles_k, first_ = mp.tab##j.first;                    \
    const bool h_ = t >= first_;                                                                                        \
    p.dC = h_ ? dC_ : p.dC; p.A = h_ ? A_ : p.A; p.lddc_b = h_ ? lddc_ : p.lddc_b; p.lda_b = h_ ? lda_ : p.lda_b;       \
    p.ws = h_ ? ws_ : p.ws; p.bias_ws = h_ ? bws_ : p.bias_ws;                                                          \
    p.N = h_ ? N_ : p.N; p.K = h_ ? K_ : p.K; p.tiles_k = h_ ? tk_ : p.tiles_k; first = h_ ? first_ : first;            \
  }
  static_assert(WG_MULTI == 8, "one M3_FROM per entry");
  M3_FROM(1) M3_FROM(2) M3_FROM(3) M3_FROM(4) M3_FROM(5) M3_FROM(6) M3_FROM(7)
#undef M3_FROM
  const int64_t nsteps_all = (p.M + ROWS - 1) / ROWS;
  const int64_t per = (nsteps_all + p.splits - 1) / p.splits;
  const int64_t s_begin = (int64_t)sp * per;
  const int64_t s_end = s_begin + per < nsteps_all ? s_begin + per : nsteps_all;
  const int nst = (int)(s_end > s_begin ? s_end - s_begin : 0);      // an empty part still writes its (zero) slab
  wgrad_tile_loop<T, false, false, false>(p, t - first, 0, sp, 0, p.M, s_begin, nst);
}

int launch_wgrad_multi(int dtype, dim3 grid, const WgradMultiDev &d, hipStream_t s) {
  const size_t lds = 4 * WgLds<half_t>::ROWS * WgLds<half_t>::STRIDE;
  M3_REQUIRE(dtype == M3_F16 || dtype == M3_BF16, "m3_wgrad_multi: 16-bit operands only");
  const void *kernel = dtype == M3_F16 ? (const void *)wgrad_multi_kernel<half_t> : (const void *)wgrad_multi_kernel<bf16_t>;
  WgradMultiDev a = d;
  void *args[] = {&a};
  (void)hipLaunchKernel(kernel, grid, dim3(WG_THREADS), args, lds, s);
  return check_launch("m3_wgrad_multi");
}

}  // namespace m3
