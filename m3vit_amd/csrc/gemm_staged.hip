// The register-staged NT GEMM kernel (gemm_nt_kernel): fp32 and every shape the LDS-DMA kernels refuse (a K tail, N or a
// leading dimension that is no multiple of 8).  The contract and the kernel choice: gemm.hip.
//
// Structure (one 128x128 output tile per 256-thread workgroup, 2x2 waves of 64x64):
//   - both operands are K-contiguous, staged global -> VGPR -> LDS in 128-byte row
//     slices (BK = 32 f32 / 64 f16), double-buffered, one barrier per K step;
//   - LDS image is XOR-swizzled at 16-byte granularity (chunk ^= (row>>1)&7) so that the
//     ds_read_b128 fragment reads of 16 different rows are bank-conflict free;
//   - MFMA 16x16x32 f16 / 16x16x4 f32 (exact), fp32 accumulate; the weight tile is the
//     MFMA "A" operand so that every lane ends up with 4 consecutive n of one row m
//     and the epilogue uses 8/16-byte vector accesses;
//   - grouped mode: workgroup -> (expert, m-tile) through the device-resident
//     tile_starts prefix (no host sync), rows past the expert's end are zero-filled and
//     never stored;
//   - tile ids are remapped so that the n-tiles of one m-tile run on the same XCD (A rows
//     come from HBM once, then from that XCD's L2).
#include "gemm_dev.h"

namespace m3 {

// MI: 16-row MFMA tiles per wave along m - 4 (a 128 x 128 tile) or 5 (160 x 128: dense fp32 launches whose 128-row tiles
// leave the chip a ragged last round, e.g. M = 25 216, N = 384: 591 tiles on 256 CUs = 3 per CU for 79 of them, 474 tiles
// of 160 rows = 2 per CU at most; fp32 is MFMA-bound, so the busiest CU's rows set the time: 384 -> 320)
template <typename T, bool KTAIL, int MI = 4>
__global__ __launch_bounds__(GEMM_THREADS, 2) void gemm_nt_kernel(const GemmDev p) {
  constexpr int BMT = 32 * MI;                     // rows of the tile
  typedef Mma<T> MM;
  typedef typename MM::frag frag;
  constexpr int BK = ROWB / (int)sizeof(T);
  constexpr int CHUNKS = ROWB / 64;   // 64-byte fragments groups per row slice = 2

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // [buf][A: BMT rows | B: 128 rows] * 128 B

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int wr = wave >> 1, wc = wave & 1;

  // ---- which tile
  // grouped: the grid is sized for the upper bound of row tiles; remap only the LIVE workgroups over the XCDs (a remap
  // over the whole grid would park the surplus ids, i.e. no work, on the last XCD)
  int ts_lane = 0;
  const int nwg = p.tile_starts ? grouped_live_tiles(p.tile_starts, p.G, lane, ts_lane) * p.n_tiles : (int)gridDim.x;
  if ((int)blockIdx.x >= nwg) return;
  const int t = xcd_remap(blockIdx.x, nwg);
  int mt, nt;
  tile_of(t, p.n_tiles, p.m_band, nwg / p.n_tiles, mt, nt);
  int g = 0;
  int64_t m_begin, m_end;
  if (p.tile_starts) {
    const TileOwner ow = grouped_tile_owner(p.tile_starts, p.group_offsets, p.G, mt, lane, ts_lane);
    g = ow.g; m_begin = ow.m_begin; m_end = ow.m_end;
  } else {
    m_begin = (int64_t)mt * BMT;
    m_end = p.M;
    if (m_begin >= m_end) return;
  }
  const int n0 = nt * BN;

  // ---- per-thread staging assignment: 4 x 16-byte chunks per operand per step
  // chunk q = tid + 256*i -> row = q >> 3 (0..127), c = q & 7.
  // Rows past the end of the group / of N are CLAMPED to a valid row instead of predicated: an
  // output element depends only on its own A row and B row, and those rows/columns are never
  // stored, so the loads can be unconditional (no branches -> hipcc keeps counted vmcnt waits).
  // Addresses are (wave-uniform 64-bit base that advances with k) + (32-bit per-lane byte offset):
  // the loads take the SGPR-base form and cost no per-step VALU address arithmetic.
  uint32_t a_off[MI], b_off[4];
  const int c_stage = tid & 7;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int row = (tid >> 3) + 32 * i;
    int64_t m = m_begin + row;
    if (m >= m_end) m = m_end - 1;
    int64_t src = m;
    if (p.a_row_idx) src = (int64_t)div_by(p.a_row_idx[m], p.a_row_div, p.a_row_sh);
    a_off[i] = (uint32_t)(src * p.lda_b) + c_stage * 16;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int n = n0 + (tid >> 3) + 32 * i;
    if (n >= p.N) n = p.N - 1;
    b_off[i] = (uint32_t)((int64_t)n * p.ldb_b) + c_stage * 16;
  }
  const char *a_base = p.A;
  const char *b_base = p.B + (int64_t)g * p.b_group_b;
  const int kbytes = p.K * (int)sizeof(T);
  const int nk = (kbytes + ROWB - 1) / ROWB;

  // LDS addressing: the XOR swizzle term (row>>1)&7 only depends on the lane (tile rows advance in
  // multiples of 16 / 32), so one base per (operand, k-chunk) plus compile-time offsets is enough.
  const int st_base = (tid >> 3) * ROWB + ((c_stage ^ ((tid >> 4) & 7)) << 4);      // + i*4096
  const int sw = (li >> 1) & 7;
  const int rdA0 = (wr * 16 * MI + li) * ROWB + ((lg ^ sw) << 4);                   // + i*2048
  const int rdA1 = (wr * 16 * MI + li) * ROWB + (((4 + lg) ^ sw) << 4);
  const int rdB0 = (wc * 64 + li) * ROWB + ((lg ^ sw) << 4) + BMT * ROWB;
  const int rdB1 = (wc * 64 + li) * ROWB + (((4 + lg) ^ sw) << 4) + BMT * ROWB;

  // Two register sets: tile t+1 waits in one set while tile t+2 is being fetched into the other,
  // so every global load has two compute phases to land (prefetch distance 2).
  u32x4 ra0[MI], rb0[4], ra1[MI], rb1[4];
  auto load_global = [&](int ks, u32x4(&ra)[MI], u32x4(&rb)[4]) {
    int kb = ks * ROWB;
    if (KTAIL && kb + c_stage * 16 >= kbytes) kb = -c_stage * 16;   // K tail: a valid chunk, zeroed at store
    const char *pa = a_base + kb, *pb = b_base + kb;
#pragma unroll
    for (int i = 0; i < MI; ++i) ra[i] = *(const u32x4 *)(pa + a_off[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) rb[i] = *(const u32x4 *)(pb + b_off[i]);
  };
  constexpr int BUFB = (BMT + BN) * ROWB;           // one buffer: both operand images
  auto store_lds = [&](int buf, const u32x4(&ra)[MI], const u32x4(&rb)[4], int ks) {
    const bool kin = !KTAIL || (ks * ROWB + c_stage * 16) < kbytes;
    char *base = smem + buf * BUFB + st_base;
#pragma unroll
    for (int i = 0; i < MI; ++i) *(u32x4 *)(base + i * 32 * ROWB) = kin ? ra[i] : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) *(u32x4 *)(base + i * 32 * ROWB + BMT * ROWB) = kin ? rb[i] : u32x4{0u, 0u, 0u, 0u};
  };

  f32x4 acc[4][MI];   // [ni][mi]: rows of the MFMA tile = n, cols = m
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < MI; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int buf) {
    const char *sb = smem + buf * BUFB;
#pragma unroll
    for (int kc = 0; kc < CHUNKS; ++kc) {
      frag fa[MI], fb[4];
      const char *pa = sb + (kc ? rdA1 : rdA0), *pb = sb + (kc ? rdB1 : rdB0);
#pragma unroll
      for (int i = 0; i < MI; ++i) fa[i] = *(const frag *)(pa + i * 16 * ROWB);
#pragma unroll
      for (int i = 0; i < 4; ++i) fb[i] = *(const frag *)(pb + i * 16 * ROWB);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = MM::mma(fb[ni], fa[mi], acc[ni][mi]);
    }
  };

  load_global(0, ra1, rb1);
  load_global(nk > 1 ? 1 : 0, ra0, rb0);
  store_lds(0, ra1, rb1, 0);
  __syncthreads();

  // Steady state (entry of an even step ks): LDS buf0 holds tile ks, set 0 holds tile ks+1 (in
  // flight).  The loop body only runs while both of its loads are in range, so every load/store is
  // unconditional and hipcc's counted vmcnt waits stay exact; the last 1-3 tiles are peeled.
  int ks = 0;
  for (; ks + 3 < nk; ks += 2) {
    load_global(ks + 2, ra1, rb1);
    __builtin_amdgcn_sched_barrier(0);          // keep the prefetch ahead of the MFMA phase
    compute(0);
    store_lds(1, ra0, rb0, ks + 1);
    __syncthreads();
    load_global(ks + 3, ra0, rb0);
    __builtin_amdgcn_sched_barrier(0);
    compute(1);
    store_lds(0, ra1, rb1, ks + 2);
    __syncthreads();
  }
  const int rem = nk - ks;
  if (rem == 3) {
    load_global(ks + 2, ra1, rb1);
    __builtin_amdgcn_sched_barrier(0);          // keep the prefetch ahead of the MFMA phase
    compute(0);
    store_lds(1, ra0, rb0, ks + 1);
    __syncthreads();
    compute(1);
    store_lds(0, ra1, rb1, ks + 2);
    __syncthreads();
    compute(0);
  } else if (rem == 2) {
    compute(0);
    store_lds(1, ra0, rb0, ks + 1);
    __syncthreads();
    compute(1);
  } else {
    compute(0);
  }

  // ---- epilogue.  Fast path: the 128x128 fp32 tile is transposed through the (now free) 64 KiB
  // of LDS so that every lane owns 8 consecutive n of one row: bias/residual/pre/C accesses become
  // 16/32-byte vectors and each wave store covers whole 256/512-byte row segments (matters most for
  // the scattered token-major store of the expert FC2 and for the two-output FC1).
  const float *bias = p.bias ? p.bias + (int64_t)g * p.N : nullptr;
  if (p.vec8) {
    // MI = 4: the whole tile at once (64 KiB).  MI = 5: 80 KiB would not fit the operand buffers' 72 KiB - the two 80-row
    // halves (wave rows wr = 0, 1) go through one after the other
    constexpr int NH = MI == 4 ? 1 : 2, HR = BMT / NH;      // passes, rows per pass
    const int cg = tid & 15, r16 = tid >> 4;
    const int n = n0 + cg * 8;
    f32x4 b0 = f32x4{0.f, 0.f, 0.f, 0.f}, b1 = b0;
    if (bias && n < p.N) { b0 = *(const f32x4 *)(bias + n); b1 = *(const f32x4 *)(bias + n + 4); }
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      __syncthreads();                       // all waves are done with the operand buffers / the previous half
      if (NH == 1 || wr == h) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) {
            const int row = (NH == 1 ? wr * 64 : 0) + mi * 16 + li;
            const int chunk = wc * 16 + ni * 4 + lg;
            *(f32x4 *)(smem + row * 512 + ((chunk ^ (row & 31)) << 4)) = acc[ni][mi];
          }
      }
      __syncthreads();
      if (n < p.N) {
#pragma unroll 2
        for (int ps = 0; ps < HR / 16; ++ps) {
          const int row = ps * 16 + r16;
          const int64_t m = m_begin + h * HR + row;
          if (m >= m_end) break;
          const int sw = row & 31;
          const f32x4 v0 = *(const f32x4 *)(smem + row * 512 + (((2 * cg) ^ sw) << 4));
          const f32x4 v1 = *(const f32x4 *)(smem + row * 512 + (((2 * cg + 1) ^ sw) << 4));
          epilogue_row_any<T>(p, m, n, v0 + b0, v1 + b1, [&](int64_t crow) {
            const int64_t srow = p.row_scale_idx ? (int64_t)p.row_scale_idx[m] : crow;
            return p.row_scale[srow / p.row_scale_div];
          });
        }
      }
    }
    return;
  }
  // Generic path (N or a leading dimension not a multiple of 8): lane holds for tile (ni, mi)
  // n = nb + 4*lg + r (r = 0..3), m = mb + li.
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int64_t m = m_begin + wr * 16 * MI + mi * 16 + li;
    if (m >= m_end) continue;
    const int64_t crow = p.c_row_idx ? (int64_t)p.c_row_idx[m] : m;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int n = n0 + wc * 64 + ni * 16 + 4 * lg;
      if (n >= p.N) continue;
      f32x4 v = acc[ni][mi];
      if (bias) {
        const f32x4 bv = *(const f32x4 *)(bias + n);
        v += bv;
      }
      if (p.pre_out) Vec4<T>::store((T *)p.pre_out + crow * p.ld_pre + n, v);
      if (p.act == M3_ACT_GELU) {
        v[0] = gelu_f(v[0]); v[1] = gelu_f(v[1]); v[2] = gelu_f(v[2]); v[3] = gelu_f(v[3]);
      }
      if (p.gpre) {
        const f32x4 pr = Vec4<T>::load((const T *)p.gpre + crow * p.ld_gpre + n);
        v[0] *= gelu_grad_f(pr[0]); v[1] *= gelu_grad_f(pr[1]);
        v[2] *= gelu_grad_f(pr[2]); v[3] *= gelu_grad_f(pr[3]);
      }
      if (p.row_scale) v *= p.row_scale[(p.row_scale_idx ? (int64_t)p.row_scale_idx[m] : crow) / p.row_scale_div];
      if (p.residual) v += *(const f32x4 *)(p.residual + crow * p.ld_res + n);
      if (p.c_f32) *(f32x4 *)((float *)p.C + crow * p.ldc + n) = v;
      else Vec4<T>::store((T *)p.C + crow * p.ldc + n, v);
    }
  }
}

// 128-row tiles: 64 KiB of LDS; tall (fp32, no K tail, dense): 160-row tiles, 72 KiB - two workgroups per CU either way
int launch_gemm_staged(const GemmDev &d, int dtype, bool tall, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)d.m_tiles_max * d.n_tiles)), block(GEMM_THREADS);
  if (tall) {
    const size_t lds5 = 2 * (160 + BN) * ROWB;
    static const hipError_t attr5 = hipFuncSetAttribute((const void *)gemm_nt_kernel<float, false, 5>,
                                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds5);
    (void)attr5;
    hipLaunchKernelGGL((gemm_nt_kernel<float, false, 5>), grid, block, lds5, s, d);
    return check_launch("m3_gemm_nt");
  }
  const size_t lds = 4 * BM * ROWB;
  const bool ktail = (d.K * dtype_size(dtype)) % ROWB != 0;
  auto go = [&](auto t) {
    if (ktail) hipLaunchKernelGGL((gemm_nt_kernel<decltype(t), true>), grid, block, lds, s, d);
    else hipLaunchKernelGGL((gemm_nt_kernel<decltype(t), false>), grid, block, lds, s, d);
  };
  if (dtype == M3_F16) go(half_t());
  else if (dtype == M3_BF16) go(bf16_t());
  else go(float());
  return check_launch("m3_gemm_nt");
}

}  // namespace m3
