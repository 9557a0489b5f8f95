// The LDS-DMA NT GEMM kernel (gemm_nt_dma_kernel): the 16-bit launches whose K rows are whole 128-byte slices and whose N
// and leading dimensions are multiples of 8.  The contract and the kernel choice: gemm.hip.
// Same tile / wave layout / epilogue as gemm_nt_kernel (gemm_staged.hip), but the operands go global -> LDS directly
// (global_load_lds_dwordx4: one wave instruction fills 8 rows x 128 B = 1 KiB of the image, lane-linear
// in LDS, with the XOR swizzle applied on the per-lane SOURCE address):
//   - no staging registers and no ds_write pass: <= 128 VGPRs and 32 KiB of LDS per workgroup, so FOUR
//     workgroups share a CU instead of two - their load / MFMA / store phases interleave, which is what
//     the K = 384 shapes of this model need (a tile spends more time in its prologue and in the
//     bandwidth-bound store phase than in MFMAs);
//   - ONE buffer of full 128-byte row slices per operand.  (A first version double-buffered 64-byte slices: a
//     64-byte slice uses half of each 128-byte line it touches and the other half is requested again one step
//     later - with four workgroups per CU the line has usually left the 32 KiB L1 by then, so the L2 -> L1
//     path (64 B/clk/CU) carried every operand byte twice and bounded the K loop.  Full-line slices halve
//     that traffic: -15..-20 % per launch at K = 384, -30 % at K = 1536.)  The double buffer is given up for
//     them: 32 KiB keeps four workgroups per CU, and it is the OTHER workgroups' MFMAs, not this one's,
//     that cover a DMA's latency.  Two barriers per K step; __syncthreads() after the DMA is also the
//     vmcnt(0) that retires it (hipcc drains LDS-DMA at a barrier).
#include "gemm_dev.h"

namespace m3 {

constexpr int DMA_RB = 128;                // bytes of a row slice = one cache line
constexpr int DMA_LDS = 2 * BM * DMA_RB;   // A + B image: 32 KiB
constexpr int DMA_LDS_ALL = DMA_LDS + BM * 4;   // + the tile's 128 per-row epilogue factors (row_scale)

// Diagnostic build only (make CXXFLAGS+=-DM3_GEMM_STAMPS, tools/gemm_stamps.py): lane 0 of wave 0 of the first STAMP_WGS
// workgroups records s_memtime at the phase boundaries - 0 entry, 1 set-up done (in front of the first DMA instruction),
// 2 + 2 ks slice ks landed, 3 + 2 ks slice ks multiplied (ks < 27), 56 / 57 the stores of an epilogue half issued, 58 stores
// acknowledged - with ordinary stores; m3_debug_gemm_stamps copies them out.  No stamp executes in the shipped kernel.
#ifdef M3_GEMM_STAMPS
constexpr int STAMP_WGS = 4096, STAMP_N = 64;
__device__ unsigned long long g_gemm_stamps[STAMP_WGS][STAMP_N];
#define M3_GEMM_STAMP(i)                                                                                              \
  do {                                                                                                                \
    if (threadIdx.x == 0 && blockIdx.x < STAMP_WGS && (i) < STAMP_N) g_gemm_stamps[blockIdx.x][(i)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define M3_GEMM_STAMP(i) do { } while (0)
#endif

// EPI: the epilogue's kind (gemm_dev.h).  HINT: the kind's one access to a tensor that nobody reads soon is non-temporal
// (common.h: cache policy by lifetime) - GELU: the store of pre_out, next read by the backward; GPRE: the load of gpre, its
// last use.  Everything else about the instance is the plain one.  (Operand loads stay plain: the column tiles of a row tile
// re-read A through L2, and with the hint on the LDS-DMA loads of A the step measured 0.6 ms slower.)
template <typename T, int EPI, bool HINT>
__global__ __launch_bounds__(GEMM_THREADS, 4) void gemm_nt_dma_kernel(const GemmDev p) {
  typedef Mma<T> MM;
  typedef typename MM::frag frag;
  constexpr int RB = DMA_RB;
  constexpr int OPB = BM * RB;               // one operand image (16 KiB)
  constexpr int CPR = RB / 16;               // 16-byte chunks per row slice
  constexpr int RPI = 64 / CPR;              // image rows filled by one wave instruction (1 KiB)
  constexpr int NPC = BM / RPI / 4;          // DMA pieces per wave per operand per step (4)
  constexpr int KCH = RB / 64;               // fragment groups per slice
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [A|B][128 rows * 128 B] = 32 KiB

  M3_GEMM_STAMP(0);                                      // entry
  // Every field the prologue and the K loop read is requested here, in front of the first branch: one batch of scalar loads
  // and one wait (left to itself hipcc fetches a field in the block that first uses it - about ten dependent round trips
  // to the argument segment, six of them in front of a dense launch's first DMA).  The empty asm pins the values in SGPRs.
  const char *const A = p.A, *const B = p.B;
  const int64_t lda_b = p.lda_b, ldb_b = p.ldb_b, b_group_b = p.b_group_b, M = p.M;
  const int32_t *const a_row_idx = p.a_row_idx, *const c_row_idx = p.c_row_idx, *const row_scale_idx = p.row_scale_idx;
  const int32_t *const group_offsets = p.group_offsets, *const tile_starts = p.tile_starts;
  const float *const row_scale = p.row_scale;
  const int a_row_div = p.a_row_div, a_row_sh = p.a_row_sh, row_scale_div = p.row_scale_div, row_scale_sh = p.row_scale_sh;
  const int N = p.N, K = p.K, G = p.G, n_tiles = p.n_tiles, m_band = p.m_band, m_tiles_max = p.m_tiles_max;
  asm volatile("" ::"s"(A), "s"(B), "s"(lda_b), "s"(ldb_b), "s"(b_group_b), "s"(M), "s"(a_row_idx), "s"(c_row_idx),
               "s"(row_scale_idx), "s"(group_offsets), "s"(tile_starts), "s"(row_scale), "s"(a_row_div), "s"(a_row_sh),
               "s"(row_scale_div), "s"(row_scale_sh), "s"(N), "s"(K), "s"(G), "s"(n_tiles), "s"(m_band), "s"(m_tiles_max));

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int wr = wave >> 1, wc = wave & 1;

  int ts_lane = 0;
  const int live_m = tile_starts ? grouped_live_tiles(tile_starts, G, lane, ts_lane) : m_tiles_max;    // live row tiles
  const int nwg = live_m * n_tiles;                                                                     // live workgroups (as in gemm_nt_kernel)
  if ((int)blockIdx.x >= nwg) return;
  const int t = xcd_remap(blockIdx.x, nwg);
  int mt, nt;
  tile_of(t, n_tiles, m_band, live_m, mt, nt);
  // (a grouped tile: its group from the prefix already in registers, then the group's row range - wave-uniform, and nobody
  // writes group_offsets while the kernel runs: through the constant address space it is one scalar load instead of the vector
  // load and two broadcasts hipcc makes of it otherwise)
  int g = 0, t0 = 0, go_begin = 0, go_end = 0;
  if (tile_starts) {
    typedef const __attribute__((address_space(4))) int32_t const_i32;
    grouped_tile_group(tile_starts, G, mt, lane, ts_lane, g, t0);
    g = __builtin_amdgcn_readfirstlane(g);
    t0 = __builtin_amdgcn_readfirstlane(t0);
    go_begin = ((const_i32 *)group_offsets)[g];
    go_end = ((const_i32 *)group_offsets)[g + 1];
  } else if ((int64_t)mt * BM >= M) {
    return;                                  // (in front of the first DMA: nothing may be in flight into LDS at an exit)
  }
  const int n0 = nt * BN;
  const int nk = (K * (int)sizeof(T)) / RB;

  // DMA assignment: wave w, piece j fills image rows (NPC*w + j)*RPI .. +RPI-1; lane l -> row + l / CPR,
  // LDS slot l % CPR, which holds source chunk (l % CPR) ^ swz(row).  Rows past the end are clamped (never stored).
  // A piece's source is a wave-uniform base (the operand, the group's weight, the K slice) plus a 32-bit lane offset (the
  // host checks the 4 GiB reach of an operand panel and of one group's weight): eight registers for the eight pieces.
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  uint32_t a_off[NPC], b_off[NPC];
  const char *const Bg = B + (int64_t)g * b_group_b;
  char *const dma_dst = smem + (NPC * wave) * 1024;
  // (the empty asms keep base and lane offset apart and the offset's zero extension next to its use - SGPR pair + 32-bit
  // VGPR in the instruction; hipcc otherwise carries eight 64-bit lane addresses through the K loop)
  auto dma_b = [&](int ks) {
    const char *base = Bg + ks * RB;
    asm("" : "+s"(base));
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
      uint32_t off = b_off[j];
      asm volatile("" : "+v"(off));
      __builtin_amdgcn_global_load_lds((glb_void *)(base + off), (lds_void *)(dma_dst + j * 1024 + OPB), 16, 0, 0);
    }
  };
  auto dma_a = [&](int ks) {
    const char *base = A + ks * RB;
    asm("" : "+s"(base));
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
      uint32_t off = a_off[j];
      asm volatile("" : "+v"(off));
      __builtin_amdgcn_global_load_lds((glb_void *)(base + off), (lds_void *)(dma_dst + j * 1024), 16, 0, 0);
    }
  };

#pragma unroll
  for (int j = 0; j < NPC; ++j) {
    const int row = (NPC * wave + j) * RPI + lane / CPR;
    const int c = (lane % CPR) ^ dma_swz(row);
    int n = n0 + row;
    if (n >= N) n = N - 1;
    b_off[j] = (uint32_t)n * (uint32_t)ldb_b + c * 16;
  }

  // Rows fit 32 bits (the host checks M)
  const int mb32 = tile_starts ? go_begin + (mt - t0) * BM : mt * BM;
  const int me32 = tile_starts ? go_end : (int)M;
  // Every index load of the prologue (the NPC gathered A rows of this lane; the row of the epilogue factor) is issued
  // before the first one is used: one memory latency in front of the A pieces instead of one per index.  The factor itself -
  // the dependent load - is requested behind the last use of an index, so that no wait for an index also waits for it.
  int32_t mrow[NPC], aix[NPC];
#pragma unroll
  for (int j = 0; j < NPC; ++j) {
    int m = mb32 + (NPC * wave + j) * RPI + lane / CPR;
    if (m >= me32) m = me32 - 1;
    mrow[j] = m;
  }
  // per-row epilogue factor (DropPath scale / gate score of the routed row): thread r < 128 requests row r's factor NOW -
  // an index load and a dependent load - so that they arrive under the K loop instead of in front of every store pass
  const bool want_rs = row_scale && tid < BM;
  const int32_t *const rs_idx = row_scale_idx ? row_scale_idx : c_row_idx;
  int rs_m = mb32 + tid;
  if (rs_m >= me32) rs_m = me32 - 1;
  int32_t rs_ix = rs_m;
  if (a_row_idx) {
#pragma unroll
    for (int j = 0; j < NPC; ++j) aix[j] = a_row_idx[mrow[j]];
  }
  if (want_rs && rs_idx) rs_ix = rs_idx[rs_m];
  if (a_row_idx) {                           // (one branch for the four rows: shift, or the 32-bit division)
    if (a_row_sh >= 0) {
#pragma unroll
      for (int j = 0; j < NPC; ++j) mrow[j] = aix[j] >> a_row_sh;
    } else {
#pragma unroll
      for (int j = 0; j < NPC; ++j) mrow[j] = aix[j] / a_row_div;
    }
  }
#pragma unroll
  for (int j = 0; j < NPC; ++j) {
    const int row = (NPC * wave + j) * RPI + lane / CPR;
    const int c = (lane % CPR) ^ dma_swz(row);
    a_off[j] = (uint32_t)mrow[j] * (uint32_t)lda_b + c * 16;
  }
  asm volatile("" : "+v"(a_off[0]), "+v"(a_off[1]), "+v"(a_off[2]), "+v"(a_off[3]));     // (made HERE, not behind the factor's request)
  static_assert(NPC == 4, "the pin above names four pieces");
  float my_rs = 1.0f;
  if (want_rs) my_rs = row_scale[div_by(rs_ix, row_scale_div, row_scale_sh)];
  // (The B pieces of slice 0 need the tile's column and group only and were tried AHEAD of the row range and the index round
  // trip: the first DMA instruction left 1 000-3 500 ticks earlier, the step and the launches did not get faster -
  // profiles/gemm_prologue.txt - so the pieces of a slice leave together.)
  M3_GEMM_STAMP(1);                                      // set-up done: slice 0 goes out
  dma_b(0);
  dma_a(0);

  int rdA[KCH], rdB[KCH];
#pragma unroll
  for (int kc = 0; kc < KCH; ++kc) {
    rdA[kc] = (wr * 64 + li) * RB + (((kc * 4 + lg) ^ dma_swz(li)) << 4);               // + i*16*RB
    rdB[kc] = (wc * 64 + li) * RB + (((kc * 4 + lg) ^ dma_swz(li)) << 4) + OPB;
  }

  f32x4 acc[4][4];   // [ni][mi]
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&]() {
    const char *sb = smem;
#pragma unroll
    for (int kc = 0; kc < KCH; ++kc) {
      frag fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        fa[i] = *(const frag *)(sb + rdA[kc] + i * 16 * RB);
        fb[i] = *(const frag *)(sb + rdB[kc] + i * 16 * RB);
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) acc[ni][mi] = MM::mma(fb[ni], fa[mi], acc[ni][mi]);
    }
  };

  for (int ks = 0;;) {        // (slice 0 is on its way)
    __syncthreads();          // vmcnt(0) + barrier: the slice has landed
    if (ks < 27) M3_GEMM_STAMP(2 + 2 * ks);
    compute();
    __syncthreads();          // everyone has read it
    if (ks < 27) M3_GEMM_STAMP(3 + 2 * ks);
    if (++ks >= nk) break;
    dma_a(ks);
    dma_b(ks);
  }

  // ---- epilogue: the fp32 tile goes through the (now free) 32 KiB in two 64-row halves (half h = waves wr == h),
  // every lane then owns 8 consecutive n of one row
  const float *bias = p.bias ? p.bias + (int64_t)g * p.N : nullptr;
  const int cg = tid & 15, r16 = tid >> 4;
  const int n = n0 + cg * 8;
  f32x4 b0 = f32x4{0.f, 0.f, 0.f, 0.f}, b1 = b0;
  if (bias && n < p.N) { b0 = *(const f32x4 *)(bias + n); b1 = *(const f32x4 *)(bias + n + 4); }
  float *const s_rs = (float *)(smem + DMA_LDS);         // (behind the operand images: written once, read after the barriers below)
  if (tid < BM) s_rs[tid] = my_rs;                       // 1.0 without row_scale
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    // specialised epilogues: this half's memory operands, requested ahead of the staging barriers (unconditional loads:
    // rows past the end are clamped)
    u32x4 gq[4];
    f32x4 rq[4][2];
    int32_t crow4[4];                            // (rows fit 32 bits: the host checks the 4 GiB reach of an operand panel)
    // (fp32 residual rows are 8 registers a pass: two passes are requested here, two behind the barriers, while
    // this wave's accumulators are on their way out - all four at once did not fit the 128-register budget)
    constexpr int NPRE = EPI == DMA_EPI_RES ? 2 : 4;
    auto fetch_epi = [&](int ps) {
      if constexpr (EPI == DMA_EPI_GPRE) gq[ps] = ld_nt<HINT>((const u32x4 *)((const T *)p.gpre + (int64_t)crow4[ps] * p.ld_gpre + n));
      if constexpr (EPI == DMA_EPI_RES) {
        rq[ps][0] = *(const f32x4 *)(p.residual + (int64_t)crow4[ps] * p.ld_res + n);
        rq[ps][1] = *(const f32x4 *)(p.residual + (int64_t)crow4[ps] * p.ld_res + n + 4);
      }
    };
    if constexpr (EPI != DMA_EPI_ANY) {
      if (n < p.N) {
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
          int m = mb32 + h * 64 + ps * 16 + r16;
          if (m >= me32) m = me32 - 1;
          crow4[ps] = c_row_idx ? c_row_idx[m] : m;
        }
#pragma unroll
        for (int ps = 0; ps < NPRE; ++ps) fetch_epi(ps);
      }
    }
    if (h) __syncthreads();
    if (wr == h) {
      // (the staging addresses are made anew for each half: shared between the halves, hipcc keeps them across half 0's
      // store pass and spills them there)
      int sli = li, slg = lg;
      asm volatile("" : "+v"(sli), "+v"(slg));
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          const int lrow = mi * 16 + sli;
          const int chunk = wc * 16 + ni * 4 + slg;
          *(f32x4 *)(smem + lrow * 512 + ((chunk ^ (lrow & 31)) << 4)) = acc[ni][mi];
        }
    }
    __syncthreads();
    if constexpr (EPI != DMA_EPI_ANY) {
      if (n < p.N) {
#pragma unroll
        for (int ps = NPRE; ps < 4; ++ps) fetch_epi(ps);
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
          const int lrow = ps * 16 + r16;
          const int64_t crow = crow4[ps];
          const int sw = lrow & 31;
          f32x4 v0 = *(const f32x4 *)(smem + lrow * 512 + (((2 * cg) ^ sw) << 4));
          f32x4 v1 = *(const f32x4 *)(smem + lrow * 512 + (((2 * cg + 1) ^ sw) << 4));
          v0 += b0; v1 += b1;
          if constexpr (EPI == DMA_EPI_GELU) {
            if constexpr (HINT) st_nt<true>((u32x4 *)((T *)p.pre_out + crow * p.ld_pre + n), pack8<T>(v0, v1));
            else Vec8<T>::store((T *)p.pre_out + crow * p.ld_pre + n, v0, v1);
#pragma unroll
            for (int j = 0; j < 4; ++j) { v0[j] = gelu_f(v0[j]); v1[j] = gelu_f(v1[j]); }
          }
          if constexpr (EPI == DMA_EPI_GPRE) {
            typedef T t8 __attribute__((ext_vector_type(8)));
            const t8 pr = __builtin_bit_cast(t8, gq[ps]);
#pragma unroll
            for (int j = 0; j < 4; ++j) { v0[j] *= gelu_grad_f((float)pr[j]); v1[j] *= gelu_grad_f((float)pr[4 + j]); }
          }
          const float sc = s_rs[h * 64 + lrow];
          v0 *= sc; v1 *= sc;
          if constexpr (EPI == DMA_EPI_RES) {
            v0 += rq[ps][0]; v1 += rq[ps][1];
            if (mb32 + h * 64 + lrow < me32) {          // (C may be the residual buffer: no duplicate read-modify-write)
              *(f32x4 *)((float *)p.C + crow * p.ldc + n) = v0;
              *(f32x4 *)((float *)p.C + crow * p.ldc + n + 4) = v1;
            }
          } else {
            Vec8<T>::store((T *)p.C + crow * p.ldc + n, v0, v1);
          }
        }
      }
    } else if (n < p.N) {
#pragma unroll 2
      for (int ps = 0; ps < 4; ++ps) {
        const int lrow = ps * 16 + r16;
        const int m = mb32 + h * 64 + lrow;
        if (m >= me32) break;
        const int sw = lrow & 31;
        const f32x4 v0 = *(const f32x4 *)(smem + lrow * 512 + (((2 * cg) ^ sw) << 4));
        const f32x4 v1 = *(const f32x4 *)(smem + lrow * 512 + (((2 * cg + 1) ^ sw) << 4));
        epilogue_row_any<T>(p, m, n, v0 + b0, v1 + b1, [&](int64_t) { return s_rs[h * 64 + lrow]; });
      }
    }
    M3_GEMM_STAMP(56 + h);                               // stores of half h issued
  }
#ifdef M3_GEMM_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  M3_GEMM_STAMP(58);                                     // my stores acknowledged
#endif
}

int launch_gemm_dma(const GemmDev &d, int dtype, int epi, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)d.m_tiles_max * d.n_tiles)), block(GEMM_THREADS);
  const int hints = cache_hints();
  auto go = [&](auto t) {
    with_epi(epi, [&](auto e) {
      constexpr int EPI = decltype(e)::value;
      constexpr int BIT = EPI == DMA_EPI_GELU ? M3_HINT_GEMM_PRE : EPI == DMA_EPI_GPRE ? M3_HINT_GEMM_GPRE : 0;   // 0: no hinted instance
      if (BIT && (hints & BIT)) {
        hipLaunchKernelGGL((gemm_nt_dma_kernel<decltype(t), EPI, BIT != 0>), grid, block, DMA_LDS_ALL, s, d);
      } else {
        hipLaunchKernelGGL((gemm_nt_dma_kernel<decltype(t), EPI, false>), grid, block, DMA_LDS_ALL, s, d);
      }
    });
  };
  if (dtype == M3_F16) go(half_t());
  else go(bf16_t());
  return check_launch("m3_gemm_nt");
}

}  // namespace m3

#ifdef M3_GEMM_STAMPS
extern "C" int m3_debug_gemm_stamps(unsigned long long *dst, int wgs, int clear) {
  using namespace m3;
  if (wgs > STAMP_WGS) wgs = STAMP_WGS;
  const size_t bytes = (size_t)wgs * STAMP_N * sizeof(unsigned long long);
  if (dst && hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_gemm_stamps), bytes) != hipSuccess) return M3_ERR_LAUNCH;
  if (clear) {
    void *sym = nullptr;
    if (hipGetSymbolAddress(&sym, HIP_SYMBOL(g_gemm_stamps)) != hipSuccess || hipMemset(sym, 0, sizeof(g_gemm_stamps)) != hipSuccess) return M3_ERR_LAUNCH;
  }
  return M3_OK;
}
#endif
