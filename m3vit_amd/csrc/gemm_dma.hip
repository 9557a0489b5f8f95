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

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int wr = wave >> 1, wc = wave & 1;

  int ts_lane = 0;
  const int nwg = p.tile_starts ? grouped_live_tiles(p.tile_starts, p.G, lane, ts_lane) * p.n_tiles : (int)gridDim.x;     // live workgroups (as in gemm_nt_kernel)
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
    m_begin = (int64_t)mt * BM;
    m_end = p.M;
    if (m_begin >= m_end) return;
  }
  const int n0 = nt * BN;

  // DMA assignment: wave w, piece j fills image rows (NPC*w + j)*RPI .. +RPI-1; lane l -> row + l / CPR,
  // LDS slot l % CPR, which holds source chunk (l % CPR) ^ swz(row).  Rows past the end are clamped (never stored).
  // Every index load of the prologue (the NPC gathered A rows of this lane; the row of the epilogue factor) is issued
  // before the first one is used: one memory latency in front of the first DMA instead of one per index (an index load
  // inside the per-piece loop, with the divide behind it, becomes its own basic block with its own wait).
  const char *a_src[NPC], *b_src[NPC];
  int64_t mrow[NPC];
  int32_t aix[NPC];
#pragma unroll
  for (int j = 0; j < NPC; ++j) {
    const int row = (NPC * wave + j) * RPI + lane / CPR;
    int64_t m = m_begin + row;
    if (m >= m_end) m = m_end - 1;
    mrow[j] = m;
  }
  if (p.a_row_idx) {
#pragma unroll
    for (int j = 0; j < NPC; ++j) aix[j] = p.a_row_idx[mrow[j]];
  }
  // per-row epilogue factor (DropPath scale / gate score of the routed row): thread r < 128 requests row r's factor NOW -
  // an index load and a dependent load - so that they arrive under the K loop instead of in front of every store pass
  const bool want_rs = p.row_scale && tid < BM;
  const int32_t *rs_idx = p.row_scale_idx ? p.row_scale_idx : p.c_row_idx;
  int64_t rs_m = m_begin + tid;
  if (rs_m >= m_end) rs_m = m_end - 1;
  int32_t rs_ix = 0;
  if (want_rs && rs_idx) rs_ix = rs_idx[rs_m];
  float my_rs = 1.0f;
  if (want_rs) {
    const int64_t srow = rs_idx ? (int64_t)rs_ix : rs_m;
    my_rs = p.row_scale[p.row_scale_div == 1 ? srow : srow / p.row_scale_div];
  }
#pragma unroll
  for (int j = 0; j < NPC; ++j) {
    const int row = (NPC * wave + j) * RPI + lane / CPR;
    const int c = (lane % CPR) ^ dma_swz(row);
    const int64_t src = p.a_row_idx ? (int64_t)div_by(aix[j], p.a_row_div, p.a_row_sh) : mrow[j];
    a_src[j] = p.A + src * p.lda_b + c * 16;
    int n = n0 + row;
    if (n >= p.N) n = p.N - 1;
    b_src[j] = p.B + (int64_t)g * p.b_group_b + (int64_t)n * p.ldb_b + c * 16;
  }
  const int nk = (p.K * (int)sizeof(T)) / RB;

  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  auto dma = [&](int ks) {
    char *dst = smem + (NPC * wave) * 1024;
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
      __builtin_amdgcn_global_load_lds((glb_void *)(a_src[j] + ks * RB), (lds_void *)(dst + j * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((glb_void *)(b_src[j] + ks * RB), (lds_void *)(dst + j * 1024 + OPB), 16, 0, 0);
    }
  };

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

  for (int ks = 0; ks < nk; ++ks) {
    dma(ks);
    __syncthreads();          // vmcnt(0) + barrier: the slice has landed
    compute();
    __syncthreads();          // everyone has read it
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
          int64_t m = m_begin + h * 64 + ps * 16 + r16;
          if (m >= m_end) m = m_end - 1;
          crow4[ps] = p.c_row_idx ? p.c_row_idx[m] : (int32_t)m;
        }
#pragma unroll
        for (int ps = 0; ps < NPRE; ++ps) fetch_epi(ps);
      }
    }
    if (h) __syncthreads();
    if (wr == h) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          const int lrow = mi * 16 + li;
          const int chunk = wc * 16 + ni * 4 + lg;
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
            if (m_begin + h * 64 + lrow < m_end) {          // (C may be the residual buffer: no duplicate read-modify-write)
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
        const int64_t m = m_begin + h * 64 + lrow;
        if (m >= m_end) break;
        const int sw = lrow & 31;
        const f32x4 v0 = *(const f32x4 *)(smem + lrow * 512 + (((2 * cg) ^ sw) << 4));
        const f32x4 v1 = *(const f32x4 *)(smem + lrow * 512 + (((2 * cg + 1) ^ sw) << 4));
        epilogue_row_any<T>(p, m, n, v0 + b0, v1 + b1, [&](int64_t) { return s_rs[h * 64 + lrow]; });
      }
    }
  }
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
