// The LDS-DMA weight-gradient kernels - 128 x 128 tiles (wgrad_dma_kernel), 256 x 256 tiles (wgrad_big_kernel) - and their
// launchers; wgrad.hip describes the call.  They share the zero row that rows past a unit's end are read from, the XOR
// swizzle of the LDS images and the condition a call must meet (wgrad_dma_form in wgrad.hip).  Compiled as part of wgrad_tiles.hip.
#include "wgrad_dev.h"

namespace m3 {

// ------------------------------------------------------------------------------------------------
// LDS-DMA variant (16-bit operands; round 5): the same 128 x 128 tile, wave layout, work units, slabs and ride-along
// reduce, but the operands go global -> LDS directly (global_load_lds_dwordx4), as in gemm_nt_dma_kernel:
//   - no staging registers, no ds_write pass, no second register set to spill: <= 128 VGPRs and ONE 32 KiB buffer (64
//     contraction rows x 128 columns of each operand), so FOUR workgroups share a CU instead of two and their DMA / MFMA
//     phases interleave; 32 MFMAs per wave between barriers instead of 16;
//   - the image rows are unpadded (a wave's DMA instruction fills 1 KiB = four 256-byte rows, lane-linear), so the
//     transposed reads are made conflict free by an XOR swizzle instead of the 288-byte stride: the 32-byte granule g of row
//     r sits at granule g ^ (r & 7) - the eight rows a half-wave's ds_read_b64_tr_b16 touches land on eight different
//     8-bank windows - applied to the per-lane SOURCE address on the way in and to the fragment addresses on the way out
//     (four address registers per operand, one per 16-column tile of the wave: an XOR does not fold into an offset field);
//   - rows past the end of a unit must contribute nothing: their source is a zero row in device memory (a DMA cannot be
//     masked into zeros at the LDS store the way the register-staged kernel does it);
//   - gather indices of step t + 1 are loaded under step t's MFMAs.
// Not for c_row_scale (the per-row factor is applied in registers on the way into LDS): those launches keep
// wgrad_tn_kernel<.., SC = true>.
__device__ __attribute__((aligned(256))) const uint32_t g_wgrad_zero_row[64] = {0};      // 256 bytes of zeros: the source of rows past a unit's end

template <typename T, bool GC, bool GA, bool SC = false>
__global__ __launch_bounds__(WG_THREADS, SC ? 3 : 4) void wgrad_dma_kernel(const WgradDev p) {
  typedef Mma<T> MM;
  typedef typename MM::frag frag;
  constexpr int ES = (int)sizeof(T);                        // 2 (f16 / bf16) or 4 (f32)
  constexpr int ROWS = 128 / ES;                            // contraction rows per step: 64 (16-bit) / 32 (f32)
  constexpr int RS = WG_T * ES;                             // image row: 128 columns = 256 / 512 bytes
  constexpr int OPB = ROWS * RS;                            // one operand image: 16 KiB
  constexpr int RPP = 1024 / RS;                            // image rows per DMA piece (1 KiB): 4 / 2
  constexpr int LPR = 64 / RPP;                             // lanes (= 16-byte chunks) per image row: 16 / 32
  constexpr int EPC = 16 / ES;                              // elements per 16-byte chunk
  constexpr int NPC = ROWS / RPP / 4;                       // DMA pieces per wave per operand per step: 4
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [dC image | A image]
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int wr = wave >> 1, wc = wave & 1;

  const int tiles = gridDim.x;
  int bz, gz;
  if (wgrad_ride_along(p, tid, bz, gz)) return;
  const int lin = blockIdx.x + tiles * (blockIdx.y + gridDim.y * bz);
  int tile, gs, g, sp, nst;
  int64_t r0, r1, s_begin;
  if (p.chunk_rows) {                          // gs = work unit; its slab is ws[gs]
    if (!wgrad_unit(p.group_offsets, p.G, p.chunk_rows, lin, tiles, lane, tile, gs, g, r0, r1)) return;
    sp = gs; s_begin = 0;
    nst = (int)((r1 - r0 + ROWS - 1) / ROWS);
  } else {
    const int log_id = xcd_remap(lin, tiles * gridDim.y * gz);
    tile = log_id % tiles; gs = log_id / tiles;
    g = gs % (int)gridDim.y; sp = gs / (int)gridDim.y;
    if (p.group_offsets && p.lpt) g = wgrad_lpt_group(p.group_offsets, p.G, g, lane);
    if (p.group_offsets) { r0 = p.group_offsets[g]; r1 = p.group_offsets[g + 1]; }
    else { r0 = 0; r1 = p.M; }
    const int64_t nsteps_all = (r1 - r0 + ROWS - 1) / ROWS;
    const int64_t per = (nsteps_all + p.splits - 1) / p.splits;
    s_begin = (int64_t)sp * per;
    int64_t s_end = s_begin + per;
    if (s_end > nsteps_all) s_end = nsteps_all;
    nst = (int)(s_end > s_begin ? s_end - s_begin : 0);
  }
  const int tn = tile / p.tiles_k, tk = tile - tn * p.tiles_k;
  const int n0 = tn * WG_T, k0 = tk * WG_T;
  const int64_t slab_id = p.chunk_rows ? (int64_t)sp : (int64_t)sp * p.G + g;

  f32x4 acc[4][4];   // [ki][ni]: MFMA rows = k, cols = n
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // DMA assignment: wave w, piece j fills image rows (4 w + j) * 4 .. + 3; lane l -> row + (l >> 4), physical 16-byte chunk
  // l & 15, which holds logical chunk (l & 15) ^ ((row & 7) << 1).  (row & 7) only depends on the parity of j and on the
  // lane, so a lane has two column offsets per operand.  Columns beyond N / K are clamped (outputs never stored).
  // Every step but a unit's last is 64 whole rows: its sources are (wave-uniform operand base) + (32-bit per-lane offset:
  // the host checks the 4 GiB reach), one address register per piece and no 64-bit arithmetic.  The last step (rows past the
  // end read a zero row, which lives in another buffer) takes 64-bit addresses picked by a bit mask - a `ok ? a : b` between
  // the two becomes a branch around each load, a basic block per piece with its own vmcnt(0).
  // fp32: a piece is two 512-byte rows, lane l -> row + (l >> 5), chunk l & 31, which holds logical chunk
  // (l & 31) ^ (((row >> 2) & 1) << 2): rows r and r + 4 - what a half-wave's ds_read_b32 touches - sit in different
  // 64-byte halves of the 128-byte bank window; ((row >> 2) & 1) = (j >> 1) & 1 for the wave's piece j.
  const int prow = lane / LPR;                               // row of this lane inside a piece
  uint32_t colC[2], colA[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = ES == 2 ? ((lane & 15) ^ ((((4 * q + prow) & 7)) << 1)) : ((lane & 31) ^ (q << 2));
    int nc = n0 + c * EPC, kc = k0 + c * EPC;
    if (nc > p.N - EPC) nc = p.N - EPC;
    if (kc > p.K - EPC) kc = p.K - EPC;
    colC[q] = (uint32_t)nc * ES; colA[q] = (uint32_t)kc * ES;
  }
  auto colq = [](int j) { return ES == 2 ? (j & 1) : ((j >> 1) & 1); };      // which of the two column offsets piece j takes
  const int rbase = (int)(r0 + s_begin * ROWS) + (NPC * wave) * RPP + prow;    // row of piece 0 in local step 0 (M < 2^31)
  const int rlast = (int)r1 - 1;
  const uint32_t ldc = (uint32_t)p.lddc_b, lda = (uint32_t)p.lda_b;
  int32_t ic[NPC], ia[NPC];
  auto load_index = [&](int step) {
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
      const int m = min(rbase + step * ROWS + RPP * j, rlast);
      if (GC) ic[j] = p.c_row_idx[m];
      if (GA) ia[j] = p.a_row_idx[m];
    }
  };
  char *const dma_dst = smem + (NPC * wave) * 1024;
  // SC (the combine's backward without d y: dC row of slot m = c_row_scale[c_row_idx[m]] * d out[c_row_idx[m] / div]): the
  // step's ROWS per-row factors go into a small LDS table behind the images - ONE 4-byte LDS-DMA of wave 0, lane l fetching
  // row l's factor through the index it loaded a step ahead - and multiply the dC fragments on their way into the MFMAs
  // (v_pk_mul_f16 with the factor rounded to fp16: one more 2^-11 rounding than the register-staged kernel's fp32 product,
  // inside the fp16 bound).  The zero rows of a unit's last step make their factors irrelevant.
  float *const s_sc = (float *)(smem + 2 * OPB);
  static_assert(!SC || (GC && !std::is_same<T, bf16_t>::value), "per-row factors: gathered dC rows, fp16 or fp32");
  int32_t sc_ix = 0;
  auto load_sc_index = [&](int step) {
    if (SC && wave == 0) sc_ix = p.c_row_idx[min((int)(r0 + s_begin * ROWS) + step * ROWS + (lane & (ROWS - 1)), rlast)];
  };
  auto dma_scores = [&]() {
    if (SC && wave == 0 && lane < ROWS)
      __builtin_amdgcn_global_load_lds((glb_void *)(p.c_row_scale + sc_ix), (lds_void *)s_sc, 4, 0, 0);
  };
  auto dma_full = [&](int step) {
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
      const int m = rbase + step * ROWS + RPP * j;
      // (gather divisors are powers of two here: the host sends anything else to the register-staged kernel)
      const uint32_t cr = GC ? (uint32_t)(ic[j] >> p.c_row_sh) : (uint32_t)m;
      const uint32_t ar = GA ? (uint32_t)(ia[j] >> p.a_row_sh) : (uint32_t)m;
      __builtin_amdgcn_global_load_lds((glb_void *)(p.dC + (cr * ldc + colC[colq(j)])), (lds_void *)(dma_dst + j * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((glb_void *)(p.A + (ar * lda + colA[colq(j)])), (lds_void *)(dma_dst + j * 1024 + OPB), 16, 0, 0);
    }
  };
  auto dma_tail = [&](int step) {
    const uint64_t zero_row = (uint64_t)(uintptr_t)g_wgrad_zero_row + (lane & 15) * 16;
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
      const int m = rbase + step * ROWS + RPP * j;
      const uint64_t ok = m <= rlast ? ~(uint64_t)0 : (uint64_t)0;
      const uint32_t cr = GC ? (uint32_t)(ic[j] >> p.c_row_sh) : (uint32_t)min(m, rlast);
      const uint32_t ar = GA ? (uint32_t)(ia[j] >> p.a_row_sh) : (uint32_t)min(m, rlast);
      const uint64_t sc = (((uint64_t)(uintptr_t)p.dC + (cr * ldc + colC[colq(j)])) & ok) | (zero_row & ~ok);
      const uint64_t sa = (((uint64_t)(uintptr_t)p.A + (ar * lda + colA[colq(j)])) & ok) | (zero_row & ~ok);
      __builtin_amdgcn_global_load_lds((glb_void *)(uintptr_t)sc, (lds_void *)(dma_dst + j * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((glb_void *)(uintptr_t)sa, (lds_void *)(dma_dst + j * 1024 + OPB), 16, 0, 0);
    }
  };

  // fragment addresses.  16-bit: lane (li, lg) supplies row 4 lg + (li >> 2) (+ 16 for the second half of a fragment, + 32 for the
  // second chunk of a step), columns col + 4 (li & 3) .. + 3 of the 16-column tile starting at col (ds_read_b64_tr_b16).
  // fp32: lane (li, lg) reads the elements (row 4 lg + r, column col + li), r = 0..3, one ds_read_b32 each (+ 16 rows for
  // the second chunk of a step); the swizzle swaps the 16-column tiles i and i ^ 1 for odd lg, so a lane has one base for
  // even and one for odd tiles per operand and the tile index stays an offset.
  int adK[4], adN[4];
  if constexpr (ES == 2) {
    const int s3 = (4 * (lg & 1) + (li >> 2)) & 7;
    const int frow = (4 * lg + (li >> 2)) * RS + 8 * (li & 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ck = (wr * 8 + 2 * i + ((li & 3) >> 1)) ^ (s3 << 1);
      const int cn = (wc * 8 + 2 * i + ((li & 3) >> 1)) ^ (s3 << 1);
      adK[i] = OPB + frow + ck * 16;
      adN[i] = frow + cn * 16;
    }
  } else {
    const int frow = 4 * lg * RS + (li & 3) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ck = (wr * 16 + 4 * i + (li >> 2)) ^ ((lg & 1) << 2);
      const int cn = (wc * 16 + 4 * i + (li >> 2)) ^ ((lg & 1) << 2);
      adK[i] = OPB + frow + ck * 16;
      adN[i] = frow + cn * 16;
    }
  }
  auto read_frag = [&](int ad, int rb) -> frag {
    if constexpr (ES == 2) {
      return __builtin_bit_cast(frag, wgrad_tr16_frag(smem + ad + rb * RS, smem + ad + (rb + 16) * RS));
    } else {
      const char *q = smem + ad + rb * RS;
      f32x4 f;
      f[0] = *(const float *)(q);
      f[1] = *(const float *)(q + RS);
      f[2] = *(const float *)(q + 2 * RS);
      f[3] = *(const float *)(q + 3 * RS);
      return f;
    }
  };

  // Bias gradient (column sums of dC over the contraction rows; once per n-tile: k-tile 0, waves wr == 0): a lane's dC
  // fragment holds 8 (fp32: 4) contraction rows of ITS column, so four v_dot2 with a pair of ones (fp32: three adds) sum
  // them - one fp32 register per 16-column tile instead of the register-staged kernel's extra MFMA row (16 accumulator
  // registers + a ones fragment: at 128 registers they spilled); the four lane groups' partial sums meet in two shuffles.
  const bool do_bias = (p.bias_ws || p.direct_db) && tk == 0 && wr == 0;
  float acc_b[4] = {0.f, 0.f, 0.f, 0.f};

  auto compute = [&]() {
#pragma unroll
    for (int kc = 0; kc < ROWS / MM::KC; ++kc) {
      frag fk[4], fn[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        fk[i] = read_frag(adK[i], kc * MM::KC);
        fn[i] = read_frag(adN[i], kc * MM::KC);
      }
      if constexpr (SC) {
        if constexpr (ES == 4) {
          const f32x4 sv = *(const f32x4 *)(s_sc + kc * 16 + 4 * lg);
#pragma unroll
          for (int i = 0; i < 4; ++i) fn[i] *= sv;
        } else {
          const f32x4 s0 = *(const f32x4 *)(s_sc + kc * 32 + 4 * lg), s1 = *(const f32x4 *)(s_sc + kc * 32 + 16 + 4 * lg);
          const f16x8 sh = wgrad_factor_f16x8(s0, s1);
#pragma unroll
          for (int i = 0; i < 4; ++i) fn[i] = __builtin_bit_cast(frag, __builtin_bit_cast(f16x8, fn[i]) * sh);
        }
      }
#pragma unroll
      for (int ki = 0; ki < 4; ++ki)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[ki][ni] = MM::mma(fk[ki], fn[ni], acc[ki][ni]);
      if (do_bias) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc_b[ni] = wgrad_colsum8<T>(fn[ni], acc_b[ni]);
      }
    }
  };

  if (nst > 0) {
    if (GC || GA) load_index(0);
    load_sc_index(0);
    for (int t = 0; t + 1 < nst; ++t) {
      dma_full(t);
      dma_scores();
      if (GC || GA) load_index(t + 1);                       // (arrives under this step's MFMAs; the barrier's vmcnt(0) covers it)
      load_sc_index(t + 1);
      __syncthreads();          // vmcnt(0) + barrier: the step's rows have landed
      compute();
      __syncthreads();          // everyone has read them
    }
    dma_tail(nst - 1);
    dma_scores();
    __syncthreads();
    compute();
  }

  if (do_bias) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      float v = acc_b[ni];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      const int n = n0 + wc * 64 + ni * 16 + li;
      if (lg == 0 && n < p.N) wgrad_store_bias(p, v, slab_id, g, n);
    }
  }
  wgrad_store_tile(p, acc, slab_id, g, n0, k0, wr, wc, li, lg);
}

// ------------------------------------------------------------------------------------------------
// 256 x 256 tiles for the ViT-Base weights (16-bit; N and K multiples of 256: 768, 2304, 3072): the 128 x 128 kernels bring
// 64 FLOP per operand byte into LDS and, with every byte of dC / A needed by K / 128 resp. N / 128 workgroups, run at what
// that path delivers (configs[3]'s experts: 1.86 GB per launch, 5.3 TB/s, 340 TFLOP/s).  This tile doubles the FLOP per
// byte: eight waves (wave (wr, wc) owns 128 k x 64 n: 8 x 4 MFMA tiles, 128 accumulator registers), one workgroup per
// CU, 64 contraction rows per step in two LDS stages of [dC image | A image] (64 rows x 512 B each): the rows of step
// t + 1 are in flight (LDS-DMA) while step t's fragments are read (ds_read_b64_tr_b16, issued as inline assembly - the
// compiler would otherwise drain the DMA before every LDS read it knows of) and multiplied.  One barrier per step.
// Image geometry: a DMA piece (1 KiB) is two rows; lane l -> row + (l >> 5), physical 16-byte chunk l & 31, which holds
// logical chunk (l & 31) ^ ((row & 7) << 1): the same 8-row XOR as the 128-wide 16-bit image, so the transposed reads
// (16 rows x 32 bytes per instruction) meet the same banks as there.  Gathers, per-row factor, fused bias sums, slabs or
// direct accumulation: as wgrad_dma_kernel.  The previous call's reduction does not ride here (512 threads): own launch.
// Diagnostic build only (make CXXFLAGS+=-DM3_WGRAD_STAMPS, tools/wgrad_big_stamps.py): lane 0 of waves 0 and 4 of the first
// workgroups of wgrad_big_kernel record s_memtime per step - after the DMA issue, after the MFMAs, after the vmcnt wait, after
// the barrier.  No stamp executes in the shipped kernel.
#ifdef M3_WGRAD_STAMPS
constexpr int WSTAMP_WGS = 512, WSTAMP_N = 2 * (2 + 4 * 24);
__device__ unsigned long long g_wbig_stamps[WSTAMP_WGS][WSTAMP_N];
#define WB_STAMP(i)                                                                                                   \
  do {                                                                                                                \
    if ((threadIdx.x & 255) == 0 && blockIdx.x < WSTAMP_WGS && blockIdx.y == 0 && blockIdx.z == 0 && (i) < WSTAMP_N / 2)   \
      g_wbig_stamps[blockIdx.x][(threadIdx.x >> 8) * (WSTAMP_N / 2) + (i)] = __builtin_amdgcn_s_memtime();             \
  } while (0)
#else
#define WB_STAMP(i) do { } while (0)
#endif
// What a 64-row step spends (in-kernel stamps, tools/wgrad_big_stamps.py, profiles/r05_wgrad_big_stamps.txt): ~800-1 550 cycles in
// which the waves sit in the ISSUE of their eight DMA instructions (a wave is held there until the CU's load path has taken
// them: the step's 64 KiB pass while nobody multiplies), ~1 800-2 300 of fragment reads + 64 MFMAs (1 024 of them MFMA), then
// the wait and the barrier: 4 250 in all, transfer and MFMA time adding up instead of overlapping.  Three re-arrangements were
// built and measured on the dense shapes, all within +-4 % of this one: a DMA instruction behind every eight MFMAs, waves 4-7
// sending theirs after multiplying instead of before, and the DMA issued in the shadow of the fragment reads.
// contraction rows per step: 64 (two stages, one step in flight ahead of the one multiplied).  32 (four stages, three in
// flight) measured level to 3 % slower (profiles/r05_wgrad_big.txt): the step is not waiting for its DMA - what
// paces it is LDS traffic (48 transposed reads per wave and step next to the 64 KiB the DMA writes), as in the 128-wide kernels
constexpr int BG_ROWS = 64;
constexpr int BG_NSTAGE = 2;                          // 128 KiB of operand stages
constexpr int BG_OPB = BG_ROWS * BG_RS;              // one operand image: 32 KiB
constexpr int BG_STAGE = 2 * BG_OPB;                 // [dC | A]
constexpr int BG_LDS = BG_NSTAGE * (BG_STAGE + 256); // the stages + every stage's per-row factors

template <typename T, bool GC, bool GA, bool SC = false>
__global__ __launch_bounds__(BG_THREADS, 1) void wgrad_big_kernel(const WgradDev p) {
  typedef Mma<T> MM;
  typedef typename MM::frag frag;
  static_assert(sizeof(T) == 2, "16-bit operands");
  static_assert(!SC || (GC && std::is_same<T, half_t>::value), "per-row factors: gathered dC rows, fp16");
  constexpr int ROWS = BG_ROWS, RS = BG_RS, NPC = ROWS / 16, NS = BG_NSTAGE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int wr = wave >> 2, wc = wave & 3;

  const int tiles = gridDim.x;
  const int lin = blockIdx.x + tiles * (blockIdx.y + gridDim.y * blockIdx.z);
  int tile, gs, g, sp, nst;
  int64_t r0, r1, s_begin;
  if (p.chunk_rows) {
    if (!wgrad_unit(p.group_offsets, p.G, p.chunk_rows, lin, tiles, lane, tile, gs, g, r0, r1)) return;
    sp = gs; s_begin = 0;
    nst = (int)((r1 - r0 + ROWS - 1) / ROWS);
  } else {
    const int log_id = xcd_remap(lin, tiles * gridDim.y * gridDim.z);
    tile = log_id % tiles; gs = log_id / tiles;
    g = gs % (int)gridDim.y; sp = gs / (int)gridDim.y;
    if (p.group_offsets && p.lpt) g = wgrad_lpt_group(p.group_offsets, p.G, g, lane);
    if (p.group_offsets) { r0 = p.group_offsets[g]; r1 = p.group_offsets[g + 1]; }
    else { r0 = 0; r1 = p.M; }
    const int64_t nsteps_all = (r1 - r0 + ROWS - 1) / ROWS;
    const int64_t per = (nsteps_all + p.splits - 1) / p.splits;
    s_begin = (int64_t)sp * per;
    int64_t s_end = s_begin + per;
    if (s_end > nsteps_all) s_end = nsteps_all;
    nst = (int)(s_end > s_begin ? s_end - s_begin : 0);
  }
  const int tn = tile / p.tiles_k, tk = tile - tn * p.tiles_k;
  const int n0 = tn * BG_T, k0 = tk * BG_T;
  const int64_t slab_id = p.chunk_rows ? (int64_t)sp : (int64_t)sp * p.G + g;

  f32x4 acc[8][4];   // [ki][ni]: MFMA rows = k, cols = n
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // DMA: wave w, piece j fills image rows 2 (NPC w + j) + (lane >> 5) of both operands
  const int prow = lane >> 5;
  uint32_t colC[NPC], colA[NPC];
#pragma unroll
  for (int j = 0; j < NPC; ++j) {
    const int irow = 2 * (NPC * wave + j) + prow;
    const int c = (lane & 31) ^ ((irow & 7) << 1);
    colC[j] = (uint32_t)(n0 + c * 8) * 2; colA[j] = (uint32_t)(k0 + c * 8) * 2;
  }
  const int rbase = (int)(r0 + s_begin * ROWS) + 2 * NPC * wave + prow;
  const int rlast = (int)r1 - 1;
  const uint32_t ldc = (uint32_t)p.lddc_b, lda = (uint32_t)p.lda_b;
  int32_t ic[NPC], ia[NPC];
  auto load_index = [&](int step) {
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
      const int m = min(rbase + step * ROWS + 2 * j, rlast);
      if (GC) ic[j] = p.c_row_idx[m];
      if (GA) ia[j] = p.a_row_idx[m];
    }
  };
  char *const s_sc = smem + NS * BG_STAGE;                        // [stage][64 floats]
  int32_t sc_ix = 0;
  auto load_sc_index = [&](int step) {
    if (SC && wave == 0) sc_ix = p.c_row_idx[min((int)(r0 + s_begin * ROWS) + step * ROWS + lane, rlast)];
  };
  auto dma = [&](int step, int stage, auto tail_c) {
    constexpr bool TAIL = decltype(tail_c)::value;
    char *const dst = smem + stage * BG_STAGE + (NPC * wave) * 1024;
    const uint64_t zero_row = (uint64_t)(uintptr_t)g_wgrad_zero_row + (lane & 15) * 16;
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
      const int m = rbase + step * ROWS + 2 * j;
      const uint32_t cr = GC ? (uint32_t)(ic[j] >> p.c_row_sh) : (uint32_t)(TAIL ? min(m, rlast) : m);
      const uint32_t ar = GA ? (uint32_t)(ia[j] >> p.a_row_sh) : (uint32_t)(TAIL ? min(m, rlast) : m);
      if constexpr (!TAIL) {
        __builtin_amdgcn_global_load_lds((glb_void *)(p.dC + (cr * ldc + colC[j])), (lds_void *)(dst + j * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((glb_void *)(p.A + (ar * lda + colA[j])), (lds_void *)(dst + j * 1024 + BG_OPB), 16, 0, 0);
      } else {                                        // rows past the unit's end read the zero row (bit-mask select: no branches)
        const uint64_t ok = m <= rlast ? ~(uint64_t)0 : (uint64_t)0;
        const uint64_t sc_ = (((uint64_t)(uintptr_t)p.dC + (cr * ldc + colC[j])) & ok) | (zero_row & ~ok);
        const uint64_t sa_ = (((uint64_t)(uintptr_t)p.A + (ar * lda + colA[j])) & ok) | (zero_row & ~ok);
        __builtin_amdgcn_global_load_lds((glb_void *)(uintptr_t)sc_, (lds_void *)(dst + j * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((glb_void *)(uintptr_t)sa_, (lds_void *)(dst + j * 1024 + BG_OPB), 16, 0, 0);
      }
    }
    if (SC && wave == 0)
      __builtin_amdgcn_global_load_lds((glb_void *)(p.c_row_scale + sc_ix), (lds_void *)(s_sc + stage * 256), 4, 0, 0);
  };

  // transposed fragment reads: lane (li, lg) supplies row 4 lg + (li >> 2) (+ 16: second half of a fragment, + 32: second
  // chunk of a 64-row step), 8 bytes at columns 4 (li & 3) .. + 3 of the 16-column tile
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_void *)smem;
  const int s3 = (4 * (lg & 1) + (li >> 2)) & 7;
  const uint32_t frow = lds0 + (uint32_t)((4 * lg + (li >> 2)) * RS + 8 * (li & 1));
  uint32_t adK[8], adN[4];
#pragma unroll
  for (int i = 0; i < 8; ++i) adK[i] = frow + BG_OPB + (uint32_t)(((wr * 16 + 2 * i + ((li & 3) >> 1)) ^ (s3 << 1)) * 16);
#pragma unroll
  for (int i = 0; i < 4; ++i) adN[i] = frow + (uint32_t)(((wc * 8 + 2 * i + ((li & 3) >> 1)) ^ (s3 << 1)) * 16);
  const uint32_t ad_sc = lds0 + NS * BG_STAGE + 16 * lg;
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
#define BG_TR(dst, addr, off) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(off))

  const bool do_bias = (p.bias_ws || p.direct_db) && tk == 0 && wr == 0;
  float acc_b[4] = {0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int stage) {
    const uint32_t so = (uint32_t)stage * BG_STAGE;
#pragma unroll
    for (int kc = 0; kc < ROWS / 32; ++kc) {
      u32x2 rk[8][2], rn[4][2];
      f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = s0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (kc == 0) { BG_TR(rn[i][0], adN[i] + so, 0); BG_TR(rn[i][1], adN[i] + so, 16 * RS); }
        else { BG_TR(rn[i][0], adN[i] + so, 32 * RS); BG_TR(rn[i][1], adN[i] + so, 48 * RS); }
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (kc == 0) { BG_TR(rk[i][0], adK[i] + so, 0); BG_TR(rk[i][1], adK[i] + so, 16 * RS); }
        else { BG_TR(rk[i][0], adK[i] + so, 32 * RS); BG_TR(rk[i][1], adK[i] + so, 48 * RS); }
      }
      if constexpr (SC) {
        const uint32_t a_ = ad_sc + (uint32_t)stage * 256;
        if (kc == 0) {
          asm volatile("ds_read_b128 %0, %1 offset:0" : "=v"(s0) : "v"(a_));
          asm volatile("ds_read_b128 %0, %1 offset:64" : "=v"(s1) : "v"(a_));
        } else {
          asm volatile("ds_read_b128 %0, %1 offset:128" : "=v"(s0) : "v"(a_));
          asm volatile("ds_read_b128 %0, %1 offset:192" : "=v"(s1) : "v"(a_));
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      frag fk[8], fn[4];
#pragma unroll
      for (int i = 0; i < 8; ++i) fk[i] = __builtin_bit_cast(frag, u32x4{rk[i][0][0], rk[i][0][1], rk[i][1][0], rk[i][1][1]});
#pragma unroll
      for (int i = 0; i < 4; ++i) fn[i] = __builtin_bit_cast(frag, u32x4{rn[i][0][0], rn[i][0][1], rn[i][1][0], rn[i][1][1]});
      if constexpr (SC) {
        const f16x8 sh = wgrad_factor_f16x8(s0, s1);
#pragma unroll
        for (int i = 0; i < 4; ++i) fn[i] = __builtin_bit_cast(frag, __builtin_bit_cast(f16x8, fn[i]) * sh);
      }
#pragma unroll
      for (int ki = 0; ki < 8; ++ki)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[ki][ni] = MM::mma(fk[ki], fn[ni], acc[ki][ni]);
      if (do_bias) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc_b[ni] = wgrad_colsum8<T>(fn[ni], acc_b[ni]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
#undef BG_TR

  // Pipeline: step t + 1 is in flight (or landed) while step t is multiplied.  A step's issue slot is
  // [its 2 NPC DMA pieces, the gather indices of the step after it]; the wait in front of the barrier is for everything
  // outstanding, so step t + 1 has landed when the barrier opens.
  const std::true_type is_tail; const std::false_type not_tail;
  auto issue = [&](int step) {                 // the DMA of `step` (its indices are in registers), then the indices of step + 1
    if (step < nst) {
      if (step + 1 == nst) dma(step, step % NS, is_tail); else dma(step, step % NS, not_tail);
      if (step + 1 < nst) { if (GC || GA) load_index(step + 1); load_sc_index(step + 1); }
    }
  };
  WB_STAMP(0);
  if (nst > 0) {
    if (GC || GA) load_index(0);
    load_sc_index(0);
#pragma unroll
    for (int q = 0; q < NS - 1; ++q) issue(q);      // the stages ahead of the one multiplied
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();               // step 0 has landed for every wave
    WB_STAMP(1);
    for (int t = 0; t < nst; ++t) {
      issue(t + NS - 1);                        // into the stage step t - 1 was multiplied from
      WB_STAMP(2 + 4 * t);
      compute(t % NS);
      WB_STAMP(3 + 4 * t);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      WB_STAMP(4 + 4 * t);
      __builtin_amdgcn_s_barrier();            // step t + 1 has landed for every wave, and every wave is done reading step t
      WB_STAMP(5 + 4 * t);
    }
  }

  if (do_bias) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      float v = acc_b[ni];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      const int n = n0 + wc * 64 + ni * 16 + li;
      if (lg == 0) wgrad_store_bias(p, v, slab_id, g, n);
    }
  }
  float *out = p.direct_dW ? p.direct_dW + (int64_t)g * p.N * p.K : p.ws + slab_id * (int64_t)p.N * p.K;
  const bool add = p.direct_dW && p.direct_beta;
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    float *row = out + (int64_t)(n0 + wc * 64 + ni * 16 + li) * p.K + k0 + wr * 128 + 4 * lg;
    f32x4 old[8];
    if (add) {
#pragma unroll
      for (int ki = 0; ki < 8; ++ki) old[ki] = *(const f32x4 *)(row + ki * 16);
    }
#pragma unroll
    for (int ki = 0; ki < 8; ++ki) *(f32x4 *)(row + ki * 16) = add ? acc[ki][ni] + old[ki] : acc[ki][ni];
  }
}

// the instances, 128 x 128: every dtype with every pair of gathers; a per-row factor on gathered fp16 / fp32 rows
struct WgDma {
  template <typename T, bool GC, bool GA, bool SC> static const void *instance() {
    if constexpr (!SC || (GC && !std::is_same<T, bf16_t>::value)) return (const void *)wgrad_dma_kernel<T, GC, GA, SC>;
    else return nullptr;
  }
};
// 256 x 256: the 16-bit dtypes with every pair of gathers; a per-row factor on gathered fp16 rows
struct WgBig {
  template <typename T, bool GC, bool GA, bool SC> static const void *instance() {
    if constexpr (sizeof(T) == 2 && (!SC || (GC && std::is_same<T, half_t>::value))) return (const void *)wgrad_big_kernel<T, GC, GA, SC>;
    else return nullptr;
  }
};

int launch_wgrad_dma(int dtype, bool gc, bool ga, bool sc, dim3 grid, const WgradDev &d, hipStream_t s) {
  const size_t ldsd = 2 * 64 * WG_T * 2 + 256;       // 32 KiB + the step's per-row factors
  return wgrad_launch_instance<WgDma>(dtype, gc, ga, sc, grid, dim3(WG_THREADS), ldsd, d, s);
}

int launch_wgrad_big(int dtype, bool gc, bool ga, bool sc, dim3 grid, const WgradDev &d, hipStream_t s) {
  static bool attr_set = false;
  if (!attr_set) {
    wgrad_each_instance<WgBig>([](int, bool, bool, bool, const void *k) {
      (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, BG_LDS);
    });
    attr_set = true;
  }
  return wgrad_launch_instance<WgBig>(dtype, gc, ga, sc, grid, dim3(BG_THREADS), BG_LDS, d, s);
}

}  // namespace m3

#ifdef M3_WGRAD_STAMPS
extern "C" int m3_debug_wbig_stamps(unsigned long long *dst, int wgs) {
  using namespace m3;
  if (wgs > WSTAMP_WGS) wgs = WSTAMP_WGS;
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_wbig_stamps), (size_t)wgs * WSTAMP_N * sizeof(unsigned long long)) == hipSuccess ? M3_OK : M3_ERR_LAUNCH;
}
#endif
